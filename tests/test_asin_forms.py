"""rt_asin (include/rt_pixelmode.h) evaluates its polynomial and its quotient once, on the argument selected by
`ax < 0.5`, where it used to call rt_asin_poly in both arms.  tools/asin_forms_host_check.cpp holds the earlier text and
compares bit patterns: +-0, denormals, the neighbours of +-2^-27, +-0.5, +-0.975 and +-1, values beyond 1, NaN and +-inf,
10^7 seeded doubles in [-1, 1] and the hemisphere sample's own argument over 10^6 consecutive engine states; no mismatch
is allowed.  The program is built with the address and undefined-behaviour sanitizers (host code only, its own main,
the runtimes linked statically).  The device's rt_asin (k_unit) must give the host's bits on the program's edge and
stream inputs."""
import os
import subprocess

import numpy as np
import pytest

import pyrt

_built = {}


def program(tmp_path_factory):
    """The check, built once per session; it runs once too and leaves its 4,096 inputs with the host's results."""
    if not _built:
        d = tmp_path_factory.mktemp("asin_forms")
        exe, data = str(d / "asin_forms_host_check"), str(d / "values.bin")
        subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-static-libasan", "-static-libubsan", "-I" + os.path.join(pyrt.ROOT, "include"),
                        os.path.join(pyrt.ROOT, "tools", "asin_forms_host_check.cpp"), "-o", exe],
                       check=True, capture_output=True, text=True, timeout=300)
        _built["run"] = subprocess.run([exe, data], capture_output=True, text=True, timeout=300)
        _built["data"] = data
    return _built


def test_one_polynomial_gives_the_bits_of_two(tmp_path_factory):
    r = program(tmp_path_factory)["run"]
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    n, bad = (int(r.stdout.split()[0]), int(r.stdout.split()[2]))
    assert n >= 11000000 and bad == 0


@pytest.mark.gpu
def test_device_asin_gives_the_host_s_bits(tmp_path_factory):
    b = program(tmp_path_factory)
    assert b["run"].returncode == 0, b["run"].stderr[-2000:]
    v = np.fromfile(b["data"], np.float64)
    x, want = v[:4096], v[4096:]
    got = pyrt.unit(pyrt.UNIT_ASIN, x).reshape(-1)
    diff = got.view(np.uint64) != want.view(np.uint64)
    # (every NaN the form returns is the one pattern 0x7ff8000000000000 on both sides)
    assert not diff.any(), "%d of %d differ, first x = %r: device %r, host %r" % (diff.sum(), len(x), x[np.argmax(diff)], got[np.argmax(diff)], want[np.argmax(diff)])
    assert np.isnan(want).any() and (np.abs(x) < 0.5).any() and (np.abs(x) >= 0.975).any()
