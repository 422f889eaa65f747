"""rt_render_adaptive's C ABI without a GPU: the entry points exist, the ctypes views have the header's layout, the
argument checks that come before any device work answer RT_ERR_INVALID; and the numpy restatement of the rule
(tests/adaptive_ref.py) on synthetic chains whose answers are known."""
import ctypes as C
import os
import subprocess

import numpy as np

import adaptive_ref
import pyrt

ROOT = pyrt.ROOT


def test_adaptive_entry_points_exist():
    L = pyrt.amd()
    for name in ("rt_render_adaptive", "rt_render_adaptive_device"):
        assert hasattr(L, name) and name in pyrt.AMD_SYMBOLS


def test_adaptive_structs_match_header(tmp_path):
    """sizeof and field offsets of rt_adaptive_params / rt_adaptive_report as the C compiler lays them out."""
    src = tmp_path / "layout.c"
    structs = (("rt_adaptive_params", pyrt.AdaptiveParams), ("rt_adaptive_report", pyrt.AdaptiveReport))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_amd.h"', "int main(void) {"]
    for st, cls in structs:
        lines.append('  printf("%%s %%zu\\n", "%s", sizeof(%s));' % (st, st))
        for n, _ in cls._fields_:
            lines.append('  printf("%%s.%%s %%zu\\n", "%s", "%s", offsetof(%s, %s));' % (st, n, st, n))
    lines += ["  return 0;", "}"]
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for st, cls in structs:
        assert int(got[st]) == C.sizeof(cls)
        for n, _ in cls._fields_:
            assert int(got["%s.%s" % (st, n)]) == getattr(cls, n).offset, (st, n)


def test_null_arguments_are_invalid_without_a_device():
    L = pyrt.amd()
    p = pyrt.make_params(16, 16, 4)
    a = pyrt.make_adaptive(0.1, 4)
    rep = pyrt.AdaptiveReport()
    rep.passes = 7
    assert L.rt_render_adaptive(None, C.byref(p), C.byref(a), None, None, None, None, C.byref(rep), None) == 1
    assert b"null" in L.rt_last_error() and rep.passes == 7  # a rejected call writes nothing
    assert L.rt_render_adaptive_device(None, C.byref(p), C.byref(a), None, None, None, None, None, None, None) == 1


def _chain(per_pass, P):
    """accumulators of passes whose per-pass sums are per_pass[k] ([h][w][4], float32), summed in float32."""
    acc = np.zeros_like(per_pass[0])
    out = []
    for d in per_pass:
        acc = (acc + d).astype(np.float32)
        out.append(acc.copy())
    return out


def test_rule_constant_pixels_retire_at_min_passes():
    h, w, P = 12, 20, 4
    d = np.zeros((h, w, 4), np.float32)
    d[..., :3] = 2.0
    d[..., 3] = P  # every sample hit
    chain = _chain([d] * 8, P)
    bg = np.zeros((h, w, 3), np.float32)
    K, active = adaptive_ref.run_rule(chain, bg, P, 0.05, 8)
    assert (K == 4).all() and active == [6] * 4  # 3 x 2 granules
    K, active = adaptive_ref.run_rule(chain, bg, P, 0.05, 8, min_passes=2)
    assert (K == 2).all()
    K, active = adaptive_ref.run_rule(chain, bg, P, 0., 8)  # threshold 0: never
    assert (K == 8).all() and active == [6] * 8


def test_rule_noisy_granule_keeps_going():
    h, w, P = 16, 16, 4
    rng = np.random.default_rng(3)
    per_pass = []
    for k in range(8):
        d = np.zeros((h, w, 4), np.float32)
        d[..., :3] = 1.0
        d[..., 3] = P
        d[3, 12, :3] = rng.uniform(0, 8, 3)  # one noisy pixel in granule (0, 1)
        per_pass.append(d)
    chain = _chain(per_pass, P)
    K, active = adaptive_ref.run_rule(chain, np.zeros((h, w, 3), np.float32), P, 0.02, 8)
    assert K[0, 1] == 8 and (K[1] == 4).all() and K[0, 0] == 4
    assert active == [4, 4, 4, 4, 1, 1, 1, 1]


def test_rule_counts_misses_against_the_background():
    """A pixel whose hits vary while its colour sum stays 0 is noisy once the background is resolved in."""
    h, w, P = 8, 8, 4
    per_pass = []
    for k in range(6):
        d = np.zeros((h, w, 4), np.float32)
        d[..., 3] = P
        d[2, 2, 3] = k % 3  # misses vary
        per_pass.append(d)
    chain = _chain(per_pass, P)
    K0, _ = adaptive_ref.run_rule(chain, np.zeros((h, w, 3), np.float32), P, 0.05, 6)
    K1, _ = adaptive_ref.run_rule(chain, np.ones((h, w, 3), np.float32), P, 0.05, 6)
    assert K0[0, 0] == 4 and K1[0, 0] == 6


def test_resolve_is_k_resolve_per_pixel():
    rng = np.random.default_rng(5)
    acc = rng.uniform(0, 30, (5, 7, 4)).astype(np.float32)
    acc[..., 3] = rng.integers(0, 8, (5, 7))
    bg = rng.uniform(0, 1, (5, 7, 3)).astype(np.float32)
    spp = np.where(rng.uniform(size=(5, 7)) < 0.5, 8, 16)
    out = adaptive_ref.resolve(acc, bg, spp)
    for y in range(5):
        for x in range(7):
            n = np.float32(spp[y, x])
            miss = np.float32(int(n) - int(acc[y, x, 3]))
            exp = acc[y, x, :3] / n + bg[y, x] * miss / n
            assert np.array_equal(out[y, x].view(np.uint32), exp.astype(np.float32).view(np.uint32))
