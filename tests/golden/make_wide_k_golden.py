#!/usr/bin/env python3
"""Regenerate tests/golden/ref_wide_k.json from the REAL reference (build container only).

Runs the stock reference program (oracle/_ref/RayTracer, reference source/Main.cpp) the way
make_golden.py does — from a build/ directory beside ../meshes — on photon-map frames with
k in {17, 40, 200}, ray and path mode, and stores the md5 of every PPM it writes (data only).
tests/test_oracle_wide_k.py checks the oracle's legacy-RNG frames against them: the yardstick
of the GPU's k > 16 frames, pinned to the reference at large k.
Usage:  python tests/golden/make_wide_k_golden.py
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(ROOT, "oracle", "_ref", "RayTracer")
MESHES = os.path.join(HERE, "meshes")
OUT = os.path.join(HERE, "ref_wide_k.json")

W, H, N, P = 48, 40, 2, 5000
KS = (17, 40, 200)
MODES = (0, 1)


def name(mode, k):
    return "cubes_%dx%d_m%d_N%d_p%d_k%d" % (W, H, mode, N, P, k)


def main():
    if not os.path.exists(REF):
        sys.exit("oracle/_ref/RayTracer is missing: it is built only where the reference sources exist")
    cases = {}
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "build"))
        os.symlink(MESHES, os.path.join(tmp, "meshes"))  # the stock binary reads ../meshes (Main.cpp:186-187)
        cwd = os.path.join(tmp, "build")
        for mode in MODES:
            for k in KS:
                out = os.path.join(cwd, name(mode, k) + ".ppm")
                args = ["-width", str(W), "-height", str(H), "-m", str(mode), "-N", str(N), "-p", str(P), "-k", str(k),
                        "-o", out]
                subprocess.run([REF] + args, cwd=cwd, check=True, capture_output=True, timeout=1800)
                md5 = hashlib.md5(open(out, "rb").read()).hexdigest()
                cases[name(mode, k)] = dict(scene="cubes", w=W, h=H, mode=mode, N=N, p=P, k=k, md5=md5,
                                            args=" ".join(args[:-2]))
                print(name(mode, k), md5, flush=True)
    with open(OUT, "w") as f:
        json.dump(cases, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
