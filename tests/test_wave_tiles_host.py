"""The wave-tile list builder (csrc/wave_tiles.h) with the fine tail, host only: tools/wave_tiles_host_check.cpp built with
the address and undefined-behaviour sanitizers and run.  Over frame sizes no footprint divides, one to three shards, every
coarse and fine shift and F = 0, 1, 2, 5, more than the list and all of it: every owned in-image pixel is covered exactly
once, the fine items are last and in order, fineFrom and the counts are right."""
import os
import subprocess

import pyrt


def test_list_builder(tmp_path):
    exe = str(tmp_path / "wave_tiles_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                    "-static-libubsan", "-I" + os.path.join(pyrt.ROOT, "ray-tracing-engine_amd", "csrc"),
                    os.path.join(pyrt.ROOT, "tools", "wave_tiles_host_check.cpp"), "-o", exe], check=True, capture_output=True, text=True,
                   timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    assert int(r.stdout.split()[0]) > 10000 and int(r.stdout.split()[2]) == 0
