#!/bin/bash
cd "$GRAFT_REPO_ROOT"
out=${1:?usage: tools/r3_check_bench.sh <log directory>}; mkdir -p "$out"
tools/run_guarded.sh "$out/t_app.log" 1100 python3 -m pytest tests/test_gpu_app.py tests/test_gpu_multi.py -x -q -m gpu || exit 1
tools/run_guarded.sh "$out/bench_default.log" 600 python3 bench.py --full --steps 10 --warmup 3 --cpu-baseline-full || exit 1
grep '^{' "$out/bench_default.log" > "$out/bench_default.json"
