#!/bin/bash
# GPU parity suite + one bench line: scripts/gpu_check.sh [pytest -k expr]
set -o pipefail
OUT=${FOVRT_OUT:-bench_out}  # where the logs go
mkdir -p $OUT
K=${1:-}
timeout -k 10 300 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread ${K:+-k "$K"} > $OUT/gpu_tests.log 2>&1 || { tail -30 $OUT/gpu_tests.log; exit 1; }
tail -2 $OUT/gpu_tests.log
timeout -k 10 200 python bench.py --full --no-cpu-baseline --steps 20 --warmup 5 > $OUT/ab_default.log 2>&1 || exit 2
