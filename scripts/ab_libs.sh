#!/bin/bash
# A/B of library variants on the bench workload: scripts/ab_libs.sh <lib.so>... (default build first)
set -o pipefail
OUT=${FOVRT_OUT:-bench_out}  # where the logs go
mkdir -p $OUT
timeout -k 10 200 python bench.py --full --no-cpu-baseline --steps 10 --warmup 3 > $OUT/ab_default.log 2>&1 || exit 1
for L in "$@"; do
  n=$(basename "$L" .so)
  FOVRT_LIB=$L timeout -k 10 200 python bench.py --full --no-cpu-baseline --steps 10 --warmup 3 > $OUT/ab_$n.log 2>&1 || exit 2
done
