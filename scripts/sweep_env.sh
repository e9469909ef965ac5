#!/bin/bash
# bench.py under a list of environment settings: scripts/sweep_env.sh "VAR=a" "VAR=b" ...
set -o pipefail
OUT=${FOVRT_OUT:-bench_out}  # where the logs go
mkdir -p $OUT
i=0
for e in "$@"; do
  env $e timeout -k 10 200 python bench.py --full --no-cpu-baseline --steps 10 --warmup 3 > $OUT/sweep_$i.log 2>&1 || exit 1
  echo "$e" > $OUT/sweep_$i.env
  i=$((i+1))
done
