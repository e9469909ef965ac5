#!/bin/bash
# End-of-round evidence on the GPU box: the default bench line, its rocprof kernel trace and HBM
# counters (scripts/profile.sh), and one bench line per BASELINE config (scripts/configs_bench.sh).
#   scripts/round_profile.sh <tag>   ->  $OUT/<tag>_bench.log, $OUT/prof_<tag>/, $OUT/cfg_C*.log
set -eo pipefail
OUT=${FOVRT_OUT:-bench_out}  # where the logs go
TAG=${1:?tag}
ROOT=${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}
cd "$ROOT"
mkdir -p $OUT
bash scripts/profile.sh "$TAG"
echo "profile done"
timeout -k 10 400 python bench.py --full > "$OUT/${TAG}_bench.log" 2>&1
echo "bench done"
bash scripts/configs_bench.sh
