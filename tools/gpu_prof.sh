#!/usr/bin/env bash
# Profiling run on the GPU box: kernel trace + stats of a short bench (rocprofv3), output
# under $RJ_OUT/prof_$TAG.  Counters (--pmc) run separately (gpu_pmc.sh).
set -o pipefail
export RJ_OUT=${RJ_OUT:-bench_out}  # where the logs go
TAG=${1:-run}
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
mkdir -p $RJ_OUT/prof_$TAG
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $RJ_OUT/prof_$TAG -o prof -- \
  python3 bench.py --full --steps ${STEPS:-5} --warmup 1 --no-cpu-baseline --no-extras ${BENCH_EXTRA:-} > $RJ_OUT/prof_$TAG/bench.log 2>&1
