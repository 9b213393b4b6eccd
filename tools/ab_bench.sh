#!/usr/bin/env bash
# A/B bench runs on the GPU box: each argument is "tag:ENV=VAL,ENV2=VAL2" (empty env list ok).
# Every run has its own time limit; the chain stops at the first failure.
set -o pipefail
export RJ_OUT=${RJ_OUT:-bench_out}  # where the logs go
mkdir -p $RJ_OUT
STEPS=${STEPS:-10}
for spec in "$@"; do
  tag=${spec%%:*}
  envs=${spec#*:}
  ( IFS=',' read -ra kvs <<< "$envs"
    for kv in "${kvs[@]}"; do [ -n "$kv" ] && export "$kv"; done
    timeout -k 10 300 python bench.py --full --steps $STEPS --warmup 2 --no-cpu-baseline ${BENCH_EXTRA:-} > $RJ_OUT/ab_$tag.log 2>&1 ) || exit $?
done
