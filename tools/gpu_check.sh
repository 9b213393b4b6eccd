#!/usr/bin/env bash
# GPU-box check run: smoke -> pytest -m gpu -> short bench.  Every GPU step has its own time
# limit and the chain stops at the first crash/timeout (exit >= 124 or signal).
set -o pipefail
export RJ_OUT=${RJ_OUT:-bench_out}  # where the logs go
mkdir -p $RJ_OUT
TAG=${1:-run}
timeout -k 10 400 python -c "import __graft_entry__ as g; g.smoke()" > $RJ_OUT/smoke_$TAG.log 2>&1 || exit $?
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread ${PYTEST_ARGS:-} > $RJ_OUT/pytest_$TAG.log 2>&1
rc=$?
echo "pytest rc=$rc" >> $RJ_OUT/pytest_$TAG.log
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then exit $rc; fi
timeout -k 10 400 python bench.py --full ${BENCH_ARGS:---steps 3 --warmup 1 --batch 256 --no-cpu-baseline} > $RJ_OUT/bench_$TAG.log 2>&1
