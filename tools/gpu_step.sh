set -o pipefail
export RJ_OUT=${RJ_OUT:-bench_out}  # where the logs go
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
mkdir -p $RJ_OUT/r6z
timeout -k 10 300 python3 -c "import __graft_entry__ as g; g.smoke()" > $RJ_OUT/r6z/smoke.log 2>&1 || { cat $RJ_OUT/r6z/smoke.log; exit 1; }
tail -1 $RJ_OUT/r6z/smoke.log
timeout -k 10 900 python3 -u -m pytest tests -m gpu -x -q --timeout 200 --timeout-method thread > $RJ_OUT/r6z/suite.log 2>&1 || { tail -30 $RJ_OUT/r6z/suite.log; exit 1; }
tail -1 $RJ_OUT/r6z/suite.log
timeout -k 10 300 python3 bench.py --full --steps 10 --no-cpu-baseline --no-extras > $RJ_OUT/r6z/bench.log 2>&1 || { tail -20 $RJ_OUT/r6z/bench.log; exit 1; }
python3 tools/bench_summary.py $RJ_OUT/r6z/bench.log
