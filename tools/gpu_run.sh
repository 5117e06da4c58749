#!/bin/bash
# GPU-box session: parity tests, bench, rocprofv3 kernel stats. Each GPU step has its own limit;
# steps are chained so that the first failure ends the session.
set -o pipefail
cd "$GRAFT_REPO_ROOT"
O=${OUT_DIR:-bench_out}
mkdir -p $O
export TMPDIR=/tmp
step() { echo "== $1"; }
step pytest
timeout -k 10 600 python -m pytest tests -q -m gpu -x -p no:cacheprovider > $O/pytest_gpu.log 2>&1; rc=$?
tail -5 $O/pytest_gpu.log
[ $rc -eq 0 ] || { echo "pytest rc=$rc"; exit $rc; }
step bench
timeout -k 10 600 python bench.py --full > $O/bench.json 2> $O/bench.err || { echo "bench failed"; tail -20 $O/bench.err; exit 1; }
cat $O/bench.json
step rocprof
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $O/prof -o run --output-format csv -- python3 bench.py --steps 2 --warmup 1 --no-cpu > $O/prof.log 2>&1 || { echo "rocprof failed"; tail -20 $O/prof.log; exit 1; }
find $O/prof -name "*stats*" | head
