#!/bin/bash
# GPU tests + bench + density bench + stamps diagnostic (no rocprof)
set -o pipefail
cd "$GRAFT_REPO_ROOT"
O=${OUT_DIR:-bench_out}
mkdir -p $O
timeout -k 10 600 python -m pytest tests -q -m gpu -x -p no:cacheprovider > $O/pytest_gpu.log 2>&1; rc=$?
tail -3 $O/pytest_gpu.log
[ $rc -eq 0 ] || exit $rc
timeout -k 10 600 python bench.py --full --no-cpu > $O/bench.json 2> $O/bench.err || { tail -20 $O/bench.err; exit 1; }
cat $O/bench.json
timeout -k 10 300 python tools/density_bench.py > $O/density.json 2> $O/density.err || { tail -20 $O/density.err; exit 1; }
cat $O/density.json
timeout -k 10 300 python tools/stamps.py 79.6 > $O/stamps.txt 2>&1 || { tail $O/stamps.txt; exit 1; }
cat $O/stamps.txt
