#!/bin/bash
# fp16x3 bring-up: its parity tests, then the bench in fp16x3 (and the other modes beside it).
set -o pipefail
cd "$GRAFT_REPO_ROOT"
O=${OUT_DIR:-bench_out}
mkdir -p $O
export TMPDIR=/tmp
TAG=${TAG:-h3}
timeout -k 10 600 python -u -m pytest tests -q -m gpu -p no:cacheprovider --timeout 300 --timeout-method thread \
    -k "${K:-fp16x3 or split}" > $O/${TAG}_pytest.log 2>&1; rc=$?
grep -E "passed|failed|FAILED|Error|assert" $O/${TAG}_pytest.log | tail -25
[ $rc -eq 0 ] || [ $rc -eq 1 ] || { echo "pytest rc=$rc"; exit $rc; }
timeout -k 10 400 python bench.py --full --precision ${PREC:-fp16x3} --no-cpu --no-tau20 > $O/${TAG}_bench.json 2> $O/${TAG}_bench.err || { tail -20 $O/${TAG}_bench.err; exit 1; }
cat $O/${TAG}_bench.json
exit $rc
