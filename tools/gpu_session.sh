#!/bin/bash
# GPU-box session: bench (all precisions + the default line with the CPU baseline), parity tests,
# density bench, rocprofv3 kernel stats of the default bench, HBM PMC passes (default precision),
# training bench + its kernel stats.  Each GPU step has its own limit; a crash/timeout ends the
# session (test failures, rc 1, do not).
#   TAG=r01_v6 bash tools/gpu_session.sh
set -o pipefail
cd "$GRAFT_REPO_ROOT"
O=${OUT_DIR:-bench_out}
mkdir -p $O
export TMPDIR=/tmp
TAG=${TAG:-run}
for p in ${PRECS:-bf16x6 fp32 bf16x3}; do
  echo "== bench $p"
  timeout -k 10 300 python bench.py --full --no-cpu --also "" --precision $p > $O/${TAG}_bench_$p.json 2> $O/bench_$p.err || { tail -20 $O/bench_$p.err; exit 1; }
  cat $O/${TAG}_bench_$p.json
done
echo "== pytest"
timeout -k 10 900 python -u -m pytest tests -q -m gpu -p no:cacheprovider --timeout 120 --timeout-method thread \
    > $O/pytest_gpu.log 2>&1; rc=$?
grep -E "passed|failed|FAILED|Error" $O/pytest_gpu.log | tail -15
[ $rc -eq 0 ] || [ $rc -eq 1 ] || { echo "pytest rc=$rc"; exit $rc; }
[ -n "$QUICK" ] && exit $rc
echo "== bench (default, with CPU baseline)"
timeout -k 10 300 python bench.py --full > $O/${TAG}_bench.json 2> $O/bench.err || { tail -20 $O/bench.err; exit 1; }
cat $O/${TAG}_bench.json
for p in fp32 bf16x6; do
  echo "== density $p"
  timeout -k 10 300 python tools/density_bench.py 255 $p > $O/${TAG}_density_$p.json 2> $O/density.err || { tail -20 $O/density.err; exit 1; }
  cat $O/${TAG}_density_$p.json
done
echo "== rocprof"
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/prof_${TAG} -o run --output-format csv -- python3 bench.py --steps 4 --warmup 1 --no-cpu --also "" > $O/prof.log 2>&1 || { echo "rocprof failed"; tail -20 $O/prof.log; exit 1; }
find $O/prof_${TAG} -name "*stats*"
echo "== pmc"
for p in ${PMC_PRECS:-bf16x6}; do
  PREC=$p bash tools/gpu_pmc.sh || exit 1
done
echo "== configs 2 and 4"
timeout -k 10 300 python bench.py --full --no-cpu --also "" --joints 65 > $O/${TAG}_bench_cfg4_joints65.json 2> $O/cfg.err || { tail -20 $O/cfg.err; exit 1; }
timeout -k 10 300 python bench.py --full --no-cpu --also "" --res 256 --importance 0 > $O/${TAG}_bench_cfg2_res256.json 2> $O/cfg.err || { tail -20 $O/cfg.err; exit 1; }
cat $O/${TAG}_bench_cfg4_joints65.json $O/${TAG}_bench_cfg2_res256.json
echo "== dataset ray sampler"
timeout -k 10 200 python tools/dataset_bench.py > $O/${TAG}_dataset_bench.json 2> $O/ds.err || { tail -20 $O/ds.err; exit 1; }
cat $O/${TAG}_dataset_bench.json
timeout -k 10 200 rocprofv3 --kernel-trace --stats -d $O/prof_ds_${TAG} -o run --output-format csv -- python3 tools/dataset_bench.py > $O/prof_ds.log 2>&1 || { echo "rocprof dataset failed"; tail -20 $O/prof_ds.log; exit 1; }
echo "== train"
timeout -k 10 300 python tools/train_bench.py > $O/${TAG}_train_bench.json 2> $O/train.err || { tail -20 $O/train.err; exit 1; }
cat $O/${TAG}_train_bench.json
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/prof_train_${TAG} -o run --output-format csv -- python3 tools/train_bench.py --steps 5 --warmup 1 > $O/prof_train.log 2>&1 || { echo "rocprof train failed"; tail -20 $O/prof_train.log; exit 1; }
exit $rc
