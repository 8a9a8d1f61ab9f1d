#!/bin/bash
# Round-4 GPU iteration with the ingest profiles: parity tests (TESTS), smoke,
# the ingest's kernel stats + SQ wave / LDS counters + FETCH / WRITE passes,
# then the full bench.  Each GPU step has its own time limit; a crash, fault or
# time limit ends the script.
set -o pipefail
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
BENCH_OUT=${BENCH_OUT:-bench_out}; mkdir -p "$BENCH_OUT"  # the full bench's line and log
mkdir -p gpurun_out
export TMPDIR=/tmp
TESTS=${TESTS:-tests}
timeout -k 10 900 python -u -m pytest $TESTS -m gpu -v -p no:cacheprovider --timeout 300 --timeout-method thread \
    > gpurun_out/pytest_gpu.log 2>&1
rc=$?
tail -3 gpurun_out/pytest_gpu.log
grep -E "^(FAILED|ERROR)" gpurun_out/pytest_gpu.log | head -20
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then echo "pytest ended with status $rc: stopping"; exit $rc; fi
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > gpurun_out/smoke.log 2>&1 || { echo "smoke failed"; tail -5 gpurun_out/smoke.log; exit 1; }
echo "smoke ok"
bash scripts/profile_r04.sh ingest_sq || exit 1
bash scripts/profile_r04.sh ingest || exit 1
timeout -k 10 700 python bench.py --full --steps 10 --warmup 3 > $BENCH_OUT/bench.json 2> $BENCH_OUT/bench.err \
  || { echo "bench failed"; tail -20 $BENCH_OUT/bench.err; exit 1; }
echo "bench ok"
python -c "import json; print(json.dumps(json.load(open('$BENCH_OUT/bench.json'))['summary']))"
exit $rc
