#!/bin/bash
# One GPU-box session: parity tests, smoke, a short full bench.  Logs go to
# $BENCH_OUT (default: bench_out/ in the repository).
# Every GPU step has its own time limit; the chain stops at the first failure.
set -o pipefail
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
BENCH_OUT=${BENCH_OUT:-bench_out}
mkdir -p "$BENCH_OUT"
export TMPDIR=/tmp
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v -p no:cacheprovider --timeout 300 --timeout-method thread > "$BENCH_OUT/pytest_gpu.log" 2>&1 \
  && echo "pytest gpu ok" \
  && timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$BENCH_OUT/smoke.log" 2>&1 \
  && echo "smoke ok" \
  && timeout -k 10 600 python bench.py --full --steps 10 --warmup 3 > "$BENCH_OUT/bench.json" 2> "$BENCH_OUT/bench.err" \
  && echo "bench ok" && cat "$BENCH_OUT/bench.json"
