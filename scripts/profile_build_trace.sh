#!/bin/bash
# Kernel trace of the headline ingest (the config-3 shape) for one library
# build: rocprofv3 kernel trace only, no counters, no sys/runtime trace.
# Usage: scripts/profile_build_trace.sh LABEL [LIBRARY]
#   LABEL    names the output, $BENCH_OUT/ktrace_LABEL/ (default bench_out/)
#   LIBRARY  a variant libmahout_cms.so (mahout_amd/build_lib.py --define ...
#            --out ...), loaded through MAHOUT_CMS_LIB; default: the tree's.
# A CMS_BUILD_SERIAL variant runs the build's class kernels one after another,
# so their durations are isolated ones; with CMS_BUILD_NO_STREAMED as well,
# k_build_mid runs once per mid list (streamed, then cached).
# Summary: scripts/summarize_build_trace.py bench_out/ktrace_LABEL
set -o pipefail
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
LABEL=${1:?label}
[ -n "$2" ] && export MAHOUT_CMS_LIB=$2
OUT=${BENCH_OUT:-bench_out}/ktrace_$LABEL
rm -rf "$OUT"
mkdir -p "$OUT"
CMD="python3 bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-extras --no-config1 --no-config2 --no-cosine-1m"
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d "$OUT/trace" -o run --output-format csv -- $CMD \
    > "$OUT/trace.log" 2>&1 || { echo "trace failed"; exit 1; }
echo "trace ok"
