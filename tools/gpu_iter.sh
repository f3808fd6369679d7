#!/bin/bash
# One GPU iteration: parity tests, bench line, rocprofv3 kernel trace (run on the GPU box).
# usage: tools/gpu_iter.sh TAG [extra bench args]     (outputs under $OUT, default bench_out)
set -o pipefail
TAG=$1; shift
export TMPDIR=/tmp
OUT=${OUT:-bench_out}
mkdir -p $OUT
timeout -k 10 400 python -m pytest tests/test_gpu_parity.py -q -m gpu -x > $OUT/gpu_$TAG.log 2>&1 || { tail -30 $OUT/gpu_$TAG.log; exit 1; }
tail -2 $OUT/gpu_$TAG.log
timeout -k 10 300 python bench.py --full --no-cpu-baseline "$@" > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err || { cat $OUT/bench_$TAG.err; exit 1; }
cat $OUT/bench_$TAG.json
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof_$TAG -o run --output-format csv -- python3 bench.py --steps 2 --full --no-cpu-baseline --no-counters "$@" > $OUT/prof_$TAG.log 2>&1 || exit 1
python3 tools/trace_summary.py trace $OUT/prof_$TAG/run_kernel_trace.csv
