#!/bin/bash
# One GPU-box pass: parity tests, default bench line, rocprof kernel stats of the same command.
set -u
OUT=$(realpath -m "${OUT:-out}"); export OUT      # results directory (default: out/)
mkdir -p $OUT
timeout 1500 python -m pytest tests -m gpu -x -q > $OUT/pytest_gpu.log 2>&1; echo "pytest rc=$?"
tail -3 $OUT/pytest_gpu.log
timeout 600 python bench.py --full > $OUT/bench_n1.json 2> $OUT/bench_n1.err; echo "bench rc=$?"
cat $OUT/bench_n1.json
export TMPDIR=/tmp
R=$PWD
cd $TMPDIR && timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -o bench -- python3 $R/bench.py --full > $OUT/bench_prof.json 2> $OUT/bench_prof.err; echo "rocprof rc=$?"
cd $R
find $OUT/prof -name '*kernel_stats.csv' | head
f=$(find $OUT/prof -name '*kernel_stats.csv' | head -1)
[ -n "$f" ] && head -12 "$f" | cut -c1-160
find $OUT/prof -name '*kernel_trace.csv' -delete
find $OUT/prof -name '*.db' -delete
cat $OUT/bench_prof.json | cut -c1-600
