#!/bin/bash
# BASELINE config 5's per-GPU workload (VideoSwin-B, 32 frames, B = 32 per GPU, fp8 forward GEMMs) as a workload: bench
# line (fp8 and bf16 on the same box), rocprofv3 kernel stats of the fp8 command, HBM-traffic + MFMA counter passes.
#   CLOVER_COMMIT=<sha> bash tools/gpu_cfg5.sh <tag>     -> $OUT/<tag>_cfg5_*   (copy into profiles/ to commit)
set -u
OUT=$(realpath -m "${OUT:-out}"); export OUT      # results directory (default: out/)
TAG=${1:-r04}
export CLOVER_COMMIT=${CLOVER_COMMIT:-unknown}
ARGS="--full --variant B --frames 32 --batch ${CFG5_BATCH:-32}"
mkdir -p $OUT
for dt in fp8 bf16; do
  timeout 900 python bench.py $ARGS --dtype $dt --steps 8 --warmup 3 --no-cpu-baseline > $OUT/${TAG}_cfg5_bench_$dt.json 2> $OUT/${TAG}_cfg5_bench_$dt.err; echo "bench $dt rc=$?"
  tail -1 $OUT/${TAG}_cfg5_bench_$dt.json | cut -c1-300
done
export TMPDIR=/tmp
R=$PWD
rm -rf $OUT/prof5; mkdir -p $OUT/prof5
(cd $TMPDIR && timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof5 -o bench -- python3 $R/bench.py $ARGS --dtype fp8 --steps 4 --warmup 2 --no-cpu-baseline --no-kernel-timing > $OUT/${TAG}_cfg5_prof.json 2> $OUT/${TAG}_cfg5_prof.err); echo "rocprof rc=$?"
f=$(find $OUT/prof5 -name '*kernel_stats.csv' | head -1)
[ -n "$f" ] && cp "$f" $OUT/${TAG}_cfg5_kernel_stats_fp8.csv && head -12 "$f" | cut -c1-150
echo "{\"commit\": \"$CLOVER_COMMIT\", \"command\": \"rocprofv3 --kernel-trace --stats -- python3 bench.py $ARGS --dtype fp8 --steps 4 --warmup 2 --no-cpu-baseline --no-kernel-timing\"}" > $OUT/${TAG}_cfg5_kernel_stats_fp8.meta.json
rm -rf $OUT/prof5
export BENCH_ARGS="$ARGS --dtype fp8"
bash tools/pmc_traffic.sh > $OUT/${TAG}_cfg5_pmc_traffic.log 2>&1; cp $OUT/pmc_traffic.json $OUT/${TAG}_cfg5_pmc_traffic.json
bash tools/pmc_mfma.sh > $OUT/${TAG}_cfg5_pmc_mfma.log 2>&1; cp $OUT/pmc_mfma.json $OUT/${TAG}_cfg5_pmc_mfma.json
rm -rf $OUT/pmc_FETCH_SIZE $OUT/pmc_WRITE_SIZE $OUT/pmc_mfma
