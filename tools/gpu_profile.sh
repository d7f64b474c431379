#!/bin/bash
# One GPU-box pass for the round's evidence: default bench line, rocprofv3 kernel stats of the same command, the two
# HBM-traffic counter passes and the MFMA / wait counter pass (each its own run, --kernel-trace only: see tools/pmc_*.sh).
#   CLOVER_COMMIT=<sha> bash tools/gpu_profile.sh <tag>      -> $OUT/<tag>_*  (copy into profiles/ to commit)
set -u
OUT=$(realpath -m "${OUT:-out}"); export OUT      # results directory (default: out/)
TAG=${1:-r03}
export CLOVER_COMMIT=${CLOVER_COMMIT:-unknown}
mkdir -p $OUT
timeout 900 python bench.py --full > $OUT/${TAG}_bench_n1.json 2> $OUT/${TAG}_bench_n1.err; echo "bench rc=$?"
tail -1 $OUT/${TAG}_bench_n1.json | cut -c1-400
export TMPDIR=/tmp
R=$PWD
rm -rf $OUT/prof; mkdir -p $OUT/prof
(cd $TMPDIR && timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -o bench -- python3 $R/bench.py --full --no-cpu-baseline > $OUT/${TAG}_bench_prof.json 2> $OUT/${TAG}_bench_prof.err); echo "rocprof rc=$?"
f=$(find $OUT/prof -name '*kernel_stats.csv' | head -1)
[ -n "$f" ] && cp "$f" $OUT/${TAG}_kernel_stats_bench_default_final.csv && head -8 "$f" | cut -c1-150
echo "{\"commit\": \"$CLOVER_COMMIT\", \"csrc_sha16\": \"$(python3 tools/csrc_hash.py)\", \"command\": \"rocprofv3 --kernel-trace --stats -- python3 bench.py --full --no-cpu-baseline\"}" > $OUT/${TAG}_kernel_stats_bench_default_final.meta.json
find $OUT/prof -name '*kernel_trace.csv' -delete; find $OUT/prof -name '*.db' -delete
bash tools/pmc_traffic.sh > $OUT/${TAG}_pmc_traffic.log 2>&1; cp $OUT/pmc_traffic.json $OUT/${TAG}_pmc_traffic.json
bash tools/pmc_mfma.sh > $OUT/${TAG}_pmc_mfma.log 2>&1; cp $OUT/pmc_mfma.json $OUT/${TAG}_pmc_mfma.json
rm -rf $OUT/pmc_FETCH_SIZE $OUT/pmc_WRITE_SIZE $OUT/pmc_mfma $OUT/prof
python3 - <<PY
import json
t=json.load(open('$OUT/${TAG}_pmc_traffic.json')); m=json.load(open('$OUT/${TAG}_pmc_mfma.json'))
for k in list(m)[:6]:
    print(k, t.get(k), m.get(k))
PY
