#!/bin/bash
# HBM traffic of the bench command from PMC counters: one rocprofv3 pass per counter (FETCH_SIZE and WRITE_SIZE do not
# fit one pass; --pmc is never combined with other trace domains).  usage: tools/pmc_bench.sh TAG
cd "$(dirname "$0")/.." && export OUT=${OUT:-out}        # outputs go under $OUT/ (default: out/)
TAG=${1:-x}
mkdir -p $OUT
export TMPDIR=/tmp
for C in FETCH_SIZE WRITE_SIZE; do
  timeout 900 rocprofv3 --pmc $C --kernel-trace -d $OUT/pmc_${TAG}_$C -o pmc -- python bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-codec-leg > $OUT/pmc_${TAG}_$C.json 2> $OUT/pmc_${TAG}_$C.err
  tail -1 $OUT/pmc_${TAG}_$C.err
done
python tools/pmc_bench_summary.py $OUT/pmc_${TAG}_FETCH_SIZE/pmc_results.db $OUT/pmc_${TAG}_WRITE_SIZE/pmc_results.db > $OUT/pmc_${TAG}.json
cat $OUT/pmc_${TAG}.json | head -c 1500
