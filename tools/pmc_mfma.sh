#!/bin/bash
# Matrix-pipe and LDS counters of the bench command, one rocprofv3 --pmc pass per counter group (never combined with other trace domains).
# usage: tools/pmc_mfma.sh TAG   -> $OUT/pmc_mfma_TAG.md
cd "$(dirname "$0")/.." && export OUT=${OUT:-out}        # outputs go under $OUT/ (default: out/)
TAG=${1:-x}
mkdir -p $OUT
export TMPDIR=/tmp
for C in SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CU_CYCLES SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE; do
  timeout 900 rocprofv3 --pmc $C --kernel-trace -d $OUT/pmcm_${TAG}_$C -o pmc -- python bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-codec-leg > /dev/null 2> $OUT/pmcm_${TAG}_$C.err
  tail -1 $OUT/pmcm_${TAG}_$C.err
done
python tools/pmc_mfma_summary.py $TAG > $OUT/pmc_mfma_$TAG.md
head -30 $OUT/pmc_mfma_$TAG.md
