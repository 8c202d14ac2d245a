#!/bin/bash
# Steady-state kernel trace of `bench.py --model $1` (bf16, 4K, 8 frames).  usage: tools/qt_model.sh MODEL
cd "$(dirname "$0")/.." && export OUT=${OUT:-out} && mkdir -p $OUT        # outputs go under $OUT/ (default: out/)
M=${1:-LiteISPNet}
export TMPDIR=/tmp
timeout 600 rocprofv3 --kernel-trace --stats -d $OUT/qt_$M -o trace -- python bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --model $M > $OUT/qt_$M.json 2> $OUT/qt_$M.err
python tools/rocpd_summary.py $OUT/qt_$M/trace_results.db --last-forwards 4 > $OUT/qt_$M.md
rm -rf $OUT/qt_$M
cut -c1-200 $OUT/qt_$M.json; head -22 $OUT/qt_$M.md | cut -c1-150
