#!/bin/bash
# Kernel trace of the default bench command, summarised per kernel.   usage: tools/quick_trace.sh TAG [bench args...]
cd "$(dirname "$0")/.." && export OUT=${OUT:-out}        # outputs go under $OUT/ (default: out/)
TAG=${1:-q}; shift
mkdir -p $OUT
export TMPDIR=/tmp
timeout 600 rocprofv3 --kernel-trace --stats -d $OUT/qt_$TAG -o trace -- python bench.py --full --steps 3 --warmup 1 --no-cpu-baseline "$@" > $OUT/qt_$TAG.json 2> $OUT/qt_$TAG.err
cut -c1-200 $OUT/qt_$TAG.json
python tools/rocpd_summary.py $OUT/qt_$TAG/trace_results.db > $OUT/qt_$TAG.md
head -45 $OUT/qt_$TAG.md | cut -c1-150
