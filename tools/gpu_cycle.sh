#!/bin/bash
# One GPU iteration: parity tests, bench (no CPU baseline), kernel-trace profile.  usage: tools/gpu_cycle.sh TAG [pytest-args]
cd "$(dirname "$0")/.." && export OUT=${OUT:-out}        # outputs go under $OUT/ (default: out/)
TAG=${1:-x}; shift
mkdir -p $OUT
timeout 600 python -m pytest tests -m gpu -q -x --timeout 300 "$@" 2>&1 | tail -15 > $OUT/pytest_$TAG.log
tail -4 $OUT/pytest_$TAG.log
export TMPDIR=/tmp
timeout 600 rocprofv3 --kernel-trace --stats -d $OUT/prof_$TAG -o trace -- python bench.py --full --steps 3 --warmup 1 --no-cpu-baseline > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err
tail -2 $OUT/bench_$TAG.err
python -c "
import json;d=json.load(open('$OUT/bench_$TAG.json'));print(d['value'],d['unit'],d['ms_per_step'],'ms/step', d['roofline']['achieved'],'TF/s conv', d['roofline']['kernel_ms_per_step'])"
