cd "$(dirname "$0")/.." && export OUT=${OUT:-out} && mkdir -p $OUT        # outputs go under $OUT/ (default: out/)
export TMPDIR=/tmp
timeout 300 rocprofv3 --kernel-trace --stats -d $OUT/prof_codec_q -o trace -- python bench.py --full --model raw_compression_tcm_final --frames 8 --steps 2 --warmup 1 --no-cpu-baseline > $OUT/codec_q.json 2> $OUT/codec_q.err
python tools/rocpd_summary.py $OUT/prof_codec_q/trace_results.db --last-forwards 2 > $OUT/codec_q.md
rm -rf $OUT/prof_codec_q
head -70 $OUT/codec_q.md | cut -c1-160
