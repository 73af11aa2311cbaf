OUT=${OUT:-out}   # output folder
mkdir -p $OUT/nb6
DV_OP_TRACE=1 timeout 300 python bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > /dev/null 2> $OUT/nb6/base.txt
DV_NB6=1 DV_OP_TRACE=1 timeout 300 python bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > /dev/null 2> $OUT/nb6/nb6.txt
python tools/compare_traces.py $OUT/nb6/base.txt $OUT/nb6/nb6.txt > $OUT/nb6/cmp.txt
grep -v "  0.0 %\|+0\.[0-9] %\|-0\.[0-9] %" $OUT/nb6/cmp.txt | head -70
