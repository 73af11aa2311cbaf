set -x
R=$PWD
OUT=${OUT:-$R/out}   # output folder
mkdir -p $OUT/q
timeout 900 python -m pytest tests -m gpu -x -q > $OUT/q/pytest.log 2>&1; echo "pytest rc=$?" >> $OUT/q/pytest.log
tail -5 $OUT/q/pytest.log
timeout 600 python bench.py --full > $OUT/q/bench.json 2> $OUT/q/bench.err; cat $OUT/q/bench.json
cd /tmp && export TMPDIR=/tmp
timeout 600 rocprofv3 --kernel-trace --stats -d $OUT/q/stats -- python $R/bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > $OUT/q/stats.log 2>&1
python $R/profiles/summarize_rocpd.py $(find $OUT/q/stats -name '*.db' | head -1) > $OUT/q/kernel_stats.txt
timeout 600 rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $OUT/q/fetch -- python $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > $OUT/q/fetch.log 2>&1
python $R/profiles/summarize_pmc.py $(find $OUT/q/fetch -name '*.db' | head -1) > $OUT/q/pmc_fetch.txt
timeout 600 rocprofv3 --kernel-trace --pmc WRITE_SIZE -d $OUT/q/write -- python $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > $OUT/q/write.log 2>&1
python $R/profiles/summarize_pmc.py $(find $OUT/q/write -name '*.db' | head -1) > $OUT/q/pmc_write.txt
rm -rf $OUT/q/stats $OUT/q/fetch $OUT/q/write
head -12 $OUT/q/kernel_stats.txt
