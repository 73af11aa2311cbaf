OUT=${OUT:-out}   # output folder
mkdir -p $OUT/r2full
timeout 1500 python -m pytest tests -m gpu -q -x > $OUT/r2full/pytest.log 2>&1; echo "rc=$?" >> $OUT/r2full/pytest.log
tail -15 $OUT/r2full/pytest.log
timeout 600 python bench.py --full > $OUT/r2full/bench.json 2> $OUT/r2full/bench.err; cat $OUT/r2full/bench.json
python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -2
