#!/bin/bash
# end-of-round checks on an MI355X machine: GPU suite, smoke, two full bench lines (kept under $OUT, default out/, copied to profiles/ by hand)
TAG=${1:-r5h}
OUT=${OUT:-out}; mkdir -p $OUT
python -m pytest tests -m gpu -x -q 2>&1 | tail -4 | tee $OUT/gpu_tests_$TAG.txt
python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -1 | tee -a $OUT/gpu_tests_$TAG.txt
for i in 1 2; do python bench.py --full --steps 20 > $OUT/bench_${TAG}_$i.json 2> /dev/null; python tools/bench_show.py $OUT/bench_${TAG}_$i.json | head -3; done
