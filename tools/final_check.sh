#!/bin/bash
# Final state check: full -m gpu suite, smoke, the full bench (CPU leg included).
# usage: bash tools/final_check.sh rNN   (writes under $GAPLAC_OUT/rNN, default bench_out/rNN)
R=${1:-r02f}
OUT=${GAPLAC_OUT:-bench_out}/$R
export TMPDIR=/tmp
mkdir -p $OUT
timeout -k 10 400 python -u -m pytest tests -m gpu -x -q --timeout 200 --timeout-method thread > $OUT/pytest_gpu.log 2>&1 || { tail -30 $OUT/pytest_gpu.log; exit 1; }
tail -2 $OUT/pytest_gpu.log
timeout -k 10 200 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1 || { tail -20 $OUT/smoke.log; exit 2; }
timeout -k 10 400 python bench.py --full > $OUT/bench.json 2> $OUT/bench.err || { tail $OUT/bench.err; exit 3; }
cut -c1-400 $OUT/bench.json
