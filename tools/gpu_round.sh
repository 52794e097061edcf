#!/bin/bash
# Development GPU round: parity probe, overlapped trace + timeline, bench.
# usage: bash tools/gpu_round.sh TAG [extra-env]   (writes under $GAPLAC_OUT, default bench_out)
TAG=${1:-dev}
OUT=${GAPLAC_OUT:-bench_out}
export TMPDIR=/tmp
mkdir -p $OUT
timeout -k 10 200 python tools/quick_gpu_check.py > $OUT/quick_$TAG.log 2>&1 || { cat $OUT/quick_$TAG.log; exit 1; }
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof_$TAG -o run --output-format csv -- python bench.py --steps 3 --warmup 1 > $OUT/prof_$TAG.log 2>&1 || { tail $OUT/prof_$TAG.log; exit 2; }
timeout -k 10 300 python bench.py --full --steps 10 --warmup 2 --skip-cpu --no-extra > $OUT/bench_$TAG.json 2>&1 || { tail $OUT/bench_$TAG.json; exit 3; }
tail -3 $OUT/quick_$TAG.log; grep -h metric $OUT/bench_$TAG.json | cut -c 150-260
python tools/kstats.py $OUT/prof_$TAG
python tools/timeline.py $OUT/prof_$TAG 10 20
