#!/bin/bash
# Round profile capture: kernel-trace stats of the benchmark command (default mode and the
# gradient mode), two PMC passes per dominant kernel (FETCH_SIZE, WRITE_SIZE; counters never
# combined with tracing domains), then the full default bench (--full).
# usage: bash tools/profile_round.sh rNN   (writes under $GAPLAC_OUT/rNN, default bench_out/rNN)
R=${1:-r01}
OUT=${GAPLAC_OUT:-bench_out}/$R
export TMPDIR=/tmp
mkdir -p $OUT
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/trace -o run --output-format csv -- python bench.py --full --steps 5 --warmup 1 --skip-cpu --no-extra > $OUT/trace.log 2>&1 || exit 1
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/trace_grad -o run --output-format csv -- python bench.py --mode grad --steps 3 --warmup 1 --skip-cpu --no-extra > $OUT/trace_grad.log 2>&1 || exit 2
timeout -s KILL 120 rocprofv3 --pmc FETCH_SIZE -d $OUT/pmc_fetch -o run --output-format csv -- python bench.py --steps 2 --warmup 1 > $OUT/pmc_fetch.log 2>&1 || exit 3
timeout -s KILL 120 rocprofv3 --pmc WRITE_SIZE -d $OUT/pmc_write -o run --output-format csv -- python bench.py --steps 2 --warmup 1 > $OUT/pmc_write.log 2>&1 || exit 4
python tools/pmc_traffic.py $OUT/pmc_fetch $OUT/pmc_write $OUT/traffic_syrk.json || exit 5
python tools/pmc_traffic.py $OUT/pmc_fetch $OUT/pmc_write $OUT/traffic_gram.json gram_queue_kernel || exit 5
timeout -s KILL 120 rocprofv3 --pmc FETCH_SIZE -d $OUT/pmc_fetch_g -o run --output-format csv -- python bench.py --mode grad --steps 1 --warmup 1 --skip-cpu --no-extra --no-profile > $OUT/pmc_fetch_g.log 2>&1 || exit 6
timeout -s KILL 120 rocprofv3 --pmc WRITE_SIZE -d $OUT/pmc_write_g -o run --output-format csv -- python bench.py --mode grad --steps 1 --warmup 1 --skip-cpu --no-extra --no-profile > $OUT/pmc_write_g.log 2>&1 || exit 7
python tools/pmc_traffic.py $OUT/pmc_fetch_g $OUT/pmc_write_g $OUT/traffic_cinv.json cinv_contract_kernel || exit 8
timeout -k 10 400 python bench.py --full > $OUT/bench.json 2> $OUT/bench.err || exit 9
cat $OUT/bench.json
