#!/bin/bash
# On the GPU: the round's closing numbers -- bench.py as the driver runs it (3 times) and with --full, then the BASELINE stand-ins.
# usage: tools/final_bench.sh [LOG_DIR]   (default bench_logs/)
OUT=${1:-bench_logs}; mkdir -p $OUT
for i in 1 2 3; do timeout -k 10 400 python bench.py --steps 20 --warmup 5 > $OUT/bench_drv$i.log 2> $OUT/bench_drv$i.err; echo "drv$i rc=$?"; done
timeout -k 10 400 python bench.py --full > $OUT/bench_full.log 2> $OUT/bench_full.err; echo "full rc=$?"
( timeout -k 10 400 python tools/run_configs.py C2 --cycles 100; timeout -k 10 400 python tools/run_configs.py C3 --cycles 60; timeout -k 10 300 python tools/run_configs.py C4 --cycles 4; timeout -k 10 300 python tools/run_configs.py C4 --cycles 2 --arithmetic exact ) 2>&1 | grep "us/step" > $OUT/soak_final.log
cut -c1-200 $OUT/soak_final.log
