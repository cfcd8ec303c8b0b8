# quick GPU iteration: parity tests, then one bench line per configuration (profiles/gpu_round.sh adds the rocprof passes)
set -e
OUT=${OUT:-bench_out}
mkdir -p $OUT
timeout -k 10 500 python -u -m pytest tests -m gpu -x -v --timeout 240 --timeout-method thread > $OUT/tq.log 2>&1
timeout -k 10 300 python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline > $OUT/bq.log 2>&1
timeout -k 10 300 python bench.py --full --pixbw --steps 10 --warmup 3 --no-cpu-baseline > $OUT/bqp.log 2>&1
