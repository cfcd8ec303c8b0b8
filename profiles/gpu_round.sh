set -e
OUT=${OUT:-bench_out}
mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 500 python -u -m pytest tests -m gpu -x -v --timeout 240 --timeout-method thread > $OUT/t1.log 2>&1
timeout -k 10 600 python bench.py --full --steps 10 --warmup 3 > $OUT/b1.log 2>&1
timeout -k 10 300 python bench.py --full --pixbw --steps 10 --warmup 3 > $OUT/b1p.log 2>&1
timeout -s KILL 150 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_fetch -o run -- python bench.py --steps 1 --warmup 1 > $OUT/pmc_fetch.log 2>&1
timeout -s KILL 150 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/pmc_write -o run -- python bench.py --steps 1 --warmup 1 > $OUT/pmc_write.log 2>&1
timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -o run -- python bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > $OUT/prof.log 2>&1
