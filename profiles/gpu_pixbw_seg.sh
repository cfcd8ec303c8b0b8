# segment-parallel pixel-bandwidth backward (default) vs the per-event serial one (libden_pix0.so):
# parity (pixel-bandwidth tests + the training-step tests), then the configs[3] emulation and the
# configs[2] bench line (--full: with its per-kernel figures)
set -e
OUT=${OUT:-bench_out}
mkdir -p $OUT
timeout -k 10 300 python -u -m pytest tests/test_pixbw_gpu.py tests/test_deblur_gpu.py tests/test_train_gpu.py -q --timeout 120 --timeout-method thread > $OUT/tpix.log 2>&1 || echo PARITY_FAIL >> $OUT/pix.txt
for v in base pix0 base pix0; do
  if [ "$v" = base ]; then lib=deblur-e-nerf_amd/libden.so; else lib=deblur-e-nerf_amd/libden_$v.so; fi
  echo "== $v" >> $OUT/pix.txt
  DEN_LIB=$lib timeout -k 10 200 python profiles/bench_ziggy.py --opt-steps 2 2>/dev/null | grep '^{' >> $OUT/pix.txt
  DEN_LIB=$lib timeout -k 10 200 python bench.py --full --pixbw --steps 10 --warmup 3 2>/dev/null | grep '^{' >> $OUT/pix.txt
done
