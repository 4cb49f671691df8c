OUT=${OUT:-bench_out}  # where the logs and records go
mkdir -p $OUT
timeout -k 10 400 python -u -m pytest tests/test_gpu_trainer.py -x -v --timeout 300 --timeout-method thread -k "overlapped or train_loop" > $OUT/ov_tests.log 2>&1 || { tail -30 $OUT/ov_tests.log; exit 1; }
tail -3 $OUT/ov_tests.log
for m in "--overlap" "" "--overlap" ""; do
  timeout -k 10 200 python bench.py --steps 30 --warmup 5 --full --no-cpu-baseline $m > $OUT/b_ov.log 2>&1 || exit 1
  tail -1 $OUT/b_ov.log | python -c "import json,sys; d=json.loads(sys.stdin.read()); print('$m', d['value'], d['ms_per_step'], d['phases'])"
done
