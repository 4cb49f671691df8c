#!/bin/bash
# policy-forward kernels on one box: numerics of the default (split-f16, 8 waves) kernel and of
# the 4-wave variant, the microbenchmark of every variant, then bench.py with the default.
OUT=${OUT:-bench_out}  # where the logs and records go
mkdir -p $OUT
timeout -k 10 300 python -u -m pytest tests/test_gpu_policy_mlp.py -x -q --timeout 200 --timeout-method thread -k "fused_policy" > $OUT/pm.log 2>&1 || { echo "pytest failed"; tail -40 $OUT/pm.log; exit 1; }
tail -1 $OUT/pm.log
MH_POLICY_WAVES=4 timeout -k 10 300 python -u -m pytest tests/test_gpu_policy_mlp.py -x -q --timeout 200 --timeout-method thread -k "fused_policy" > $OUT/pm4.log 2>&1 || { echo "pytest (4 waves) failed"; tail -40 $OUT/pm4.log; exit 1; }
tail -1 $OUT/pm4.log
for k in "x3 8" "x3 4" "x6 4" "f32 4"; do
  set -- $k
  MH_POLICY_KERNEL=$1 MH_POLICY_WAVES=$2 timeout -k 10 120 python tools/policy_bench.py 65536 50 | sed "s/^/waves=$2 /" || exit 1
done
timeout -k 10 200 python bench.py --steps 20 --warmup 5 --full --no-cpu-baseline > $OUT/b_x3.log 2>&1 || exit 1
tail -1 $OUT/b_x3.log | python -c "import json,sys; d=json.loads(sys.stdin.read()); print(d['value'], d['ms_per_step'], d['kernels']['policy_forward'], d['phases'])"
