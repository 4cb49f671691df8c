#!/bin/bash
# bench.py A/B of the working tree vs an older tree unpacked into $AB_TREE (git archive <commit>,
# engine built in place), alternating ${AB_REPS:-3} times on one box; $OUT/ab_tree.jsonl.
OUT=${OUT:-bench_out}  # where the logs and records go
mkdir -p $OUT
: > $OUT/ab_tree.jsonl
ROOT=$(pwd)
for i in $(seq ${AB_REPS:-3}); do
  for arm in head old; do
    d=$ROOT; [ $arm = old ] && d=$ROOT/$AB_TREE
    (cd "$d" && timeout -k 10 240 python bench.py --steps ${AB_STEPS:-40} --warmup 5 --full --no-cpu-baseline) > $OUT/ab_run.log 2>&1 || { tail -20 $OUT/ab_run.log; exit 1; }
    tail -1 $OUT/ab_run.log | python -c "import json,sys; d=json.loads(sys.stdin.read()); print(json.dumps({'tree': '$arm', 'value': d['value'], 'ms_per_step': d['ms_per_step'], 'phases': d['phases']}))" | tee -a $OUT/ab_tree.jsonl
  done
done
