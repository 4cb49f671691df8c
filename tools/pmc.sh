#!/bin/bash
# HBM traffic of the bench's kernels from rocprofv3 PMC counters, one counter per pass
# (MI355X_MICROARCH.md: FETCH_SIZE and WRITE_SIZE cannot share a pass; no trace domains here).
cd /tmp && export TMPDIR=/tmp
cd "$GRAFT_REPO_ROOT"
OUT=${OUT:-bench_out}  # where the counter files and logs go
mkdir -p $OUT
for c in FETCH_SIZE WRITE_SIZE; do
  rm -rf $OUT/pmc_$c
  timeout -k 10 900 rocprofv3 --pmc $c -d $OUT/pmc_$c -o pmc --output-format csv -- \
    python3 bench.py --steps 3 --warmup 3 --full --no-cpu-baseline > $OUT/pmc_$c.log 2>&1
  rc=$?
  echo "pmc $c rc=$rc"
  [ $rc -ne 0 ] && { tail -20 $OUT/pmc_$c.log; exit $rc; }
done
find $OUT/pmc_* -name "*counter_collection*"
