#!/bin/bash
# Kernel traces of the data-parallel kernel path (bench.py --dp-path) for this build and the
# round's starting build (tools/ablate/base), summarised per step (tools/prof_summary.py).
set -u
cd "$GRAFT_REPO_ROOT"
RESULTS=${RESULTS:-bench_out}; mkdir -p "$RESULTS"
export TMPDIR=/tmp
for v in new base; do
  d=$GRAFT_REPO_ROOT; [ $v = base ] && d=$GRAFT_REPO_ROOT/tools/ablate/base
  rm -rf $RESULTS/dptr_$v
  (cd $d && timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d "$PWD/$RESULTS/dptr_$v" -o run -- python3 bench.py --full --dp-path --cpu-sample 0 --steps 10 --warmup 3) > $RESULTS/dptr_$v.log 2>&1 || exit $?
  f=$(find $RESULTS/dptr_$v -name "*kernel_trace.csv" | head -1)
  python3 tools/prof_summary.py "$f" 10 > $RESULTS/dptr_${v}_steps.txt
  echo "$v $(grep -m1 'busy us/step' $RESULTS/dptr_${v}_steps.txt)"
done
