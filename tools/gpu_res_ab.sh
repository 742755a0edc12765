#!/bin/bash
# The packed residual pass: the probe's isolated timings, then ResNet-18 kernel stats with the
# packed pass off / on (same plans; per-kernel averages from rocprofv3 --stats).
set -u
cd "$GRAFT_REPO_ROOT"
RESULTS=${RESULTS:-bench_out}; mkdir -p "$RESULTS"
export TMPDIR=/tmp
timeout -k 5 60 tools/probes/exit_probe > $RESULTS/exit_probe2.txt 2>&1 || exit $?
cat $RESULTS/exit_probe2.txt
for pk in 0 1; do
  rm -rf $RESULTS/res_pk$pk
  NITI_RES_PK=$pk timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$PWD/$RESULTS/res_pk$pk" -o run -- python3 bench.py --full --arch resnet18 --cpu-sample 0 --steps 10 --warmup 3 --load-plans tools/probes/plans_resnet18_r06.json > $RESULTS/res_pk$pk.log 2>&1 || exit $?
  echo "pk $pk $(grep -o '"ms_per_step": [0-9.]*' $RESULTS/res_pk$pk.log)"
  f=$(find $RESULTS/res_pk$pk -name '*kernel_stats.csv' | head -1)
  grep -i "residual_requant" "$f"
done
