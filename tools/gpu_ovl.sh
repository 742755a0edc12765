# Overlap policy A/B on the default bench (autotuned): side stream default / high / low priority, no overlap.
set -u
cd "$(dirname "$0")/.."; RESULTS=${RESULTS:-bench_out}; mkdir -p "$RESULTS"
show() { python3 -c "import json,sys; d=json.loads([l for l in open(sys.argv[1]) if l.startswith('{')][-1]); r=d['roofline']; print(sys.argv[2], d['value'], d['ms_per_step'], r['avg_launch_us'], r['frac'], r['isolated']['avg_launch_us'], r['plan'])" $1 "$2"; }
for V in ${OVL_VARIANTS:-"def::" "noov::--no-overlap"}; do
  name=${V%%:*}; rest=${V#*:}; envs=${rest%%:*}; args=${rest#*:}
  env $envs timeout -k 10 300 python3 bench.py --full --cpu-sample 0 $args > $RESULTS/ovl_$name.log 2>&1
  rc=$?; [ $rc -eq 0 ] || { echo "$name rc=$rc"; tail -5 $RESULTS/ovl_$name.log; exit $rc; }
  show $RESULTS/ovl_$name.log $name
done
