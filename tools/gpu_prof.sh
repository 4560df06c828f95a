#!/bin/bash
# Profile session of a round (ROUND=r05_a ...): bench line, rocprofv3 kernel-trace stats (grouped default and --chunks 1) of `bench.py --timed-only`
# (warmup + the timed region of the driver's run: --steps 20 --warmup 5, nothing else), PMC passes over the same window (--chunks 1), the other configurations.
cd "$(dirname "$0")/.."; ROOT=$PWD
OUT=${OUT:-bench_out}; mkdir -p "$OUT/${ROUND:-r05}"; OUT=$(cd "$OUT" && pwd); export OUT; R=$OUT/${ROUND:-r05}
export TMPDIR=/tmp
echo "=== bench"; timeout 900 python bench.py --full 2>&1 | tail -1 > $R/bench_line.json; cut -c1-300 $R/bench_line.json
for mode in grouped chunks1; do
  extra=""; [ $mode = chunks1 ] && extra="--chunks 1"
  (cd /tmp && timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $R/prof_$mode -- python $ROOT/bench.py --steps 20 --warmup 5 --timed-only $extra > $R/prof_$mode.log 2>&1)
  f=$(find $R/prof_$mode -name "*kernel_stats*.csv" | head -1); cp $f $R/kernel_stats_$mode.csv; echo "== $mode"; head -6 $f | cut -c1-200
  t=$(find $R/prof_$mode -name "*kernel_trace.csv" | head -1)
  python3 - "$t" <<'PY'
import csv, sys, collections
rows = list(csv.DictReader(open(sys.argv[1])))
acc = collections.defaultdict(list); res = {}
for r in rows:
    n = r['Kernel_Name']
    k = next((x for x in ('dojo_stepc_kernel', 'dojo_stepp_kernel', 'dojo_gradp_kernel', 'dojo_step_kernel', 'dojo_grad_kernel') if x in n), None)
    if k: acc[k].append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) * 1e-6); res[k] = (r.get('LDS_Block_Size', '?'), r.get('Scratch_Size', '?'), r.get('VGPR_Count', '?'), r.get('Accum_VGPR_Count', '?'), r.get('Grid_Size', '?'))
for k, v in acc.items(): print("   %-18s n=%4d mean %.3f ms min %.3f max %.3f | LDS %s scratch %s VGPR %s AGPR %s grid %s" % ((k, len(v), sum(v) / len(v), min(v), max(v)) + res[k]))
PY
  rm -rf $R/prof_$mode
done
echo "=== pmc"; bash tools/gpu_pmc.sh > $R/pmc.log 2>&1; cp $OUT/pmc/pmc_summary.txt $OUT/pmc/pmc_traffic.json $R/; tail -3 $R/pmc.log | cut -c1-400
rm -rf $OUT/pmc/SQ_* $OUT/pmc/FETCH* $OUT/pmc/WRITE*
echo "=== configs"; bash tools/gpu_configs_bench.sh 2>&1 | tee $R/configs.txt
