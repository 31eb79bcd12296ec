cd $GRAFT_REPO_ROOT
# the dieted two-wave form against the plain one, in alternation: SCTC_CTC_DIET_MIN_B beyond every batch switches the diet off
# (a -DSCTC_FUSED_NO_DIET build measures the same, but needs the flag for capi_ctc.hip too: csrc/ctc_plan.h)
for rep in 1 2 3; do
for min_b in 1025 1000000; do
  echo -n "SCTC_CTC_DIET_MIN_B=$min_b: "
  SCTC_CTC_DIET_MIN_B=$min_b timeout 300 python tools/ctc_paths_bench.py --shapes sat,sat1k,cfg2 --paths fused --reps 5 2>&1 | grep "^{" | python -c "
import sys, json
print(' | '.join('%s B=%d %.3f ms' % (d['shape'], d['B'], d['gpu_ms']) for d in map(json.loads, sys.stdin)))"
done; done
