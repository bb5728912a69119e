# Same-box A/B: the product library against a build of another commit ($PREV_LIB, default
# tools/bin/ab_prev/libjsplace.so), alternating: the bench's headline and tools/devpath_loop.py on configs
# $CFGS (default 5,3) twice each, then tools/svc_probe.py. Output goes to $OUT_ROOT/$TAG (defaults build/ab
# and ab; give scripts/gpu_run.sh's output directory as OUT_ROOT to collect it with scripts/collect_profiles.sh).
#   TAG=name CFGS=5,3 PREV_LIB=path bash scripts/ab_same_box.sh
# The other library is made by hand; nothing builds it: a `git worktree add DIR COMMIT` of the commit to
# compare against, `make` in DIR, then copy DIR/jobset_amd/libjsplace.so to $PREV_LIB.
set -u
cd "$(dirname "$0")/.."; OUT=${OUT_ROOT:-build/ab}/${TAG:-ab}; mkdir -p $OUT
PREV_LIB=${PREV_LIB:-tools/bin/ab_prev/libjsplace.so}
[ -f "$PREV_LIB" ] || { echo "no library to compare against at $PREV_LIB"; exit 2; }
for v in new prev new2 prev2; do
  lib=""; case $v in prev*) lib=$PREV_LIB;; esac
  JSP_LIB_PATH=$lib timeout -k 10 120 python bench.py --gpus 1 --steps 20 --warmup 5 > $OUT/bench_$v.json 2> $OUT/bench_$v.err || { cat $OUT/bench_$v.err; exit 1; }
  JSP_LIB_PATH=$lib timeout -k 10 200 python -u tools/devpath_loop.py ${CFGS:-5,3} 2 > $OUT/devpath_$v.txt 2>&1 || { cat $OUT/devpath_$v.txt; exit 1; }
done
for v in new prev; do
  lib=""; case $v in prev*) lib=$PREV_LIB;; esac
  JSP_LIB_PATH=$lib timeout -k 10 200 python -u tools/svc_probe.py 1000 ${CFGS:-5,3} > $OUT/svc_$v.txt 2>&1 || { cat $OUT/svc_$v.txt; exit 1; }
done
tail -qn 1 $OUT/bench_*.json; grep -H "cfg" $OUT/devpath_*.txt; grep -H "timing=" $OUT/svc_*.txt
