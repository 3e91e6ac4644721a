#!/bin/bash
# Same-device A/B of two trees:  tools/ab.sh <treeA> <treeB> <rounds> [bench.py args]   (prints ms_per_step per run)
# Tiled inference instead of the training step:  AB_INFER=1 [AB_ARGS_A=..] [AB_ARGS_B="--window pyramid"] tools/ab.sh <treeA> <treeB> <rounds>
# runs each tree's tools/bench_infer.py (with that tree's arguments) and prints ms_per_image and the three stage times per run.
A=$1; B=$2; R=$3; shift 3
for i in $(seq $R); do
  for T in $A $B; do
    if [ -n "$AB_INFER" ]; then
      if [ "$T" = "$A" ]; then X=$AB_ARGS_A; else X=$AB_ARGS_B; fi
      timeout -k 10 300 python3 $T/tools/bench_infer.py $X | python3 -c "import json,sys; d=json.loads(sys.stdin.readlines()[-1]); print('$T', '[$X]', d['ms_per_image'], d['gather_ms'], d['forward_ms'], d['blend_ms'])" || exit 1
      continue
    fi
    python3 $T/bench.py --steps 30 --warmup 8 --no-cpu-baseline --events none "$@" | python3 -c "import json,sys; d=json.loads(sys.stdin.readlines()[-1]); print('$T', d['dtype'], d['ms_per_step'], d['value'])"
  done
done
