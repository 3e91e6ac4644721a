#!/bin/bash
# What the data-parallel code path costs on ONE rank (RCCL collectives on the second stream, staged losses), and what the
# roofline events of the timed region cost (bench.py --full):  OUT=<dir> tools/dp_overhead.sh [prof]  ->  $OUT/dpo_*.json ;
# with "prof" also a kernel trace of the DP run
set -u
R=$PWD
O=$R/${OUT:?OUT: directory for the bench lines, relative to the repository root}
mkdir -p $O
export TMPDIR=/tmp
python3 bench.py --steps 30 --warmup 5 --full --no-cpu-baseline --no-extra > $O/dpo_plain.json 2>$O/dpo_plain.err
python3 bench.py --steps 30 --warmup 5 --full --no-cpu-baseline --no-extra --events none > $O/dpo_plain_noev.json 2>$O/dpo_plain.err
PATCHGAN_DP_FORCE=1 python3 bench.py --steps 30 --warmup 5 --full --no-cpu-baseline --no-extra > $O/dpo_dp.json 2>$O/dpo_dp.err
PATCHGAN_DP_FORCE=1 python3 bench.py --steps 30 --warmup 5 --full --no-cpu-baseline --no-extra --events none > $O/dpo_dp_noev.json 2>$O/dpo_dp.err
if [ "${1:-}" = prof ]; then
cd /tmp
PATCHGAN_DP_FORCE=1 rocprofv3 --kernel-trace --stats -d $O/dpo_prof -o s --output-format csv -- python3 $R/bench.py --steps 10 --warmup 3 --full --no-cpu-baseline --no-extra --events none > $O/dpo_prof.json 2>/dev/null
cd $R
cp $(find $O/dpo_prof -name "*kernel_stats.csv" | head -1) $O/dpo_dp_stats.csv
cp $(find $O/dpo_prof -name "*kernel_trace.csv" | head -1) $O/dpo_dp_trace.csv
rm -rf $O/dpo_prof
fi
