#!/bin/bash
# Collect the rocprofv3 evidence for one round on the GPU box:  OUT=<dir> tools/collect_profiles.sh <tag> [bench.py args]
#   $OUT/<tag>/stats   --kernel-trace --stats of `bench.py --steps 20 --warmup 5 --full` (the sampling steps of --full included)
#   $OUT/<tag>/fetch   --pmc FETCH_SIZE                     (separate passes: the TCC counters do not fit together)
#   $OUT/<tag>/write   --pmc WRITE_SIZE
#   $OUT/<tag>/mfma    --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE
#   $OUT/<tag>.bench.json   the line of `bench.py --steps 20 --warmup 5 --full --no-extra` (roofline, per-kernel table, CPU baseline)
# then OUT=<dir> tools/summarize_profiles.py <tag> turns them into profiles/<tag>_kernel_stats.csv, profiles/<tag>_pmc_traffic.json
# and profiles/<tag>_bench.json.  OUT is relative to the repository root.
set -e
TAG=${1:?tag}
shift
EXTRA="$@"          # extra bench.py arguments, e.g. --config cfg4 --dtype bf16
R=$PWD
O=$R/${OUT:?OUT: output directory, relative to the repository root}
mkdir -p $O
export TMPDIR=/tmp
cd /tmp
# the kernel trace is of the DRIVER's command shape (20 timed steps behind 5 warm-up ones, hipGraph replays, the eager sampling steps after them)
ARGS="$R/bench.py --steps 20 --warmup 5 --full --no-cpu-baseline --no-extra $EXTRA"
rocprofv3 --kernel-trace --stats -d $O/$TAG/stats -o s --output-format csv -- python3 $ARGS > $O/$TAG.stats_bench.json 2>/dev/null
# counters: launch by launch (a counter pass serialises the kernels anyway), two steps
ARGS="$R/bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-extra --events none --no-graph $EXTRA"
rocprofv3 --pmc FETCH_SIZE -d $O/$TAG/fetch -o f --output-format csv -- python3 $ARGS > /dev/null 2>&1
rocprofv3 --pmc WRITE_SIZE -d $O/$TAG/write -o w --output-format csv -- python3 $ARGS > /dev/null 2>&1
rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE -d $O/$TAG/mfma -o m --output-format csv -- python3 $ARGS > /dev/null 2>&1
cd $R
python3 bench.py --steps 20 --warmup 5 --full --no-extra $EXTRA > $O/$TAG.bench.json
ls -R $O/$TAG | head -40
