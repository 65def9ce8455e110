#!/bin/bash
# usage (GPU box, repo root): tools/prof_default.sh <outdir-under-gpurun_out>
# kernel trace of a --full pipelined run (three contexts: oracle check and host-I/O leg included) without the FEM / stereo / matcher-loop legs
# and the CPU baseline: per-kernel averages as the timed region sees them
set -e
REPO=$(cd "$(dirname "$0")/.." && pwd)
OUT=$GRAFT_REPO_ROOT/gpurun_out/$1
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace_default -- python3 $REPO/bench.py --full --no-fem --no-cpu-baseline > $OUT/trace_default.log 2>&1
tail -c 400 $OUT/trace_default.log
