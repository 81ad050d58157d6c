#!/bin/bash
# rocprofv3 kernel trace of a short bench whose weight is the batched (BASELINE config 3) leg, which
# runs under --full; summarised where it ran, so the raw trace stays in /tmp (the log and the summary
# go to $OUT, default bench_out/).  Usage: bash scripts/prof_batched.sh [tag] [batch]
set -o pipefail
TAG=${1:-b32}
B=${2:-32}
OUT=${OUT:-bench_out}
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
mkdir -p "$OUT"
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d /tmp/prof_$TAG -o run -- \
    python3 bench.py --full --steps 1 --warmup 0 --frames 24 --no-cpu-baseline --batch $B --batch-frames 48 \
    > "$OUT"/prof_$TAG.log 2>&1 &&
python3 scripts/rocprof_summary.py $(find /tmp/prof_$TAG -name '*results.db' -print -quit) "$OUT"/prof_$TAG \
    >> "$OUT"/prof_$TAG.log 2>&1 && echo PROF_DONE
