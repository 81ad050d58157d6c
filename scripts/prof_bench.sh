#!/bin/bash
# rocprofv3 kernel trace + stats of a short bench run (--full: the summary reads the roofline legs),
# summarised where it ran (the raw trace stays in /tmp; the log and the summary go to $OUT, default
# bench_out/).  Usage: bash scripts/prof_bench.sh [tag]
set -o pipefail
TAG=${1:-r04}
OUT=${OUT:-bench_out}
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
mkdir -p "$OUT"
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d /tmp/prof_$TAG -o run -- \
    python3 bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-pmc > "$OUT"/prof_bench_$TAG.log 2>&1 &&
python3 scripts/rocprof_summary.py "$(find /tmp/prof_$TAG -name '*results.db' -print -quit)" \
    "$OUT"/prof_$TAG --bench "$OUT"/prof_bench_$TAG.log >> "$OUT"/prof_bench_$TAG.log 2>&1 &&
echo PROF_DONE
