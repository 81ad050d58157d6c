#!/bin/bash
# One GPU pass: gpu parity tests, smoke(), the whole bench line (--full), and a rocprofv3
# kernel-trace of a short bench, summarised where it ran (the raw trace stays in /tmp; logs and
# summaries go to $OUT, default bench_out/).  Every GPU step has its own time limit; steps are
# chained with && so the first failure ends the call.
# Usage: bash scripts/gpu_check.sh [tag] [extra pytest args...]
set -o pipefail
TAG=${1:-r03}
shift
OUT=${OUT:-bench_out}
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
mkdir -p "$OUT"
timeout -k 10 720 python -u -m pytest tests -x -v --timeout 180 --timeout-method thread -m gpu "$@" \
    > "$OUT"/gpu_tests_$TAG.log 2>&1 && tail -3 "$OUT"/gpu_tests_$TAG.log &&
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > "$OUT"/smoke_$TAG.log 2>&1 &&
tail -1 "$OUT"/smoke_$TAG.log &&
timeout -k 10 420 python -u bench.py --full > "$OUT"/bench_$TAG.log 2>&1 && tail -1 "$OUT"/bench_$TAG.log &&
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d /tmp/prof_$TAG -o run -- \
    python3 bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-pmc > "$OUT"/prof_bench_$TAG.log 2>&1 &&
python3 scripts/rocprof_summary.py "$(find /tmp/prof_$TAG -name '*results.db' -print -quit)" \
    "$OUT"/prof_$TAG --bench "$OUT"/prof_bench_$TAG.log >> "$OUT"/prof_bench_$TAG.log 2>&1 &&
echo GPU_CHECK_DONE
