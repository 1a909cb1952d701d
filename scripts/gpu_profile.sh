#!/bin/bash
# Full evidence run: GPU tests, smoke, default bench line, rocprofv3 kernel stats and PMC (FETCH_SIZE / WRITE_SIZE) passes.
set -u
cd "${GRAFT_REPO_ROOT:-/root/repo}"
TAG=${1:-r3}
mkdir -p "${OUTDIR:-bench_out}" && export OUTDIR="$(cd "${OUTDIR:-bench_out}" && pwd)"   # absolute: the same folder after any cd, and in the scripts this one calls
export PYTHONPATH="$PWD"
[ "${SKIP_TESTS:-0}" = 1 ] || timeout 2400 python -m pytest tests -m gpu -q 2>&1 | tail -30 | tee "$OUTDIR"/pytest_gpu.log
timeout 300 python __graft_entry__.py smoke 2>&1 | tail -2 | tee "$OUTDIR"/smoke.log
timeout 900 python bench.py --full 2> "$OUTDIR"/bench_${TAG}.err | tail -1 > "$OUTDIR"/bench_${TAG}.log
cd /tmp && export TMPDIR=/tmp
R="$OLDPWD"
timeout 900 rocprofv3 --kernel-trace --stats -d "$OUTDIR/prof_${TAG}" -- python "$R/bench.py" --full --steps 3 --warmup 1 --cpu-sample 0 --no-steady > "$OUTDIR/prof_${TAG}.log" 2>&1
timeout 900 rocprofv3 --pmc FETCH_SIZE --kernel-trace -d "$OUTDIR/pmc_fetch_${TAG}" -- python "$R/bench.py" --full --steps 1 --warmup 0 --cpu-sample 0 --no-steady > "$OUTDIR/pmc_fetch_${TAG}.log" 2>&1
timeout 900 rocprofv3 --pmc WRITE_SIZE --kernel-trace -d "$OUTDIR/pmc_write_${TAG}" -- python "$R/bench.py" --full --steps 1 --warmup 0 --cpu-sample 0 --no-steady > "$OUTDIR/pmc_write_${TAG}.log" 2>&1
cd "$R"
python scripts/prof_summary.py "$OUTDIR"/prof_${TAG} 300 > "$OUTDIR"/prof_${TAG}_summary.txt 2>&1
head -16 "$OUTDIR"/prof_${TAG}_summary.txt | cut -c1-170
python scripts/pmc_summary.py "$OUTDIR"/pmc_fetch_${TAG} "$OUTDIR"/pmc_write_${TAG} "$OUTDIR"/${TAG} | cut -c1-150
