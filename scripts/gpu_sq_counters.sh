#!/bin/bash
# One rocprofv3 SQ-counter pass (8 SQ slots, --kernel-trace only) over one bench step: stall breakdown per kernel.
set -u
cd "${GRAFT_REPO_ROOT:-/root/repo}"
TAG=${1:-r2}
mkdir -p "${OUTDIR:-bench_out}" && export OUTDIR="$(cd "${OUTDIR:-bench_out}" && pwd)"   # absolute: the same folder after any cd, and in the scripts this one calls
export PYTHONPATH="$PWD"
R="$PWD"
cd /tmp && export TMPDIR=/tmp
timeout 900 rocprofv3 --pmc SQ_WAVE_CYCLES SQ_ACTIVE_INST_ANY SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_LDS_IDX_ACTIVE SQ_LDS_BANK_CONFLICT \
    --kernel-trace -d "$OUTDIR/sq_${TAG}" -- python "$R/bench.py" --full --steps 1 --warmup 0 --cpu-sample 0 --no-steady > "$OUTDIR/sq_${TAG}.log" 2>&1
cd "$R"
tail -3 "$OUTDIR"/sq_${TAG}.log | cut -c1-300
python scripts/sq_summary.py "$OUTDIR"/sq_${TAG} "$OUTDIR"/${TAG}_sq_stall_breakdown.txt | cut -c1-170
rm -rf "$OUTDIR"/sq_${TAG}      # the raw counter database (> 64 MiB) stays on the box
