#!/bin/bash
# One GPU session into the folder $1: GPU tests, smoke, the bench with --full, rocprofv3 kernel-trace summary.  Every GPU
# step has its own time limit and the script stops at the first failure of a GPU step (no retries).
set -o pipefail
cd "$GRAFT_REPO_ROOT" || exit 1
export TMPDIR=/tmp
OUT=${1:?usage: gpu_check.sh <output folder>}
mkdir -p "$OUT"
timeout -k 10 600 python -m pytest tests -q -m gpu > "$OUT/t_gpu.log" 2>&1
echo "pytest rc=$?" >> "$OUT/t_gpu.log"
timeout -k 10 200 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.log" 2>&1 || exit 1
timeout -k 10 300 python bench.py --full > "$OUT/bench.json" 2> "$OUT/bench.err" || exit 1
if [ "${QLX_PROFILE:-1}" = "1" ]; then
  timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof" -o bench -- \
    python3 bench.py --full --steps 10 --cpu-sample 0 > "$OUT/prof_bench.json" 2> "$OUT/prof.err" || exit 1
fi
exit 0
