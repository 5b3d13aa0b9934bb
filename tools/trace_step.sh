# Kernel trace of a short bench run on the GPU machine + the concurrency summary of one step (tools/trace_gaps.py): per-queue busy
# time, overlap histogram, what the main queue waited for.  The step summarised is one of the eager steps --full runs behind the
# timed region.  From the repo root: bash tools/trace_step.sh OUT_DIR
OUT=$(realpath -m "${1:?usage: tools/trace_step.sh OUT_DIR}")
ROOT=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --output-format csv -d "$OUT/tr" -o tr -- python3 "$ROOT/bench.py" --full --steps 8 --warmup 3 --no-cpu-baseline > "$OUT/tr.log" 2>&1
cd "$ROOT"
cut -c120-180 "$OUT/tr.log" | tail -1
python3 tools/trace_gaps.py $(ls -t "$OUT"/tr/*kernel_trace.csv | head -1)
python3 tools/step_kernels.py $(ls -t "$OUT"/tr/*kernel_trace.csv | head -1) "$OUT/step_kernels.txt"
