#!/usr/bin/env bash
# GPU validation run used with gpurun: tests, smoke, short bench, rocprof stats.
set -euo pipefail
cd "$(dirname "$0")/../.."
export TMPDIR=/tmp
mkdir -p gpurun_out
python tools/build_ext.py > gpurun_out/build.log 2>&1
timeout -k 10 600 python -m pytest tests -m gpu -q -p no:cacheprovider > gpurun_out/pytest_gpu.log 2>&1 || { echo "pytest failed"; tail -50 gpurun_out/pytest_gpu.log; exit 1; }
tail -3 gpurun_out/pytest_gpu.log
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > gpurun_out/smoke.log 2>&1
tail -2 gpurun_out/smoke.log
# --full: the record keeps the engine-only rates, the 1/10/100-user levels, the in-process and bf16 windows
BENCH_OUT=${BENCH_OUT:-bench_out}
mkdir -p "$BENCH_OUT"
timeout -k 10 600 python bench.py --full --steps ${STEPS:-100} --warmup 10 > "$BENCH_OUT/bench.json" 2> "$BENCH_OUT/bench.err"
cat "$BENCH_OUT/bench.json"
