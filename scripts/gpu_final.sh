#!/bin/bash
# GPU-box round check: smoke, multi-rank RCCL parity, the -m gpu suite, the
# default bench line (--full: with its CPU baselines).  Stops at the first
# failing step.  Logs go to $OUT (default build/gpu_logs).
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT:-build/gpu_logs}; mkdir -p "$OUT"
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.log" 2>&1
rc=$?; echo "smoke rc=$rc" >> "$OUT/smoke.log"; if [ $rc -ne 0 ]; then exit $rc; fi
timeout -k 10 500 python -u -m pytest tests/test_gpu_multi.py -x -v --timeout 330 --timeout-method thread > "$OUT/pytest_multi.log" 2>&1
rc=$?; echo "multi rc=$rc" >> "$OUT/pytest_multi.log"; if [ $rc -ne 0 ]; then exit $rc; fi
timeout -k 10 600 python -u -m pytest tests -m gpu -q -x --timeout 300 --timeout-method thread --ignore=tests/test_gpu_multi.py > "$OUT/pytest_gpu.log" 2>&1
rc=$?; echo "pytest rc=$rc" >> "$OUT/pytest_gpu.log"; if [ $rc -ne 0 ]; then exit $rc; fi
timeout -k 10 300 python bench.py --full > "$OUT/bench_default.log" 2>&1
rc=$?; echo "bench rc=$rc" >> "$OUT/bench_default.log"
exit $rc
