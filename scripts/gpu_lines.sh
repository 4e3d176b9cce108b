#!/bin/bash
# Bench lines on one box, untraced, then a rocprofv3 kernel-trace of each:
#   LINES="name:args;name:args" bash scripts/gpu_lines.sh
# Each line: python bench.py <args> --full --no-cpu-baseline (every kernel of the
# step in `kernels`) -> $OUT/<name>_r<rep>.json, then (TRACE=1) rocprofv3
# --kernel-trace --stats -> $OUT/<name>_trace/.  OUT defaults to build/gpu_logs/lines.
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT:-build/gpu_logs/lines}; mkdir -p "$OUT"
export TMPDIR=/tmp
IFS=';' read -ra L <<< "$LINES"
for item in "${L[@]}"; do
  name="${item%%:*}"; args="${item#*:}"
  for rep in $(seq 1 ${REPS:-1}); do
    timeout -k 10 240 python bench.py $args --full --no-cpu-baseline > "$OUT/${name}_r${rep}.json" 2> "$OUT/${name}_r${rep}.err"
    rc=$?; echo "$name rep $rep rc=$rc" >> "$OUT/status.txt"; [ $rc -ne 0 ] && exit $rc
  done
  if [ -n "$TRACE" ]; then
    timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$OUT/${name}_trace" -o run -- python3 bench.py $args --full --no-cpu-baseline > "$OUT/${name}_traced.json" 2> "$OUT/${name}_traced.err"
    rc=$?; echo "$name traced rc=$rc" >> "$OUT/status.txt"; [ $rc -ne 0 ] && exit $rc
  fi
done
exit 0
