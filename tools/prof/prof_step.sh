#!/bin/bash
# rocprofv3 kernel stats of the benchmark step (the full bench line: bench.py --full).  Run on the GPU box from the repo root:
#   bash tools/prof/prof_step.sh <tag> [bench args]
# Writes $OUT/<tag>_kernel_stats.csv (OUT defaults to prof_out; the summary to copy into profiles/) and prints the per-kernel table.
cd /tmp && export TMPDIR=/tmp && cd - > /dev/null
TAG=${1:-prof}; shift
OUT=${OUT:-prof_out}; mkdir -p "$OUT"
rm -rf "$OUT/_prof_$TAG"
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/_prof_$TAG" -o p -- python3 bench.py --full --no-cpu-baseline --no-verify --no-ceiling --steps 100 --warmup 10 "$@" > "$OUT/${TAG}_bench.json" 2> "$OUT/${TAG}_prof.err"
F=$(find "$OUT/_prof_$TAG" -name '*kernel_stats.csv' | head -1)
cp "$F" "$OUT/${TAG}_kernel_stats.csv"
python3 tools/prof/kstats.py "$OUT/${TAG}_kernel_stats.csv" | head -12
rm -rf "$OUT/_prof_$TAG"
