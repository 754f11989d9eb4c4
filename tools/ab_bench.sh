#!/bin/bash
# A/B of end-to-end frame time inside ONE gpurun call (boxes differ by several percent): interleaved rounds of
# `bench.py --steps 20` per variant.  A variant is "-" (the default build) or extra bench.py arguments starting with "--"
# (e.g. --prefetch).
# usage: tools/ab_bench.sh <rounds> <variant> [<variant> ...]
rounds=$1; shift
for r in $(seq 1 $rounds); do
  for v in "$@"; do
    args=""; [ "$v" != "-" ] && args=$v
    ms=$(python bench.py --steps 20 --warmup 3 --quick $args 2>/dev/null | python -c "import sys,json; d=json.loads(sys.stdin.readline()); print(d['ms_per_step'], 'per-step min/median/max', d['step_ms_min_median_max'])")
    echo "round $r variant [$v] ms_per_step $ms"
  done
done
