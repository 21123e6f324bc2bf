#!/bin/bash
# development: small-batch lines (config 3 = 1 seed, config 4's per-GPU load at N = 8 = 8 seeds); JSON lines under $OUT
OUT=${OUT:-build_ab/small_batch}
mkdir -p "$OUT"
for S in 1 8 16; do
  timeout -k 10 300 python bench.py --no-cpu-baseline --no-extra --seeds-per-gpu $S --steps 5 > "$OUT/bench_s${S}.json" 2>/dev/null
  python3 - "$OUT/bench_s${S}.json" $S <<'PY'
import json, sys
path, s = sys.argv[1:3]
d = json.loads(open(path).read().strip().splitlines()[-1])
print("seeds", s, round(d["value"], 1), {k: round(v, 2) for k, v in d["phases_ms_per_step"].items()}, "plain", d["uninstrumented"] and {k: round(v, 2) for k, v in d["uninstrumented"]["phases_ms_per_step"].items()})
PY
done
