#!/bin/bash
# host-buffer boundary (u8 in, sparse out) at pipeline depth 2 and 3:  bash tools/host_depth.sh
OUT=${OUT:-bench_out}/ab
mkdir -p $OUT
for d in 2 3; do
  timeout 600 python3 bench.py --full --steps 20 --warmup 4 --no-cpu-baseline --pmc-traffic 0 --pipeline-depth $d > $OUT/hd$d.json 2> $OUT/hd$d.err
  python3 - $d $OUT <<'PY'
import json, sys
d = json.loads(open(f"{sys.argv[2]}/hd{sys.argv[1]}.json").read().strip().splitlines()[-1])
h = d["host_inclusive"]
print("depth", sys.argv[1], round(d["ms_per_step"], 3), {k: round(v, 3) for k, v in h.items() if not k.endswith("what")}, "single frame", round(d.get("single_frame_ms", 0), 3))
PY
done
