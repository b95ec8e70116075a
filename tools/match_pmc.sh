#!/bin/bash
# SQ counters of the descriptor matcher's kernels on a 19 764 x 19 300 pair of descriptor-shaped rows: one --pmc pass of its own
# (no tracing beside it).  Prints the per-kernel sums; DESIGN.md section 3a reads the tile kernel's line.
set -u
export TMPDIR=/tmp
OUT=${OUT:-bench_out/match_pmc}
rm -rf "$OUT"; mkdir -p "$OUT"
cat > "$OUT/case.py" <<'PY'
import os, sys
ROOT = os.getcwd()
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import match_ref as M
from sift_amd.sift import Context
rng = np.random.default_rng(0)
q, t = M.desc_rows(rng, 19764), M.desc_rows(rng, 19300)
ctx = Context(0)
for _ in range(3):
    ctx.knn2(q, t)
ctx.close()
PY
timeout -k 10 300 rocprofv3 --pmc SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_VALU \
    --output-format csv -d "$OUT" -- python3 "$OUT/case.py" > "$OUT/run.log" 2>&1 || { tail -5 "$OUT/run.log"; exit 1; }
python3 - "$OUT" <<'PY'
import collections, csv, glob, sys
acc = collections.defaultdict(lambda: collections.defaultdict(float))
for f in glob.glob(sys.argv[1] + "/**/*counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        name = r["Kernel_Name"].split("(")[0]
        if "match_" in name:
            acc[name][r["Counter_Name"]] += float(r["Counter_Value"])
for name in sorted(acc):
    print(name, {k: f"{v:.4g}" for k, v in sorted(acc[name].items())})
PY
