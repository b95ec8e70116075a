#!/bin/bash
# One call: GPU parity tests, smoke, bench, rocprof kernel stats.  Logs land in $OUT (default bench_out/).
set -u
OUT=${OUT:-bench_out}
mkdir -p $OUT
export TMPDIR=/tmp
rocminfo 2>/dev/null | grep -m2 -E "gfx|Marketing" > $OUT/device.txt
lscpu | grep -E "Model name|^CPU\(s\)" >> $OUT/device.txt
timeout 1500 python -m pytest tests -m gpu -q -x --tb=short -p no:cacheprovider > $OUT/pytest_gpu.log 2>&1
echo "pytest exit $?" >> $OUT/pytest_gpu.log
tail -5 $OUT/pytest_gpu.log
timeout 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1; echo "smoke exit $?" >> $OUT/smoke.log; tail -2 $OUT/smoke.log
timeout 900 python bench.py --full --steps ${STEPS:-3} --warmup 1 > $OUT/bench.log 2> $OUT/bench.err; echo "bench exit $?"; tail -c 2500 $OUT/bench.log; tail -5 $OUT/bench.err
timeout 600 python bench.py --steps ${STEPS:-3} --warmup 1 --no-cpu-baseline --no-extras --pipeline-depth 1 > $OUT/bench_depth1.log 2>/dev/null; echo "bench depth 1 exit $?"; grep -o "ms_per_step\": [0-9.]*" $OUT/bench_depth1.log
if [ "${PROF:-1}" = "1" ]; then
  rm -rf $OUT/prof
  timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -- python3 bench.py --steps 8 --warmup 2 --no-cpu-baseline --no-extras > $OUT/prof_bench.log 2>&1
  echo "rocprof exit $?"
  find $OUT/prof -name "*kernel_stats*" | head -3
  f=$(find $OUT/prof -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && head -25 "$f" | cut -c1-200
  # keep the merge-back small: drop the per-dispatch trace
  find $OUT/prof -name "*kernel_trace.csv" -size +20M -delete
  t=$(find $OUT/prof -name "*kernel_trace.csv" | head -1); [ -n "$t" ] && python3 tools/timeline_window.py "$t" 8000 500 > $OUT/timeline_pipelined.txt 2>&1
  # single-step timeline (one step at a time)
  rm -rf $OUT/prof1
  timeout 900 rocprofv3 --kernel-trace --output-format csv -d $OUT/prof1 -- python3 bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-extras --pipeline-depth 1 > $OUT/prof1_bench.log 2>&1
  t=$(find $OUT/prof1 -name "*kernel_trace.csv" | head -1); [ -n "$t" ] && python3 tools/timeline.py "$t" > $OUT/timeline.txt 2>&1
  rm -rf $OUT/prof1
fi
