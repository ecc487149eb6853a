#!/bin/bash
# Run on the GPU box (via gpurun): rocprofv3 kernel-trace stats + PMC passes of bench.py.
# Outputs under gpurun_out/prof/; summarise afterwards with tools/summarize_profile.py.
set -u
R=${GRAFT_REPO_ROOT:-$PWD}
OUT=$R/gpurun_out/prof
rm -rf $OUT; mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
BENCH="python3 $R/bench.py --full --no-cpu-baseline --no-clock-probe"   # no probe / sampler legs: the per-kernel rows hold the step kernels only
# Every rocprofv3 run has its own time limit, and the script stops at the first run that fails or times out: nothing more
# is started on a device that may have just faulted.  The PMC runs collect counters with --kernel-trace only.
run() {   # run <tag> <seconds> <rocprofv3 arguments...>
  local tag=$1 secs=$2
  shift 2
  timeout -k 10 "$secs" rocprofv3 "$@" > "$OUT/$tag.log" 2>&1
  local rc=$?
  if [ $rc -ne 0 ]; then
    echo "$tag failed (exit $rc; 124 or 137: time limit)"
    tail -5 "$OUT/$tag.log"
    exit $rc
  fi
}
run stats 480 --kernel-trace --stats --output-format csv -d $OUT/stats -- $BENCH --no-extra-configs --steps 10 --warmup 2
for pass in "FETCH_SIZE" "WRITE_SIZE" "SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAVES SQ_INSTS_SALU SQ_INSTS_SMEM SQ_WAIT_INST_ANY" "GRBM_GUI_ACTIVE GRBM_COUNT" "SQ_INSTS_VALU_TRANS SQ_ACTIVE_INST_ANY SQ_WAIT_ANY SQ_INSTS_LDS SQ_LDS_BANK_CONFLICT" "TCC_HIT_sum TCC_MISS_sum"; do
  tag=$(echo $pass | tr ' ' '_' | cut -c1-40)
  run pmc_$tag 300 --pmc $pass --kernel-trace --output-format csv -d $OUT/pmc_$tag -- $BENCH --no-extras --steps 3 --warmup 1
done
find $OUT -name "*.csv" | head -40
