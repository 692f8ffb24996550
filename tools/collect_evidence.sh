#!/bin/bash
# Everything under profiles/<TAG>_* in one GPU call: the PMC passes (MFMA utilisation / instruction mix, HBM traffic of the 3x3
# kernels), the per-shape tables, the ablation table, the full bench line, and the rocprofv3 --kernel-trace --stats summaries of the
# bench command (four batches in flight = the timed region; one batch at a time = what roofline.frac is measured on).
#   gpurun --timeout 3000 -- 'TAG=r06 COMMIT=<hash> bash tools/collect_evidence.sh'
# writes gpurun_out/$TAG/*; copy what is to be judged into profiles/ (README there names every file and its tool).
# Trouble ends it: every step that opens the GPU runs under its own time limit, and the first step that fails — a time limit
# (124 / 137), an abort (134), a segmentation fault (139) or a plain error — ends the script with that status.  Nothing is
# started on the GPU after it; the closing message names the step.
set -o pipefail
cd ${GRAFT_REPO_ROOT:-.}
TAG=${TAG:-r06}
COMMIT=${COMMIT:-$(git rev-parse --short HEAD 2>/dev/null)}
export COMMIT
DT=${DT:-f16}
O=gpurun_out/$TAG
mkdir -p $O

stop() { echo "collect_evidence: stopped at step '$1' with exit status $2; nothing further was started" >&2; exit $2; }
# gpu_step <name> <seconds> <stdout file> <stderr file> <command ...>: the command under `timeout -k 10 <seconds>`
gpu_step() {
  local name=$1 secs=$2 out=$3 err=$4
  shift 4
  echo "== $name (limit $secs s)"
  if [ "$err" = "$out" ]; then timeout -k 10 $secs "$@" > $out 2>&1; else timeout -k 10 $secs "$@" > $out 2> $err; fi
  local rc=$?
  [ $rc -eq 0 ] || stop "$name" $rc
}
# host_step <name> <command ...>: copies and post-processing (no GPU), checked the same way
host_step() {
  local name=$1
  shift
  "$@"
  local rc=$?
  [ $rc -eq 0 ] || stop "$name" $rc
}

# Time limits: the two 900 s of the PMC passes are the ones this script always had (each pass script also limits its own
# rocprofv3 runs).  No log of a whole round-6 run is in the tree, so the others come from what the step does: a shape table is
# a few dozen stand-alone launches (600 s); the ablation table and the traced bench are several / one serialised bench runs
# (900 s); the final bench line is one full run with the CPU baseline (900 s).
gpu_step pmc_util 900 $O/pmc_util.log $O/pmc_util.log bash tools/pmc_util.sh $O/pmc_util $DT
gpu_step pmc_traffic 900 $O/pmc_traffic.log $O/pmc_traffic.log bash tools/pmc_traffic.sh $O/pmc_traffic $DT
host_step "copy pmc_conv3x3.json" cp $O/pmc_traffic/pmc_conv3x3.json $O/pmc_conv3x3.json
host_step "copy pmc_mfma_util.json" cp $O/pmc_util/summary.json $O/${TAG}_pmc_mfma_util.json
gpu_step shape_table_nf64 600 $O/${TAG}_by_shape_nf64.md /dev/null python tools/shape_table.py 64 $DT
gpu_step shape_table_nf128 600 $O/${TAG}_by_shape_nf128.md /dev/null python tools/shape_table.py 128 $DT
gpu_step ablate_bench 900 $O/${TAG}_ablation.txt $O/${TAG}_ablation.txt python tools/ablate_bench.py
cd /tmp && export TMPDIR=/tmp && cd "$OLDPWD"
for MODE in inflight alone; do
  EXTRA=""; SUF=""
  if [ $MODE = alone ]; then EXTRA="--in-flight 1"; SUF="_alone"; fi
  rm -rf /tmp/kt
  gpu_step kernel_trace_$MODE 900 $O/${TAG}_kt$SUF.log $O/${TAG}_kt$SUF.log rocprofv3 --kernel-trace --stats -d /tmp/kt -o kt --output-format csv -- python bench.py --full --dtype $DT --no-cpu-baseline --no-extra-modes --no-roofline $EXTRA
  STATS=$(find /tmp/kt -name "*kernel_stats.csv" | head -1)
  [ -n "$STATS" ] || stop "kernel_trace_$MODE: no kernel_stats.csv under /tmp/kt" 1
  host_step "copy kernel_stats$SUF.csv" cp "$STATS" $O/${TAG}_kernel_stats$SUF.csv
  python tools/kernel_stats_md.py $O/${TAG}_kernel_stats$SUF.csv "rocprofv3 --kernel-trace --stats summary of \`python bench.py --full --dtype $DT --no-cpu-baseline --no-extra-modes --no-roofline $EXTRA\` ($TAG, commit $COMMIT; $MODE: 2 warm-up + 8 timed steps + the latency / bit-identity extras; the tracer serialises dispatches)" > $O/${TAG}_bench_${DT}${SUF}_kernel_stats.md || stop "kernel_stats_md $MODE" $?
done
# (the bench line last: its roofline.frac_rocprof reads the summaries just written when they have been copied to profiles/)
host_step "copy the summaries to profiles/" cp $O/${TAG}_bench_${DT}_kernel_stats.md $O/${TAG}_bench_${DT}_alone_kernel_stats.md $O/${TAG}_pmc_mfma_util.json profiles/
host_step "copy pmc_conv3x3.json to profiles/" cp $O/pmc_conv3x3.json profiles/pmc_conv3x3.json
gpu_step bench_full 900 $O/${TAG}_bench_$DT.json $O/${TAG}_bench_$DT.err python bench.py --full --dtype $DT
tail -c 1500 $O/${TAG}_bench_$DT.json
echo "collect_evidence: all steps done"
