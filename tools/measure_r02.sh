#!/bin/bash
# Round-2 measurement batch (run on the GPU box from the repo root): the driver's bench line, rocprofv3 kernel stats per workload
# and the --pmc passes (each counter group in its own run, kernel trace only) behind the roofline figures.
# Outputs under gpurun_out/measure2/; copy the summaries into profiles/ (tools/collect_profiles_r02.sh).
# usage: tools/measure_r02.sh [bench|stats|pmc|all]   (default all)
R=$PWD
O=$R/gpurun_out/measure2
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
B="python $R/bench.py --full"
WHAT=${1:-all}
HEAD=$(cat $R/.git_head 2>/dev/null || echo unknown)
if [ "$WHAT" = bench ] || [ "$WHAT" = all ]; then
  timeout 900 $B --gpus 1 --steps 20 --warmup 5 > $O/bench_default.json 2> $O/bench_default.err
fi
if [ "$WHAT" = stats ] || [ "$WHAT" = all ]; then
  for wl in cascade hog_svm ffp15 sdm; do
    S=10; [ $wl = ffp15 ] && S=3
    FP=""; [ $wl = cascade ] && FP="--frames-per-step 128"
    # cascade: ONE call in flight and the host stages inline, so that a kernel's duration is its own (with six calls in flight the
    # kernels of different calls share the CUs and every average is inflated 2-3x); bench.py's live figure (kernel_probe) is taken
    # the same way
    ENVX=""; [ $wl = cascade ] && ENVX="env FD_BENCH_SLOTS=1 FD_FRAMES_ASYNC=0"
    [ $wl = sdm ] && ENVX="env FD_BENCH_SDM_THREADS=1"   # same reason: three batches in flight share the CUs
    timeout 300 $ENVX rocprofv3 --kernel-trace --stats --output-format csv -d $O/stats_$wl -- $B --workload $wl --also none --steps $S --warmup 2 $FP --no-cpu-baseline > $O/stats_$wl.json 2> $O/stats_$wl.err
  done
fi
if [ "$WHAT" = pmc ] || [ "$WHAT" = all ]; then
  for wl in cascade ffp15 sdm hog_svm; do
    S=3; FP=""; [ $wl = cascade ] && FP="--frames-per-step 64"; [ $wl = ffp15 ] && S=2; [ $wl = sdm ] && FP="--frames-per-step 2"; [ $wl = hog_svm ] && FP="--frames-per-step 4"
    CMD="$B --workload $wl --also none --steps $S --warmup 1 $FP --no-cpu-baseline"
    i=0
    for grp in "SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAVES GRBM_GUI_ACTIVE" \
               "SQ_ACTIVE_INST_ANY SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_ACTIVE_INST_LDS SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INSTS_VMEM_RD SQ_VALU_MFMA_BUSY_CYCLES" \
               "FETCH_SIZE" "WRITE_SIZE"; do
      i=$((i+1))
      timeout 300 rocprofv3 --kernel-trace --pmc $grp --output-format csv -d $O/pmc_${wl}_$i -- $CMD > /dev/null 2> $O/pmc_${wl}_$i.err
    done
    K=k_wvm; [ $wl = sdm ] && K=k_sdm_descriptors; [ $wl = hog_svm ] && K=k_svm_rbf_mfma
    python $R/tools/pmc_summary.py $wl $O/r02_pmc.json $K "rocprofv3 --kernel-trace --pmc <group> (4 separate passes) -- python bench.py --workload $wl --also none --steps $S --warmup 1 $FP --no-cpu-baseline; git head $HEAD" $O/pmc_${wl}_1 $O/pmc_${wl}_2 $O/pmc_${wl}_3 $O/pmc_${wl}_4 > $O/pmc_$wl.summary 2>&1
  done
fi
ls $O | head -50
cat $O/bench_default.json 2>/dev/null | head -c 6000
