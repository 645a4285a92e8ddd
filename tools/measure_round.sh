#!/bin/bash
# Full measurement set of one build on the GPU box (run through gpurun; outputs under gpurun_out/):
#   tools/measure_round.sh TAG [default|s20w5|pickplace ...]      (no part given: all three)
# bench (Newton headline + PGS beside it + the pick_place leg + cpu_baseline), then per solver and per bench argument
# set -- bench.py's own default (--steps 200 --warmup 20) AND the driver's end-of-round arguments (--steps 20 --warmup 5)
# -- a kernel trace + stats and five separate PMC passes (FETCH_SIZE | WRITE_SIZE | SQ_* | SQ_INSTS_VALU_*_F32/F64 |
# MFMA ops); the same for the pick_place leg (stats + FETCH / WRITE / SQ).  Counter passes carry --kernel-trace only
# (never sys / runtime / hip / hsa traces) and run the SAME bench arguments as the line they annotate, so that per-launch
# counter means and the timed launch duration describe the same launches.  The raw per-dispatch CSVs are summarised ON
# THE BOX (tools/summarize_profiles.py / summarize_pickplace.py with PROFILES_OUT=gpurun_out/TAG_profiles) and deleted:
# copy gpurun_out/TAG_profiles/* into profiles/ afterwards.
set -e
T=$1; shift
PARTS="${*:-default s20w5 pickplace}"
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
export PROFILES_OUT=gpurun_out/${T}_profiles
mkdir -p $PROFILES_OUT
R=gpurun_out/${T}_raw
mkdir -p $R
passes() {  # solver K W [pertick]   (pertick: the window is shorter than the library's queue_min_ticks: one launch per tick and env group)
  S=$1; K=$2; W=$3; X=s${K}w${W}; PT=${4:-0}
  A="--solver $S --steps $K --warmup $W --no-cpu-baseline --no-second-window --no-pick-place"
  rocprofv3 --kernel-trace --stats --output-format csv -d $R/prof_${S}_$X -- python bench.py $A > $PROFILES_OUT/${T}_bench_under_rocprof_${S}_$X.json 2>/dev/null
  rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $R/fetch_${S}_$X -- python bench.py $A > /dev/null 2>&1
  rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $R/write_${S}_$X -- python bench.py $A > /dev/null 2>&1
  rocprofv3 --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_INSTS_LDS SQ_ACTIVE_INST_VALU SQ_WAIT_INST_LDS SQ_LDS_BANK_CONFLICT SQ_WAIT_ANY --kernel-trace --output-format csv -d $R/sq_${S}_$X -- python bench.py $A > /dev/null 2>&1
  rocprofv3 --pmc SQ_INSTS_VALU_ADD_F32 SQ_INSTS_VALU_MUL_F32 SQ_INSTS_VALU_FMA_F32 SQ_INSTS_VALU_TRANS_F32 SQ_INSTS_VALU_ADD_F64 SQ_INSTS_VALU_MUL_F64 SQ_INSTS_VALU_FMA_F64 SQ_INSTS_SALU --kernel-trace --output-format csv -d $R/flop_${S}_$X -- python bench.py $A > /dev/null 2>&1 || echo "flop counter pass failed for $S $X"
  rocprofv3 --pmc SQ_INSTS_VALU_MFMA_MOPS_F32 SQ_INSTS_MFMA SQ_INSTS_VMEM_RD SQ_INSTS_SMEM --kernel-trace --output-format csv -d $R/mfma_${S}_$X -- python bench.py $A > /dev/null 2>&1 || echo "mfma counter pass failed for $S $X"
  PER_TICK=$PT BENCH_STEPS=$K BENCH_WARMUP=$W MFMA_DIR=$R/mfma_${S}_$X python tools/summarize_profiles.py $T $S $R/prof_${S}_$X $R/fetch_${S}_$X $R/write_${S}_$X $R/sq_${S}_$X $R/flop_${S}_$X "round 5" > /dev/null
  if [ $PT = 1 ]; then python tools/trace_summary.py $R/prof_${S}_$X $([ $S = PGS ] && echo k_step || echo k_step_newton) $W > $PROFILES_OUT/${T}_launch_chain_${S}_$X.log 2>&1 || true
  else python tools/trace_summary.py $R/prof_${S}_$X $([ $S = PGS ] && echo k_step_queue || echo k_step_queue_newton) $([ $W -ge 8 ] && echo 1 || echo 0) > $PROFILES_OUT/${T}_launch_chain_${S}_$X.log 2>&1 || true; fi
  rm -rf $R/prof_${S}_$X $R/fetch_${S}_$X $R/write_${S}_$X $R/sq_${S}_$X $R/flop_${S}_$X $R/mfma_${S}_$X
  echo "passes done: $S $X"
}
for P in $PARTS; do
  case $P in
    default)
      python bench.py --full > $PROFILES_OUT/${T}_bench.json 2> $PROFILES_OUT/${T}_bench.err
      passes Newton 200 20; passes PGS 200 20 ;;
    s20w5)
      python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-pick-place > $PROFILES_OUT/${T}_bench_s20w5.json 2>/dev/null
      passes Newton 20 5 1; passes PGS 20 5 1 ;;
    pickplace)
      A="--pick-place-only --solver Newton"
      python bench.py $A > $PROFILES_OUT/${T}_bench_pickplace.json 2>/dev/null
      rocprofv3 --kernel-trace --stats --output-format csv -d $R/pp_stats -- python bench.py $A > /dev/null 2>&1
      rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $R/pp_fetch -- python bench.py $A > /dev/null 2>&1
      rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $R/pp_write -- python bench.py $A > /dev/null 2>&1
      rocprofv3 --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_INSTS_LDS SQ_ACTIVE_INST_VALU SQ_WAIT_INST_LDS SQ_LDS_BANK_CONFLICT SQ_WAIT_ANY --kernel-trace --output-format csv -d $R/pp_sq -- python bench.py $A > /dev/null 2>&1
      rocprofv3 --pmc SQ_INSTS_VALU_ADD_F32 SQ_INSTS_VALU_MUL_F32 SQ_INSTS_VALU_FMA_F32 SQ_INSTS_VALU_TRANS_F32 SQ_INSTS_VALU_ADD_F64 SQ_INSTS_VALU_MUL_F64 SQ_INSTS_VALU_FMA_F64 SQ_INSTS_VALU_MFMA_MOPS_F32 --kernel-trace --output-format csv -d $R/pp_flop -- python bench.py $A > /dev/null 2>&1 || echo "pickplace flop pass failed"
      python tools/summarize_pickplace.py $T $R/pp_stats $R/pp_fetch $R/pp_write $R/pp_sq $R/pp_flop > /dev/null
      rm -rf $R/pp_stats $R/pp_fetch $R/pp_write $R/pp_sq $R/pp_flop
      echo "passes done: pickplace" ;;
  esac
done
rmdir $R 2>/dev/null || true
ls -la $PROFILES_OUT
