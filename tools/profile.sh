#!/bin/bash
# rocprofv3 evidence of a round (run on the MI355X box through gpurun): kernel trace + stats of the default bench, then the
# counter passes -- each --pmc pass in its OWN run, never combined with trace domains other than --kernel-trace.
# Every step runs under its own time limit and the first one that fails ends the run: nothing more is started on the card.
# Outputs under gpurun_out/prof_<tag>/; tools/pmc_summary.py <tag> condenses them into profiles/.
#   gpurun -- 'bash tools/profile.sh r04'   then here:   python tools/pmc_summary.py r04
# PROFILE_TARGETS="c2 c5" limits the counter passes, PROFILE_BENCH_ARGS replaces the traced bench's arguments (default: the
# --full run, up to seven minutes).  PROFILE_STEPS="trace pmc attrib" chooses the steps (default: all three); with
# OBCA_LIB=<dev build> (tools/build_variant.sh) the counter passes measure that build, e.g. the parent's:
#   OBCA_LIB=libobca_mpc_base.so PROFILE_STEPS=attrib bash tools/profile.sh r20base
set -u
TAG=${1:-r04}
OUT=$PWD/gpurun_out/prof_$TAG
mkdir -p $OUT
export TMPDIR=/tmp
REPO=$PWD
cd /tmp
run() { (cd $REPO && "$@"); }
STEPS=${PROFILE_STEPS:-trace pmc attrib}
has() { case " $STEPS " in *" $1 "*) return 0;; esac; return 1; }
# 1. kernel trace + stats of the bench itself (the roofline figures of bench.py come from the same command)
has trace && { (cd $REPO && timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace -o $TAG -- python bench.py ${PROFILE_BENCH_ARGS:---steps 4 --warmup 1 --full --no-cpu-baseline} > $OUT/bench_under_rocprof.json 2> $OUT/bench_under_rocprof.err) || { echo "bench under rocprofv3 failed"; exit 1; }; }
# 2. counter passes on the dominant kernels only
has pmc && for tgt in ${PROFILE_TARGETS:-c2 c5 c3g}; do
  for ctr in FETCH_SIZE WRITE_SIZE "SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_INSTS_VALU SQ_WAVES"; do
    name=$(echo $ctr | tr ' ' '_' | cut -c1-40)
    (cd $REPO && timeout -k 10 400 rocprofv3 --kernel-trace --pmc $ctr --output-format csv -d $OUT/pmc_${tgt}_$name -o $TAG -- python tools/gpu_profile_targets.py $tgt 3 > $OUT/pmc_${tgt}_$name.log 2>&1) || { echo "pass $tgt $name failed"; exit 1; }
  done
done
# 3. where the headline kernel's waits come from: instruction fetch (the iteration loop is larger than the instruction cache)
# and LDS.  Groups of their own, one pass each, headline kernel only; SQ_WAIT_INST_ANY and SQ_WAVE_CYCLES ride with the LDS
# group so that the LDS share of the waits comes from one pass.
has attrib && for ctr in "SQC_ICACHE_REQ SQC_ICACHE_HITS SQC_ICACHE_MISSES SQ_IFETCH" "SQ_WAIT_INST_LDS SQ_INSTS_LDS SQ_ACTIVE_INST_LDS SQ_LDS_BANK_CONFLICT SQ_WAIT_INST_ANY SQ_WAVE_CYCLES"; do
  name=$(echo $ctr | tr ' ' '_' | cut -c1-40)
  (cd $REPO && timeout -k 10 400 rocprofv3 --kernel-trace --pmc $ctr --output-format csv -d $OUT/pmc_c2_$name -o $TAG -- python tools/gpu_profile_targets.py c2 3 > $OUT/pmc_c2_$name.log 2>&1) || { echo "pass c2 $name failed"; tail -5 $OUT/pmc_c2_$name.log; exit 1; }
done
ls $OUT
