#!/bin/bash
# dev tool: the library from the sources in the tree with extra compile flags, as libobca_mpc_<name>.so next to the product
# library (git-ignored); __graft_entry__.build() with these flags, so the objects live in csrc/_build under the flag set's
# own directory.  OBCA_LIB=libobca_mpc_<name>.so selects it in tools/gpu_variant_bench.py, gpu_cmp_builds.py, gpu_prof.py.
# Every translation unit of the product build (__graft_entry__.HIP_SOURCES): the package loads no library that lacks one of
# its exports.
#   tools/build_variant.sh prof -DOBCA_PROFILE        per-phase shader-clock counters (tools/gpu_prof.py)
#   tools/build_variant.sh straight -DOBCA_LOOP_R4=false -DOBCA_LOOP_R56=false     form of the ladder's passes per kernel (csrc/obca_kernel.hip: solve_passes)
#   tools/build_variant.sh cnt -DOBCA_PROFILE -DOBCA_MATH_COUNT       calls of the out-of-line math per iteration (OBCA_MATH_COUNT=1 tools/gpu_prof.py)
#   tools/build_variant.sh liblog -DOBCA_LIBRARY_LOG / sepsc -DOBCA_SEPARATE_SINCOS     the library's log() / separate sin() and cos() back (csrc/obca_kernel.hip: dlog, dsincos)
set -e
NAME=$1; shift
python "$(dirname "$0")/../__graft_entry__.py" variant "$NAME" -- "$@"
