#!/bin/bash
# dev tool: the library from the sources in the tree with extra compile flags, as libobca_mpc_<name>.so next to the product
# library (git-ignored); objects under /tmp.  OBCA_LIB=libobca_mpc_<name>.so selects it in tools/gpu_variant_bench.py,
# gpu_cmp_builds.py, gpu_prof.py.  Every translation unit of the product build (__graft_entry__.HIP_SOURCES): the package loads
# no library that lacks one of its exports.
#   tools/build_variant.sh prof -DOBCA_PROFILE        per-phase shader-clock counters (tools/gpu_prof.py)
#   tools/build_variant.sh straight -DOBCA_LOOP_R4=false -DOBCA_LOOP_R56=false     form of the ladder's passes per kernel (csrc/obca_kernel.hip: solve_passes)
set -e
NAME=$1; shift
cd "$(dirname "$0")/../vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd/csrc"
OBJ=/tmp/obca_variant_$NAME
rm -rf $OBJ; mkdir -p $OBJ
for f in $(python -c "import sys; sys.path.insert(0, '../..'); import __graft_entry__ as g; print(' '.join(s[:-4] for s in g.HIP_SOURCES))"); do
  hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=on -Wno-pass-failed "$@" -c $f.hip -o $OBJ/$f.o &
done
wait
g++ -shared -fPIC -o ../libobca_mpc_$NAME.so $OBJ/*.o -lm
ls -la ../libobca_mpc_$NAME.so
