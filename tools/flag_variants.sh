#!/bin/bash
# dev tool: compile ONLY the headline kernel's translation unit (obca_kernel_s5_3_6.hip) with extra backend flags, link it with the
# product's other objects into libobca_mpc_<name>.so (git-ignored) for an A/B on the GPU (tools/ab_run.sh);
# __graft_entry__.build(only=...), one variant after the other.
#   tools/flag_variants.sh name1 "flags1" name2 "flags2" ...
set -e
while [ $# -ge 2 ]; do
  NAME=$1; FLAGS=$2; shift 2
  python "$(dirname "$0")/../__graft_entry__.py" variant "$NAME" --only obca_kernel_s5_3_6 -- $FLAGS
done
