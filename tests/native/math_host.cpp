// CPU build of the solver's elementary functions (csrc/obca_math.h) -- tests only.
#include "../../vehicle_motion_planning_with_obstacles_avoidance_using_mpc_amd/csrc/obca_math.h"

extern "C" void math_host_log(long long n, const double* in, double* out) {
    for (long long i = 0; i < n; ++i) out[i] = obca_log(in[i]);
}
