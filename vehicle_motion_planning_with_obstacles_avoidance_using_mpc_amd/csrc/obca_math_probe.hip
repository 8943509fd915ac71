// obca_math_probe.hip -- test hook: the solver's elementary functions (csrc/obca_math.h) and the device library's, evaluated
// on a device array, so that the tests can hold the device's obca_log against the host build's and the shared-reduction
// sine / cosine against the separate calls, word for word.  Not part of the C ABI of include/obca_mpc.h; the binding is
// _lib.math_probe().  One lane per element, no LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "obca_device.h"
#include "obca_math.h"

namespace {

constexpr int BLOCK = 256;

// kind 0: out[i] = obca_log(in[i]);  1: out[i] = log(in[i]) of the device library;
// kind 2: out[2 i], out[2 i + 1] = sine, cosine by obca_sincos (what dsincos of csrc/obca_kernel.hip calls);  3: by sin() and cos()
__global__ void __launch_bounds__(BLOCK) math_probe_kernel(int kind, int64_t n, const double* in, double* out) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const double x = in[i];
    if (kind == 0) out[i] = obca_log(x);
    else if (kind == 1) out[i] = log(x);
    else if (kind == 2) { double s, c; obca_sincos(x, &s, &c); out[2 * i] = s; out[2 * i + 1] = c; }
    else { out[2 * i] = sin(x); out[2 * i + 1] = cos(x); }
}

}  // namespace

// in: n doubles; out: n doubles (kinds 0, 1) or 2 n (kinds 2, 3).  Every argument is checked before the first HIP call.
extern "C" int obca_math_probe(int32_t kind, int64_t n, const double* in, double* out, int32_t device, void* hip_stream) {
    if (kind < 0 || kind > 3 || n < 1 || n > (1 << 24) || !in || !out || device < 0) return OBCA_E_INVAL;
    ObcaDeviceGuard guard(device);
    if (!guard.ok) return OBCA_E_HIP;
    const int64_t blocks = (n + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(math_probe_kernel, dim3((unsigned)blocks), dim3(BLOCK), 0, (hipStream_t)hip_stream, (int)kind, n, in, out);
    return hipGetLastError() == hipSuccess ? OBCA_OK : OBCA_E_HIP;
}
