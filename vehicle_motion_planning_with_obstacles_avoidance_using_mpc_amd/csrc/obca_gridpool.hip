// obca_gridpool.hip -- obca_grid_pool of include/obca_mpc.h: B occupancy grids -> B scene pools of axis-parallel rectangles,
// the inverse of obca_rasterise_batch.  The cover, the rows of a rectangle and the spare slots are defined in
// csrc/obca_gridpool_core.h; the kernel reproduces that serial definition integer for integer.
//
// Layout: one wavefront (= one block of 64) per map.  Dynamic LDS holds the map as rows * W 64-bit words (W = ceil(cols/64),
// at most 4096 words = 32 KB) followed by the K rectangles found (K x 4 int32).
//   load   for each row and each 64-column word, __ballot(byte != 0) IS the word; lanes beyond cols ballot 0 and form no address.
//   cover  wave-uniform; every step is a bit operation spread over the lanes, no atomics:
//            seed    the first non-zero word in row-major order: lanes test 64 words at a time, a ballot and a count of
//                    trailing zeros find it.  Words before the last seed's word stay zero, so the scan resumes there.
//            run     the trailing ones from the seed bit, continued into the next word of the row while a word is exhausted
//            height  lane j tests row r + 1 + j against the run's mask, all of its words; the first failing lane of the ballot
//                    is the height; rows beyond the grid fail; repeated in chunks of 64 rows
//            clear   the rectangle's rows spread over the lanes
//          Every seed clears its own bit at least, so the loop ends after `count` steps.
//   emit   lane k < K writes slot k: four 16-byte stores for pool_A, four words of pool_b, the rect; spare slots included.
//          Lane 0 writes count and ok.
// The block is one wavefront, so __syncthreads() between a step's LDS writes and the next step's reads costs no waiting on
// another wavefront; all control flow around it is wave-uniform.
#include <hip/hip_runtime.h>
#include "obca_device.h"
#include "obca_gridpool_core.h"

namespace {

constexpr int WAVE = 64;

struct GridPoolArgs {
    int32_t rows, cols, K;
    double res, pad, far;
    const uint8_t* grid;
    double *pool_A, *pool_b;
    int32_t *rect, *count, *ok;
};

// the bits of columns lo_c .. hi_c (both inside word w of the row) that fall into word w
__device__ inline uint64_t run_mask(int w, int c0, int c1) {
    const int lo = (c0 >> 6) == w ? (c0 & 63) : 0, hi = (c1 >> 6) == w ? (c1 & 63) : 63;
    return (~0ull >> (63 - hi)) & (~0ull << lo);
}

__global__ void __launch_bounds__(WAVE) gridpool_kernel(GridPoolArgs P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x, rows = P.rows, cols = P.cols, K = P.K;
    const int W = gridpool::words_per_row(cols), nwords = rows * W;
    uint64_t* bits = reinterpret_cast<uint64_t*>(smem);
    int32_t* s_rect = reinterpret_cast<int32_t*>(smem + (size_t)nwords * 8);
    const int64_t inst = blockIdx.x;
    const uint8_t* g = P.grid + inst * rows * cols;

    // load
    for (int q = 0; q < nwords; ++q) {
        const int r = q / W, c = (q - r * W) * 64 + lane;
        const bool occ = c < cols && g[(int64_t)r * cols + c] != 0;
        const uint64_t m = __ballot(occ);
        if (lane == (q & 63)) bits[q] = m;
    }
    __syncthreads();

    // cover
    int n = 0, pos = 0;
    for (;;) {
        int first = -1;
        for (int base = pos; base < nwords; base += WAVE) {
            const int q = base + lane;
            const uint64_t m = __ballot(q < nwords && bits[q] != 0);
            if (m != 0) { first = base + __builtin_ctzll(m); break; }
        }
        if (first < 0) break;
        const int r = first / W, w0 = first - r * W;
        uint64_t wv = bits[first];                                   // the same word in every lane
        const int bit = __builtin_ctzll(wv);
        const int c0 = w0 * 64 + bit;
        // run: ones from the seed bit; zeros shifted in from above end it inside the word unless bit == 0 and the word is full
        uint64_t inv = ~(wv >> bit);
        int len = inv != 0 ? __builtin_ctzll(inv) : 64, w = w0;
        while (bit + len == (w - w0 + 1) * 64 && w + 1 < W) {        // exhausted word w: continue in word w + 1
            ++w;
            inv = ~bits[r * W + w];
            const int more = inv != 0 ? __builtin_ctzll(inv) : 64;
            len += more;
            if (more < 64) break;
        }
        const int c1 = c0 + len - 1, w1 = c1 >> 6;
        // height
        int r1 = r;
        for (;;) {
            const int row = r1 + 1 + lane;
            bool okrow = row < rows;
            if (okrow)
                for (int q = w0; q <= w1; ++q) {
                    const uint64_t mk = run_mask(q, c0, c1);
                    okrow = okrow && (bits[row * W + q] & mk) == mk;
                }
            const uint64_t fail = __ballot(!okrow);
            if (fail != 0) { r1 += __builtin_ctzll(fail); break; }
            r1 += WAVE;
        }
        __syncthreads();                                             // every lane has read before any lane clears
        for (int row = r + lane; row <= r1; row += WAVE)
            for (int q = w0; q <= w1; ++q) bits[row * W + q] &= ~run_mask(q, c0, c1);
        if (n < K && lane == 0) { s_rect[4 * n] = r; s_rect[4 * n + 1] = c0; s_rect[4 * n + 2] = r1; s_rect[4 * n + 3] = c1; }
        ++n;
        pos = first;
        __syncthreads();
    }
    __syncthreads();

    // emit
    if (lane < K) {
        double A[8], b[4];
        int32_t q[4];
        gridpool::slot(lane, n, s_rect, P.res, P.pad, P.far, A, b, q);
        const int64_t s = inst * K + lane;
        double2* Ao = reinterpret_cast<double2*>(P.pool_A + s * 8);
        for (int j = 0; j < 4; ++j) Ao[j] = make_double2(A[2 * j], A[2 * j + 1]);
        for (int j = 0; j < 4; ++j) P.pool_b[s * 4 + j] = b[j];
        if (P.rect)
            for (int j = 0; j < 4; ++j) P.rect[s * 4 + j] = q[j];
    }
    if (lane == 0) {
        P.count[inst] = n;
        P.ok[inst] = n <= K ? 1 : 0;
    }
}

}  // namespace

extern "C" int obca_grid_pool(const uint8_t* grid, int32_t B, int32_t rows, int32_t cols, int32_t K, double resolution, double pad,
                              double far, double* pool_A, double* pool_b, int32_t* rect, int32_t* count, int32_t* ok,
                              int32_t device, void* hip_stream) {
    // every argument is checked before the first HIP call: a refused call has no side effect
    if (gridpool::args_check(B, rows, cols, K, resolution, pad, far, grid, pool_A, pool_b, count, ok) != 0 || device < 0)
        return OBCA_E_INVAL;
    GridPoolArgs P;
    P.rows = rows; P.cols = cols; P.K = K; P.res = resolution; P.pad = pad; P.far = far;
    P.grid = grid; P.pool_A = pool_A; P.pool_b = pool_b; P.rect = rect; P.count = count; P.ok = ok;
    const size_t lds = (size_t)rows * gridpool::words_per_row(cols) * 8 + (size_t)K * 4 * sizeof(int32_t);      // <= 32 KB + 1 KB
    ObcaDeviceGuard guard(device);
    if (!guard.ok) return OBCA_E_HIP;
    hipLaunchKernelGGL(gridpool_kernel, dim3((unsigned)B), dim3(WAVE), lds, (hipStream_t)hip_stream, P);
    return hipGetLastError() == hipSuccess ? OBCA_OK : OBCA_E_HIP;
}
