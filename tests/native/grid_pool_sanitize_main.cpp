// Stand-alone sanitizer run of the grid-to-pool core (csrc/obca_gridpool_core.h through grid_pool_host.cpp) -- no test, run
// by hand:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all
//       tests/native/grid_pool_sanitize_main.cpp -o grid_pool_sanitize && ./grid_pool_sanitize
// Every buffer is a heap allocation of exactly the size the call may touch, so that a read or write one element outside it is
// reported: the smallest shape (1 x 1, K = 1; occupied and empty) and 130 x 129 with K = 64 (three words per row, the last
// holding one column; more than two chunks of 64 rows) on three maps: full, a checkerboard that overflows K, and random.
// Prints "grid pool sanitize ok" and returns 0 when the outputs are also what they must be.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "grid_pool_host.cpp"

template <class T> static T* heap(size_t n) { return (T*)std::malloc(n * sizeof(T)); }

static int run(const uint8_t* src, int B, int rows, int cols, int K, const int* want_count) {
    const size_t cells = (size_t)B * rows * cols, slots = (size_t)B * K;
    uint8_t* grid = heap<uint8_t>(cells);
    std::memcpy(grid, src, cells);
    double *A = heap<double>(slots * 8), *b = heap<double>(slots * 4);
    int *rect = heap<int>(slots * 4), *count = heap<int>(B), *ok = heap<int>(B);
    int bad = grid_pool_host(grid, B, rows, cols, K, 1.0, 0.5, 100.0, A, b, rect, count, ok);
    for (int i = 0; i < B && !bad; ++i) {
        if (want_count[i] >= 0 && count[i] != want_count[i]) bad = 10;
        if (ok[i] != (count[i] <= K ? 1 : 0)) bad = 11;
        // the rectangles written cover occupied cells only, and all of them where ok
        long area = 0, occupied = 0;
        for (int q = 0; q < rows * cols; ++q) occupied += grid[(size_t)i * rows * cols + q] != 0;
        for (int k = 0; k < K; ++k) {
            const int* q = rect + ((size_t)i * K + k) * 4;
            if (k >= count[i]) { if (q[0] != -1 || b[((size_t)i * K + k) * 4] != -100.0) bad = 12; continue; }
            if (q[0] < 0 || q[2] >= rows || q[1] < 0 || q[3] >= cols || q[2] < q[0] || q[3] < q[1]) { bad = 13; continue; }
            for (int r = q[0]; r <= q[2]; ++r)
                for (int c = q[1]; c <= q[3]; ++c)
                    if (grid[((size_t)i * rows + r) * cols + c] == 0) bad = 14;
            area += (long)(q[2] - q[0] + 1) * (q[3] - q[1] + 1);
        }
        if (ok[i] ? area != occupied : area >= occupied) bad = 15;
    }
    for (size_t q = 0; q < slots * 8 && !bad; ++q) if (std::isnan(A[q])) bad = 16;
    for (size_t q = 0; q < slots * 4 && !bad; ++q) if (std::isnan(b[q])) bad = 16;
    // rect may be NULL
    if (!bad && grid_pool_host(grid, B, rows, cols, K, 1.0, 0.0, 100.0, A, b, nullptr, count, ok) != 0) bad = 17;
    std::free(grid); std::free(A); std::free(b); std::free(rect); std::free(count); std::free(ok);
    return bad;
}

int main() {
    const uint8_t one[2] = {7, 0};
    const int c1[2] = {1, 0};
    int rc = run(one, 2, 1, 1, 1, c1);
    if (rc) return rc;
    const int rows = 130, cols = 129, cells = rows * cols;
    uint8_t* g = heap<uint8_t>((size_t)3 * cells);
    unsigned long long s = 2024;
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) {
            s = s * 6364136223846793005ull + 1442695040888963407ull;
            g[r * cols + c] = 1;
            g[cells + r * cols + c] = (r + c) & 1;
            g[2 * cells + r * cols + c] = (s >> 33) % 10 < 9;
        }
    const int c3[3] = {1, cells / 2, -1};
    rc = run(g, 3, rows, cols, 64, c3);
    std::free(g);
    if (rc) return 100 + rc;
    std::printf("grid pool sanitize ok\n");
    return 0;
}
