// Field pairs (i < j) in itertools.combinations(range(F), 2) order, the order every pair-wise layer of the reference enumerates
// them in: pair index <-> (i, j), on the device.  (ffm_kernels.hip keeps its own ffm_pair_of: it works in int and is not the same function.)
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace dctr {

// first pair index of row i
__device__ __forceinline__ int64_t pair_row_start(int64_t i, int F) { return i * (2 * (int64_t)F - i - 1) / 2; }

// the pair at index p: the root of the quadratic as a guess, corrected against the exact row starts
__device__ inline void pair_at(int64_t p, int F, int* pi, int* pj) {
    const double b = 2.0 * F - 1.0;
    int64_t i = (int64_t)((b - sqrt(b * b - 8.0 * (double)p)) * 0.5);
    if (i < 0) i = 0;
    if (i > F - 2) i = F - 2;
    while (i > 0 && pair_row_start(i, F) > p) --i;
    while (i < F - 2 && pair_row_start(i + 1, F) <= p) ++i;
    *pi = (int)i;
    *pj = (int)(p - pair_row_start(i, F) + i + 1);
}

}  // namespace dctr
