// What dctr_ifm_fwd (ifm_kernels.hip) and dctr_ifm_bwd (ifm_bwd_kernels.hip) share: the tile constants of the MFMA passes and the
// wave reductions of the row passes.
#pragma once
#include <math.h>
#include <stdint.h>
#include "dctr_common.h"
#include "tile_route.h"

namespace dctr_ifm {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int IFM_THREADS = 256;
constexpr int IFM_ROWS = 16;                      // samples of a wave
constexpr int IFM_WG_ROWS = 64;                   // samples of a workgroup
constexpr int IFM_KC = 64;                        // source columns per LDS chunk
constexpr int IFM_APITCH = IFM_KC + 4;            // bank = 4 * row + k-slot: the 64 operand reads of an MFMA hit 64 banks
constexpr int IFM_SMALL_WG_BELOW = 2;             // one-wave workgroups while four-wave ones would number fewer than this many per CU

__device__ __forceinline__ float ifm_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ float ifm_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// the lanes of a row pass: power of two >= min(d, 64)
static inline int ifm_group_lanes(int d) {
    int dp = 1;
    while (dp < d && dp < 64) dp <<= 1;
    return dp;
}

}  // namespace dctr_ifm
