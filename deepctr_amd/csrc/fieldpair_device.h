// What the FEFM forward (fieldpair_kernels.hip) and backward (fieldpair_bwd_kernels.hip) share on the device: the X tile's layout
// and swizzle, and the fetch of a pair's weight matrix at E <= 16.  The backward loads the same tile as the forward; this header is
// what makes "the same" hold.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mfma_tile.h"

namespace dctr {

// X [F][16 M][ldx]: rows are stored without padding, the 16-B chunks of a row XOR-swizzled by (s >> 1) & 3.
// float offset of 16-B chunk `chunk` of sample row s inside one field of X (rows of ldx floats, ldx % 16 == 0)
__device__ __forceinline__ int fp_xoff(int s, int chunk, int ldx) { return s * ldx + ((chunk ^ ((s >> 1) & 3)) << 2); }
// float offset of element k of sample row s
__device__ __forceinline__ int fp_xel(int s, int k, int ldx) { return fp_xoff(s, k >> 2, ldx) + (k & 3); }

// the weight matrices are in global memory: a pointer read back from the LDS table is generic to the compiler, and a generic (flat)
// load counts against the LDS counter as well, which would tie every ds_read wait to the L2 round trip
typedef const __attribute__((address_space(1))) float* fp_gptr;
typedef const __attribute__((address_space(1))) f32x4* fp_gptr4;

// the S operands of Q pairs at E <= 16, before the add: row[q][tt] = W[c][4g + tt], col[q][tt] = W[4g + tt][c] (indices clamped:
// the product meets zero padding of X there)
template <int Q>
struct FpRaw {
    float row[Q][4], col[Q][4];
};

// fetches the matrices wp[q0 .. q0 + Q - 1] (the table has np entries; a task's pairs past it repeat the last)
template <int Q>
__device__ __forceinline__ void fp_load_small(const float* const* wp, int q0, int np, int E, bool vec, FpRaw<Q>& raw) {
    const int lane = threadIdx.x & 63, g = lane >> 4, c = min(lane & 15, E - 1);
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const fp_gptr w = (fp_gptr)wp[min(q0 + q, np - 1)];
        if (vec && ((uintptr_t)w & 15) == 0) {
            const f32x4 t = *(fp_gptr4)(w + c * E + min(4 * g, E - 4));
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) raw.row[q][tt] = t[tt];
        } else {
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) raw.row[q][tt] = w[c * E + min(4 * g + tt, E - 1)];
        }
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) raw.col[q][tt] = w[min(4 * g + tt, E - 1) * E + c];
    }
}

}  // namespace dctr
