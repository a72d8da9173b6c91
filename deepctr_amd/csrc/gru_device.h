// What the DynamicGRU forward (gru_kernels.hip) and its backward (gru_bwd_kernels.hip) share: the step's two-part GEMM on the f32
// matrix cores and the LDS row pitch of a resident weight matrix.  The backward recomputes the gates and the candidate with the
// forward's own arithmetic, so both read one definition.
#pragma once
#include <stdint.h>

#include "mfma_tile.h"

namespace dctr {

// C[16 x 16] = A1[16 x E] W[0:E, cols] + A2[16 x E] W[E:2E, cols]: mfma_tile.h's operand layout (k-slot g of a lane walks
// k = g KQ + t, A zero-padded to 4 KQ columns), W with its own row pitch, two accumulators so that consecutive MFMAs do not depend
template <typename IDX>
__device__ __forceinline__ f32x4 gru_gemm(const float* A1, const float* A2, int lda, int E, int KQ, const float* W, int ldw, int N,
                                          int n_base) {
    const int lane = threadIdx.x & 63, g = lane >> 4, j = lane & 15;
    const float* wcol = W + min(n_base + j, N - 1);
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int part = 0; part < 2; ++part) {
        const float* arow = (part ? A2 : A1) + j * lda + g * KQ;
        const float* wp = wcol + (IDX)(part * E) * ldw;
        for (int t0 = 0; t0 < KQ; t0 += 4) {
            const float4 a4 = *reinterpret_cast<const float4*>(arow + t0);
            float b[4];
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) b[tt] = wp[(IDX)min(g * KQ + t0 + tt, E - 1) * ldw];
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.x, b[0], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.y, b[1], acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.z, b[2], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.w, b[3], acc1, 0, 0, 0);
        }
    }
    return acc0 + acc1;
}

// row pitch >= n of a weight matrix in LDS: the k-slot groups g and g + 1 of a B-operand read (one ds_read_b32 serves 32 lanes = two
// groups, KQ rows apart) land 16 banks apart when KQ * pitch = 16 (mod 32)
static inline int gru_pitch(int n, int KQ) {
    for (int p = n; p < n + 32; ++p)
        if (((int64_t)KQ * p) % 32 == 16) return p;
    return n;
}

}  // namespace dctr
