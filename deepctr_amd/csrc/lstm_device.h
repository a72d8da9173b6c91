// What the BiLSTM forward (lstm_kernels.hip) and its backward (lstm_bwd_kernels.hip) share: the step's four-gate GEMM on the f32
// matrix cores, the recurrent gate, and the LDS row pitches of the tiles and of a resident weight matrix.  The backward recomputes
// the gates with the forward's own arithmetic, so both read one definition.
#pragma once
#include <math.h>
#include <stdint.h>

#include "dctr_common.h"
#include "mfma_tile.h"

namespace dctr {

// acc[q][16 x 16] += A[16 x K] W[0:K, q u + cols] for the four gates q: mfma_tile.h's operand layout (k-slot g of a lane walks
// k = g KQ + t, A zero-padded to 4 KQ columns), W [K, 4u] with its own row pitch; the four accumulators are independent, so
// consecutive MFMAs never wait for each other.  MASKED: A is multiplied element by element with the tile M of A's layout (the
// input dropout of a training forward) on its way into the matrix core.
template <typename IDX, bool MASKED = false>
__device__ __forceinline__ void lstm_gemm4(const float* A, int lda, int K, int KQ, const float* W, int ldw, int u, int col,
                                           f32x4 (&acc)[4], const float* M = nullptr) {
    const int lane = threadIdx.x & 63, g = lane >> 4, j = lane & 15;
    const float* arow = A + j * lda + g * KQ;
    const float* wp = W + col;
    for (int t0 = 0; t0 < KQ; t0 += 4) {
        float4 a4 = *reinterpret_cast<const float4*>(arow + t0);
        if (MASKED) {
            const float4 m4 = *reinterpret_cast<const float4*>(M + j * lda + g * KQ + t0);
            a4.x *= m4.x; a4.y *= m4.y; a4.z *= m4.z; a4.w *= m4.w;
        }
        const float av[4] = {a4.x, a4.y, a4.z, a4.w};
        float b[4][4];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            const float* wr = wp + (IDX)min(g * KQ + t0 + tt, K - 1) * ldw;
#pragma unroll
            for (int q = 0; q < 4; ++q) b[tt][q] = wr[q * u];
        }
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[tt], b[tt][q], acc[q], 0, 0, 0);
        }
    }
}

__device__ __forceinline__ float lstm_gate(float z, int hard) {
    return hard ? fminf(fmaxf(fmaf(0.2f, z, 0.5f), 0.f), 1.f) : sigmoidf_(z);
}

// row pitch >= n of a weight matrix in LDS: the k-slot groups g and g + 1 of a B-operand read (one ds_read_b32 serves 32 lanes = two
// groups, KQ rows apart) land 16 banks apart when KQ * pitch = 16 (mod 32)
static inline int lstm_pitch(int n, int KQ) {
    for (int p = n; p < n + 32; ++p)
        if (((int64_t)KQ * p) % 32 == 16) return p;
    return n;
}

// pitches of a [16, n] tile that is an A operand (n padded to the MFMA's 16 and 4 floats on: rows 4 banks apart), its k-slot
// length, and the pitch of the cell-state tile (odd)
struct LstmPitch {
    int ldx, ld, ldc, KQx, KQh, ldw0, ldw, ldwh;
};
static inline LstmPitch lstm_pitches(int64_t Din, int64_t u) {
    LstmPitch p;
    const int padx = (int)((Din + 15) & ~(int64_t)15), padu = (int)((u + 15) & ~(int64_t)15);
    p.ldx = padx + 4;
    p.ld = padu + 4;
    p.ldc = (int)u | 1;
    p.KQx = padx >> 2;
    p.KQh = padu >> 2;
    p.ldw0 = lstm_pitch((int)(4 * u), p.KQx);
    p.ldw = p.ldwh = lstm_pitch((int)(4 * u), p.KQh);
    return p;
}

}  // namespace dctr
