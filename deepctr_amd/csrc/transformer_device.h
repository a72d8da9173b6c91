// Device pieces of the Transformer block that the forward (transformer_kernels.hip) and the backward (transformer_bwd_kernels.hip)
// share: the backward recomputes a layer with exactly these functions, so its recomputed activations are the forward's bits.
#pragma once
#include <math.h>
#include "dctr_common.h"
#include "mfma_tile.h"

namespace {

constexpr int TF_THREADS = 256;
constexpr int TF_WAVES = TF_THREADS / 64;
constexpr int TF_DC = 16;                       // output columns of one head a thread accumulates per pass over the keys
constexpr int TF_MAX_S = 16;
constexpr size_t TF_LDS_TARGET = 80 * 1024;
constexpr int TF_NW = 9;                        // pointers per layer: query, key, value, fw1, fw2, ln_gamma, ln_beta, pe_q, pe_k
constexpr float TF_NEG = -4294967295.f;         // -2^32 + 1 (rounds to -2^32 in fp32, as the reference's constant does)

__device__ __forceinline__ float tf_dot(const float* a, const float* b, int n) {
    float s = 0.f;
    for (int c = 0; c < n; ++c) s = fmaf(a[c], b[c], s);
    return s;
}

// LayerNormalization over the E columns of every row of A: one wave per row
__device__ __forceinline__ void tf_layer_norm(float* A, int rows, int ldx, int E, const float* __restrict__ gamma,
                                              const float* __restrict__ beta, float eps) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int r = wave; r < rows; r += TF_WAVES) {
        float* row = A + r * ldx;
        float s = 0.f;
        for (int c = lane; c < E; c += 64) s += row[c];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        const float mean = s / (float)E;
        float v = 0.f;
        for (int c = lane; c < E; c += 64) {
            const float t = row[c] - mean;
            v = fmaf(t, t, v);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        const float sd = sqrtf(v / (float)E + eps);
        for (int c = lane; c < E; c += 64) row[c] = (row[c] - mean) / sd * gamma[c] + beta[c];
    }
}

// Q = Xq Wq, K = Xk Wk, V = Xk Wv: one 16 x 16 output tile per wave task
__device__ __forceinline__ void tf_project_qkv(const float* A, const float* Bk, float* Qb, float* Kb, float* Vb, const float* const* W,
                                               int RT, int CT, int ST, int E, int KQ, int ldx, int ldq) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int t = wave; t < RT * CT * 3; t += TF_WAVES) {
        const int m = t % 3, rest = t / 3, ct = rest % CT, rt = rest / CT;
        dctr::f32x4 acc[1] = {{0.f, 0.f, 0.f, 0.f}};
        dctr::tile_gemm_kn<1>((m == 0 ? A : Bk) + rt * 16 * ldx, ldx, E, KQ, W[m], E, ct * 16, acc);
        float* dst = m == 0 ? Qb : m == 1 ? Kb : Vb;
        const int col = ct * 16 + (lane & 15), row0 = rt * 16 + 4 * (lane >> 4);
        if (col < E) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (row0 + r < ST) dst[(row0 + r) * ldq + col] = acc[0][r];
        }
    }
}

// attention + query mask + residual of the (row, head) items of nvalid samples, written over Xq (A).  STATS: the row's max and
// query mask / sum go to stats[(row * H + h) * 3 + {0, 1}] for the backward.
template <bool STATS>
__device__ __forceinline__ void tf_attention(float* A, const float* Qb, const float* Kb, const float* Vb, const float* qm, const float* km,
                                             int nvalid, int T, int H, int d, int ldx, int ldq, int blinding, int use_res, float sqrt_d,
                                             float* stats) {
    const float NEG = TF_NEG;
    for (int it = threadIdx.x; it < nvalid * T * H; it += TF_THREADS) {
        const int h = it % H, row = it / H, s = row / T, tq = row - s * T;
        const float* q = Qb + row * ldq + h * d;
        const float* kb = Kb + s * T * ldq + h * d;
        const float* vb = Vb + s * T * ldq + h * d;
        const float* kmask = km + s * T;
        const int blind = blinding ? tq : -1;
        float mx = -INFINITY;
        for (int j = 0; j < T; ++j) {
            float sc = tf_dot(q, kb + j * ldq, d) / sqrt_d;
            if (kmask[j] == 0.f || j == blind) sc = NEG;
            mx = fmaxf(mx, sc);
        }
        const float qmask = qm[row];
        for (int c0 = 0; c0 < d; c0 += TF_DC) {
            float acc[TF_DC];
#pragma unroll
            for (int c = 0; c < TF_DC; ++c) acc[c] = 0.f;
            float sum = 0.f;
            for (int j = 0; j < T; ++j) {
                float sc = tf_dot(q, kb + j * ldq, d) / sqrt_d;
                if (kmask[j] == 0.f || j == blind) sc = NEG;
                const float e = __expf(sc - mx);
                sum += e;
                const float* vj = vb + j * ldq + c0;
#pragma unroll
                for (int c = 0; c < TF_DC; ++c)
                    if (c0 + c < d) acc[c] = fmaf(e, vj[c], acc[c]);
            }
            const float inv = qmask / sum;
            if constexpr (STATS) {
                stats[it * 3] = mx;
                stats[it * 3 + 1] = inv;
            }
            float* xo = A + row * ldx + h * d + c0;
#pragma unroll
            for (int c = 0; c < TF_DC; ++c) {
                if (c0 + c < d) {
                    float o = acc[c] * inv;
                    if (use_res) o += xo[c];
                    xo[c] = o;
                }
            }
        }
    }
}

}  // namespace
