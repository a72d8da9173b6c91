// Backward of the Transformer stack (transformer_kernels.hip; reference deepctr/layers/sequence.py:523-635): every layer, one
// persistent launch plus one launch that sums the workgroups' weight-gradient partials.  include/dctr.h states the math.
//
// A workgroup owns a tile of S samples, as the forward does.  Per layer, last to first, it
//   * reloads the layer's input (x for layer 0, the tape after it) and recomputes the layer with the forward's own device functions
//     (transformer_device.h: the MFMA projections, the two-pass attention walk, tf_layer_norm) and the forward's feed-forward loop, so
//     Xq, Xk, Q, K, V, the pre-LayerNorm rows a and f and the feed-forward input r are the forward's bits; the attention walk also
//     leaves the row's max and query mask / sum per (row, head);
//   * LayerNorm backward: a wave per row for mean / sd, a thread per column for d_gamma / d_beta, a wave per row for dx;
//   * feed-forward backward in groups of 64 rows: each wave rebuilds the [16, 4E] hidden slab h of its row tile and forms
//     dh = (df fw2^T) [h > 0] beside it, the four waves then share the output tiles of d_fw1 += r^T dh and d_fw2 += h^T df over the
//     group's 64 rows, and each wave adds dh fw1^T to its rows' gradient;
//   * attention backward, thread per (row, head), no [T, T] matrix: the query walk forms sum p~ dP (the third number of the row) and
//     dQ, the key walk dK and dV from the three numbers of every query row;
//   * d_query / d_key / d_value = X^T dY and dXq = dQ Wq^T (+ da), dXk = dK Wk^T + dV Wv^T; d_pe_q / d_pe_k; dXq + dXk is the
//     gradient of the layer before, or dx.
// Every matrix product is v_mfma_f32_16x16x4_f32 (exact fp32): Y W^T through tile_gemm_nk on the forward's weight layout, X^T dY
// through tfb_gemm_tn below (both operands read column-wise from the tile, k = the tile's rows).
// Weight gradients: a workgroup adds each tile's contribution to its own partial block [n_layers][P] at the head of its workspace
// slice (zeroed at the start of the launch; tiles in a fixed order), transformer_bwd_reduce_kernel adds the blocks in workgroup order
// onto d_layers.  No atomics: the same bits on every call.
//
// Cost model, FLOP per sample and layer (the forward's 22 T E^2 + 4 T^2 E recomputed, feed-forward hidden slab twice under
// LayerNorm: + 8 T E^2):  backward proper 2 x (6 T E^2 + 16 T E^2) matrix products (Y W^T and X^T dY) + attention 4 T^2 E (query walk:
// scores and dP twice) + 8 T^2 E (key walk) ~ 44 T E^2 + 12 T^2 E; with the recompute 66 .. 74 T E^2 + 16 T^2 E
//   (T 50, E 32: 2.25 + 0.96 = 3.21 MFLOP, ops.transformer_bwd_flops; + recompute 1.45 + 0.41 = 5.07 MFLOP, 3.5x the forward).
// Tile, floats: 6 pad16(S T) (pad16(E) + 4)  [Xq, Xk, a -> dQ, r -> dK, f -> dV, gradient]  +  3 S T (E | 1)  [Q, K, V]  +
//   2 min(64, pad16(S T)) (pad16(4E) + 4)  [h, dh]  +  3 S T H  [row numbers]  +  2 pad16(S T)  [LayerNorm mean, sd]  +  2 S T  [masks].
//   S: the largest <= 16 within the 160 KiB of a workgroup (at most 256 workgroups are launched, one per CU, so unlike the forward
//   nothing is kept free for a second one); a sample past that (or route GENERAL) takes S = 1 with the tile behind the partial block
//   in the workgroup's workspace slice.  T 50, E 32, H 8, S 1: 13,824 + 4,952 + 16,896 + 1,200 + 128 + 100 = 37,100 floats
//   = 145 KiB (one workgroup per CU).
#include <math.h>
#include "dctr_common.h"
#include "tile_route.h"
#include "mfma_tile.h"
#include "transformer_device.h"

namespace {

constexpr int TFB_MAX_LAYERS = DCTR_TRANSFORMER_BWD_MAX_LAYERS;
constexpr int TFB_GROUP = TF_WAVES * 16;        // rows of one feed-forward group: a 16-row tile per wave

struct TfbParams {
    const float* x;
    int64_t batch;
    int64_t x_stride, x_row_stride;
    int32_t T, E, d, H, n_layers;
    int32_t use_pe, use_res, use_ffn, use_ln, blinding, output_type;
    float sqrt_d, eps;
    int32_t S, ldx, ldq, ldh;
    int64_t part_floats;     // [n_layers][P] partial weight gradients at the head of a slice (0: no weight gradients asked)
    int64_t layer_floats;    // P
    int64_t slice_floats;    // a workgroup's workspace slice
    const int32_t* q_len;
    const int32_t* k_len;
    const uint8_t* q_mask;
    const uint8_t* k_mask;
    const float* W[TFB_MAX_LAYERS][TF_NW];
    const float* tape;
    const float* d_out;
    int64_t d_out_stride, d_out_row_stride;
    float* dx;
    int64_t dx_stride, dx_row_stride;
    int32_t accumulate;
    float* ws;
};

// offset of weight m's gradient inside a layer's partial block: query, key, value [E, E], fw1 [E, 4E], fw2 [4E, E], gamma, beta [E],
// pe_q, pe_k [T, E]; m == 9: the block's size P
__host__ __device__ inline int64_t tfb_off(int m, int64_t E, int64_t T) {
    const int64_t e2 = E * E;
    switch (m) {
        case 0: return 0;
        case 1: return e2;
        case 2: return 2 * e2;
        case 3: return 3 * e2;
        case 4: return 7 * e2;
        case 5: return 11 * e2;
        case 6: return 11 * e2 + E;
        case 7: return 11 * e2 + 2 * E;
        case 8: return 11 * e2 + 2 * E + T * E;
        default: return 11 * e2 + 2 * E + 2 * T * E;
    }
}

// C[16 x 16] = X[:, i0 .. i0+15]^T Y[:, j0 .. j0+15] over `rows` rows (a multiple of 16) of two row-major tiles: lane (i, g)
// supplies X[k0 + g][i0 + i] and Y[k0 + g][j0 + i]; two accumulators hide the MFMA's dependent latency.
__device__ __forceinline__ dctr::f32x4 tfb_gemm_tn(const float* X, int ldx, const float* Y, int ldy, int rows, int i0, int j0) {
    const int lane = threadIdx.x & 63, g = lane >> 4, j = lane & 15;
    const float* xp = X + g * ldx + i0 + j;
    const float* yp = Y + g * ldy + j0 + j;
    dctr::f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < rows; k0 += 8) {
        a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(xp[k0 * ldx], yp[k0 * ldy], a0, 0, 0, 0);
        a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(xp[(k0 + 4) * ldx], yp[(k0 + 4) * ldy], a1, 0, 0, 0);
    }
    return a0 + a1;
}

// dst[i0 + 4g + r][j0 + j] += acc[r] inside an [M, N] row-major partial
__device__ __forceinline__ void tfb_add_tile(float* dst, int M, int N, int i0, int j0, const dctr::f32x4& acc) {
    const int lane = threadIdx.x & 63, col = j0 + (lane & 15), row0 = i0 + 4 * (lane >> 4);
    if (col < N) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (row0 + r < M) dst[(int64_t)(row0 + r) * N + col] += acc[r];
    }
}

// LayerNorm backward over the rows of Xp (the rows LayerNorm read) with their gradient in G, replaced by the gradient of Xp.
// pg / pb: the workgroup's d_gamma / d_beta partials (nullptr: not asked).  Ends with a barrier.
__device__ __forceinline__ void tfb_layer_norm_bwd(const float* Xp, float* G, float* rstat, int rows, int ldx, int E,
                                                   const float* __restrict__ gamma, float eps, float* pg, float* pb) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int r = wave; r < rows; r += TF_WAVES) {        // mean and sd as tf_layer_norm forms them
        const float* row = Xp + r * ldx;
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
        if (lane == 0) {
            rstat[2 * r] = mean;
            rstat[2 * r + 1] = sqrtf(v / (float)E + eps);
        }
    }
    __syncthreads();
    if (pg) {
        for (int c = tid; c < E; c += TF_THREADS) {
            float sg = 0.f, sb = 0.f;
            for (int r = 0; r < rows; ++r) {
                const float g = G[r * ldx + c];
                sg = fmaf(g, (Xp[r * ldx + c] - rstat[2 * r]) / rstat[2 * r + 1], sg);
                sb += g;
            }
            pg[c] += sg;
            pb[c] += sb;
        }
        __syncthreads();
    }
    for (int r = wave; r < rows; r += TF_WAVES) {
        const float* row = Xp + r * ldx;
        float* grow = G + r * ldx;
        const float mean = rstat[2 * r], sd = rstat[2 * r + 1];
        float s1 = 0.f, s2 = 0.f;
        for (int c = lane; c < E; c += 64) {
            const float gh = grow[c] * gamma[c];
            s1 += gh;
            s2 = fmaf(gh, (row[c] - mean) / sd, s2);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            s1 += __shfl_xor(s1, o, 64);
            s2 += __shfl_xor(s2, o, 64);
        }
        const float m1 = s1 / (float)E, m2 = s2 / (float)E;
        for (int c = lane; c < E; c += 64) grow[c] = (grow[c] * gamma[c] - m1 - (row[c] - mean) / sd * m2) / sd;
    }
    __syncthreads();
}

template <bool GLOBAL_WS>
__global__ __launch_bounds__(TF_THREADS) void transformer_bwd_kernel(TfbParams p) {
    extern __shared__ __attribute__((aligned(16))) float tfb_lds[];
    float* part = p.ws + (int64_t)blockIdx.x * p.slice_floats;
    float* X = GLOBAL_WS ? part + p.part_floats : tfb_lds;
    const int S = p.S, T = p.T, E = p.E, d = p.d, H = p.H, ST = S * T, ldx = p.ldx, ldq = p.ldq, ldh = p.ldh;
    const int rows_pad = (ST + 15) & ~15, nbuf = rows_pad * ldx;
    float* Xk = X + nbuf;
    float* A1 = Xk + nbuf;       // a, the rows the first LayerNorm reads; dQ once they are spent
    float* R1 = A1 + nbuf;       // r, the feed-forward input; then dK
    float* F = R1 + nbuf;        // f, the rows the second LayerNorm reads; then dV
    float* G = F + nbuf;         // the gradient on its way down the layer
    float* Qb = G + nbuf;
    float* Kb = Qb + ST * ldq;
    float* Vb = Kb + ST * ldq;
    const int grows = min(TFB_GROUP, rows_pad);     // rows of the two hidden slabs
    float* Hs = Qb + ((3 * ST * ldq + 3) & ~3);
    float* DHs = Hs + grows * ldh;
    float* stats = DHs + grows * ldh;
    float* rstat = stats + ((3 * ST * H + 3) & ~3);
    float* qm = rstat + 2 * rows_pad;
    float* km = qm + ST;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int RT = rows_pad >> 4, CT = (E + 15) >> 4, E4 = 4 * E, CTH = (E4 + 15) >> 4;
    const int KQ = ((E + 15) & ~15) >> 2, KQH = ((E4 + 15) & ~15) >> 2;
    const bool ffn = p.use_ffn && p.use_res, wgrad = p.part_floats != 0;
    const int64_t n_tiles = (p.batch + S - 1) / S;
    const int64_t oW1 = tfb_off(3, E, T), oW2 = tfb_off(4, E, T), oG = tfb_off(5, E, T), oB = tfb_off(6, E, T), oPq = tfb_off(7, E, T),
                  oPk = tfb_off(8, E, T);

    for (int64_t e = tid; e < p.part_floats; e += TF_THREADS) part[e] = 0.f;
    __syncthreads();

    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t b0 = tile * S;
        const int nvalid = (int)min((int64_t)S, p.batch - b0);
        for (int e = tid; e < ST; e += TF_THREADS) {
            const int s = e / T, t = e - s * T;
            float q = 0.f, k = 0.f;
            if (s < nvalid) {
                const int64_t b = b0 + s;
                q = p.q_len ? (t < p.q_len[b] ? 1.f : 0.f) : p.q_mask ? (p.q_mask[b * T + t] ? 1.f : 0.f) : 1.f;
                k = p.k_len ? (t < p.k_len[b] ? 1.f : 0.f) : p.k_mask ? (p.k_mask[b * T + t] ? 1.f : 0.f) : 1.f;
            }
            qm[e] = q;
            km[e] = k;
        }
        // the gradient of the last layer's output; zeros in the K padding, the rows of samples past the batch and the row padding
        for (int e = tid; e < nbuf; e += TF_THREADS) {
            const int r = e / ldx, c = e - r * ldx;
            const int s = r / T, t = r - s * T;
            float v = 0.f;
            if (r < ST && s < nvalid && c < E) {
                if (p.output_type == DCTR_TRANSFORMER_OUT_NONE) {
                    v = p.d_out[(b0 + s) * p.d_out_stride + (int64_t)t * p.d_out_row_stride + c];
                } else {
                    v = p.d_out[(b0 + s) * p.d_out_stride + c];
                    if (p.output_type == DCTR_TRANSFORMER_OUT_MEAN) v = v / (float)T;
                }
            }
            G[e] = v;
        }
        __syncthreads();
        for (int l = p.n_layers - 1; l >= 0; --l) {
            const float* const* W = p.W[l];
            float* pl = part + (int64_t)l * p.layer_floats;
            // ---- the layer's forward again ----
            for (int e = tid; e < nbuf; e += TF_THREADS) {
                const int r = e / ldx, c = e - r * ldx;
                const int s = r / T, t = r - s * T;
                float xv = 0.f;
                if (r < ST && s < nvalid && c < E)
                    xv = l == 0 ? p.x[(b0 + s) * p.x_stride + (int64_t)t * p.x_row_stride + c]
                                : p.tape[(((int64_t)(l - 1) * p.batch + b0 + s) * T + t) * E + c];
                float qv = xv, kv = xv;
                if (p.use_pe && r < ST && c < E) {
                    qv = xv + W[7][t * E + c];
                    kv = xv + W[8][t * E + c];
                }
                X[e] = qv;
                Xk[e] = kv;
                A1[e] = qv;
            }
            __syncthreads();
            tf_project_qkv(X, Xk, Qb, Kb, Vb, W, RT, CT, ST, E, KQ, ldx, ldq);
            __syncthreads();
            tf_attention<true>(A1, Qb, Kb, Vb, qm, km, nvalid, T, H, d, ldx, ldq, p.blinding, p.use_res, p.sqrt_d, stats);
            __syncthreads();
            for (int e = tid; e < nbuf; e += TF_THREADS) R1[e] = A1[e];
            __syncthreads();
            if (p.use_ln) {
                tf_layer_norm(R1, ST, ldx, E, W[5], W[6], p.eps);
                __syncthreads();
            }
            if (p.use_ffn) {
                if (p.use_ln) {
                    // f = r + relu(r fw1) fw2, the forward's loop on a copy of r, for the second LayerNorm's backward
                    for (int e = tid; e < nbuf; e += TF_THREADS) F[e] = R1[e];
                    __syncthreads();
                    if (ffn) {
                        float* slab = Hs + wave * 16 * ldh;
                        for (int rt0 = 0; rt0 < RT; rt0 += TF_WAVES) {
                            const int rt = rt0 + wave;
                            if (rt < RT) {
                                for (int ct = 0; ct < CTH; ++ct) {
                                    dctr::f32x4 acc[1] = {{0.f, 0.f, 0.f, 0.f}};
                                    dctr::tile_gemm_kn<1>(F + rt * 16 * ldx, ldx, E, KQ, W[3], E4, ct * 16, acc);
                                    const int col = ct * 16 + (lane & 15), r0 = 4 * (lane >> 4);
#pragma unroll
                                    for (int r = 0; r < 4; ++r) slab[(r0 + r) * ldh + col] = col < E4 ? fmaxf(acc[0][r], 0.f) : 0.f;
                                }
                            }
                            __syncthreads();
                            if (rt < RT) {
                                for (int ct = 0; ct < CT; ++ct) {
                                    dctr::f32x4 acc[1] = {{0.f, 0.f, 0.f, 0.f}};
                                    dctr::tile_gemm_kn<1>(slab, ldh, E4, KQH, W[4], E, ct * 16, acc);
                                    const int col = ct * 16 + (lane & 15), row0 = rt * 16 + 4 * (lane >> 4);
                                    if (col < E) {
#pragma unroll
                                        for (int r = 0; r < 4; ++r)
                                            if (row0 + r < ST) F[(row0 + r) * ldx + col] += acc[0][r];
                                    }
                                }
                            }
                            __syncthreads();
                        }
                    }
                    tfb_layer_norm_bwd(F, G, rstat, ST, ldx, E, W[5], p.eps, wgrad ? pl + oG : nullptr, wgrad ? pl + oB : nullptr);
                }
                if (ffn) {
                    // ---- feed-forward backward, 64 rows at a time ----
                    float* hs = Hs + wave * 16 * ldh;
                    float* dhs = DHs + wave * 16 * ldh;
                    for (int rt0 = 0; rt0 < RT; rt0 += TF_WAVES) {
                        const int rt = rt0 + wave;
                        if (rt < RT) {
                            for (int ct = 0; ct < CTH; ++ct) {
                                dctr::f32x4 acc[1] = {{0.f, 0.f, 0.f, 0.f}};
                                dctr::tile_gemm_kn<1>(R1 + rt * 16 * ldx, ldx, E, KQ, W[3], E4, ct * 16, acc);
                                dctr::f32x4 dacc[1] = {{0.f, 0.f, 0.f, 0.f}};
                                dctr::tile_gemm_nk<1>(G + rt * 16 * ldx, ldx, E, KQ, W[4], E4, ct * 16, dacc);
                                const int col = ct * 16 + (lane & 15), r0 = 4 * (lane >> 4);
#pragma unroll
                                for (int r = 0; r < 4; ++r) {
                                    const float hv = col < E4 ? fmaxf(acc[0][r], 0.f) : 0.f;
                                    hs[(r0 + r) * ldh + col] = hv;
                                    dhs[(r0 + r) * ldh + col] = hv > 0.f ? dacc[0][r] : 0.f;
                                }
                            }
                        } else if (wave * 16 < grows) {
                            for (int e = lane; e < 16 * ldh; e += 64) {
                                hs[e] = 0.f;
                                dhs[e] = 0.f;
                            }
                        }
                        __syncthreads();
                        if (wgrad) {
                            const int rows_g = min(TFB_GROUP, rows_pad - rt0 * 16);
                            for (int t = wave; t < 2 * CT * CTH; t += TF_WAVES) {
                                const int which = t / (CT * CTH), rest = t - which * CT * CTH, ct = rest % CT, cth = rest / CT;
                                if (which == 0)     // d_fw1 [E, 4E] += r^T dh
                                    tfb_add_tile(pl + oW1, E, E4, ct * 16, cth * 16,
                                                 tfb_gemm_tn(R1 + rt0 * 16 * ldx, ldx, DHs, ldh, rows_g, ct * 16, cth * 16));
                                else                // d_fw2 [4E, E] += h^T df
                                    tfb_add_tile(pl + oW2, E4, E, cth * 16, ct * 16,
                                                 tfb_gemm_tn(Hs, ldh, G + rt0 * 16 * ldx, ldx, rows_g, cth * 16, ct * 16));
                            }
                            __syncthreads();
                        }
                        if (rt < RT) {      // dr = df + dh fw1^T
                            for (int ct = 0; ct < CT; ++ct) {
                                dctr::f32x4 acc[1] = {{0.f, 0.f, 0.f, 0.f}};
                                dctr::tile_gemm_nk<1>(dhs, ldh, E4, KQH, W[3], E, ct * 16, acc);
                                const int col = ct * 16 + (lane & 15), row0 = rt * 16 + 4 * (lane >> 4);
                                if (col < E) {
#pragma unroll
                                    for (int r = 0; r < 4; ++r)
                                        if (row0 + r < ST) G[(row0 + r) * ldx + col] += acc[0][r];
                                }
                            }
                        }
                        __syncthreads();
                    }
                }
            }
            if (p.use_ln) tfb_layer_norm_bwd(A1, G, rstat, ST, ldx, E, W[5], p.eps, wgrad ? pl + oG : nullptr, wgrad ? pl + oB : nullptr);
            // ---- attention backward: G holds da ----
            for (int e = tid; e < nbuf; e += TF_THREADS) {
                A1[e] = 0.f;        // dQ
                R1[e] = 0.f;        // dK
                F[e] = 0.f;         // dV
            }
            __syncthreads();
            for (int it = tid; it < nvalid * T * H; it += TF_THREADS) {     // query walk: sum p~ dP, then dQ
                const int h = it % H, row = it / H, s = row / T, tq = row - s * T;
                float* st = stats + it * 3;
                const float mx = st[0], inv = st[1];
                if (inv == 0.f) {       // a masked query: p~ = 0 everywhere
                    st[2] = 0.f;
                    continue;
                }
                const float* q = Qb + row * ldq + h * d;
                const float* kb = Kb + s * T * ldq + h * d;
                const float* vb = Vb + s * T * ldq + h * d;
                const float* kmask = km + s * T;
                const float* dO = G + row * ldx + h * d;
                const int blind = p.blinding ? tq : -1;
                float delta = 0.f;
                for (int j = 0; j < T; ++j) {
                    float sc = tf_dot(q, kb + j * ldq, d) / p.sqrt_d;
                    if (kmask[j] == 0.f || j == blind) sc = TF_NEG;
                    delta = fmaf(__expf(sc - mx) * inv, tf_dot(dO, vb + j * ldq, d), delta);
                }
                st[2] = delta;
                for (int c0 = 0; c0 < d; c0 += TF_DC) {
                    float acc[TF_DC];
#pragma unroll
                    for (int c = 0; c < TF_DC; ++c) acc[c] = 0.f;
                    for (int j = 0; j < T; ++j) {
                        if (kmask[j] == 0.f || j == blind) continue;        // where() passes no gradient to a replaced score
                        const float sc = tf_dot(q, kb + j * ldq, d) / p.sqrt_d;
                        const float ds = __expf(sc - mx) * inv * (tf_dot(dO, vb + j * ldq, d) - delta) / p.sqrt_d;
                        const float* kj = kb + j * ldq + c0;
#pragma unroll
                        for (int c = 0; c < TF_DC; ++c)
                            if (c0 + c < d) acc[c] = fmaf(ds, kj[c], acc[c]);
                    }
                    float* dq = A1 + row * ldx + h * d + c0;
#pragma unroll
                    for (int c = 0; c < TF_DC; ++c)
                        if (c0 + c < d) dq[c] = acc[c];
                }
            }
            __syncthreads();
            for (int it = tid; it < nvalid * T * H; it += TF_THREADS) {     // key walk: dK and dV
                const int h = it % H, row = it / H, s = row / T, tk = row - s * T;
                const float* kj = Kb + row * ldq + h * d;
                const float* vj = Vb + row * ldq + h * d;
                const bool key_off = km[row] == 0.f;
                for (int c0 = 0; c0 < d; c0 += TF_DC) {
                    float dk[TF_DC], dv[TF_DC];
#pragma unroll
                    for (int c = 0; c < TF_DC; ++c) dk[c] = dv[c] = 0.f;
                    for (int i = 0; i < T; ++i) {
                        const int ri = s * T + i;
                        const float* st = stats + (ri * H + h) * 3;
                        const float inv = st[1];
                        if (inv == 0.f) continue;
                        const bool off = key_off || (p.blinding && i == tk);
                        const float* qi = Qb + ri * ldq + h * d;
                        const float* dO = G + ri * ldx + h * d;
                        const float sc = off ? TF_NEG : tf_dot(qi, kj, d) / p.sqrt_d;
                        const float pt = __expf(sc - st[0]) * inv;
                        const float ds = off ? 0.f : pt * (tf_dot(dO, vj, d) - st[2]) / p.sqrt_d;
#pragma unroll
                        for (int c = 0; c < TF_DC; ++c) {
                            if (c0 + c < d) {
                                dv[c] = fmaf(pt, dO[c0 + c], dv[c]);
                                dk[c] = fmaf(ds, qi[c0 + c], dk[c]);
                            }
                        }
                    }
                    float* dkp = R1 + row * ldx + h * d + c0;
                    float* dvp = F + row * ldx + h * d + c0;
#pragma unroll
                    for (int c = 0; c < TF_DC; ++c) {
                        if (c0 + c < d) {
                            dkp[c] = dk[c];
                            dvp[c] = dv[c];
                        }
                    }
                }
            }
            __syncthreads();
            if (wgrad) {        // d_query += Xq^T dQ, d_key += Xk^T dK, d_value += Xk^T dV
                for (int t = wave; t < 3 * CT * CT; t += TF_WAVES) {
                    const int m = t % 3, rest = t / 3, jt = rest % CT, it = rest / CT;
                    tfb_add_tile(pl + tfb_off(m, E, T), E, E, it * 16, jt * 16,
                                 tfb_gemm_tn(m == 0 ? X : Xk, ldx, m == 0 ? A1 : m == 1 ? R1 : F, ldx, rows_pad, it * 16, jt * 16));
                }
                __syncthreads();
            }
            // dXq = dQ Wq^T (+ da) over G, dXk = dK Wk^T + dV Wv^T over Xq's buffer
            for (int t = wave; t < 2 * RT * CT; t += TF_WAVES) {
                const int which = t & 1, rest = t >> 1, ct = rest % CT, rt = rest / CT;
                dctr::f32x4 acc[1] = {{0.f, 0.f, 0.f, 0.f}};
                const int col = ct * 16 + (lane & 15), row0 = rt * 16 + 4 * (lane >> 4);
                if (which == 0) {
                    dctr::tile_gemm_nk<1>(A1 + rt * 16 * ldx, ldx, E, KQ, W[0], E, ct * 16, acc);
                    if (col < E) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            float* g = G + (row0 + r) * ldx + col;
                            *g = p.use_res ? *g + acc[0][r] : acc[0][r];
                        }
                    }
                } else {
                    dctr::tile_gemm_nk<1>(R1 + rt * 16 * ldx, ldx, E, KQ, W[1], E, ct * 16, acc);
                    dctr::tile_gemm_nk<1>(F + rt * 16 * ldx, ldx, E, KQ, W[2], E, ct * 16, acc);
                    if (col < E) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) X[(row0 + r) * ldx + col] = acc[0][r];
                    }
                }
            }
            __syncthreads();
            // d_pe_q / d_pe_k: the sums over the tile's samples; G = dXq + dXk, the gradient of the layer's input
            for (int e = tid; e < T * E; e += TF_THREADS) {
                const int t = e / E, c = e - t * E;
                float sq = 0.f, sk = 0.f;
                for (int s = 0; s < S; ++s) {
                    const int i = (s * T + t) * ldx + c;
                    const float g = G[i], xk = X[i];
                    sq += g;
                    sk += xk;
                    G[i] = g + xk;
                }
                if (wgrad && p.use_pe) {
                    pl[oPq + e] += sq;
                    pl[oPk + e] += sk;
                }
            }
            __syncthreads();
        }
        if (p.dx) {
            const int n = T * E;
            for (int e = tid; e < nvalid * n; e += TF_THREADS) {
                const int s = e / n, rem = e - s * n, t = rem / E, c = rem - t * E;
                float* o = p.dx + (b0 + s) * p.dx_stride + (int64_t)t * p.dx_row_stride + c;
                const float g = G[(s * T + t) * ldx + c];
                *o = p.accumulate ? *o + g : g;
            }
        }
        __syncthreads();    // the buffers are reloaded for the next tile
    }
}

struct TfbReduce {
    float* d[TFB_MAX_LAYERS][TF_NW];
    const float* ws;
    int64_t layer_floats, slice_floats, total;
    int32_t E, T, grid;
};

// d_layers[l][m] += the workgroups' partials, in workgroup order
__global__ __launch_bounds__(TF_THREADS) void transformer_bwd_reduce_kernel(TfbReduce p) {
    for (int64_t e = (int64_t)blockIdx.x * TF_THREADS + threadIdx.x; e < p.total; e += (int64_t)gridDim.x * TF_THREADS) {
        const int l = (int)(e / p.layer_floats);
        const int64_t rem = e - l * p.layer_floats;
        int m = 0;
        while (m < TF_NW - 1 && rem >= tfb_off(m + 1, p.E, p.T)) ++m;
        float* dst = p.d[l][m];
        if (!dst) continue;
        float s = 0.f;
        for (int g = 0; g < p.grid; ++g) s += p.ws[g * p.slice_floats + e];
        dst[rem - tfb_off(m, p.E, p.T)] += s;
    }
}

struct TfbPlan {
    bool global, fits;
    int S, ldx, ldq, ldh, grid;
    int64_t tile_floats, layer_floats, part_floats, slice_floats;
    size_t bytes;
};

int64_t tfb_tile_floats(int S, int T, int H, int ldx, int ldq, int ldh) {
    const int64_t st = (int64_t)S * T, rp = (st + 15) & ~(int64_t)15;
    return 6 * rp * ldx + ((3 * st * ldq + 3) & ~(int64_t)3) + 2 * (rp < TFB_GROUP ? rp : (int64_t)TFB_GROUP) * ldh + ((3 * st * H + 3) & ~(int64_t)3) + 2 * rp +
           ((2 * st + 3) & ~(int64_t)3);
}

void tfb_plan(const dctr_transformer_train_args_t* t, TfbPlan* pl) {
    const dctr_transformer_args_t* a = &t->fwd;
    const int T = a->seq_len, E = a->dim, H = a->head_num;
    pl->ldx = ((E + 15) & ~15) + 4;
    pl->ldq = E | 1;
    pl->ldh = a->use_feed_forward && a->use_res ? ((4 * E + 15) & ~15) + 4 : 0;
    int S = TF_MAX_S;
    // (the launch has at most 256 workgroups, one per CU: nothing is gained by leaving room for a second one, a larger tile fills
    // more of the four waves and adds its weight-gradient tiles to the partials once for more samples)
    while (S > 1 && (size_t)tfb_tile_floats(S, T, H, pl->ldx, pl->ldq, pl->ldh) * 4 > DCTR_LDS_MAX) --S;
    pl->fits = (size_t)tfb_tile_floats(S, T, H, pl->ldx, pl->ldq, pl->ldh) * 4 <= DCTR_LDS_MAX;
    pl->global = !pl->fits || a->route == DCTR_TRANSFORMER_ROUTE_GENERAL;
    pl->S = pl->global ? 1 : S;
    pl->tile_floats = tfb_tile_floats(pl->S, T, H, pl->ldx, pl->ldq, pl->ldh);
    pl->layer_floats = tfb_off(9, E, T);
    pl->part_floats = (a->n_layers * pl->layer_floats + 3) & ~(int64_t)3;
    pl->slice_floats = pl->part_floats + (pl->global ? pl->tile_floats : 0);
    int64_t grid = dctr_workspace_slices((size_t)pl->slice_floats * 4).grid_max;       // <= 256 workgroups and <= 256 MiB, but one
    const int64_t n_tiles = dctr_ceil_div(a->batch > 0 ? a->batch : 1, pl->S);
    if (grid > n_tiles) grid = n_tiles;
    if (t->max_blocks > 0 && grid > t->max_blocks) grid = t->max_blocks;
    pl->grid = (int)grid;
    pl->bytes = (size_t)pl->slice_floats * 4 * (size_t)grid;
}

int tfb_check(const dctr_transformer_train_args_t* t) {
    DCTR_REQUIRE(t, DCTR_E_NULL, "transformer_bwd: null args");
    const dctr_transformer_args_t* a = &t->fwd;
    const int rc = dctr_transformer_route(a);       // the forward's checks of sizes, strides, flags, masks and route
    if (rc < 0) return rc;
    DCTR_REQUIRE((uint32_t)t->accumulate <= 1u, DCTR_E_ENUM, "transformer_bwd: accumulate must be 0 or 1");
    DCTR_REQUIRE(t->max_blocks >= 0, DCTR_E_ENUM, "transformer_bwd: max_blocks < 0");
    if (a->output_type == DCTR_TRANSFORMER_OUT_NONE)
        DCTR_REQUIRE(!t->d_out || (t->d_out_row_stride >= a->dim && t->d_out_stride >= ((int64_t)a->seq_len - 1) * t->d_out_row_stride + a->dim),
                     DCTR_E_DIM, "transformer_bwd: d_out strides smaller than the [seq_len, dim] block");
    else
        DCTR_REQUIRE(!t->d_out || t->d_out_stride >= a->dim, DCTR_E_DIM, "transformer_bwd: d_out_stride < dim");
    DCTR_REQUIRE(!t->dx || (t->dx_row_stride >= a->dim && t->dx_stride >= ((int64_t)a->seq_len - 1) * t->dx_row_stride + a->dim), DCTR_E_DIM,
                 "transformer_bwd: dx strides smaller than the [seq_len, dim] block");
    return DCTR_OK;
}

int tfb_supported(const dctr_transformer_train_args_t* t, bool say) {
    const dctr_transformer_args_t* a = &t->fwd;
    if (a->keys && a->keys != a->queries) {
        if (say) dctr_set_error("transformer_bwd: separate keys are not supported (self-attention only)");
        return 0;
    }
    if (a->n_layers > TFB_MAX_LAYERS) {
        if (say) dctr_set_error("transformer_bwd: %d layers, at most %d", a->n_layers, TFB_MAX_LAYERS);
        return 0;
    }
    TfbPlan pl;
    tfb_plan(t, &pl);
    if (a->route == DCTR_TRANSFORMER_ROUTE_FUSED && !pl.fits) {
        if (say) dctr_set_error("transformer_bwd: one sample of seq_len %d, dim %d does not fit the fused route's LDS", a->seq_len, a->dim);
        return 0;
    }
    return 1;
}

}  // namespace

extern "C" int dctr_transformer_bwd_supported(const dctr_transformer_train_args_t* t) {
    if (tfb_check(t) != DCTR_OK) return 0;
    return tfb_supported(t, false);
}

extern "C" size_t dctr_transformer_bwd_workspace_bytes(const dctr_transformer_train_args_t* t) {
    if (tfb_check(t) != DCTR_OK || !tfb_supported(t, false)) return 0;
    TfbPlan pl;
    tfb_plan(t, &pl);
    return pl.bytes;
}

extern "C" int dctr_transformer_bwd(const dctr_transformer_train_args_t* t, void* stream) {
    int rc = tfb_check(t);
    if (rc != DCTR_OK) return rc;
    if (!tfb_supported(t, true)) return DCTR_E_UNSUPPORTED;
    const dctr_transformer_args_t* a = &t->fwd;
    DCTR_REQUIRE(a->queries && a->layers && t->d_out, DCTR_E_NULL, "transformer_bwd: null x / layers / d_out");
    const bool ffn = a->use_feed_forward && a->use_res;
    for (int l = 0; l < a->n_layers; ++l) {
        const float* const* w = a->layers + TF_NW * l;
        DCTR_REQUIRE(w[0] && w[1] && w[2], DCTR_E_NULL, "transformer_bwd: layer %d: null query / key / value", l);
        DCTR_REQUIRE(!ffn || (w[3] && w[4]), DCTR_E_NULL, "transformer_bwd: layer %d: null fw1 / fw2", l);
        DCTR_REQUIRE(!a->use_layer_norm || (w[5] && w[6]), DCTR_E_NULL, "transformer_bwd: layer %d: null ln_gamma / ln_beta", l);
        DCTR_REQUIRE(!a->use_positional_encoding || (w[7] && w[8]), DCTR_E_NULL, "transformer_bwd: layer %d: null pe_q / pe_k", l);
    }
    const size_t tape_need = (size_t)(a->n_layers - 1) * (size_t)a->batch * a->seq_len * a->dim * sizeof(float);
    DCTR_REQUIRE(!tape_need || (t->tape && t->tape_bytes >= tape_need), DCTR_E_NULL,
                 "transformer_bwd: the tape needs %zu bytes (dctr_transformer_tape_bytes)", tape_need);
    TfbPlan pl;
    tfb_plan(t, &pl);
    DCTR_REQUIRE_WORKSPACE("transformer_bwd", "dctr_transformer_bwd_workspace_bytes", t->workspace, t->workspace_bytes, pl.bytes);
    if (a->batch == 0) return DCTR_OK;
    bool any = false;
    if (t->d_layers)
        for (int i = 0; i < a->n_layers * TF_NW; ++i) any = any || t->d_layers[i] != nullptr;
    TfbParams p = {};
    p.x = a->queries;
    p.batch = a->batch;
    p.x_stride = a->q_stride;
    p.x_row_stride = a->q_row_stride;
    p.T = a->seq_len;
    p.E = a->dim;
    p.d = a->att_embedding_size;
    p.H = a->head_num;
    p.n_layers = a->n_layers;
    p.use_pe = a->use_positional_encoding;
    p.use_res = a->use_res;
    p.use_ffn = a->use_feed_forward;
    p.use_ln = a->use_layer_norm;
    p.blinding = a->blinding;
    p.output_type = a->output_type;
    p.sqrt_d = (float)sqrt((double)a->att_embedding_size);
    p.eps = a->ln_eps;
    p.S = pl.S;
    p.ldx = pl.ldx;
    p.ldq = pl.ldq;
    p.ldh = pl.ldh;
    p.part_floats = any ? pl.part_floats : 0;
    p.layer_floats = pl.layer_floats;
    p.slice_floats = pl.slice_floats;
    p.q_len = a->query_lengths;
    p.k_len = a->key_lengths;
    p.q_mask = a->query_mask;
    p.k_mask = a->key_mask;
    for (int l = 0; l < a->n_layers; ++l)
        for (int m = 0; m < TF_NW; ++m) p.W[l][m] = a->layers[TF_NW * l + m];
    p.tape = (const float*)t->tape;
    p.d_out = t->d_out;
    p.d_out_stride = t->d_out_stride;
    p.d_out_row_stride = t->d_out_row_stride;
    p.dx = t->dx;
    p.dx_stride = t->dx_stride;
    p.dx_row_stride = t->dx_row_stride;
    p.accumulate = t->accumulate;
    p.ws = (float*)t->workspace;
    if (!p.dx && !any) return DCTR_OK;
    if (pl.global) {
        // the tile follows the partial block in the slice whether or not weight gradients are asked
        p.part_floats = pl.part_floats;
        DCTR_LAUNCH(transformer_bwd_kernel<true>, dim3((unsigned)pl.grid), dim3(TF_THREADS), 0, (hipStream_t)stream, p);
    } else {
        const size_t lds = (size_t)pl.tile_floats * sizeof(float);
        static thread_local size_t granted[DCTR_MAX_DEVICES] = {0};
        hipError_t e = dctr_grant_lds((const void*)transformer_bwd_kernel<false>, lds, granted);
        DCTR_REQUIRE(e == hipSuccess, (int)e, "transformer_bwd: cannot raise dynamic LDS: %s", hipGetErrorString(e));
        DCTR_LAUNCH(transformer_bwd_kernel<false>, dim3((unsigned)pl.grid), dim3(TF_THREADS), lds, (hipStream_t)stream, p);
    }
    rc = dctr_launch_status("dctr_transformer_bwd");
    if (rc != DCTR_OK || !any) return rc;
    TfbReduce r = {};
    const bool live[TF_NW] = {true, true, true, ffn, ffn, (bool)a->use_layer_norm, (bool)a->use_layer_norm,
                              (bool)a->use_positional_encoding, (bool)a->use_positional_encoding};
    for (int l = 0; l < a->n_layers; ++l)
        for (int m = 0; m < TF_NW; ++m) r.d[l][m] = live[m] ? t->d_layers[TF_NW * l + m] : nullptr;
    r.ws = (const float*)t->workspace;
    r.layer_floats = pl.layer_floats;
    r.slice_floats = pl.slice_floats;
    r.total = (int64_t)a->n_layers * pl.layer_floats;
    r.E = a->dim;
    r.T = a->seq_len;
    r.grid = pl.grid;
    const int64_t blocks = dctr_ceil_div(r.total, TF_THREADS);
    DCTR_LAUNCH(transformer_bwd_reduce_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(TF_THREADS), 0, (hipStream_t)stream, r);
    return dctr_launch_status("dctr_transformer_bwd (reduce)");
}
