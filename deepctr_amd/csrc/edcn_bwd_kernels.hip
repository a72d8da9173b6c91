// EDCN's tower, backward (dctr_edcn_bwd): the gradient of the tower with its head from x, the live weights and the tape of c / h / br
// that dctr_edcn_train_fwd (edcn_kernels.hip) wrote.
//
// Per round, in reverse (dbr, dc, dh: the gradients of br, c, h; xin = x for round 0, else br of the round before from the tape):
//     bridge   c + h: dc += dbr, dh += dbr  |  c * h: dc += dbr h, dh += dbr c  |  Dense: dz = dbr [br > 0], dc += dz Wb[0:D]^T,
//              dh += dz Wb[D:2D]^T, dWb = [c, h]^T dz, dbb = sum dz
//     DNN      dz = dh [h > 0], dWd = deep^T dz, dbd = sum dz, ddeep = dz Wd^T
//     cross    vector (s = cross . w): dcross = dc (s + 1) + w (dc . cross), dw = sum (dc . cross) cross, db = sum dc
//              matrix (u = W cross + b, q = dc * cross): dcross = dc * (u + 1) + W^T q, dW = q^T cross, db = sum q   (u is recomputed)
//     gates    deep = xin * gd, cross = xin * gc (recomputed): dxin = ddeep gd + dcross gc, dG[f] = sum_{b, e} d * xin,
//              d_gate = inv_tau g * (dG - sum_f g dG)
//
// Three passes, no atomics:
//   edcn_bwd_row_kernel   a workgroup owns tiles of 16 rows and walks all rounds in reverse with four [16, ld] tiles in LDS (G0: dbr,
//                         later q and the next dbr; G1: dc; G2: dh; G3: cross, later ddeep).  The input-gradient products run on
//                         v_mfma_f32_16x16x4_f32 (mfma_tile.h).  It leaves dz (DNN), q and dz (bridge) of every row in the workspace,
//                         and adds its column sums (biases, the vector dw, the gates' per-column sums, d_head_w) to its OWN row of
//                         per-workgroup partials.
//   edcn_bwd_wgrad_kernel P^T Q over a batch slice for each [D, D] weight gradient (MFMA, operands read from HBM / L2) -> partials
//   edcn_bwd_wsum_kernel / edcn_bwd_vsum_kernel   add the partials in a fixed order (slices 0 .. S-1, workgroups 0 .. n-1), apply the
//                         gate a recomputed operand carries (deep = xin * gd: a row scale of dWd; cross = xin * gc: a column scale of
//                         the matrix dW) and the softmax backward of the gates.
#include <math.h>
#include "dctr_common.h"
#include "tile_route.h"
#include "mfma_tile.h"
#include "edcn_device.h"

namespace {

constexpr int ED_BWD_R = 16;                      // rows of a tile
constexpr int ED_BWD_WGS = DCTR_GLOBAL_WGS;       // at most this many row workgroups (rows of column-sum partials)
constexpr int ED_BWD_MAX_SLICES = DCTR_GLOBAL_WGS;
constexpr int ED_BWD_SLICE_ROWS = 256;            // the library's slices hold about this many rows
constexpr int ED_BWD_AUTO_SLICES = 16;
constexpr int ED_WG_THREADS = 256;                // weight-gradient pass: four waves, a [16, 64] output tile each
constexpr int ED_VS_THREADS = 256;

// column sums of a round, D floats each, in a workgroup's row of partials; then d_head_w [3D]
enum { ED_CS_CROSS_B = 0, ED_CS_DNN_B, ED_CS_BRIDGE_B, ED_CS_CROSS_W, ED_CS_GATE_D, ED_CS_GATE_C, ED_CS_N };
// [D, D] products of a round
enum { ED_WK_DNN = 0, ED_WK_CROSS, ED_WK_BRIDGE_C, ED_WK_BRIDGE_H, ED_WK_N };

struct EdBwdRound {
    const float *g_deep, *g_cross, *cross_w, *cross_b, *dnn_w, *bridge_w;
};

struct EdBwdRow {
    int64_t batch;
    const float* x;               // already advanced by x_offset
    int64_t x_stride;
    const float* tape;
    int32_t F, d, D, rounds, mode, bridge, act, bridge_act, ld, want_head;
    float inv_tau;
    EdBwdRound rd[ED_MAX_ROUNDS];
    const float* head_w;
    const float* d_logit;
    const float* d_out;
    int64_t d_out_stride;
    float* dx;                    // already advanced by dx_offset
    int64_t dx_stride;
    int32_t accumulate;
    float* z;                     // NULL, or [rounds, B, zp]: dz (DNN) | q (matrix cross, at zq) | dz (bridge Dense, at zb)
    int32_t zp, zq, zb;
    float* colpart;               // [gridDim.x, nv]
    int64_t nv;
    float* gates_out;             // [rounds, 2, F]: the softmaxes, for the sum kernels
};

template <int TPW>
__device__ __forceinline__ void ed_zero(dctr::f32x4 (&acc)[TPW]) {
#pragma unroll
    for (int c = 0; c < TPW; ++c) acc[c] = dctr::f32x4{0.f, 0.f, 0.f, 0.f};
}

template <int TPW>
__global__ __launch_bounds__(ED_THREADS) void edcn_bwd_row_kernel(EdBwdRow p) {
    extern __shared__ __attribute__((aligned(16))) float eb_lds[];
    constexpr int R = ED_BWD_R;
    const int ld = p.ld, D = p.D, F = p.F, d = p.d;
    float* G0 = eb_lds;
    float* G1 = G0 + R * ld;
    float* G2 = G1 + R * ld;
    float* G3 = G2 + R * ld;
    float* Gd = G3 + R * ld;
    float* Gc = Gd + F;
    float* Sr = Gc + F;           // [R]: s = cross . w of a row (vector cross)
    float* Tr = Sr + R;           // [R]: dc . cross
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int CT = (D + 16 * TPW - 1) / (16 * TPW), KQ = dctr::pad16(D) >> 2;
    const int64_t n_tiles = (p.batch + R - 1) / R, D3 = 3 * (int64_t)D;
    const int row0 = 4 * (lane >> 4);
    float* part = p.colpart + (int64_t)blockIdx.x * p.nv;
    const bool relu = p.act == DCTR_ACT_RELU, brelu = p.bridge_act == DCTR_ACT_RELU;

    for (int64_t e = tid; e < p.nv; e += ED_THREADS) part[e] = 0.f;
    // the K padding of the four tiles is read by the products and written by nobody
    for (int e = tid; e < 4 * R * ld; e += ED_THREADS) eb_lds[e] = 0.f;
    __syncthreads();

    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t b0 = tile * R;
        const int nvalid = (int)min((int64_t)R, p.batch - b0);
        // the seeds of the last round: d_out + d_logit * head_w -> dc (G1), dh (G2), dbr (G0); rows past the batch stay zero throughout
        for (int k = tid; k < D; k += ED_THREADS) {
            const float hc = p.d_logit ? p.head_w[k] : 0.f, hh = p.d_logit ? p.head_w[D + k] : 0.f, hb = p.d_logit ? p.head_w[2 * D + k] : 0.f;
            for (int r = 0; r < R; ++r) {
                float vc = 0.f, vh = 0.f, vb = 0.f;
                if (r < nvalid) {
                    if (p.d_out) {
                        const float* o = p.d_out + (b0 + r) * p.d_out_stride + k;
                        vc = o[0];
                        vh = o[D];
                        vb = o[2 * (int64_t)D];
                    }
                    if (p.d_logit) {
                        const float dl = p.d_logit[b0 + r];
                        vc = fmaf(dl, hc, vc);
                        vh = fmaf(dl, hh, vh);
                        vb = fmaf(dl, hb, vb);
                    }
                }
                G1[r * ld + k] = vc;
                G2[r * ld + k] = vh;
                G0[r * ld + k] = vb;
            }
        }
        if (p.want_head) {
            const float* last = p.tape + ((int64_t)(p.rounds - 1) * p.batch + b0) * D3;
            for (int64_t col = tid; col < D3; col += ED_THREADS) {
                float s = 0.f;
                for (int r = 0; r < nvalid; ++r) s = fmaf(p.d_logit[b0 + r], last[r * D3 + col], s);
                part[(int64_t)p.rounds * ED_CS_N * D + col] += s;
            }
        }
        __syncthreads();
        for (int i = p.rounds - 1; i >= 0; --i) {
            const EdBwdRound& rd = p.rd[i];
            const float* tp = p.tape + ((int64_t)i * p.batch + b0) * D3;                 // c | h | br of this round, rows of 3D
            const float* xin = i == 0 ? p.x + b0 * p.x_stride : p.tape + ((int64_t)(i - 1) * p.batch + b0) * D3 + 2 * (int64_t)D;
            const int64_t xin_stride = i == 0 ? p.x_stride : D3;
            float* z = p.z ? p.z + ((int64_t)i * p.batch + b0) * p.zp : nullptr;
            float* cs = part + (int64_t)i * ED_CS_N * D;
            if (wave == 0) ed_gate(rd.g_deep, F, p.inv_tau, Gd, lane);
            if (wave == 1) ed_gate(rd.g_cross, F, p.inv_tau, Gc, lane);
            __syncthreads();
            if (blockIdx.x == 0 && tile == 0) {
                for (int f = tid; f < F; f += ED_THREADS) {
                    p.gates_out[((int64_t)i * 2) * F + f] = Gd[f];
                    p.gates_out[((int64_t)i * 2 + 1) * F + f] = Gc[f];
                }
            }
            // ---- bridge
            if (p.bridge == DCTR_EDCN_BRIDGE_CONCAT) {
                for (int k = tid; k < D; k += ED_THREADS) {
                    float s = 0.f;
                    for (int r = 0; r < nvalid; ++r) {
                        float v = G0[r * ld + k];
                        if (brelu && !(tp[r * D3 + 2 * (int64_t)D + k] > 0.f)) v = 0.f;
                        G0[r * ld + k] = v;
                        if (z) z[(int64_t)r * p.zp + p.zb + k] = v;
                        s += v;
                    }
                    cs[ED_CS_BRIDGE_B * D + k] += s;
                }
                __syncthreads();
                for (int t = wave; t < 2 * CT; t += ED_WAVES) {
                    const int which = t / CT, ct = t - which * CT;
                    dctr::f32x4 acc[TPW];
                    ed_zero<TPW>(acc);
                    dctr::tile_gemm_nk<TPW>(G0, ld, D, KQ, rd.bridge_w + (int64_t)which * D * D, D, ct * 16 * TPW, acc);
                    float* dst = which == 0 ? G1 : G2;
                    const int col0 = ct * 16 * TPW + TPW * (lane & 15);
#pragma unroll
                    for (int c = 0; c < TPW; ++c) {
                        const int col = col0 + c;
                        if (col < D) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) dst[(row0 + r) * ld + col] += acc[c][r];
                        }
                    }
                }
                __syncthreads();
            } else {
                const bool prod = p.bridge == DCTR_EDCN_BRIDGE_HADAMARD;
                for (int k = tid; k < D; k += ED_THREADS) {
                    for (int r = 0; r < nvalid; ++r) {
                        const float v = G0[r * ld + k];
                        const float cv = prod ? tp[r * D3 + k] : 1.f, hv = prod ? tp[r * D3 + D + k] : 1.f;
                        G1[r * ld + k] += v * hv;
                        G2[r * ld + k] += v * cv;
                    }
                }
            }
            // ---- dz of the DNN -> G2; cross = xin * gate -> G3  (a thread owns its columns in these passes: no barrier between them)
            for (int k = tid; k < D; k += ED_THREADS) {
                const float gc = Gc[k / d];
                float s = 0.f;
                for (int r = 0; r < R; ++r) {
                    float v = 0.f, xv = 0.f;
                    if (r < nvalid) {
                        v = G2[r * ld + k];
                        if (relu && !(tp[r * D3 + D + k] > 0.f)) v = 0.f;
                        if (z) z[(int64_t)r * p.zp + k] = v;
                        xv = xin[r * xin_stride + k] * gc;
                        s += v;
                    }
                    G2[r * ld + k] = v;
                    G3[r * ld + k] = xv;
                }
                cs[ED_CS_DNN_B * D + k] += s;
            }
            __syncthreads();
            // ---- cross: dcross -> G1 (matrix: all but the W^T q term, with q -> G0)
            if (p.mode == DCTR_CROSS_VECTOR) {
                for (int r = wave; r < R; r += ED_WAVES) {
                    float s = 0.f, t = 0.f;
                    for (int k = lane; k < D; k += 64) {
                        const float xv = G3[r * ld + k];
                        s = fmaf(xv, rd.cross_w[k], s);
                        t = fmaf(xv, G1[r * ld + k], t);
                    }
                    s = ed_wave_sum(s);
                    t = ed_wave_sum(t);
                    if (lane == 0) {
                        Sr[r] = s;
                        Tr[r] = t;
                    }
                }
                __syncthreads();
                for (int k = tid; k < D; k += ED_THREADS) {
                    const float w = rd.cross_w[k];
                    float sb = 0.f, sw = 0.f;
                    for (int r = 0; r < R; ++r) {
                        const float dc = G1[r * ld + k];
                        sb += dc;
                        sw = fmaf(Tr[r], G3[r * ld + k], sw);
                        G1[r * ld + k] = dc * (Sr[r] + 1.f) + w * Tr[r];
                    }
                    cs[ED_CS_CROSS_B * D + k] += sb;
                    cs[ED_CS_CROSS_W * D + k] += sw;
                }
                __syncthreads();
            } else {
                for (int ct = wave; ct < CT; ct += ED_WAVES) {
                    dctr::f32x4 acc[TPW];
                    ed_zero<TPW>(acc);
                    dctr::tile_gemm_nk<TPW>(G3, ld, D, KQ, rd.cross_w, D, ct * 16 * TPW, acc);
                    const int col0 = ct * 16 * TPW + TPW * (lane & 15);
#pragma unroll
                    for (int c = 0; c < TPW; ++c) {
                        const int col = col0 + c;
                        if (col < D) {
                            const float b = rd.cross_b[col];
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const int at = (row0 + r) * ld + col;
                                const float dc = G1[at];
                                G0[at] = dc * G3[at];
                                G1[at] = dc * (acc[c][r] + b + 1.f);
                            }
                        }
                    }
                }
                __syncthreads();
                for (int k = tid; k < D; k += ED_THREADS) {
                    float s = 0.f;
                    for (int r = 0; r < nvalid; ++r) {
                        const float q = G0[r * ld + k];
                        if (z) z[(int64_t)r * p.zp + p.zq + k] = q;
                        s += q;
                    }
                    cs[ED_CS_CROSS_B * D + k] += s;
                }
            }
            // ---- ddeep = dz Wd^T -> G3 (the cross operand is dead);  matrix: dcross += W^T q
            const int n_tasks = p.mode == DCTR_CROSS_MATRIX ? 2 * CT : CT;
            for (int t = wave; t < n_tasks; t += ED_WAVES) {
                const int which = t / CT, ct = t - which * CT;
                dctr::f32x4 acc[TPW];
                ed_zero<TPW>(acc);
                const int col0 = ct * 16 * TPW + TPW * (lane & 15);
                if (which == 0) {
                    dctr::tile_gemm_nk<TPW>(G2, ld, D, KQ, rd.dnn_w, D, ct * 16 * TPW, acc);
                } else {
                    dctr::tile_gemm_kn<TPW>(G0, ld, D, KQ, rd.cross_w, D, ct * 16 * TPW, acc);
                }
                // (which == 0 writes G3 while other waves may still read it as the u product's operand? no: that product ended at the
                //  barrier above; G3 is read here by nobody)
#pragma unroll
                for (int c = 0; c < TPW; ++c) {
                    const int col = col0 + c;
                    if (col < D) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int at = (row0 + r) * ld + col;
                            if (which == 0) G3[at] = acc[c][r];
                            else G1[at] += acc[c][r];
                        }
                    }
                }
            }
            __syncthreads();
            // ---- gates: dxin -> G0 (the next dbr), the gates' column sums; dc = dh = 0 for the round before
            for (int k = tid; k < D; k += ED_THREADS) {
                const float gd = Gd[k / d], gc = Gc[k / d];
                float sd = 0.f, sc = 0.f;
                for (int r = 0; r < R; ++r) {
                    const float dd = G3[r * ld + k], dcr = G1[r * ld + k];
                    const float xv = r < nvalid ? xin[r * xin_stride + k] : 0.f;
                    sd = fmaf(dd, xv, sd);
                    sc = fmaf(dcr, xv, sc);
                    G0[r * ld + k] = dd * gd + dcr * gc;
                    G1[r * ld + k] = 0.f;
                    G2[r * ld + k] = 0.f;
                }
                cs[ED_CS_GATE_D * D + k] += sd;
                cs[ED_CS_GATE_C * D + k] += sc;
            }
            __syncthreads();
        }
        if (p.dx) {
            for (int k = tid; k < D; k += ED_THREADS) {
                for (int r = 0; r < nvalid; ++r) {
                    float* o = p.dx + (b0 + r) * p.dx_stride + k;
                    o[0] = p.accumulate ? o[0] + G0[r * ld + k] : G0[r * ld + k];
                }
            }
        }
        __syncthreads();        // the tiles are seeded again for the next tile
    }
}

struct EdBwdWg {
    int64_t batch, slice_rows;
    const float* x;               // already advanced by x_offset
    int64_t x_stride;
    const float* tape;
    const float* z;
    int32_t D, rounds, zp, zq, zb, n_kinds;
    int32_t kinds[ED_WK_N];
    float* partials;              // [S, rounds, n_kinds, D, D]
};

// G[m, n] = sum over the slice's rows of P[b, m] Q[b, n]: a wave takes a [16, 64] tile; the batch is the MFMA's k
__global__ __launch_bounds__(ED_WG_THREADS) void edcn_bwd_wgrad_kernel(EdBwdWg p) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, j = lane & 15;
    const int D = p.D, MT = (D + 15) >> 4, NTL = (D + 63) >> 6;
    const int task = blockIdx.x * (ED_WG_THREADS / 64) + wave;
    if (task >= MT * NTL) return;
    const int m0 = (task / NTL) * 16, n0 = (task % NTL) * 64;
    const int s = blockIdx.y, i = blockIdx.z / p.n_kinds, kidx = blockIdx.z - i * p.n_kinds, kind = p.kinds[kidx];
    const int64_t b_lo = min((int64_t)s * p.slice_rows, p.batch), b_hi = min(b_lo + p.slice_rows, p.batch), D3 = 3 * (int64_t)D;
    const float* xin = i == 0 ? p.x : p.tape + (int64_t)(i - 1) * p.batch * D3 + 2 * (int64_t)D;
    const int64_t xin_stride = i == 0 ? p.x_stride : D3;
    const float* zi = p.z + (int64_t)i * p.batch * p.zp;
    const float* ti = p.tape + (int64_t)i * p.batch * D3;
    const float *P, *Q;
    int64_t ps, qs;
    if (kind == ED_WK_DNN) {
        P = xin, ps = xin_stride, Q = zi, qs = p.zp;
    } else if (kind == ED_WK_CROSS) {
        P = zi + p.zq, ps = p.zp, Q = xin, qs = xin_stride;
    } else {
        P = ti + (kind == ED_WK_BRIDGE_H ? D : 0), ps = D3, Q = zi + p.zb, qs = p.zp;
    }
    const bool mon = m0 + j < D;
    bool non[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) non[c] = n0 + 16 * c + j < D;
    dctr::f32x4 acc[4];
    ed_zero<4>(acc);
    constexpr int U = 4;            // k-steps in flight: their loads are issued before the first MFMA
    for (int64_t b0 = b_lo; b0 < b_hi; b0 += 4 * U) {
        float av[U], bv[U][4];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t b = b0 + 4 * u + g;
            const bool bon = b < b_hi;
            const int64_t br = bon ? b : b_lo;
            av[u] = (bon && mon) ? P[br * ps + m0 + j] : 0.f;
#pragma unroll
            for (int c = 0; c < 4; ++c) bv[u][c] = (bon && non[c]) ? Q[br * qs + n0 + 16 * c + j] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], bv[u][c], acc[c], 0, 0, 0);
        }
    }
    float* dst = p.partials + (((int64_t)s * p.rounds + i) * p.n_kinds + kidx) * D * D;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int n = n0 + 16 * c + j;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + 4 * g + r;
            if (m < D && n < D) dst[(int64_t)m * D + n] = acc[c][r];
        }
    }
}

struct EdBwdWsum {
    int32_t D, d, F, rounds, n_kinds, S;
    int32_t kinds[ED_WK_N];
    const float* partials;
    const float* gates;           // [rounds, 2, F]
    float* out[ED_MAX_ROUNDS][ED_WK_N];         // by kind; NULL: not wanted
};

// element (m, n) of a weight gradient: its S partials added in the order 0 .. S-1, times the gate its recomputed operand carries
__global__ __launch_bounds__(ED_VS_THREADS) void edcn_bwd_wsum_kernel(EdBwdWsum p) {
    const int i = blockIdx.y / p.n_kinds, kidx = blockIdx.y - i * p.n_kinds, kind = p.kinds[kidx];
    float* out = p.out[i][kind];
    if (!out) return;
    const int64_t DD = (int64_t)p.D * p.D, e = (int64_t)blockIdx.x * ED_VS_THREADS + threadIdx.x;
    if (e >= DD) return;
    const int64_t slice = (int64_t)p.rounds * p.n_kinds * DD;
    const float* src = p.partials + ((int64_t)i * p.n_kinds + kidx) * DD + e;
    float v = 0.f;
    for (int s = 0; s < p.S; ++s) v += src[s * slice];
    const int m = (int)(e / p.D), n = (int)(e - (int64_t)m * p.D);
    if (kind == ED_WK_DNN) v *= p.gates[((int64_t)i * 2) * p.F + m / p.d];
    if (kind == ED_WK_CROSS) v *= p.gates[((int64_t)i * 2 + 1) * p.F + n / p.d];
    out[e] = v;
}

struct EdBwdVsum {
    int32_t D, d, F, rounds, n_wgs;
    float inv_tau;
    int64_t nv;
    const float* colpart;
    const float* gates;
    float* vec[ED_MAX_ROUNDS][4];   // cross_b, dnn_b, bridge_b, cross_w (vector): NULL: not wanted
    float* gate[ED_MAX_ROUNDS][2];  // d of the deep / cross gate's F weights
    float* head;
};

// blocks [0, 4 rounds): a D-sized gradient; block 4 rounds: d_head_w; then 2 rounds blocks: a gate.  Workgroup partials in order 0 .. n-1.
__global__ __launch_bounds__(ED_VS_THREADS) void edcn_bwd_vsum_kernel(EdBwdVsum p) {
    extern __shared__ float vs_lds[];
    const int tid = threadIdx.x, blk = blockIdx.x, D = p.D;
    if (blk < 4 * p.rounds) {
        const int i = blk >> 2, w = blk & 3;
        float* out = p.vec[i][w];
        if (!out) return;
        const int slot = w == 0 ? ED_CS_CROSS_B : w == 1 ? ED_CS_DNN_B : w == 2 ? ED_CS_BRIDGE_B : ED_CS_CROSS_W;
        const float* src = p.colpart + ((int64_t)i * ED_CS_N + slot) * D;
        for (int k = tid; k < D; k += ED_VS_THREADS) {
            float v = 0.f;
            for (int g = 0; g < p.n_wgs; ++g) v += src[g * p.nv + k];
            out[k] = v;
        }
        return;
    }
    if (blk == 4 * p.rounds) {
        if (!p.head) return;
        const float* src = p.colpart + (int64_t)p.rounds * ED_CS_N * D;
        for (int k = tid; k < 3 * D; k += ED_VS_THREADS) {
            float v = 0.f;
            for (int g = 0; g < p.n_wgs; ++g) v += src[g * p.nv + k];
            p.head[k] = v;
        }
        return;
    }
    const int gi = blk - 4 * p.rounds - 1, i = gi >> 1, w = gi & 1, F = p.F;
    float* out = p.gate[i][w];
    if (!out) return;
    float* dG = vs_lds;           // [F], then the dot product
    const float* G = p.gates + ((int64_t)i * 2 + w) * F;
    const float* src = p.colpart + ((int64_t)i * ED_CS_N + (w == 0 ? ED_CS_GATE_D : ED_CS_GATE_C)) * D;
    for (int f = tid; f < F; f += ED_VS_THREADS) {
        float v = 0.f;
        for (int g = 0; g < p.n_wgs; ++g)
            for (int e = 0; e < p.d; ++e) v += src[g * p.nv + f * p.d + e];
        dG[f] = v;
    }
    __syncthreads();
    if (tid < 64) {
        float s = 0.f;
        for (int f = tid; f < F; f += 64) s = fmaf(G[f], dG[f], s);
        s = ed_wave_sum(s);
        if (tid == 0) dG[F] = s;
    }
    __syncthreads();
    const float dot = dG[F];
    for (int f = tid; f < F; f += ED_VS_THREADS) out[f] = p.inv_tau * G[f] * (dG[f] - dot);
}

struct EdBwdPlan {
    int D, ld, tpw, n_kinds, S;
    int kinds[ED_WK_N];
    bool want_w;
    int zp, zq, zb;
    int64_t slice_rows, nv;
    size_t lds, gates_bytes, col_bytes, z_bytes, partial_bytes, ws_bytes;
};

size_t ed_bwd_lds(int F, int D) { return (4 * (size_t)ED_BWD_R * ed_ld(D) + 2 * (size_t)F + 2 * ED_BWD_R) * sizeof(float); }

bool ed_bwd_supported(const dctr_edcn_args_t* a) {
    if (a->fields < 1 || a->dim < 1 || a->cross_num < 1 || a->cross_num > ED_MAX_ROUNDS || (int64_t)a->fields * a->dim > (1 << 24)) return false;
    if (a->mode != DCTR_CROSS_VECTOR && a->mode != DCTR_CROSS_MATRIX) return false;
    if (a->bridge != DCTR_EDCN_BRIDGE_ADD && a->bridge != DCTR_EDCN_BRIDGE_HADAMARD && a->bridge != DCTR_EDCN_BRIDGE_CONCAT) return false;
    if (!ed_fused_act(a->activation) || (a->bridge == DCTR_EDCN_BRIDGE_CONCAT && !ed_fused_act(a->bridge_activation))) return false;
    if (a->bn_scale || a->bn_shift || a->route == DCTR_EDCN_ROUTE_LAYERED) return false;
    return ed_bwd_lds(a->fields, a->fields * a->dim) <= DCTR_LDS_MAX;
}

size_t ed_round16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

void ed_bwd_plan(const dctr_edcn_train_args_t* t, EdBwdPlan* pl) {
    const dctr_edcn_args_t* a = &t->fwd;
    const int D = a->fields * a->dim, L = a->cross_num;
    const size_t B = (size_t)(a->batch > 0 ? a->batch : 0);
    pl->D = D;
    pl->ld = ed_ld(D);
    pl->tpw = ed_tpw(D);
    pl->lds = ed_bwd_lds(a->fields, D);
    const bool matrix = a->mode == DCTR_CROSS_MATRIX, concat = a->bridge == DCTR_EDCN_BRIDGE_CONCAT;
    pl->n_kinds = 0;
    pl->kinds[pl->n_kinds++] = ED_WK_DNN;
    if (matrix) pl->kinds[pl->n_kinds++] = ED_WK_CROSS;
    if (concat) {
        pl->kinds[pl->n_kinds++] = ED_WK_BRIDGE_C;
        pl->kinds[pl->n_kinds++] = ED_WK_BRIDGE_H;
    }
    pl->want_w = t->d_dnn_w || (matrix && t->d_cross_w) || (concat && t->d_bridge_w);
    pl->zq = D;
    pl->zb = matrix ? 2 * D : D;
    pl->zp = (1 + (matrix ? 1 : 0) + (concat ? 1 : 0)) * D;
    pl->nv = (int64_t)L * ED_CS_N * D + 3 * (int64_t)D;
    pl->gates_bytes = ed_round16((size_t)L * 2 * a->fields * 4);
    pl->col_bytes = ed_round16((size_t)ED_BWD_WGS * pl->nv * 4);
    pl->z_bytes = pl->want_w ? ed_round16((size_t)L * B * pl->zp * 4) : 0;
    pl->S = 0;
    pl->slice_rows = 0;
    pl->partial_bytes = 0;
    if (pl->want_w) {
        int64_t S = t->slices;
        if (S == 0) {
            S = dctr_ceil_div((int64_t)B, ED_BWD_SLICE_ROWS);
            if (S > ED_BWD_AUTO_SLICES) S = ED_BWD_AUTO_SLICES;
        }
        const int64_t by_rows = dctr_ceil_div((int64_t)B, 4);
        if (S > by_rows) S = by_rows;
        if (S < 1) S = 1;
        pl->S = (int)S;
        pl->slice_rows = (dctr_ceil_div((int64_t)B, S) + 3) / 4 * 4;
        if (pl->slice_rows < 4) pl->slice_rows = 4;
        pl->partial_bytes = (size_t)S * L * pl->n_kinds * D * D * 4;
    }
    pl->ws_bytes = pl->gates_bytes + pl->col_bytes + pl->z_bytes + pl->partial_bytes;
}

int ed_bwd_check(const dctr_edcn_train_args_t* t) {
    DCTR_REQUIRE(t, DCTR_E_NULL, "edcn_bwd: null args");
    int rc = edcn_check(&t->fwd);
    if (rc != DCTR_OK) return rc;
    const int64_t D = (int64_t)t->fwd.fields * t->fwd.dim;
    DCTR_REQUIRE(!t->d_out || t->d_out_stride >= 3 * D, DCTR_E_DIM, "edcn_bwd: d_out_stride %lld < 3 * fields * dim = %lld",
                 (long long)t->d_out_stride, (long long)(3 * D));
    DCTR_REQUIRE(!t->dx || (t->dx_offset >= 0 && t->dx_offset + D <= t->dx_stride), DCTR_E_DIM,
                 "edcn_bwd: dx columns [%lld, %lld) in rows of %lld", (long long)t->dx_offset, (long long)(t->dx_offset + D),
                 (long long)t->dx_stride);
    DCTR_REQUIRE(t->accumulate == 0 || t->accumulate == 1, DCTR_E_ENUM, "edcn_bwd: accumulate = %d", t->accumulate);
    DCTR_REQUIRE(t->slices >= 0 && t->slices <= ED_BWD_MAX_SLICES, DCTR_E_DIM, "edcn_bwd: slices = %d: 0 (the library's choice) or 1 .. %d",
                 t->slices, ED_BWD_MAX_SLICES);
    return DCTR_OK;
}

}  // namespace

extern "C" int dctr_edcn_bwd_supported(const dctr_edcn_train_args_t* t) { return t && ed_bwd_supported(&t->fwd) ? 1 : 0; }

extern "C" size_t dctr_edcn_bwd_workspace_bytes(const dctr_edcn_train_args_t* t) {
    if (!t || ed_bwd_check(t) != DCTR_OK || !ed_bwd_supported(&t->fwd)) return 0;
    EdBwdPlan pl;
    ed_bwd_plan(t, &pl);
    return pl.ws_bytes;
}

extern "C" int dctr_edcn_bwd(const dctr_edcn_train_args_t* t, void* stream) {
    int rc = ed_bwd_check(t);
    if (rc != DCTR_OK) return rc;
    const dctr_edcn_args_t* a = &t->fwd;
    DCTR_REQUIRE(ed_bwd_supported(a), DCTR_E_UNSUPPORTED,
                 "edcn_bwd: %d fields of dim %d, %d rounds, bridge %d, activations %d / %d%s: not the backward's (dctr_edcn_bwd_supported)",
                 a->fields, a->dim, a->cross_num, a->bridge, a->activation, a->bridge_activation, a->bn_scale ? ", a BatchNormalization affine" : "");
    const int D = a->fields * a->dim, L = a->cross_num, F = a->fields;
    const bool matrix = a->mode == DCTR_CROSS_MATRIX, concat = a->bridge == DCTR_EDCN_BRIDGE_CONCAT;
    DCTR_REQUIRE(a->x && a->gates && a->cross_w && a->cross_b && a->dnn_w && a->dnn_b, DCTR_E_NULL,
                 "edcn_bwd: null x / gates / cross_w / cross_b / dnn_w / dnn_b");
    DCTR_REQUIRE(!concat || a->bridge_w, DCTR_E_NULL, "edcn_bwd: the concatenation bridge needs bridge_w");
    bool aligned = true;
    for (int i = 0; i < L; ++i) {
        DCTR_REQUIRE(a->gates[2 * i] && a->gates[2 * i + 1] && a->cross_w[i] && a->cross_b[i] && a->dnn_w[i], DCTR_E_NULL,
                     "edcn_bwd: round %d: null weight", i);
        DCTR_REQUIRE(!concat || a->bridge_w[i], DCTR_E_NULL, "edcn_bwd: round %d: null bridge weight", i);
        aligned = aligned && (!matrix || dctr_aligned16(a->cross_w[i]));
    }
    DCTR_REQUIRE(t->tape, DCTR_E_NULL, "edcn_bwd: null tape (dctr_edcn_train_fwd writes it)");
    DCTR_REQUIRE(dctr_aligned16(t->tape), DCTR_E_ALIGN, "edcn_bwd: tape not 16-B aligned");
    DCTR_REQUIRE(t->d_logit || t->d_out, DCTR_E_NULL, "edcn_bwd: neither d_logit nor d_out");
    DCTR_REQUIRE(!t->d_logit || a->head_w, DCTR_E_NULL, "edcn_bwd: d_logit without head_w");
    DCTR_REQUIRE(!t->d_head_w || t->d_logit, DCTR_E_NULL, "edcn_bwd: d_head_w without d_logit");
    DCTR_REQUIRE(concat || (!t->d_bridge_w && !t->d_bridge_b), DCTR_E_NULL, "edcn_bwd: d_bridge_w / d_bridge_b exist with the concatenation bridge only");
    EdBwdPlan pl;
    ed_bwd_plan(t, &pl);
    const hipStream_t st = (hipStream_t)stream;
    const size_t DD = (size_t)D * D;
    if (a->batch == 0) {
        // an empty batch: the sums over it are zeros (dx has no rows)
        hipError_t e = hipSuccess;
        for (int i = 0; i < L && e == hipSuccess; ++i) {
            for (int w = 0; w < 2 && e == hipSuccess; ++w)
                if (t->d_gates && t->d_gates[2 * i + w]) e = hipMemsetAsync(t->d_gates[2 * i + w], 0, (size_t)F * 4, st);
            if (e == hipSuccess && t->d_cross_w && t->d_cross_w[i]) e = hipMemsetAsync(t->d_cross_w[i], 0, (matrix ? DD : (size_t)D) * 4, st);
            if (e == hipSuccess && t->d_cross_b && t->d_cross_b[i]) e = hipMemsetAsync(t->d_cross_b[i], 0, (size_t)D * 4, st);
            if (e == hipSuccess && t->d_dnn_w && t->d_dnn_w[i]) e = hipMemsetAsync(t->d_dnn_w[i], 0, DD * 4, st);
            if (e == hipSuccess && t->d_dnn_b && t->d_dnn_b[i]) e = hipMemsetAsync(t->d_dnn_b[i], 0, (size_t)D * 4, st);
            if (e == hipSuccess && t->d_bridge_w && t->d_bridge_w[i]) e = hipMemsetAsync(t->d_bridge_w[i], 0, 2 * DD * 4, st);
            if (e == hipSuccess && t->d_bridge_b && t->d_bridge_b[i]) e = hipMemsetAsync(t->d_bridge_b[i], 0, (size_t)D * 4, st);
        }
        if (e == hipSuccess && t->d_head_w) e = hipMemsetAsync(t->d_head_w, 0, 3 * (size_t)D * 4, st);
        DCTR_REQUIRE(e == hipSuccess, (int)e, "edcn_bwd: %s", hipGetErrorString(e));
        return DCTR_OK;
    }
    DCTR_REQUIRE_WORKSPACE("edcn_bwd", "dctr_edcn_bwd_workspace_bytes", t->workspace, t->workspace_bytes, pl.ws_bytes);
    char* ws = (char*)t->workspace;
    float* gates_ws = (float*)ws;
    float* colpart = (float*)(ws + pl.gates_bytes);
    float* z = pl.want_w ? (float*)(ws + pl.gates_bytes + pl.col_bytes) : nullptr;
    float* partials = pl.want_w ? (float*)(ws + pl.gates_bytes + pl.col_bytes + pl.z_bytes) : nullptr;
    const int64_t n_tiles = dctr_ceil_div(a->batch, (int64_t)ED_BWD_R);
    int64_t cap = dctr_n_cus();
    if (cap > ED_BWD_WGS) cap = ED_BWD_WGS;
    const int n_wgs = (int)(n_tiles < cap ? n_tiles : cap);
    {
        EdBwdRow p = {};
        p.batch = a->batch;
        p.x = a->x + a->x_offset;
        p.x_stride = a->x_stride;
        p.tape = t->tape;
        p.F = F;
        p.d = a->dim;
        p.D = D;
        p.rounds = L;
        p.mode = a->mode;
        p.bridge = a->bridge;
        p.act = a->activation;
        p.bridge_act = a->bridge_activation;
        p.ld = pl.ld;
        p.want_head = t->d_head_w ? 1 : 0;
        p.inv_tau = a->inv_tau;
        for (int i = 0; i < L; ++i) {
            EdBwdRound& r = p.rd[i];
            r.g_deep = a->gates[2 * i];
            r.g_cross = a->gates[2 * i + 1];
            r.cross_w = a->cross_w[i];
            r.cross_b = a->cross_b[i];
            r.dnn_w = a->dnn_w[i];
            r.bridge_w = concat ? a->bridge_w[i] : nullptr;
        }
        p.head_w = a->head_w;
        p.d_logit = t->d_logit;
        p.d_out = t->d_out;
        p.d_out_stride = t->d_out_stride;
        p.dx = t->dx ? t->dx + t->dx_offset : nullptr;
        p.dx_stride = t->dx_stride;
        p.accumulate = t->accumulate;
        p.z = z;
        p.zp = pl.zp;
        p.zq = pl.zq;
        p.zb = pl.zb;
        p.colpart = colpart;
        p.nv = pl.nv;
        p.gates_out = gates_ws;
        const int tpw = aligned ? pl.tpw : 1;    // (tile_gemm_kn's 8- / 16-byte loads of the matrix cross kernel need it aligned)
        const void* fn = tpw == 4 ? (const void*)edcn_bwd_row_kernel<4> : tpw == 2 ? (const void*)edcn_bwd_row_kernel<2>
                                                                                   : (const void*)edcn_bwd_row_kernel<1>;
        static thread_local size_t granted[3][DCTR_MAX_DEVICES] = {{0}};
        hipError_t e = dctr_grant_lds(fn, pl.lds, granted[tpw == 4 ? 2 : tpw == 2 ? 1 : 0]);
        DCTR_REQUIRE(e == hipSuccess, (int)e, "edcn_bwd: cannot raise dynamic LDS: %s", hipGetErrorString(e));
        const dim3 grid((unsigned)n_wgs), block(ED_THREADS);
        if (tpw == 4)
            DCTR_LAUNCH(edcn_bwd_row_kernel<4>, grid, block, pl.lds, st, p);
        else if (tpw == 2)
            DCTR_LAUNCH(edcn_bwd_row_kernel<2>, grid, block, pl.lds, st, p);
        else
            DCTR_LAUNCH(edcn_bwd_row_kernel<1>, grid, block, pl.lds, st, p);
        rc = dctr_launch_status("dctr_edcn_bwd (row pass)");
        if (rc != DCTR_OK) return rc;
    }
    if (pl.want_w) {
        EdBwdWg p = {};
        EdBwdWsum q = {};
        p.batch = a->batch;
        p.slice_rows = pl.slice_rows;
        p.x = a->x + a->x_offset;
        p.x_stride = a->x_stride;
        p.tape = t->tape;
        p.z = z;
        p.D = q.D = D;
        p.rounds = q.rounds = L;
        p.zp = pl.zp;
        p.zq = pl.zq;
        p.zb = pl.zb;
        p.n_kinds = q.n_kinds = pl.n_kinds;
        for (int k = 0; k < pl.n_kinds; ++k) p.kinds[k] = q.kinds[k] = pl.kinds[k];
        p.partials = partials;
        q.partials = partials;
        q.gates = gates_ws;
        q.d = a->dim;
        q.F = F;
        q.S = pl.S;
        for (int i = 0; i < L; ++i) {
            q.out[i][ED_WK_DNN] = t->d_dnn_w ? t->d_dnn_w[i] : nullptr;
            q.out[i][ED_WK_CROSS] = matrix && t->d_cross_w ? t->d_cross_w[i] : nullptr;
            q.out[i][ED_WK_BRIDGE_C] = concat && t->d_bridge_w ? t->d_bridge_w[i] : nullptr;
            q.out[i][ED_WK_BRIDGE_H] = q.out[i][ED_WK_BRIDGE_C] ? q.out[i][ED_WK_BRIDGE_C] + DD : nullptr;
        }
        const int MT = (D + 15) >> 4, NTL = (D + 63) >> 6;
        const dim3 grid((unsigned)dctr_ceil_div((int64_t)MT * NTL, ED_WG_THREADS / 64), (unsigned)pl.S, (unsigned)(L * pl.n_kinds));
        DCTR_LAUNCH(edcn_bwd_wgrad_kernel, grid, dim3(ED_WG_THREADS), 0, st, p);
        rc = dctr_launch_status("dctr_edcn_bwd (weight-gradient pass)");
        if (rc != DCTR_OK) return rc;
        const dim3 sgrid((unsigned)dctr_ceil_div((int64_t)DD, ED_VS_THREADS), (unsigned)(L * pl.n_kinds));
        DCTR_LAUNCH(edcn_bwd_wsum_kernel, sgrid, dim3(ED_VS_THREADS), 0, st, q);
        rc = dctr_launch_status("dctr_edcn_bwd (weight-gradient sum)");
        if (rc != DCTR_OK) return rc;
    }
    {
        EdBwdVsum v = {};
        v.D = D;
        v.d = a->dim;
        v.F = F;
        v.rounds = L;
        v.n_wgs = n_wgs;
        v.inv_tau = a->inv_tau;
        v.nv = pl.nv;
        v.colpart = colpart;
        v.gates = gates_ws;
        for (int i = 0; i < L; ++i) {
            v.vec[i][0] = t->d_cross_b ? t->d_cross_b[i] : nullptr;
            v.vec[i][1] = t->d_dnn_b ? t->d_dnn_b[i] : nullptr;
            v.vec[i][2] = concat && t->d_bridge_b ? t->d_bridge_b[i] : nullptr;
            v.vec[i][3] = !matrix && t->d_cross_w ? t->d_cross_w[i] : nullptr;
            v.gate[i][0] = t->d_gates ? t->d_gates[2 * i] : nullptr;
            v.gate[i][1] = t->d_gates ? t->d_gates[2 * i + 1] : nullptr;
        }
        v.head = t->d_head_w;
        DCTR_LAUNCH(edcn_bwd_vsum_kernel, dim3((unsigned)(6 * L + 1)), dim3(ED_VS_THREADS), ((size_t)F + 1) * sizeof(float), st, v);
    }
    return dctr_launch_status("dctr_edcn_bwd");
}
