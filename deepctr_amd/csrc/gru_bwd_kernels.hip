// Backward of dctr_gru_fwd (gru_kernels.hip) for ONE DynamicGRU layer: backpropagation through all T steps in one launch.
//
// The forward saved its sequence h_seq [B, T, E]; nothing else.  A workgroup of 4 waves owns a tile of 16 samples (the M of
// v_mfma_f32_16x16x4_f32) and walks the steps from the tile's longest sample down to 0 with the gradient dh of the state in LDS.
// Per step, five phases with one barrier each:
//   L. x_t (scaled by its score with scale_input) and h_{t-1} (h_seq's row t - 1, zero at t = 0) into LDS for the rows with
//      t < length, zeros for the others; d_out's row is added to dh (sequence output), or d_out at t = length - 1 (final state);
//   G. [r | u] = sigmoid([x_t | h_{t-1}] Wg + bg) exactly as the forward's gate phase (gru_device.h: gru_gemm), r, r h, u to LDS;
//   C. c = tanh([x_t | r h] Wc + bc) the same way; in the accumulator layout the cell's gradient: dzc = dc (1 - c^2),
//      dzu = du u (1 - u), dh <- dh u' (or dh (1 - a)), the per-element share of d a_t; rows past their length keep dh and give zeros;
//   D1. [dx_c | d(rh)] = dzc Wc^T from the SAME weight copy (the B operand walks a weight row: no transposed copy),
//      dzr = d(rh) h_{t-1} r (1 - r), dh += d(rh) r;  dWc += [x_t | r h]^T dzc with the tile's 16 rows as the reduction (4 MFMAs per
//      16 x 16 tile of the gradient), dbc += column sums;
//   D2. [dx_g | dh_g] = [dzr | dzu] Wg^T, dx_t = dx_c + dx_g to HBM, dh += dh_g;  dWg += [x_t | h_{t-1}]^T [dzr | dzu], dbg.
// d a_t is reduced over the row by 16 lanes with shuffles in a fixed order.  dx, d_att and dh use no atomics: the same bits on every
// call.  The 6 E^2 + 3 E weight-gradient sums stay in LDS over all steps and all tiles of the workgroup and leave with one atomicAdd
// per element and workgroup; the grid is bounded (2 workgroups per compute unit, or max_blocks).
// RESIDENT route: Wg, Wc and the biases in LDS next to the sums and the 11 tiles (E <= 48); STREAMED: the same code with the weights
// read from global / L2 (E <= 65).  From E = 66 the sums and tiles alone pass the 160 KiB: DCTR_E_UNSUPPORTED.
//
// Cost model per sample and step: 6 E^2 MACs recomputed + 12 E^2 for the four gradient products.
#include <math.h>
#include "dctr_common.h"
#include "tile_route.h"
#include "mfma_tile.h"
#include "gru_device.h"

namespace {

using dctr::gru_gemm;
using dctr::gru_pitch;

constexpr int GB_THREADS = 256;
constexpr int GB_WAVES = GB_THREADS / 64;
constexpr int GB_ROWS = 16;                     // samples of a tile
constexpr int GB_TILES = 11;                    // X, HP, RH, R, U, DH, DZC, DZR, DZU, DXC, DA
constexpr int GB_NW = DCTR_GRU_LAYER_PTRS;

struct GbParams {
    const float* x;
    int64_t batch, x_stride, x_row_stride;
    const int32_t* len;
    const float* att;
    int64_t att_stride;
    int32_t T, E, cell, scale_input, return_sequence;
    int32_t ld, KQ, ldwg, ldwc;
    const float* W[GB_NW];
    float* dW[GB_NW];
    const float* h;
    int64_t h_stride, h_row_stride;
    const float* dout;
    int64_t dout_stride, dout_row_stride;
    float* dx;
    int64_t dx_stride, dx_row_stride;
    float* datt;
    int64_t datt_stride;
    int32_t accumulate;
};

// C[16 x 16] = A[16 x K] W[n_base + j, k_off : k_off + K]^T: the B operand of lane (g, j) walks row n_base + j of W (row pitch ldw),
// so the product with the transposed weight reads the forward's copy.  Rows past n_last are clamped (the caller discards them), A is
// zero-padded to 4 KQ columns.
__device__ __forceinline__ dctr::f32x4 gb_gemm_t(const float* A, int lda, int K, int KQ, const float* W, int ldw, int k_off, int n_base,
                                                 int n_last, dctr::f32x4 acc0) {
    const int lane = threadIdx.x & 63, g = lane >> 4, j = lane & 15;
    const float* arow = A + j * lda + g * KQ;
    const float* wrow = W + min(n_base + j, n_last) * ldw + k_off;
    dctr::f32x4 acc1 = {0.f, 0.f, 0.f, 0.f};
    for (int t0 = 0; t0 < KQ; t0 += 4) {
        const float4 a4 = *reinterpret_cast<const float4*>(arow + t0);
        float b[4];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) b[tt] = wrow[min(g * KQ + t0 + tt, K - 1)];
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.x, b[0], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.y, b[1], acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.z, b[2], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.w, b[3], acc1, 0, 0, 0);
    }
    return acc0 + acc1;
}

// aw[e0 + 4 g + r][c0 + j] += sum_rows A[row][e0 + 4 g + r] B[row][c0 + j] for the rows e < E and columns c < E of one 16 x 16 tile:
// the 16 rows of the sample tile are the reduction.  Columns of A and B past E are the tiles' zero padding.
__device__ __forceinline__ void gb_outer(const float* A, const float* B, int ld, int E, int et, int ct, float* aw, int ldaw) {
    const int lane = threadIdx.x & 63, g = lane >> 4, j = lane & 15;
    const float* ap = A + g * ld + et * 16 + j;
    const float* bp = B + g * ld + ct * 16 + j;
    dctr::f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k0 = 0; k0 < GB_ROWS; k0 += 4) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[k0 * ld], bp[k0 * ld], acc, 0, 0, 0);
    const int col = ct * 16 + j, e0 = et * 16 + 4 * g;
    if (col < E) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (e0 + r < E) aw[(e0 + r) * ldaw + col] += acc[r];
    }
}

template <bool RESIDENT>
__global__ __launch_bounds__(GB_THREADS) void gru_bwd_kernel(GbParams p) {
    extern __shared__ __attribute__((aligned(16))) float gb_lds[];
    const int E = p.E, T = p.T, ld = p.ld, KQ = p.KQ;
    const int tile = GB_ROWS * ld;
    int* lens = reinterpret_cast<int*>(gb_lds);
    float* tiles = gb_lds + GB_ROWS;
    float* X = tiles;
    float* HP = X + tile;
    float* RH = HP + tile;
    float* R = RH + tile;
    float* U = R + tile;
    float* DH = U + tile;
    float* DZC = DH + tile;
    float* DZR = DZC + tile;
    float* DZU = DZR + tile;
    float* DXC = DZU + tile;
    float* DA = DXC + tile;
    // the weight-gradient sums: dWg [2E, 2E], dbg [2E], dWc [2E, E], dbc [E]
    float* AWg = tiles + GB_TILES * tile;
    float* Abg = AWg + 4 * E * E;
    float* AWc = Abg + 2 * E;
    float* Abc = AWc + 2 * E * E;
    const int acc_floats = 6 * E * E + 3 * E;
    float* wl = AWg + ((acc_floats + 3) & ~3);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, j = lane & 15;
    const int ldwg = RESIDENT ? p.ldwg : 2 * E, ldwc = RESIDENT ? p.ldwc : E;
    const float* Wg = RESIDENT ? wl : p.W[0];
    const float* Wc = RESIDENT ? Wg + 2 * E * ldwg : p.W[2];
    const float* bg = RESIDENT ? Wc + 2 * E * ldwc : p.W[1];
    const float* bc = RESIDENT ? bg + 2 * E : p.W[3];
    if (RESIDENT) {
        float* d = wl;
        for (int e = tid; e < 2 * E * 2 * E; e += GB_THREADS) d[(e / (2 * E)) * ldwg + e % (2 * E)] = p.W[0][e];
        d += 2 * E * ldwg;
        for (int e = tid; e < 2 * E * E; e += GB_THREADS) d[(e / E) * ldwc + e % E] = p.W[2][e];
        d += 2 * E * ldwc;
        for (int e = tid; e < 2 * E; e += GB_THREADS) d[e] = p.W[1][e];
        for (int e = tid; e < E; e += GB_THREADS) d[2 * E + e] = p.W[3][e];
    }
    for (int e = tid; e < acc_floats; e += GB_THREADS) AWg[e] = 0.f;
    const bool gated = p.cell != DCTR_GRU_CELL_GRU;
    const bool want_att = p.datt && (gated || p.scale_input);
    const int CT = (E + 15) >> 4;
    const int n_x = GB_ROWS * E;
    const int64_t n_tiles = (p.batch + GB_ROWS - 1) / GB_ROWS;

    for (int64_t tl = blockIdx.x; tl < n_tiles; tl += gridDim.x) {
        const int64_t b0 = tl * GB_ROWS;
        const int nvalid = (int)min((int64_t)GB_ROWS, p.batch - b0);
        __syncthreads();        // the previous tile is done with lens and the tiles
        if (tid < GB_ROWS) lens[tid] = tid < nvalid ? min(max(p.len[b0 + tid], 0), T) : 0;
        // dh = 0 behind the last step, zeros in the K padding of every tile
        for (int e = tid; e < GB_TILES * tile; e += GB_THREADS) tiles[e] = 0.f;
        __syncthreads();
        int t_max = 0;
#pragma unroll
        for (int r = 0; r < GB_ROWS; ++r) t_max = max(t_max, lens[r]);

        for (int t = t_max - 1; t >= 0; --t) {
            // ---- L: the step's operands ------------------------------------------------------------------------------------------
            for (int e = tid; e < n_x; e += GB_THREADS) {
                const int row = e / E, c = e - row * E;
                const int len = lens[row];
                float xv = 0.f, hv = 0.f;
                if (t < len) {
                    xv = p.x[(b0 + row) * p.x_stride + (int64_t)t * p.x_row_stride + c];
                    if (p.scale_input) xv *= p.att[(b0 + row) * p.att_stride + t];
                    if (t > 0) hv = p.h[(b0 + row) * p.h_stride + (int64_t)(t - 1) * p.h_row_stride + c];
                    if (p.return_sequence)
                        DH[row * ld + c] += p.dout[(b0 + row) * p.dout_stride + (int64_t)t * p.dout_row_stride + c];
                    else if (t == len - 1)
                        DH[row * ld + c] += p.dout[(b0 + row) * p.dout_stride + c];
                }
                X[row * ld + c] = xv;
                HP[row * ld + c] = hv;
            }
            float a[4] = {0.f, 0.f, 0.f, 0.f};
            if (gated || p.scale_input) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (t < lens[4 * g + r]) a[r] = p.att[(b0 + 4 * g + r) * p.att_stride + t];
            }
            __syncthreads();
            // ---- G: the gates again ----------------------------------------------------------------------------------------------
            for (int ct = wave; ct < 2 * CT; ct += GB_WAVES) {
                // the halves r | u tile separately, so that a column tile never straddles them
                const int half = ct >= CT, cb = (half ? ct - CT : ct) * 16;
                const dctr::f32x4 acc = gru_gemm<int>(X, HP, ld, E, KQ, Wg + half * E, ldwg, E, cb);
                const int col = cb + j;
                if (col < E) {
                    const float b = bg[half * E + col];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int o = (4 * g + r) * ld + col;
                        const float v = dctr::sigmoidf_(acc[r] + b);
                        if (half) {
                            U[o] = v;
                        } else {
                            R[o] = v;
                            RH[o] = v * HP[o];
                        }
                    }
                }
            }
            __syncthreads();
            // ---- C: the candidate again and the cell's gradient -------------------------------------------------------------------
            for (int ct = wave; ct < CT; ct += GB_WAVES) {
                const dctr::f32x4 acc = gru_gemm<int>(X, RH, ld, E, KQ, Wc, ldwc, E, ct * 16);
                const int col = ct * 16 + j;
                if (col < E) {
                    const float b = bc[col];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = 4 * g + r, o = row * ld + col;
                        const float c = dctr::tanh_fast(acc[r] + b);
                        const float h = HP[o], u = U[o], dh = DH[o];
                        float dc, du, dhp, da = 0.f;
                        if (p.cell == DCTR_GRU_CELL_AGRU) {
                            dc = dh * a[r];
                            dhp = dh * (1.f - a[r]);
                            da = dh * (c - h);
                            du = 0.f;
                        } else {
                            const float up = p.cell == DCTR_GRU_CELL_AUGRU ? (1.f - a[r]) * u : u;
                            const float dup = dh * (h - c);
                            dc = dh * (1.f - up);
                            dhp = dh * up;
                            du = dup;
                            if (p.cell == DCTR_GRU_CELL_AUGRU) {
                                du = dup * (1.f - a[r]);
                                da = -dup * u;
                            }
                        }
                        if (!(t < lens[row])) {
                            dc = 0.f;
                            du = 0.f;
                            da = 0.f;
                            dhp = dh;
                        }
                        DZC[o] = dc * (1.f - c * c);
                        DZU[o] = du * u * (1.f - u);
                        DH[o] = dhp;
                        if (gated) DA[o] = da;
                    }
                }
            }
            __syncthreads();
            // ---- D1: through the candidate kernel -------------------------------------------------------------------------------
            {
                const int n_mm = 2 * CT, n_dw = p.dW[2] ? 2 * CT * CT : 0;
                for (int k = wave; k < n_mm + n_dw; k += GB_WAVES) {
                    if (k < n_mm) {
                        const int half = k >= CT, cb = (half ? k - CT : k) * 16;
                        const dctr::f32x4 z = {0.f, 0.f, 0.f, 0.f};
                        const dctr::f32x4 acc = gb_gemm_t(DZC, ld, E, KQ, Wc, ldwc, 0, half * E + cb, half * E + E - 1, z);
                        const int col = cb + j;
                        if (col < E) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const int o = (4 * g + r) * ld + col;
                                if (half) {
                                    const float rr = R[o];
                                    DZR[o] = acc[r] * HP[o] * (rr * (1.f - rr));
                                    DH[o] += acc[r] * rr;
                                } else {
                                    DXC[o] = acc[r];
                                }
                            }
                        }
                    } else {
                        const int u = k - n_mm, part = u / (CT * CT), rest = u - part * CT * CT, et = rest / CT, ct = rest - et * CT;
                        gb_outer(part ? RH : X, DZC, ld, E, et, ct, AWc + part * E * E, E);
                    }
                }
                if (p.dW[3]) {
                    for (int c = tid; c < E; c += GB_THREADS) {
                        float s = 0.f;
#pragma unroll
                        for (int r = 0; r < GB_ROWS; ++r) s += DZC[r * ld + c];
                        Abc[c] += s;
                    }
                }
            }
            __syncthreads();
            // ---- D2: through the gate kernel ------------------------------------------------------------------------------------
            {
                const int n_mm = 2 * CT, n_dw = p.dW[0] ? 4 * CT * CT : 0;
                for (int k = wave; k < n_mm + n_dw; k += GB_WAVES) {
                    if (k < n_mm) {
                        const int half = k >= CT, cb = (half ? k - CT : k) * 16;
                        const dctr::f32x4 z = {0.f, 0.f, 0.f, 0.f};
                        dctr::f32x4 acc = gb_gemm_t(DZR, ld, E, KQ, Wg, ldwg, 0, half * E + cb, half * E + E - 1, z);
                        acc = gb_gemm_t(DZU, ld, E, KQ, Wg, ldwg, E, half * E + cb, half * E + E - 1, acc);
                        const int col = cb + j;
                        if (col < E) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const int row = 4 * g + r, o = row * ld + col;
                                if (half) {
                                    DH[o] += acc[r];
                                    continue;
                                }
                                const bool live = t < lens[row];
                                float v = live ? DXC[o] + acc[r] : 0.f;
                                if (p.scale_input) {
                                    float xr = 0.f;
                                    if (live) xr = p.x[(b0 + row) * p.x_stride + (int64_t)t * p.x_row_stride + col];
                                    DA[o] = v * xr;
                                    v *= a[r];
                                }
                                if (p.dx && row < nvalid) {
                                    float* d = p.dx + (b0 + row) * p.dx_stride + (int64_t)t * p.dx_row_stride + col;
                                    if (!p.accumulate)
                                        *d = v;
                                    else if (live)
                                        *d += v;
                                }
                            }
                        }
                    } else {
                        const int u = k - n_mm, pa = u / (2 * CT * CT), r1 = u - pa * 2 * CT * CT, pb = r1 / (CT * CT), r2 = r1 - pb * CT * CT;
                        const int et = r2 / CT, ct = r2 - et * CT;
                        gb_outer(pa ? HP : X, pb ? DZU : DZR, ld, E, et, ct, AWg + pa * E * 2 * E + pb * E, 2 * E);
                    }
                }
                if (p.dW[1]) {
                    for (int c = tid; c < 2 * E; c += GB_THREADS) {
                        const float* src = c < E ? DZR + c : DZU + (c - E);
                        float s = 0.f;
#pragma unroll
                        for (int r = 0; r < GB_ROWS; ++r) s += src[r * ld];
                        Abg[c] += s;
                    }
                }
            }
            __syncthreads();
            // ---- d a_t: 16 lanes per row, a fixed order (DA is next written behind two barriers of the following step) ------------
            if (want_att) {
                const int row = tid >> 4, l16 = tid & 15;
                float s = 0.f;
                for (int c = l16; c < E; c += 16) s += DA[row * ld + c];
                s += __shfl_xor(s, 8, 16);
                s += __shfl_xor(s, 4, 16);
                s += __shfl_xor(s, 2, 16);
                s += __shfl_xor(s, 1, 16);
                if (l16 == 0 && row < nvalid) p.datt[(b0 + row) * p.datt_stride + t] = s;
            }
        }
        // the steps past the tile's longest sample
        if (p.dx && !p.accumulate) {
            const int64_t n = (int64_t)(T - t_max) * E;
            for (int64_t e = tid; e < nvalid * n; e += GB_THREADS) {
                const int row = (int)(e / n);
                const int64_t rem = e - row * n;
                const int t = t_max + (int)(rem / E), c = (int)(rem % E);
                p.dx[(b0 + row) * p.dx_stride + (int64_t)t * p.dx_row_stride + c] = 0.f;
            }
        }
        if (want_att) {
            const int n = T - t_max;
            for (int e = tid; e < nvalid * n; e += GB_THREADS) {
                const int row = e / n;
                p.datt[(b0 + row) * p.datt_stride + t_max + (e - row * n)] = 0.f;
            }
        }
    }
    __syncthreads();
    // one atomic per workgroup and weight-gradient element
    const int n_w[GB_NW] = {4 * E * E, 2 * E, 2 * E * E, E};
    const float* src[GB_NW] = {AWg, Abg, AWc, Abc};
#pragma unroll
    for (int m = 0; m < GB_NW; ++m) {
        float* dst = p.dW[m];
        if (!dst) continue;
        for (int i = tid; i < n_w[m]; i += GB_THREADS) atomicAdd(&dst[i], src[m][i]);
    }
}

struct GbPlan {
    bool ok, resident;
    int ld, KQ, ldwg, ldwc;
    size_t lds_bytes;
};

void gb_plan(const dctr_gru_args_t* a, GbPlan* pl) {
    const int64_t E = a->dim;
    pl->ok = false;
    pl->resident = false;
    pl->lds_bytes = 0;
    // (E > 4096 is far past the LDS bound below and keeps its arithmetic in range)
    if (a->n_layers != 1 || (a->scale_input && a->cell != DCTR_GRU_CELL_GRU) || E > 4096) return;
    pl->ld = (int)(((E + 15) & ~(int64_t)15) + 4);
    pl->KQ = (int)(((E + 15) & ~(int64_t)15) >> 2);
    pl->ldwg = gru_pitch((int)(2 * E), pl->KQ);
    pl->ldwc = gru_pitch((int)E, pl->KQ);
    const int64_t acc = (6 * E * E + 3 * E + 3) & ~(int64_t)3;
    const int64_t base = GB_ROWS + (int64_t)GB_TILES * GB_ROWS * pl->ld + acc;
    const int64_t w = 2 * E * pl->ldwg + 2 * E * pl->ldwc + 3 * E;
    if ((size_t)base * 4 > DCTR_LDS_MAX) return;
    pl->ok = true;
    pl->resident = (size_t)(base + w) * 4 <= DCTR_LDS_MAX && a->route != DCTR_GRU_ROUTE_STREAMED;
    pl->lds_bytes = (size_t)(base + (pl->resident ? w : 0)) * 4;
}

// the forward's size checks (gru_check of gru_kernels.hip; out / out strides / workspace are not read) and the backward's own
int gb_check(const dctr_gru_bwd_args_t* b) {
    DCTR_REQUIRE(b, DCTR_E_NULL, "gru_bwd: null args");
    const dctr_gru_args_t* a = &b->fwd;
    DCTR_REQUIRE(a->batch >= 0 && a->seq_len >= 1 && a->dim >= 1, DCTR_E_DIM, "gru_bwd: bad sizes");
    DCTR_REQUIRE(a->n_layers >= 1 && a->n_layers <= 2, DCTR_E_DIM, "gru_bwd: n_layers must be 1 or 2, got %d", a->n_layers);
    DCTR_REQUIRE(a->dim <= (1 << 20), DCTR_E_DIM, "gru_bwd: dim %d exceeds 2^20", a->dim);
    DCTR_REQUIRE(a->cell >= DCTR_GRU_CELL_GRU && a->cell <= DCTR_GRU_CELL_AUGRU, DCTR_E_ENUM, "gru_bwd: unknown cell %d", a->cell);
    DCTR_REQUIRE((uint32_t)(a->scale_input | a->return_sequence) <= 1u && (uint32_t)b->accumulate <= 1u, DCTR_E_ENUM,
                 "gru_bwd: scale_input, return_sequence and accumulate must be 0 or 1");
    DCTR_REQUIRE(a->route >= DCTR_GRU_ROUTE_AUTO && a->route <= DCTR_GRU_ROUTE_STREAMED, DCTR_E_ENUM, "gru_bwd: unknown route %d", a->route);
    DCTR_REQUIRE(b->max_blocks >= 0, DCTR_E_DIM, "gru_bwd: max_blocks = %d", b->max_blocks);
    const int64_t block = ((int64_t)a->seq_len - 1);
    DCTR_REQUIRE(a->x_row_stride >= a->dim && a->x_stride >= block * a->x_row_stride + a->dim, DCTR_E_DIM,
                 "gru_bwd: x strides smaller than the [seq_len, dim] block");
    DCTR_REQUIRE(b->h_row_stride >= a->dim && b->h_stride >= block * b->h_row_stride + a->dim, DCTR_E_DIM,
                 "gru_bwd: h_seq strides smaller than the [seq_len, dim] block");
    if (a->return_sequence)
        DCTR_REQUIRE(b->d_out_row_stride >= a->dim && b->d_out_stride >= block * b->d_out_row_stride + a->dim, DCTR_E_DIM,
                     "gru_bwd: d_out strides smaller than the [seq_len, dim] block");
    else
        DCTR_REQUIRE(b->d_out_stride >= a->dim, DCTR_E_DIM, "gru_bwd: d_out_stride < dim");
    if (b->dx)
        DCTR_REQUIRE(b->dx_row_stride >= a->dim && b->dx_stride >= block * b->dx_row_stride + a->dim, DCTR_E_DIM,
                     "gru_bwd: dx strides smaller than the [seq_len, dim] block");
    if (a->cell != DCTR_GRU_CELL_GRU || a->scale_input) {
        DCTR_REQUIRE(a->att_stride >= a->seq_len, DCTR_E_DIM, "gru_bwd: att_stride < seq_len");
        DCTR_REQUIRE(!b->d_att || b->d_att_stride >= a->seq_len, DCTR_E_DIM, "gru_bwd: d_att_stride < seq_len");
    }
    return DCTR_OK;
}

}  // namespace

extern "C" int dctr_gru_bwd_supported(const dctr_gru_bwd_args_t* b) {
    if (gb_check(b) != DCTR_OK) return 0;
    GbPlan pl;
    gb_plan(&b->fwd, &pl);
    if (b->fwd.route == DCTR_GRU_ROUTE_RESIDENT && !pl.resident) return 0;
    return pl.ok ? 1 : 0;
}

extern "C" size_t dctr_gru_bwd_workspace_bytes(const dctr_gru_bwd_args_t* b) {
    (void)b;                    // every supported shape runs out of the LDS
    return 0;
}

extern "C" int dctr_gru_bwd(const dctr_gru_bwd_args_t* b, void* stream) {
    int rc = gb_check(b);
    if (rc != DCTR_OK) return rc;
    const dctr_gru_args_t* a = &b->fwd;
    GbPlan pl;
    gb_plan(a, &pl);
    DCTR_REQUIRE(pl.ok, DCTR_E_UNSUPPORTED,
                 "gru_bwd: one layer of dim <= 65 (got %d layer(s), dim %d), and scale_input with the plain GRU cell only", a->n_layers, a->dim);
    DCTR_REQUIRE(a->route != DCTR_GRU_ROUTE_RESIDENT || pl.resident, DCTR_E_UNSUPPORTED,
                 "gru_bwd: the weights of dim %d do not fit the resident route's LDS", a->dim);
    DCTR_REQUIRE(a->x && a->lengths && a->layers && b->h_seq && b->d_out, DCTR_E_NULL, "gru_bwd: null x / lengths / layers / h_seq / d_out");
    DCTR_REQUIRE(!(a->cell != DCTR_GRU_CELL_GRU || a->scale_input) || a->att_scores, DCTR_E_NULL,
                 "gru_bwd: the attention-gated cells and scale_input need att_scores");
    for (int m = 0; m < GB_NW; ++m) DCTR_REQUIRE(a->layers[m], DCTR_E_NULL, "gru_bwd: null gate / candidate kernel or bias");
    if (a->batch == 0) return DCTR_OK;
    GbParams p = {};
    p.x = a->x;
    p.batch = a->batch;
    p.x_stride = a->x_stride;
    p.x_row_stride = a->x_row_stride;
    p.len = a->lengths;
    p.att = a->att_scores;
    p.att_stride = a->att_stride;
    p.T = a->seq_len;
    p.E = a->dim;
    p.cell = a->cell;
    p.scale_input = a->scale_input;
    p.return_sequence = a->return_sequence;
    p.ld = pl.ld;
    p.KQ = pl.KQ;
    p.ldwg = pl.ldwg;
    p.ldwc = pl.ldwc;
    for (int m = 0; m < GB_NW; ++m) {
        p.W[m] = a->layers[m];
        p.dW[m] = b->d_layers ? b->d_layers[m] : nullptr;
    }
    p.h = b->h_seq;
    p.h_stride = b->h_stride;
    p.h_row_stride = b->h_row_stride;
    p.dout = b->d_out;
    p.dout_stride = b->d_out_stride;
    p.dout_row_stride = b->d_out_row_stride;
    p.dx = b->dx;
    p.dx_stride = b->dx_stride;
    p.dx_row_stride = b->dx_row_stride;
    p.datt = b->d_att;
    p.datt_stride = b->d_att_stride;
    p.accumulate = b->accumulate;
    const int64_t n_tiles = dctr_ceil_div(a->batch, GB_ROWS);
    const int64_t cap = b->max_blocks > 0 ? (int64_t)b->max_blocks : (int64_t)2 * dctr_n_cus();
    const dim3 grid((unsigned)(n_tiles < cap ? n_tiles : cap)), block(GB_THREADS);
    if (pl.resident) {
        static thread_local size_t granted[DCTR_MAX_DEVICES] = {0};
        hipError_t e = dctr_grant_lds((const void*)gru_bwd_kernel<true>, pl.lds_bytes, granted);
        DCTR_REQUIRE(e == hipSuccess, (int)e, "gru_bwd: cannot raise dynamic LDS: %s", hipGetErrorString(e));
        DCTR_LAUNCH((gru_bwd_kernel<true>), grid, block, pl.lds_bytes, (hipStream_t)stream, p);
    } else {
        static thread_local size_t granted[DCTR_MAX_DEVICES] = {0};
        hipError_t e = dctr_grant_lds((const void*)gru_bwd_kernel<false>, pl.lds_bytes, granted);
        DCTR_REQUIRE(e == hipSuccess, (int)e, "gru_bwd: cannot raise dynamic LDS: %s", hipGetErrorString(e));
        DCTR_LAUNCH((gru_bwd_kernel<false>), grid, block, pl.lds_bytes, (hipStream_t)stream, p);
    }
    return dctr_launch_status("dctr_gru_bwd");
}
