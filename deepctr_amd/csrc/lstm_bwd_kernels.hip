// Backward of dctr_bilstm_train_fwd (lstm_kernels.hip): backpropagation through time of both stacks, all layers and all steps.
//
// The training forward left a tape of h_t and c_t for every (layer, direction, step, sample).  The two stacks are independent between
// x and the merge, so a workgroup of 4 waves owns (a tile of 16 samples — the M of v_mfma_f32_16x16x4_f32 —, a direction) and walks
// that stack's layers from last to first with the layer's gradient sequence DY [T, 16, u] and its masked input sequence IN [T, 16, D]
// in LDS.  DY starts as the merge's backward; a layer overwrites DY[t] with the gradient of its input, which is the next layer's DY;
// layer 0 writes it to the direction's own dx buffer.  A layer's input is rebuilt from the tape (h of the layer below, plus the chain
// of residual inputs in the forward's order of additions, so the bits are the forward's) and multiplied by the layer's mask once.
// Per step, in the reverse of the direction's walk, two phases with one barrier each:
//   G. z = [in_t m | h_prev] [W; U] + b exactly as the forward's step (lstm_device.h: lstm_gemm4, the h part skipped at the first
//      step), the gates; in the accumulator layout the lane that owns unit j of a sample reads c_prev and c_t from the tape and forms
//      dc, dz = [dz_i | dz_f | dz_g | dz_o] (four A-operand tiles in LDS) and dc_prev = dc f (in LDS, only it touches the element);
//      dz and the rows [in_t m | h_prev] also go to the workspace for the weight gradients;
//   D. [d(in m)_t | dh_prev] = dz [W; U]^T from the SAME weight copy (the B operand walks a weight row: no transposed copy), four
//      chained products over the gate quarters; d_in_t = d(in m)_t m (+ DY[t] when the layer is residual) -> DY[t] / dx, dh_prev -> DH;
//      h of the step after next is loaded from the tape for the next G.
// RESIDENT route: W, U and b of the current (layer, direction) in LDS next to the tiles, pitched as the forward's; STREAMED: the same
// code with the weights read from global / L2.  Tiles that exceed the 160 KiB: DCTR_E_UNSUPPORTED (no workspace route).
// The weight gradients: 8u^2 + 4u floats per LSTM do not fit the LDS next to the tiles at u = 64, so ONE dctr_gemm::sgemm_grouped
// launch forms [dW; dU; db] = [in m | h_prev | 1]^T dz of every (layer, direction) from the stored rows, cut into stored k-slices,
// and lstm_bwd_sum_kernel adds the slices in a fixed order into d_layers and the two directions' input gradients into dx.  Three
// launches, no atomics: the same bits on every call.
//
// Cost model per sample: the forward's T x 2 x 4u (D + u) MACs per layer recomputed, as many for dz [W; U]^T and as many for the
// weight gradients.
#include <math.h>
#include "dctr_common.h"
#include "dctr_gemm.h"
#include "tile_route.h"
#include "mfma_tile.h"
#include "lstm_device.h"

// lstm_kernels.hip: the forward's argument checks, and whether the training forward (which writes the tape) takes the shape
int dctr_lstm_check_args(const dctr_lstm_args_t* a);
bool dctr_lstm_train_fwd_fits(const dctr_lstm_args_t* a);

namespace {

using dctr::lstm_gemm4;

constexpr int LB_THREADS = 256;
constexpr int LB_WAVES = LB_THREADS / 64;
constexpr int LB_ROWS = 16;                     // samples of a tile
constexpr int LB_MAX_LAYERS = 4;                // two groups of the grouped GEMM (8) per layer
constexpr int LB_NW = DCTR_LSTM_LAYER_PTRS;
constexpr int LB_SLICE_ROWS = 512;              // rows of [T B] per stored k-slice of the weight-gradient GEMM (at most 32 slices)

struct LbParams {
    const float* x;
    int64_t batch, x_stride, x_row_stride;
    int32_t T, Din, u, L, res_layers, merge, d0, nd;
    int32_t ldx, ld, lda, ldc, KQx, KQh, ldw0, ldw, ldwh;
    const float* W[LB_MAX_LAYERS][LB_NW];
    const float* mask[LB_MAX_LAYERS][2];
    const float* tape;
    const float* dout;
    int64_t dout_stride, dout_row_stride;
    const float* dout_bw;
    int64_t dout_bw_stride, dout_bw_row_stride;
    float* dxw[2];                              // [B, T, Din] per direction, or NULL: dx is not wanted
    float* wdz[LB_MAX_LAYERS][2];               // [T B, 4u] rows (t B + b), or NULL: no weight gradient of this LSTM is wanted
    float* wa[LB_MAX_LAYERS][2];                // [T B, D + u]
};

__device__ __forceinline__ const float* lb_tape(const LbParams& p, int l, int d, int t, int which) {
    return p.tape + ((((int64_t)l * 2 + d) * p.T + t) * 2 + which) * p.batch * p.u;
}

// output of layer l of direction d at (t, sample b, column c), l = -1: x.  h of the highest non-residual layer k <= l (x when every
// layer down to 0 is residual), then h_{k+1} + ., ..., h_l + . : the forward's additions in its order
__device__ __forceinline__ float lb_y(const LbParams& p, int l, int d, int t, int64_t b, int c) {
    int k = l;
    while (k >= 0 && k >= p.L - p.res_layers) --k;
    float v = k < 0 ? p.x[b * p.x_stride + (int64_t)t * p.x_row_stride + c] : lb_tape(p, k, d, t, 0)[b * p.u + c];
    for (++k; k <= l; ++k) v = lb_tape(p, k, d, t, 0)[b * p.u + c] + v;
    return v;
}

// acc += A[16 x K] W[n_base + j, k_off : k_off + K]^T: the B operand of lane (g, j) walks row n_base + j of W (row pitch ldw), so
// the product with the transposed weight reads the forward's copy.  Rows past n_last are clamped (the caller discards them), A is
// zero-padded to 4 KQ columns.  Two accumulators, so that consecutive MFMAs do not depend.
__device__ __forceinline__ void lb_gemm_t(const float* A, int lda, int K, int KQ, const float* wrow, dctr::f32x4& acc0, dctr::f32x4& acc1) {
    const int lane = threadIdx.x & 63, g = lane >> 4, j = lane & 15;
    const float* arow = A + j * lda + g * KQ;
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
}

template <bool RESIDENT>
__global__ __launch_bounds__(LB_THREADS) void bilstm_bwd_kernel(LbParams p) {
    extern __shared__ __attribute__((aligned(16))) float lb_lds[];
    const int T = p.T, Din = p.Din, u = p.u, L = p.L, ld = p.ld, ldc = p.ldc;
    const int st = LB_ROWS * ld, at = LB_ROWS * p.lda;      // a [16, u] tile; an input tile at the wider of the two pitches
    float* DY = lb_lds;                                     // [T] the gradient of the layer's output sequence, then of its input
    float* IN = DY + T * st;                                // [T] the layer's masked input sequence
    float* HP = IN + T * at;                                // h_prev of the step
    float* DH = HP + st;                                    // the gradient reaching h_t from the step behind it
    float* DZ = DH + st;                                    // [4] dz by gate quarter
    float* MK = DZ + 4 * st;                                // the layer's mask in the layout of its input tile
    float* DC = MK + at;                                    // dc_prev
    const int tile_floats = (T + 6) * st + (T + 1) * at + ((LB_ROWS * ldc + 3) & ~3);
    float* wl = lb_lds + tile_floats;                       // RESIDENT only
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, j = lane & 15;
    const int CT = (u + 15) >> 4;
    const int64_t B = p.batch;
    const int64_t n_items = ((B + LB_ROWS - 1) / LB_ROWS) * p.nd;

    for (int64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const int d = p.d0 + (int)(item % p.nd);
        const int64_t b0 = (item / p.nd) * LB_ROWS;
        const int nvalid = (int)min((int64_t)LB_ROWS, B - b0);
        __syncthreads();        // the previous item is done with the tiles
        // zeros in the K padding of every tile and in the rows past the batch
        for (int e = tid; e < tile_floats; e += LB_THREADS) lb_lds[e] = 0.f;
        __syncthreads();
        // ---- the merge's backward ------------------------------------------------------------------------------------------------
        for (int e = tid; e < T * nvalid * u; e += LB_THREADS) {
            const int t = e / (nvalid * u), rem = e - t * (nvalid * u);
            const int row = rem / u, c = rem - row * u;
            const int64_t b = b0 + row;
            float v;
            if (p.merge == DCTR_LSTM_MERGE_NONE && d) {
                v = p.dout_bw[b * p.dout_bw_stride + (int64_t)t * p.dout_bw_row_stride + c];
            } else {
                v = p.dout[b * p.dout_stride + (int64_t)t * p.dout_row_stride + (p.merge == DCTR_LSTM_MERGE_CONCAT && d ? u + c : c)];
                if (p.merge == DCTR_LSTM_MERGE_AVE) v = v / 2.f;
                if (p.merge == DCTR_LSTM_MERGE_MUL) v *= lb_y(p, L - 1, 1 - d, t, b, c);
            }
            DY[t * st + row * ld + c] = v;
        }
        for (int l = L - 1; l >= 0; --l) {
            const int D = l ? u : Din, KQa = l ? p.KQh : p.KQx, lda = l ? ld : p.ldx, ati = LB_ROWS * lda;
            const int CTx = (D + 15) >> 4;
            const int ldwx = RESIDENT ? (l ? p.ldw : p.ldw0) : 4 * u, ldwh = RESIDENT ? p.ldwh : 4 * u;
            const bool res = l >= L - p.res_layers;
            const bool want_in = l > 0 || p.dxw[d] != nullptr;
            const float* Wx = RESIDENT ? wl : p.W[l][3 * d];
            const float* Wh = RESIDENT ? Wx + D * ldwx : p.W[l][3 * d + 1];
            const float* bv = RESIDENT ? Wh + u * ldwh : p.W[l][3 * d + 2];
            float* wdz = p.wdz[l][d];
            float* wa = p.wa[l][d];
            // (the barrier behind the previous layer's last step released IN, MK, HP, DH and the weights)
            if (RESIDENT) {
                float* dst = wl;
                for (int m = 0; m < 2; ++m) {
                    const float* sw = p.W[l][3 * d + m];
                    const int rows = m ? u : D, pitch = m ? ldwh : ldwx;
                    for (int e = tid; e < rows * 4 * u; e += LB_THREADS) {
                        const int row = e / (4 * u);
                        dst[row * pitch + (e - row * 4 * u)] = sw[e];
                    }
                    dst += rows * pitch;
                }
                const float* sb = p.W[l][3 * d + 2];
                for (int e = tid; e < 4 * u; e += LB_THREADS) dst[e] = sb[e];
            }
            {
                const float* mk = p.mask[l][d];
                for (int e = tid; e < ati; e += LB_THREADS) {
                    const int row = e / lda, c = e - row * lda;
                    MK[e] = (row < nvalid && c < D) ? (mk ? mk[(b0 + row) * D + c] : 1.f) : 0.f;
                }
                // the whole pitch: layer 0 and the layers above it lay the tile out differently
                for (int e = tid; e < T * ati; e += LB_THREADS) {
                    const int t = e / ati, rem = e - t * ati;
                    const int row = rem / lda, c = rem - row * lda;
                    float v = 0.f;
                    if (row < nvalid && c < D) {
                        v = lb_y(p, l - 1, d, t, b0 + row, c);
                        if (mk) v *= mk[(b0 + row) * D + c];
                    }
                    IN[e] = v;
                }
                // h_prev of the walk's last step (time T - 2 forwards, 1 backwards), no gradient from behind it
                for (int e = tid; e < LB_ROWS * u; e += LB_THREADS) {
                    const int row = e / u, c = e - row * u;
                    const int tp = d ? 1 : T - 2;
                    HP[row * ld + c] = (T > 1 && row < nvalid) ? lb_tape(p, l, d, tp, 0)[(b0 + row) * u + c] : 0.f;
                    DH[row * ld + c] = 0.f;
                }
            }
            __syncthreads();
            for (int s = T - 1; s >= 0; --s) {
                const int td = d ? T - 1 - s : s;               // the step's time position
                const int tp = d ? td + 1 : td - 1;             // that of the step before it in the walk (s > 0)
                // ---- G: the gates again, the cell's gradient -----------------------------------------------------------------------
                for (int ct = wave; ct < CT; ct += LB_WAVES) {
                    const int col = ct * 16 + j, colc = min(col, u - 1);
                    dctr::f32x4 acc[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float b = bv[q * u + colc];
                        acc[q] = dctr::f32x4{b, b, b, b};
                    }
                    lstm_gemm4<int>(IN + td * ati, lda, D, KQa, Wx, ldwx, u, colc, acc);
                    if (s) lstm_gemm4<int>(HP, ld, u, p.KQh, Wh, ldwh, u, colc, acc);          // h_0 = 0
                    if (col < u) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int row = 4 * g + r, o = row * ld + col;
                            const bool live = row < nvalid;
                            const float ig = dctr::sigmoidf_(acc[0][r]), fg = dctr::sigmoidf_(acc[1][r]);
                            const float og = dctr::sigmoidf_(acc[3][r]), gg = dctr::tanh_fast(acc[2][r]);
                            const float cp = (s && live) ? lb_tape(p, l, d, tp, 1)[(b0 + row) * u + col] : 0.f;     // c_0 = 0
                            const float cc = live ? lb_tape(p, l, d, td, 1)[(b0 + row) * u + col] : 0.f;
                            const float tc = dctr::tanh_fast(cc);
                            const float dh = DH[o] + DY[td * st + o];
                            float* dcp = DC + row * ldc + col;
                            const float dc = (s == T - 1 ? 0.f : *dcp) + dh * og * (1.f - tc * tc);
                            *dcp = dc * fg;
                            float dz[4];
                            dz[0] = dc * gg * (ig * (1.f - ig));
                            dz[1] = dc * cp * (fg * (1.f - fg));
                            dz[2] = dc * ig * (1.f - gg * gg);
                            dz[3] = dh * tc * (og * (1.f - og));
#pragma unroll
                            for (int q = 0; q < 4; ++q) {
                                DZ[q * st + o] = dz[q];
                                if (wdz && live) wdz[((int64_t)td * B + b0 + row) * (4 * u) + q * u + col] = dz[q];
                            }
                        }
                    }
                }
                if (wa) {       // the rows [in_t m | h_prev] of the weight-gradient GEMM
                    const int w = D + u;
                    for (int e = tid; e < nvalid * w; e += LB_THREADS) {
                        const int row = e / w, c = e - row * w;
                        wa[((int64_t)td * B + b0 + row) * w + c] = c < D ? IN[td * ati + row * lda + c] : HP[row * ld + c - D];
                    }
                }
                __syncthreads();
                // ---- D: through the kernels ---------------------------------------------------------------------------------------
                {
                    const int k0 = want_in ? 0 : CTx, k1 = CTx + (s ? CT : 0);             // (dh_prev of the first step goes nowhere)
                    for (int k = k0 + wave; k < k1; k += LB_WAVES) {
                        const bool is_h = k >= CTx;
                        const int cb = (is_h ? k - CTx : k) * 16, N = is_h ? u : D;
                        const float* wrow = (is_h ? Wh : Wx) + min(cb + j, N - 1) * (is_h ? ldwh : ldwx);
                        dctr::f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                        for (int q = 0; q < 4; ++q) lb_gemm_t(DZ + q * st, ld, u, p.KQh, wrow + q * u, acc0, acc1);
                        const dctr::f32x4 acc = acc0 + acc1;
                        const int col = cb + j;
                        if (col < N) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const int row = 4 * g + r;
                                if (is_h) {
                                    DH[row * ld + col] = acc[r];
                                    continue;
                                }
                                float v = acc[r] * MK[row * lda + col];
                                if (res) v += DY[td * st + row * ld + col];                 // (a residual layer has D = u)
                                if (l)
                                    DY[td * st + row * ld + col] = v;
                                else if (row < nvalid)
                                    p.dxw[d][((b0 + row) * T + td) * Din + col] = v;
                            }
                        }
                    }
                    // h_prev of the next step of this loop
                    if (s) {
                        const int tpp = d ? tp + 1 : tp - 1;
                        for (int e = tid; e < LB_ROWS * u; e += LB_THREADS) {
                            const int row = e / u, c = e - row * u;
                            HP[row * ld + c] = (s > 1 && row < nvalid) ? lb_tape(p, l, d, tpp, 0)[(b0 + row) * u + c] : 0.f;
                        }
                    }
                }
                __syncthreads();
            }
        }
    }
}

// the last launch: blockIdx.y < n_groups sums the stored k-slices of [dW; dU; db] of one LSTM in their order and adds them to
// d_layers; blockIdx.y == n_groups adds the directions' input gradients into dx
struct LbSum {
    int32_t n_groups, slices[2 * LB_MAX_LAYERS], D[2 * LB_MAX_LAYERS], u;
    const float* parts[2 * LB_MAX_LAYERS];
    float* dst[2 * LB_MAX_LAYERS][3];
    const float* dxw[2];
    float* dx;
    int64_t batch, dx_stride, dx_row_stride;
    int32_t T, Din, accumulate;
};

__global__ __launch_bounds__(256) void lstm_bwd_sum_kernel(LbSum s) {
    const int gi = (int)blockIdx.y;
    const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    if (gi < s.n_groups) {
        const int N = 4 * s.u, D = s.D[gi];
        const int64_t n = (int64_t)(D + s.u + 1) * N;
        for (int64_t i = i0; i < n; i += step) {
            float v = 0.f;
            for (int k = 0; k < s.slices[gi]; ++k) v += s.parts[gi][k * n + i];
            const int row = (int)(i / N);
            const int m = row < D ? 0 : row < D + s.u ? 1 : 2;
            float* dst = s.dst[gi][m];
            if (dst) dst[i - (int64_t)(m == 0 ? 0 : m == 1 ? D : D + s.u) * N] += v;
        }
    } else if (s.dx) {
        const int64_t n = s.batch * s.T * s.Din;
        for (int64_t i = i0; i < n; i += step) {
            const int c = (int)(i % s.Din);
            const int64_t r = i / s.Din;
            const int t = (int)(r % s.T);
            float v = s.dxw[0][i];
            if (s.dxw[1]) v += s.dxw[1][i];
            float* o = s.dx + (r / s.T) * s.dx_stride + (int64_t)t * s.dx_row_stride + c;
            *o = s.accumulate ? *o + v : v;
        }
    }
}

struct LbPlan {
    bool ok, resident;
    dctr::LstmPitch lp;
    int lda;
    size_t lds_bytes;
    int d0, nd, slices;
    // the workspace, in floats from its start (each block a multiple of 4 floats)
    int64_t dxw[2], wdz[LB_MAX_LAYERS][2], wa[LB_MAX_LAYERS][2], parts[LB_MAX_LAYERS][2], ws_floats;
};

void lb_plan(const dctr_lstm_args_t* a, LbPlan* pl) {
    const int64_t T = a->seq_len, Din = a->in_dim, u = a->units, L = a->n_layers, B = a->batch;
    *pl = LbPlan{};
    // (u, Din or T past 4096 are far past the LDS bound below and keep its arithmetic in range)
    if (a->recurrent_activation != 0 || L > LB_MAX_LAYERS || u > 4096 || Din > 4096 || T > 4096) return;
    dctr_lstm_args_t fa = *a;
    fa.route = DCTR_LSTM_ROUTE_AUTO;
    if (a->route == DCTR_LSTM_ROUTE_WORKSPACE || !dctr_lstm_train_fwd_fits(&fa)) return;
    pl->lp = dctr::lstm_pitches(Din, u);
    pl->lda = pl->lp.ldx > pl->lp.ld ? pl->lp.ldx : pl->lp.ld;
    const int64_t st = (int64_t)LB_ROWS * pl->lp.ld, at = (int64_t)LB_ROWS * pl->lda;
    const int64_t tiles = (T + 6) * st + (T + 1) * at + ((LB_ROWS * (int64_t)pl->lp.ldc + 3) & ~(int64_t)3);
    const int64_t w0 = Din * pl->lp.ldw0 + u * pl->lp.ldwh + 4 * u, w1 = u * pl->lp.ldw + u * pl->lp.ldwh + 4 * u;
    const int64_t w = L > 1 && w1 > w0 ? w1 : w0;
    if ((size_t)tiles * 4 > DCTR_LDS_MAX) return;
    const bool res_fits = (size_t)(tiles + w) * 4 <= DCTR_LDS_MAX;
    if (a->route == DCTR_LSTM_ROUTE_RESIDENT && !res_fits) return;
    pl->ok = true;
    pl->resident = res_fits && a->route != DCTR_LSTM_ROUTE_STREAMED;
    pl->lds_bytes = (size_t)(tiles + (pl->resident ? w : 0)) * 4;
    pl->d0 = a->merge_mode == DCTR_LSTM_MERGE_BW ? 1 : 0;
    pl->nd = (a->merge_mode == DCTR_LSTM_MERGE_FW || a->merge_mode == DCTR_LSTM_MERGE_BW) ? 1 : 2;
    const int64_t rows = T * B;
    pl->slices = rows < 0x7fffffffLL ? dctr_gemm::k_slices((int)rows, LB_SLICE_ROWS) : 1;
    int64_t f = 0;
    auto take = [&f](int64_t n) {
        const int64_t at_ = f;
        f += (n + 3) & ~(int64_t)3;
        return at_;
    };
    for (int d = pl->d0; d < pl->d0 + pl->nd; ++d) pl->dxw[d] = take(B * T * Din);
    for (int l = 0; l < L; ++l)
        for (int d = pl->d0; d < pl->d0 + pl->nd; ++d) {
            const int64_t D = l ? u : Din;
            pl->wdz[l][d] = take(rows * 4 * u);
            pl->wa[l][d] = take(rows * (D + u));
            pl->parts[l][d] = take((int64_t)pl->slices * (D + u + 1) * 4 * u);
        }
    pl->ws_floats = f;
}

int lb_check(const dctr_lstm_train_args_t* t) {
    DCTR_REQUIRE(t, DCTR_E_NULL, "bilstm_bwd: null args");
    const dctr_lstm_args_t* a = &t->fwd;
    // (fwd.route is the backward's own here: RESIDENT asks for ITS weights in LDS, whatever the forward's plan can hold)
    DCTR_REQUIRE(a->route >= DCTR_LSTM_ROUTE_AUTO && a->route <= DCTR_LSTM_ROUTE_WORKSPACE, DCTR_E_ENUM, "bilstm_bwd: unknown route %d", a->route);
    dctr_lstm_args_t f = *a;
    f.route = DCTR_LSTM_ROUTE_AUTO;
    int rc = dctr_lstm_check_args(&f);
    if (rc != DCTR_OK) return rc;
    DCTR_REQUIRE((uint32_t)t->accumulate <= 1u, DCTR_E_ENUM, "bilstm_bwd: accumulate must be 0 or 1");
    DCTR_REQUIRE(t->max_blocks >= 0, DCTR_E_DIM, "bilstm_bwd: max_blocks = %d", t->max_blocks);
    DCTR_REQUIRE((int64_t)a->seq_len * a->batch < 0x7fffffffLL, DCTR_E_DIM, "bilstm_bwd: seq_len x batch exceeds 2^31");
    const int64_t block = (int64_t)a->seq_len - 1;
    const int64_t w = a->merge_mode == DCTR_LSTM_MERGE_CONCAT ? 2 * (int64_t)a->units : a->units;
    DCTR_REQUIRE(t->d_out_row_stride >= w && t->d_out_stride >= block * t->d_out_row_stride + w, DCTR_E_DIM,
                 "bilstm_bwd: d_out strides smaller than the [seq_len, %lld] block", (long long)w);
    if (a->merge_mode == DCTR_LSTM_MERGE_NONE)
        DCTR_REQUIRE(t->d_out_bw_row_stride >= a->units && t->d_out_bw_stride >= block * t->d_out_bw_row_stride + a->units, DCTR_E_DIM,
                     "bilstm_bwd: d_out_bw strides smaller than the [seq_len, units] block");
    if (t->dx)
        DCTR_REQUIRE(t->dx_row_stride >= a->in_dim && t->dx_stride >= block * t->dx_row_stride + a->in_dim, DCTR_E_DIM,
                     "bilstm_bwd: dx strides smaller than the [seq_len, in_dim] block");
    return DCTR_OK;
}

}  // namespace

extern "C" int dctr_bilstm_bwd_supported(const dctr_lstm_train_args_t* t) {
    if (lb_check(t) != DCTR_OK) return 0;
    LbPlan pl;
    lb_plan(&t->fwd, &pl);
    return pl.ok ? 1 : 0;
}

extern "C" size_t dctr_bilstm_bwd_workspace_bytes(const dctr_lstm_train_args_t* t) {
    if (lb_check(t) != DCTR_OK) return 0;
    LbPlan pl;
    lb_plan(&t->fwd, &pl);
    return pl.ok ? (size_t)pl.ws_floats * sizeof(float) : 0;
}

extern "C" int dctr_bilstm_bwd(const dctr_lstm_train_args_t* t, void* stream) {
    int rc = lb_check(t);
    if (rc != DCTR_OK) return rc;
    const dctr_lstm_args_t* a = &t->fwd;
    LbPlan pl;
    lb_plan(a, &pl);
    DCTR_REQUIRE(pl.ok, DCTR_E_UNSUPPORTED,
                 "bilstm_bwd: sigmoid recurrent activation, at most %d layers and tiles within the LDS on the asked route (got activation %d, "
                 "%d layer(s), %d units over %d steps, route %d)",
                 LB_MAX_LAYERS, a->recurrent_activation, a->n_layers, a->units, a->seq_len, a->route);
    DCTR_REQUIRE(a->x && a->layers && t->d_out, DCTR_E_NULL, "bilstm_bwd: null x / layers / d_out");
    DCTR_REQUIRE(a->merge_mode != DCTR_LSTM_MERGE_NONE || t->d_out_bw, DCTR_E_NULL, "bilstm_bwd: merge_mode none needs d_out_bw");
    for (int l = 0; l < a->n_layers; ++l)
        for (int m = 0; m < LB_NW; ++m)
            DCTR_REQUIRE(a->layers[LB_NW * l + m], DCTR_E_NULL, "bilstm_bwd: layer %d: null kernel / recurrent kernel / bias", l);
    if (a->batch == 0) return DCTR_OK;
    DCTR_REQUIRE(t->tape && t->tape_bytes >= dctr_bilstm_tape_bytes(a), DCTR_E_NULL,
                 "bilstm_bwd: needs the tape of dctr_bilstm_tape_bytes() bytes that dctr_bilstm_train_fwd wrote");
    DCTR_REQUIRE_WORKSPACE("bilstm_bwd", "dctr_bilstm_bwd_workspace_bytes", t->workspace, t->workspace_bytes,
                           (size_t)pl.ws_floats * sizeof(float));
    float* ws = (float*)t->workspace;
    hipStream_t st = (hipStream_t)stream;
    const int L = a->n_layers, u = a->units, Din = a->in_dim;
    LbParams p = {};
    p.x = a->x;
    p.batch = a->batch;
    p.x_stride = a->x_stride;
    p.x_row_stride = a->x_row_stride;
    p.T = a->seq_len;
    p.Din = Din;
    p.u = u;
    p.L = L;
    p.res_layers = a->res_layers < L ? a->res_layers : L;
    p.merge = a->merge_mode;
    p.d0 = pl.d0;
    p.nd = pl.nd;
    p.ldx = pl.lp.ldx;
    p.ld = pl.lp.ld;
    p.lda = pl.lda;
    p.ldc = pl.lp.ldc;
    p.KQx = pl.lp.KQx;
    p.KQh = pl.lp.KQh;
    p.ldw0 = pl.lp.ldw0;
    p.ldw = pl.lp.ldw;
    p.ldwh = pl.lp.ldwh;
    p.tape = (const float*)t->tape;
    p.dout = t->d_out;
    p.dout_stride = t->d_out_stride;
    p.dout_row_stride = t->d_out_row_stride;
    p.dout_bw = t->d_out_bw;
    p.dout_bw_stride = t->d_out_bw_stride;
    p.dout_bw_row_stride = t->d_out_bw_row_stride;
    dctr_gemm::GroupDesc gd[2 * LB_MAX_LAYERS];
    LbSum sg = {};
    sg.u = u;
    const int rows = (int)((int64_t)a->seq_len * a->batch);
    int64_t max_n = 0;
    for (int d = pl.d0; d < pl.d0 + pl.nd; ++d) p.dxw[d] = t->dx ? ws + pl.dxw[d] : nullptr;
    for (int l = 0; l < L; ++l)
        for (int d = pl.d0; d < pl.d0 + pl.nd; ++d) {
            const int D = l ? u : Din;
            for (int m = 0; m < 3; ++m) p.W[l][3 * d + m] = a->layers[LB_NW * l + 3 * d + m];
            p.mask[l][d] = t->masks ? t->masks[2 * l + d] : nullptr;
            float* dst[3];
            bool any = false;
            for (int m = 0; m < 3; ++m) {
                dst[m] = t->d_layers ? t->d_layers[LB_NW * l + 3 * d + m] : nullptr;
                any = any || dst[m];
            }
            if (!any) continue;
            p.wdz[l][d] = ws + pl.wdz[l][d];
            p.wa[l][d] = ws + pl.wa[l][d];
            // [dW; dU; db] [D + u + 1, 4u] (row-major) = [in m | h_prev | 1]^T dz: column-major C'(4u x (D + u + 1)) = dz'(4u x rows) [A' ; 1]^T
            const int gi = sg.n_groups++;
            dctr_gemm::GroupDesc& g = gd[gi];
            g = dctr_gemm::GroupDesc{};
            g.op_a = dctr_gemm::OP_N;
            g.op_b = dctr_gemm::OP_T;
            g.m = 4 * u;
            g.n = D + u + 1;
            g.k = rows;
            g.A = p.wdz[l][d];
            g.lda = 4 * u;
            g.B = p.wa[l][d];
            g.ldb = D + u;
            g.C = ws + pl.parts[l][d];
            g.ldc = 4 * u;
            g.batch = 1;
            g.ones_last = 1;
            g.k_slices = pl.slices;
            g.slice_stride_c = (int64_t)g.n * g.m;
            sg.slices[gi] = pl.slices;
            sg.D[gi] = D;
            sg.parts[gi] = g.C;
            for (int m = 0; m < 3; ++m) sg.dst[gi][m] = dst[m];
            max_n = g.slice_stride_c > max_n ? g.slice_stride_c : max_n;
        }
    const int64_t n_items = dctr_ceil_div(a->batch, LB_ROWS) * pl.nd;
    const int64_t cap = t->max_blocks > 0 ? (int64_t)t->max_blocks : (int64_t)2 * dctr_n_cus();
    const dim3 grid((unsigned)(n_items < cap ? n_items : cap)), block(LB_THREADS);
    if (pl.resident) {
        static thread_local size_t granted[DCTR_MAX_DEVICES] = {0};
        hipError_t e = dctr_grant_lds((const void*)bilstm_bwd_kernel<true>, pl.lds_bytes, granted);
        DCTR_REQUIRE(e == hipSuccess, (int)e, "bilstm_bwd: cannot raise dynamic LDS: %s", hipGetErrorString(e));
        DCTR_LAUNCH((bilstm_bwd_kernel<true>), grid, block, pl.lds_bytes, st, p);
    } else {
        static thread_local size_t granted[DCTR_MAX_DEVICES] = {0};
        hipError_t e = dctr_grant_lds((const void*)bilstm_bwd_kernel<false>, pl.lds_bytes, granted);
        DCTR_REQUIRE(e == hipSuccess, (int)e, "bilstm_bwd: cannot raise dynamic LDS: %s", hipGetErrorString(e));
        DCTR_LAUNCH((bilstm_bwd_kernel<false>), grid, block, pl.lds_bytes, st, p);
    }
    rc = dctr_launch_status("dctr_bilstm_bwd");
    if (rc != DCTR_OK) return rc;
    if (sg.n_groups) {
        const int rg = dctr_gemm::sgemm_grouped(st, gd, sg.n_groups);
        DCTR_REQUIRE(rg == 0, DCTR_E_UNSUPPORTED, "bilstm_bwd: sgemm_grouped(dW) failed (%d)", rg);
    }
    if (sg.n_groups || t->dx) {
        sg.dxw[0] = p.dxw[pl.d0];
        sg.dxw[1] = pl.nd == 2 ? p.dxw[1] : nullptr;
        sg.dx = t->dx;
        sg.batch = a->batch;
        sg.dx_stride = t->dx_stride;
        sg.dx_row_stride = t->dx_row_stride;
        sg.T = a->seq_len;
        sg.Din = Din;
        sg.accumulate = t->accumulate;
        const int64_t n_dx = t->dx ? a->batch * a->seq_len * Din : 0;
        max_n = n_dx > max_n ? n_dx : max_n;
        const int64_t gx = dctr_ceil_div(max_n, (int64_t)256);
        hipLaunchKernelGGL(lstm_bwd_sum_kernel, dim3((unsigned)(gx > 1024 ? 1024 : gx), (unsigned)(sg.n_groups + 1)), dim3(256), 0, st, sg);
    }
    return dctr_launch_status("dctr_bilstm_bwd");
}
