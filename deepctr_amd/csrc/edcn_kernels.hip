// EDCN's tower (reference deepctr/models/edcn.py:66-87) with RegulationModule (layers/core.py:270-321) and BridgeModule
// (layers/interaction.py:1502-1565), forward.
//
// With F fields of width d, D = F d, per sample and round i < cross_num (deep = cross = x before round 0):
//     deep  = deep  * softmax_f(g_{2i}   / tau)[field of the column]        (RegulationModule: F live weights, softmax over fields)
//     cross = cross * softmax_f(g_{2i+1} / tau)[field of the column]
//     c  = cross * (cross . w) + b + cross              (CrossNet(1) 'vector')     |  cross * (W cross + b) + cross   ('matrix')
//     h  = act(bn(deep Wd + bd))                        (DNN([D]))
//     br = c + h | c * h | act_b([c, h] Wb + bb)        (BridgeModule)
//     deep = cross = br
//     logit = [c, h, br] . head_w + add + global_bias (, sigmoid)
//
// dctr_edcn_fwd, the fused route: ONE launch runs every round for a tile of R rows.  Four [R, ld] tiles live in LDS from the row's
// first read to the logit: X1 (the DNN's input, later br), X2 (the cross input), C and H.  A round: waves 0 / 1 take the two softmaxes
// over the F live weights; every thread gates its elements (X2 = X1 * gate_cross, X1 *= gate_deep: the A operands are staged gated, no
// gated copy exists in HBM); the D x D products run on v_mfma_f32_16x16x4_f32 (mfma_tile.h: tile_gemm_kn for the Keras-layout DNN and
// bridge kernels, tile_gemm_nk for the matrix cross), one 16 x 16*TPW output tile per wave task with bias / BatchNormalization affine /
// activation / the cross formula as the task's epilogue; the vector cross is one dot product per row and wave.  The concatenation
// bridge is two products into one accumulator (c with Wb's rows [0, D), h with rows [D, 2D)).  The tail takes the three dot products
// with head_w per row in one wave.  No atomics: the same bits on every call.
// More than 32 rounds run as chained launches through a [B, D] workspace that carries br.
//
// dctr_edcn_regulate / dctr_edcn_bridge: the two elementwise steps of the layered route (shapes past the LDS, attention pooling,
// other activations), which the host builds from the DNN / CrossNet / GEMM entry points.
#include <math.h>
#include "dctr_common.h"
#include "tile_route.h"
#include "mfma_tile.h"
#include "edcn_device.h"

namespace {

constexpr int ED_EW_THREADS = 256;
constexpr int ED_GATE_LDS_FIELDS = 8192;          // dctr_edcn_regulate keeps its gates in LDS up to this many fields

struct EdRound {
    const float *g_deep, *g_cross, *cross_w, *cross_b, *dnn_w, *dnn_b, *bn_scale, *bn_shift, *bridge_w, *bridge_b;
};

struct EdParams {
    int64_t batch;
    const float* x;               // already advanced by x_offset
    int64_t x_stride;
    int32_t F, d, D, rounds, mode, bridge, act, bridge_act, R, ld;
    float inv_tau;
    EdRound rd[ED_MAX_ROUNDS];
    const float* head_w;
    const float* add[4];
    const float* global_bias;
    int32_t sigmoid_out;
    float* logit;
    float* out;                   // already advanced by out_offset
    int64_t out_stride;
    float* br_out;                // chained launches: [B, D]
    float* tape;                  // TAPE: [rounds, B, 3D], c / h / br of every round
};

// TAPE: the training forward (dctr_edcn_train_fwd) also writes c, h, br of every round; the arithmetic is the inference kernel's
template <int TPW, bool TAPE>
__global__ __launch_bounds__(ED_THREADS) void edcn_fwd_kernel(EdParams p) {
    extern __shared__ __attribute__((aligned(16))) float ed_lds[];
    const int R = p.R, ld = p.ld, D = p.D, F = p.F, d = p.d;
    float* X1 = ed_lds;
    float* X2 = X1 + R * ld;
    float* C = X2 + R * ld;
    float* H = C + R * ld;
    float* Gd = H + R * ld;
    float* Gc = Gd + F;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int RT = R >> 4, CT = (D + 16 * TPW - 1) / (16 * TPW), KQ = dctr::pad16(D) >> 2;
    const int64_t n_tiles = (p.batch + R - 1) / R;

    // the K padding of the four tiles is read by the products and written by nobody
    for (int e = tid; e < 4 * R * ld; e += ED_THREADS) ed_lds[e] = 0.f;
    __syncthreads();

    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t b0 = tile * R;
        const int nvalid = (int)min((int64_t)R, p.batch - b0);
        for (int e = tid; e < R * D; e += ED_THREADS) {
            const int r = e / D, k = e - r * D;
            X1[r * ld + k] = r < nvalid ? p.x[(b0 + r) * p.x_stride + k] : 0.f;
        }
        for (int i = 0; i < p.rounds; ++i) {
            const EdRound& rd = p.rd[i];
            if (wave == 0) ed_gate(rd.g_deep, F, p.inv_tau, Gd, lane);
            if (wave == 1) ed_gate(rd.g_cross, F, p.inv_tau, Gc, lane);
            __syncthreads();
            for (int e = tid; e < R * D; e += ED_THREADS) {
                const int r = e / D, k = e - r * D, f = k / d;
                const float v = X1[r * ld + k];
                X2[r * ld + k] = v * Gc[f];
                X1[r * ld + k] = v * Gd[f];
            }
            __syncthreads();
            if (p.mode == DCTR_CROSS_VECTOR) {
                for (int r = wave; r < R; r += ED_WAVES) {
                    const float* xr = X2 + r * ld;
                    float s = 0.f;
                    for (int k = lane; k < D; k += 64) s = fmaf(xr[k], rd.cross_w[k], s);
                    s = ed_wave_sum(s);
                    for (int k = lane; k < D; k += 64) C[r * ld + k] = xr[k] * s + rd.cross_b[k] + xr[k];
                }
            }
            // h = act(bn(X1 Wd + bd)) -> H;  matrix cross: c = X2 * (W X2 + b) + X2 -> C
            const int per = RT * CT, n_tasks = p.mode == DCTR_CROSS_MATRIX ? 2 * per : per;
            for (int t = wave; t < n_tasks; t += ED_WAVES) {
                const int which = t / per, rest = t - which * per, rt = rest / CT, ct = rest - rt * CT;
                dctr::f32x4 acc[TPW];
#pragma unroll
                for (int c = 0; c < TPW; ++c) acc[c] = dctr::f32x4{0.f, 0.f, 0.f, 0.f};
                const int row0 = rt * 16 + 4 * (lane >> 4), col0 = ct * 16 * TPW + TPW * (lane & 15);
                if (which == 0) {
                    dctr::tile_gemm_kn<TPW>(X1 + rt * 16 * ld, ld, D, KQ, rd.dnn_w, D, ct * 16 * TPW, acc);
#pragma unroll
                    for (int c = 0; c < TPW; ++c) {
                        const int col = col0 + c;
                        if (col < D) {
                            const float b = rd.dnn_b[col];
                            const float sc = rd.bn_scale ? rd.bn_scale[col] : 1.f, sh = rd.bn_scale ? rd.bn_shift[col] : 0.f;
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                float v = acc[c][r] + b;
                                if (rd.bn_scale) v = v * sc + sh;
                                H[(row0 + r) * ld + col] = ed_act(v, p.act);
                            }
                        }
                    }
                } else {
                    dctr::tile_gemm_nk<TPW>(X2 + rt * 16 * ld, ld, D, KQ, rd.cross_w, D, ct * 16 * TPW, acc);
#pragma unroll
                    for (int c = 0; c < TPW; ++c) {
                        const int col = col0 + c;
                        if (col < D) {
                            const float b = rd.cross_b[col];
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const float xv = X2[(row0 + r) * ld + col];
                                C[(row0 + r) * ld + col] = xv * (acc[c][r] + b) + xv;
                            }
                        }
                    }
                }
            }
            __syncthreads();
            // br -> X1 (its gated contents are dead: every product of this round has been taken)
            if (p.bridge == DCTR_EDCN_BRIDGE_CONCAT) {
                for (int t = wave; t < per; t += ED_WAVES) {
                    const int rt = t / CT, ct = t - rt * CT;
                    dctr::f32x4 acc[TPW];
#pragma unroll
                    for (int c = 0; c < TPW; ++c) acc[c] = dctr::f32x4{0.f, 0.f, 0.f, 0.f};
                    dctr::tile_gemm_kn<TPW>(C + rt * 16 * ld, ld, D, KQ, rd.bridge_w, D, ct * 16 * TPW, acc);
                    dctr::tile_gemm_kn<TPW>(H + rt * 16 * ld, ld, D, KQ, rd.bridge_w + (int64_t)D * D, D, ct * 16 * TPW, acc);
                    const int row0 = rt * 16 + 4 * (lane >> 4), col0 = ct * 16 * TPW + TPW * (lane & 15);
#pragma unroll
                    for (int c = 0; c < TPW; ++c) {
                        const int col = col0 + c;
                        if (col < D) {
                            const float b = rd.bridge_b[col];
#pragma unroll
                            for (int r = 0; r < 4; ++r) X1[(row0 + r) * ld + col] = ed_act(acc[c][r] + b, p.bridge_act);
                        }
                    }
                }
            } else {
                const bool prod = p.bridge == DCTR_EDCN_BRIDGE_HADAMARD;
                for (int e = tid; e < R * D; e += ED_THREADS) {
                    const int r = e / D, k = e - r * D;
                    const float cv = C[r * ld + k], hv = H[r * ld + k];
                    X1[r * ld + k] = prod ? cv * hv : cv + hv;
                }
            }
            __syncthreads();
            if (TAPE) {         // (reads only: the next round's gating follows its own barrier)
                for (int e = tid; e < nvalid * D; e += ED_THREADS) {
                    const int r = e / D, k = e - r * D;
                    float* o = p.tape + ((int64_t)i * p.batch + b0 + r) * (3 * (int64_t)D) + k;
                    o[0] = C[r * ld + k];
                    o[D] = H[r * ld + k];
                    o[2 * (int64_t)D] = X1[r * ld + k];
                }
            }
        }
        if (p.out) {
            for (int e = tid; e < nvalid * D; e += ED_THREADS) {
                const int r = e / D, k = e - r * D;
                float* o = p.out + (b0 + r) * p.out_stride + k;
                o[0] = C[r * ld + k];
                o[D] = H[r * ld + k];
                o[2 * (int64_t)D] = X1[r * ld + k];
            }
        }
        if (p.br_out) {
            for (int e = tid; e < nvalid * D; e += ED_THREADS) {
                const int r = e / D, k = e - r * D;
                p.br_out[(b0 + r) * D + k] = X1[r * ld + k];
            }
        }
        if (p.logit) {
            for (int r = wave; r < nvalid; r += ED_WAVES) {
                float acc = 0.f;
                for (int k = lane; k < D; k += 64) acc = fmaf(C[r * ld + k], p.head_w[k], acc);
                for (int k = lane; k < D; k += 64) acc = fmaf(H[r * ld + k], p.head_w[D + k], acc);
                for (int k = lane; k < D; k += 64) acc = fmaf(X1[r * ld + k], p.head_w[2 * D + k], acc);
                acc = ed_wave_sum(acc);
                if (lane == 0) {
#pragma unroll
                    for (int a = 0; a < 4; ++a)
                        if (p.add[a]) acc += p.add[a][b0 + r];
                    if (p.global_bias) acc += p.global_bias[0];
                    p.logit[b0 + r] = p.sigmoid_out ? 1.f / (1.f + expf(-acc)) : acc;
                }
            }
        }
        __syncthreads();        // X1 is staged again for the next tile
    }
}

// RegulationModule twice over one read: deep = x * gate(g_deep), cross = x * gate(g_cross) (either output may be absent).
// LDS_GATES: the two softmaxes wait in LDS; else every element takes its own exp from the block's max and sum.
template <bool LDS_GATES>
__global__ __launch_bounds__(ED_EW_THREADS) void edcn_regulate_kernel(const float* __restrict__ x, int64_t x_stride, int64_t batch, int F, int d,
                                                                      const float* __restrict__ g_deep, const float* __restrict__ g_cross,
                                                                      float inv_tau, float* deep, int64_t deep_stride, float* cross,
                                                                      int64_t cross_stride) {
    extern __shared__ __attribute__((aligned(16))) float rg_lds[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    float* Gd = rg_lds;
    float* Gc = rg_lds + (LDS_GATES ? F : 2);
    if (LDS_GATES) {
        if (wave == 0 && deep) ed_gate(g_deep, F, inv_tau, Gd, lane);
        if (wave == 1 && cross) ed_gate(g_cross, F, inv_tau, Gc, lane);
    } else if (wave < 2) {          // {max, sum of exp} of each gate
        const float* g = wave == 0 ? g_deep : g_cross;
        if (wave == 0 ? deep != nullptr : cross != nullptr) {
            float m = -INFINITY, s = 0.f;
            for (int f = lane; f < F; f += 64) m = fmaxf(m, g[f] * inv_tau);
            m = ed_wave_max(m);
            for (int f = lane; f < F; f += 64) s += expf(g[f] * inv_tau - m);
            s = ed_wave_sum(s);
            if (lane == 0) {
                (wave == 0 ? Gd : Gc)[0] = m;
                (wave == 0 ? Gd : Gc)[1] = s;
            }
        }
    }
    __syncthreads();
    const int64_t D = (int64_t)F * d, total = batch * D;
    for (int64_t e = (int64_t)blockIdx.x * ED_EW_THREADS + tid; e < total; e += (int64_t)gridDim.x * ED_EW_THREADS) {
        const int64_t r = e / D;
        const int k = (int)(e - r * D), f = k / d;
        const float v = x[r * x_stride + k];
        if (deep) deep[r * deep_stride + k] = v * (LDS_GATES ? Gd[f] : expf(g_deep[f] * inv_tau - Gd[0]) / Gd[1]);
        if (cross) cross[r * cross_stride + k] = v * (LDS_GATES ? Gc[f] : expf(g_cross[f] * inv_tau - Gc[0]) / Gc[1]);
    }
}

// BridgeModule's elementwise forms, one wave per row: c + h, c * h, softmax(ax) * c + softmax(ah) * h (row softmaxes over the D columns)
__global__ __launch_bounds__(ED_EW_THREADS) void edcn_bridge_kernel(int kind, const float* __restrict__ c, int64_t c_stride,
                                                                    const float* __restrict__ h, int64_t h_stride, const float* __restrict__ ax,
                                                                    int64_t ax_stride, const float* __restrict__ ah, int64_t ah_stride,
                                                                    int64_t batch, int D, float* out, int64_t out_stride) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t)blockIdx.x * (ED_EW_THREADS / 64) + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * (ED_EW_THREADS / 64);
    for (int64_t r = wave0; r < batch; r += n_waves) {
        const float* cr = c + r * c_stride;
        const float* hr = h + r * h_stride;
        float* o = out + r * out_stride;
        if (kind == DCTR_EDCN_BRIDGE_ATTENTION) {
            const float* xr = ax + r * ax_stride;
            const float* yr = ah + r * ah_stride;
            float mx = -INFINITY, my = -INFINITY, sx = 0.f, sy = 0.f;
            for (int k = lane; k < D; k += 64) {
                mx = fmaxf(mx, xr[k]);
                my = fmaxf(my, yr[k]);
            }
            mx = ed_wave_max(mx);
            my = ed_wave_max(my);
            for (int k = lane; k < D; k += 64) {
                sx += expf(xr[k] - mx);
                sy += expf(yr[k] - my);
            }
            sx = ed_wave_sum(sx);
            sy = ed_wave_sum(sy);
            for (int k = lane; k < D; k += 64) o[k] = expf(xr[k] - mx) / sx * cr[k] + expf(yr[k] - my) / sy * hr[k];
        } else if (kind == DCTR_EDCN_BRIDGE_HADAMARD) {
            for (int k = lane; k < D; k += 64) o[k] = cr[k] * hr[k];
        } else {
            for (int k = lane; k < D; k += 64) o[k] = cr[k] + hr[k];
        }
    }
}

}  // namespace

extern "C" int dctr_edcn_route(const dctr_edcn_args_t* a) {
    int rc = edcn_check(a);
    if (rc != DCTR_OK) return rc;
    EdPlan pl;
    edcn_plan(a, &pl);
    return pl.fused ? DCTR_EDCN_ROUTE_FUSED : DCTR_EDCN_ROUTE_LAYERED;
}

extern "C" size_t dctr_edcn_workspace_bytes(const dctr_edcn_args_t* a) {
    if (edcn_check(a) != DCTR_OK) return 0;
    EdPlan pl;
    edcn_plan(a, &pl);
    return pl.ws_bytes;
}

// dctr_edcn_fwd (tape = NULL) and dctr_edcn_train_fwd (the tape kernel; one launch: cross_num <= ED_MAX_ROUNDS)
static int edcn_run(const dctr_edcn_args_t* a, float* tape, void* stream) {
    int rc = edcn_check(a);
    if (rc != DCTR_OK) return rc;
    EdPlan pl;
    edcn_plan(a, &pl);
    DCTR_REQUIRE(pl.fused, DCTR_E_UNSUPPORTED,
                 "edcn_fwd: %d fields of dim %d, bridge %d, activations %d / %d, route %d: not on the fused route (dctr_edcn_route); the host "
                 "runs the layered one", a->fields, a->dim, a->bridge, a->activation, a->bridge_activation, a->route);
    const int D = a->fields * a->dim, L = a->cross_num;
    DCTR_REQUIRE(a->x && a->gates && a->cross_w && a->cross_b && a->dnn_w && a->dnn_b, DCTR_E_NULL,
                 "edcn_fwd: null x / gates / cross_w / cross_b / dnn_w / dnn_b");
    DCTR_REQUIRE(a->bridge != DCTR_EDCN_BRIDGE_CONCAT || (a->bridge_w && a->bridge_b), DCTR_E_NULL,
                 "edcn_fwd: the concatenation bridge needs bridge_w / bridge_b");
    DCTR_REQUIRE((a->bn_scale == nullptr) == (a->bn_shift == nullptr), DCTR_E_NULL, "edcn_fwd: bn_scale and bn_shift come together");
    bool aligned = true;
    for (int i = 0; i < L; ++i) {
        DCTR_REQUIRE(a->gates[2 * i] && a->gates[2 * i + 1] && a->cross_w[i] && a->cross_b[i] && a->dnn_w[i] && a->dnn_b[i], DCTR_E_NULL,
                     "edcn_fwd: round %d: null weight", i);
        DCTR_REQUIRE(a->bridge != DCTR_EDCN_BRIDGE_CONCAT || (a->bridge_w[i] && a->bridge_b[i]), DCTR_E_NULL,
                     "edcn_fwd: round %d: null bridge weight", i);
        DCTR_REQUIRE(!a->bn_scale || ((a->bn_scale[i] == nullptr) == (a->bn_shift[i] == nullptr)), DCTR_E_NULL,
                     "edcn_fwd: round %d: bn_scale and bn_shift come together", i);
        aligned = aligned && dctr_aligned16(a->dnn_w[i]) && (a->bridge != DCTR_EDCN_BRIDGE_CONCAT || dctr_aligned16(a->bridge_w[i]));
    }
    DCTR_REQUIRE(a->logit || a->out, DCTR_E_NULL, "edcn_fwd: neither logit nor out");
    DCTR_REQUIRE(!a->logit || a->head_w, DCTR_E_NULL, "edcn_fwd: logit without head_w");
    DCTR_REQUIRE(!a->out || (a->out_offset >= 0 && a->out_offset + 3 * (int64_t)D <= a->out_stride), DCTR_E_DIM,
                 "edcn_fwd: out columns [%lld, %lld) in rows of %lld", (long long)a->out_offset, (long long)(a->out_offset + 3 * (int64_t)D),
                 (long long)a->out_stride);
    if (pl.ws_bytes) {
        DCTR_REQUIRE(a->workspace && a->workspace_bytes >= pl.ws_bytes, DCTR_E_NULL,
                     "edcn_fwd: %d rounds need a workspace of %zu bytes (dctr_edcn_workspace_bytes)", L, pl.ws_bytes);
        DCTR_REQUIRE(dctr_aligned16(a->workspace), DCTR_E_ALIGN, "edcn_fwd: workspace not 16-B aligned");
    }
    if (a->batch == 0) return DCTR_OK;
    const int tpw = aligned ? pl.tpw : 1;        // (the 8- / 16-byte weight loads need aligned kernels; D % (16 TPW) == 0 keeps the rows so)
    const void* fn = tape ? (tpw == 4 ? (const void*)edcn_fwd_kernel<4, true> : tpw == 2 ? (const void*)edcn_fwd_kernel<2, true>
                                                                                         : (const void*)edcn_fwd_kernel<1, true>)
                          : (tpw == 4 ? (const void*)edcn_fwd_kernel<4, false> : tpw == 2 ? (const void*)edcn_fwd_kernel<2, false>
                                                                                          : (const void*)edcn_fwd_kernel<1, false>);
    static thread_local size_t granted[6][DCTR_MAX_DEVICES] = {{0}};
    hipError_t e = dctr_grant_lds(fn, pl.lds, granted[(tape ? 3 : 0) + (tpw == 4 ? 2 : tpw == 2 ? 1 : 0)]);
    DCTR_REQUIRE(e == hipSuccess, (int)e, "edcn_fwd: cannot raise dynamic LDS: %s", hipGetErrorString(e));
    const int64_t n_tiles = dctr_ceil_div(a->batch, (int64_t)pl.R), cap = 4 * (int64_t)dctr_n_cus();
    const dim3 grid((unsigned)(n_tiles < cap ? n_tiles : cap)), block(ED_THREADS);
    const hipStream_t st = (hipStream_t)stream;
    for (int l0 = 0; l0 < L; l0 += ED_MAX_ROUNDS) {
        const int nl = L - l0 < ED_MAX_ROUNDS ? L - l0 : ED_MAX_ROUNDS;
        const bool first = l0 == 0, last = l0 + nl == L;
        EdParams p = {};
        p.batch = a->batch;
        p.x = first ? a->x + a->x_offset : (const float*)a->workspace;
        p.x_stride = first ? a->x_stride : D;
        p.F = a->fields;
        p.d = a->dim;
        p.D = D;
        p.rounds = nl;
        p.mode = a->mode;
        p.bridge = a->bridge;
        p.act = a->activation;
        p.bridge_act = a->bridge_activation;
        p.R = pl.R;
        p.ld = pl.ld;
        p.inv_tau = a->inv_tau;
        for (int i = 0; i < nl; ++i) {
            EdRound& r = p.rd[i];
            const int k = l0 + i;
            r.g_deep = a->gates[2 * k];
            r.g_cross = a->gates[2 * k + 1];
            r.cross_w = a->cross_w[k];
            r.cross_b = a->cross_b[k];
            r.dnn_w = a->dnn_w[k];
            r.dnn_b = a->dnn_b[k];
            r.bn_scale = a->bn_scale ? a->bn_scale[k] : nullptr;
            r.bn_shift = a->bn_scale ? a->bn_shift[k] : nullptr;
            r.bridge_w = a->bridge == DCTR_EDCN_BRIDGE_CONCAT ? a->bridge_w[k] : nullptr;
            r.bridge_b = a->bridge == DCTR_EDCN_BRIDGE_CONCAT ? a->bridge_b[k] : nullptr;
        }
        if (last) {
            p.head_w = a->head_w;
            for (int i = 0; i < 4; ++i) p.add[i] = a->logit ? a->add[i] : nullptr;
            p.global_bias = a->logit ? a->global_bias : nullptr;
            p.sigmoid_out = a->sigmoid_out;
            p.logit = a->logit;
            p.out = a->out ? a->out + a->out_offset : nullptr;
            p.out_stride = a->out_stride;
        } else {
            p.br_out = (float*)a->workspace;        // a tile reads its rows before it writes them: in place
        }
        p.tape = tape;
#define ED_FWD_LAUNCH(T, TAPE) DCTR_LAUNCH((edcn_fwd_kernel<T, TAPE>), grid, block, pl.lds, st, p)
        if (tape) {
            if (tpw == 4) ED_FWD_LAUNCH(4, true);
            else if (tpw == 2) ED_FWD_LAUNCH(2, true);
            else ED_FWD_LAUNCH(1, true);
        } else {
            if (tpw == 4) ED_FWD_LAUNCH(4, false);
            else if (tpw == 2) ED_FWD_LAUNCH(2, false);
            else ED_FWD_LAUNCH(1, false);
        }
#undef ED_FWD_LAUNCH
        rc = dctr_launch_status("dctr_edcn_fwd");
        if (rc != DCTR_OK) return rc;
    }
    return DCTR_OK;
}

extern "C" int dctr_edcn_fwd(const dctr_edcn_args_t* a, void* stream) { return edcn_run(a, nullptr, stream); }

extern "C" size_t dctr_edcn_tape_bytes(const dctr_edcn_train_args_t* t) {
    if (!t || edcn_check(&t->fwd) != DCTR_OK) return 0;
    return (size_t)t->fwd.cross_num * (size_t)t->fwd.batch * 3 * (size_t)t->fwd.fields * t->fwd.dim * sizeof(float);
}

extern "C" int dctr_edcn_train_fwd(const dctr_edcn_train_args_t* t, void* stream) {
    DCTR_REQUIRE(t, DCTR_E_NULL, "edcn_train_fwd: null args");
    int rc = edcn_check(&t->fwd);
    if (rc != DCTR_OK) return rc;
    DCTR_REQUIRE(dctr_edcn_bwd_supported(t), DCTR_E_UNSUPPORTED,
                 "edcn_train_fwd: these shapes / options are not the backward's (dctr_edcn_bwd_supported)");
    DCTR_REQUIRE(t->fwd.batch == 0 || t->tape, DCTR_E_NULL, "edcn_train_fwd: null tape (dctr_edcn_tape_bytes)");
    DCTR_REQUIRE(t->fwd.batch == 0 || dctr_aligned16(t->tape), DCTR_E_ALIGN, "edcn_train_fwd: tape not 16-B aligned");
    return edcn_run(&t->fwd, t->tape, stream);
}

extern "C" int dctr_edcn_regulate(const float* x, int64_t x_stride, int64_t batch, int32_t fields, int32_t dim, const float* g_deep,
                                  const float* g_cross, float inv_tau, float* deep, int64_t deep_stride, float* cross, int64_t cross_stride,
                                  void* stream) {
    DCTR_REQUIRE(batch >= 0 && fields >= 1 && dim >= 1 && (int64_t)fields * dim <= (1 << 24), DCTR_E_DIM,
                 "edcn_regulate: batch = %lld, fields = %d, dim = %d", (long long)batch, fields, dim);
    const int64_t D = (int64_t)fields * dim;
    DCTR_REQUIRE(deep || cross, DCTR_E_NULL, "edcn_regulate: neither output");
    DCTR_REQUIRE(x && (!deep || g_deep) && (!cross || g_cross), DCTR_E_NULL, "edcn_regulate: null x / gate weights");
    DCTR_REQUIRE(x_stride >= D && (!deep || deep_stride >= D) && (!cross || cross_stride >= D), DCTR_E_DIM,
                 "edcn_regulate: a row pitch below fields * dim = %lld", (long long)D);
    DCTR_REQUIRE(inv_tau == inv_tau && inv_tau - inv_tau == 0.f, DCTR_E_DIM, "edcn_regulate: 1 / tau is not finite");
    if (batch == 0) return DCTR_OK;
    const int64_t blocks = dctr_ceil_div(batch * D, (int64_t)ED_EW_THREADS * 4), cap = 16 * (int64_t)dctr_n_cus();
    const dim3 grid((unsigned)(blocks < cap ? blocks : cap)), block(ED_EW_THREADS);
    if (fields <= ED_GATE_LDS_FIELDS)
        DCTR_LAUNCH(edcn_regulate_kernel<true>, grid, block, 2 * (size_t)fields * sizeof(float), (hipStream_t)stream, x, x_stride, batch,
                    fields, dim, g_deep, g_cross, inv_tau, deep, deep_stride, cross, cross_stride);
    else
        DCTR_LAUNCH(edcn_regulate_kernel<false>, grid, block, 4 * sizeof(float), (hipStream_t)stream, x, x_stride, batch, fields, dim, g_deep,
                    g_cross, inv_tau, deep, deep_stride, cross, cross_stride);
    return dctr_launch_status("dctr_edcn_regulate");
}

extern "C" int dctr_edcn_bridge(int32_t kind, const float* c, int64_t c_stride, const float* h, int64_t h_stride, const float* ax,
                                int64_t ax_stride, const float* ah, int64_t ah_stride, int64_t batch, int32_t dim, float* out,
                                int64_t out_stride, void* stream) {
    DCTR_REQUIRE(kind == DCTR_EDCN_BRIDGE_ADD || kind == DCTR_EDCN_BRIDGE_HADAMARD || kind == DCTR_EDCN_BRIDGE_ATTENTION, DCTR_E_ENUM,
                 "edcn_bridge: kind %d is no elementwise bridge", kind);
    DCTR_REQUIRE(batch >= 0 && dim >= 1, DCTR_E_DIM, "edcn_bridge: batch = %lld, dim = %d", (long long)batch, dim);
    DCTR_REQUIRE(c && h && out, DCTR_E_NULL, "edcn_bridge: null c / h / out");
    DCTR_REQUIRE(kind != DCTR_EDCN_BRIDGE_ATTENTION || (ax && ah), DCTR_E_NULL, "edcn_bridge: attention pooling needs the two score rows");
    DCTR_REQUIRE(c_stride >= dim && h_stride >= dim && out_stride >= dim &&
                     (kind != DCTR_EDCN_BRIDGE_ATTENTION || (ax_stride >= dim && ah_stride >= dim)), DCTR_E_DIM,
                 "edcn_bridge: a row pitch below dim = %d", dim);
    if (batch == 0) return DCTR_OK;
    const int64_t blocks = dctr_ceil_div(batch, (int64_t)(ED_EW_THREADS / 64)), cap = 16 * (int64_t)dctr_n_cus();
    const dim3 grid((unsigned)(blocks < cap ? blocks : cap)), block(ED_EW_THREADS);
    DCTR_LAUNCH(edcn_bridge_kernel, grid, block, 0, (hipStream_t)stream, kind, c, c_stride, h, h_stride, ax, ax_stride, ah, ah_stride, batch,
                dim, out, out_stride);
    return dctr_launch_status("dctr_edcn_bridge");
}
