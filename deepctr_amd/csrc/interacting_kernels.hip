// InteractingLayer.call (reference deepctr/layers/interaction.py:749-779) x n_layers: the AutoInt stack (models/autoint.py:61-64),
// optionally with the Dense(1) over its flattened output (autoint.py:65-79) taken on chip.
//
// Reference per layer: Q, K, V = tensordot(X, W_{Q,K,V}) ([B, F, d*H] each, materialised), split into heads and stacked
// ([H, B, F, d]), scores = Q K^T ([H, B, F, F], / sqrt(d) when scaling), softmax over the keys, P V, heads concatenated on the last
// axis, + X W_res, ReLU.  TensorFlow writes every one of those tensors to HBM.
//
// Here one launch runs every layer.  A workgroup owns a tile of S samples; their [S*F, E_l] activations X, and Q, K, V, R
// ([S*F, d*H] each) stay in LDS from the layer-0 input to the last layer's output:
//   * projections: X W for each of the four weights on v_mfma_f32_16x16x4_f32 (mfma_tile.h: row tiles of 16 of the S*F rows, K padded
//     to 16 with zeros, W streamed from L2 in its Keras layout) — exact fp32, k-ordered;
//   * attention: one thread per (sample, query field, head) walks the F keys twice — the row max, then exp(s - max), its sum and
//     the P V accumulation in registers (up to 16 output columns per pass over the keys) — so no score matrix exists anywhere;
//     1 / sum, the residual and the ReLU are its epilogue, written in place of X (which the projections no longer need);
//   * output: the flattened last layer to `out`, and / or its dot product with head_w reduced per sample by one wave -> logit[b].
// A sample too large for the LDS (large F, wide d*H) takes the same kernel with those buffers in a per-workgroup slice of the
// workspace (the "general route": S = 1, <= 256 persistent workgroups): nothing is refused for its size.
// Cost model (F 26, E 16, d 8, H 2, 3 layers): 53,248 FLOP projections + 2 x 21,632 attention per layer -> 289.5 kFLOP / sample.
#include <math.h>
#include "dctr_common.h"
#include "mfma_tile.h"
#include "tile_route.h"

namespace {

constexpr int IA_MAX_LAYERS = 32;               // layers per launch (more: launches chained through out / the workspace)
constexpr int IA_THREADS = 256;
constexpr int IA_DC = 16;                       // output columns of one head a thread accumulates per pass over the keys
constexpr int IA_MAX_S = 16;                    // samples per workgroup tile
constexpr size_t IA_LDS_TARGET = 80 * 1024;     // two workgroups per CU where the samples allow it

struct IaParams {
    const float* x;
    int64_t batch;
    int64_t x_stride;
    int32_t F, E, n_layers, d, H, use_res, scaling;
    float sqrt_d;            // (float) sqrt(d): the reference divides the fp32 scores by the fp32 constant
    int32_t S;               // samples per tile
    int32_t ldx, ldq;        // row strides (floats) of X and of Q / K / V / R
    int64_t tile_floats;     // floats of one tile's buffers (general route: the per-workgroup workspace slice)
    const float* W[IA_MAX_LAYERS][4];
    float* out;
    int64_t out_stride;
    const float* head_w;
    float* logit;
    float* ws;               // general route only
};

__device__ __forceinline__ float ia_dot(const float* a, const float* b, int n) {
    float s = 0.f;
    for (int c = 0; c < n; ++c) s = fmaf(a[c], b[c], s);
    return s;
}

template <bool GLOBAL_WS>
__global__ __launch_bounds__(IA_THREADS) void interacting_kernel(IaParams p) {
    extern __shared__ __attribute__((aligned(16))) float ia_lds[];
    float* X = GLOBAL_WS ? p.ws + (int64_t)blockIdx.x * p.tile_floats : ia_lds;
    const int S = p.S, F = p.F, d = p.d, H = p.H, dH = d * H, SF = S * F, ldx = p.ldx, ldq = p.ldq;
    const int rows_pad = (SF + 15) & ~15;
    float* Qb = X + rows_pad * ldx;
    float* Kb = Qb + SF * ldq;
    float* Vb = Kb + SF * ldq;
    float* Rb = Vb + SF * ldq;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int nw = p.use_res ? 4 : 3;
    const int RT = rows_pad >> 4, CT = (dH + 15) >> 4;
    const int64_t n_tiles = (p.batch + S - 1) / S;

    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t b0 = tile * S;
        const int nvalid = (int)min((int64_t)S, p.batch - b0);
        // layer-0 input; zeros in the K padding, in the rows of samples past the batch and in the row padding
        for (int e = tid; e < rows_pad * ldx; e += IA_THREADS) {
            const int r = e / ldx, c = e - r * ldx;
            const int s = r / F, f = r - s * F;
            float v = 0.f;
            if (r < SF && s < nvalid && c < p.E) v = p.x[(b0 + s) * p.x_stride + (int64_t)f * p.E + c];
            X[e] = v;
        }
        __syncthreads();
        int K = p.E;
        for (int l = 0; l < p.n_layers; ++l) {
            const int KQ = ((K + 15) & ~15) >> 2;
            // Q, K, V (, R) = X W: one 16 x 16 output tile per wave task
            for (int t = wave; t < RT * CT * nw; t += IA_THREADS / 64) {
                const int m = t % nw, rest = t / nw, ct = rest % CT, rt = rest / CT;
                dctr::f32x4 acc[1] = {{0.f, 0.f, 0.f, 0.f}};
                dctr::tile_gemm_kn<1>(X + rt * 16 * ldx, ldx, K, KQ, p.W[l][m], dH, ct * 16, acc);
                float* dst = m == 0 ? Qb : m == 1 ? Kb : m == 2 ? Vb : Rb;
                const int col = ct * 16 + (lane & 15), row0 = rt * 16 + 4 * (lane >> 4);
                if (col < dH) {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (row0 + r < SF) dst[(row0 + r) * ldq + col] = acc[0][r];
                }
            }
            __syncthreads();
            // attention + residual + ReLU, written over X (read by nobody now)
            for (int it = tid; it < nvalid * F * H; it += IA_THREADS) {
                const int h = it % H, row = it / H, s = row / F;
                const float* q = Qb + row * ldq + h * d;
                const float* kb = Kb + s * F * ldq + h * d;
                const float* vb = Vb + s * F * ldq + h * d;
                float mx = -INFINITY;
                for (int j = 0; j < F; ++j) {
                    float sc = ia_dot(q, kb + j * ldq, d);
                    if (p.scaling) sc = sc / p.sqrt_d;
                    mx = fmaxf(mx, sc);
                }
                for (int c0 = 0; c0 < d; c0 += IA_DC) {
                    float acc[IA_DC];
#pragma unroll
                    for (int c = 0; c < IA_DC; ++c) acc[c] = 0.f;
                    float sum = 0.f;
                    for (int j = 0; j < F; ++j) {
                        float sc = ia_dot(q, kb + j * ldq, d);
                        if (p.scaling) sc = sc / p.sqrt_d;
                        const float e = __expf(sc - mx);
                        sum += e;
                        const float* vj = vb + j * ldq + c0;
#pragma unroll
                        for (int c = 0; c < IA_DC; ++c)
                            if (c0 + c < d) acc[c] = fmaf(e, vj[c], acc[c]);
                    }
                    const float inv = 1.f / sum;
                    float* xo = X + row * ldx + h * d + c0;
                    const float* rr = Rb + row * ldq + h * d + c0;
#pragma unroll
                    for (int c = 0; c < IA_DC; ++c) {
                        if (c0 + c < d) {
                            float o = acc[c] * inv;
                            if (p.use_res) o += rr[c];
                            xo[c] = fmaxf(o, 0.f);
                        }
                    }
                }
            }
            // the next layer reads K = d*H columns padded to 16: clear what the layer-0 input left in that padding
            const int zc = ((dH + 15) & ~15) - dH;
            for (int e = tid; e < SF * zc; e += IA_THREADS) {
                const int r = e / zc;
                X[r * ldx + dH + (e - r * zc)] = 0.f;
            }
            __syncthreads();
            K = dH;
        }
        if (p.out) {
            const int n = F * dH;
            for (int e = tid; e < nvalid * n; e += IA_THREADS) {
                const int s = e / n, rem = e - s * n, f = rem / dH, c = rem - f * dH;
                p.out[(b0 + s) * p.out_stride + rem] = X[(s * F + f) * ldx + c];
            }
        }
        if (p.logit) {
            const int n = F * dH;
            for (int s = wave; s < nvalid; s += IA_THREADS / 64) {
                float acc = 0.f;
                for (int e = lane; e < n; e += 64) {
                    const int f = e / dH, c = e - f * dH;
                    acc = fmaf(X[(s * F + f) * ldx + c], p.head_w[e], acc);
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
                if (lane == 0) p.logit[b0 + s] = acc;
            }
        }
        __syncthreads();    // X is reloaded for the next tile
    }
}

struct IaPlan {
    bool global;            // the general route (buffers in the workspace)
    int S, ldx, ldq;
    int64_t tile_floats;
    int grid_max;           // general route: workgroups the workspace has slices for
    size_t route_bytes;     // workspace of the general route (0 on the LDS route)
    size_t chain_bytes;     // > 32 layers without `out`: the activations between launches
};

int64_t ia_tile_floats(int S, int F, int ldx, int ldq, int nb) {
    const int64_t sf = (int64_t)S * F;
    const int64_t v = ((sf + 15) & ~(int64_t)15) * ldx + nb * sf * ldq;
    return (v + 3) & ~(int64_t)3;
}

void ia_plan(const dctr_interacting_args_t* a, IaPlan* pl) {
    const int dH = a->att_embedding_size * a->head_num;
    const int wmax = a->dim > dH ? a->dim : dH;
    pl->ldx = ((wmax + 15) & ~15) + 4;
    pl->ldq = dH | 1;
    const int nb = a->use_res ? 4 : 3;
    int S = IA_MAX_S;
    while (S > 1 && (size_t)ia_tile_floats(S, a->fields, pl->ldx, pl->ldq, nb) * 4 > IA_LDS_TARGET) --S;
    pl->chain_bytes = 0;
    if (a->n_layers > IA_MAX_LAYERS && !a->out)
        pl->chain_bytes = (size_t)(a->batch > 0 ? a->batch : 0) * a->fields * dH * sizeof(float);
    // S > 1 left the loop under IA_LDS_TARGET: only a single sample's tile can exceed the LDS and take the general route
    pl->S = S;
    pl->tile_floats = ia_tile_floats(S, a->fields, pl->ldx, pl->ldq, nb);
    const dctr_tile_route r = dctr_plan_tile_route((size_t)pl->tile_floats * 4);
    pl->global = r.global;
    pl->grid_max = r.grid_max;
    pl->route_bytes = r.route_bytes;
}

int ia_check(const dctr_interacting_args_t* a) {
    DCTR_REQUIRE(a, DCTR_E_NULL, "interacting_fwd: null args");
    DCTR_REQUIRE(a->batch >= 0 && a->fields >= 1 && a->dim >= 1 && a->n_layers >= 1 && a->att_embedding_size >= 1 &&
                     a->head_num >= 1, DCTR_E_DIM, "interacting_fwd: bad sizes");
    const int64_t dH = (int64_t)a->att_embedding_size * a->head_num;
    const int64_t wmax = a->dim > dH ? a->dim : dH;
    // a tile's buffers are indexed in 32 bits: about 400 M floats per sample
    DCTR_REQUIRE(dH <= (1 << 24) && a->dim <= (1 << 24) && ((int64_t)a->fields + 16) * (wmax + 20) * 5 < 0x7fffffffLL, DCTR_E_DIM,
                 "interacting_fwd: one sample's buffers exceed 2^31 floats");
    DCTR_REQUIRE(a->x_stride >= (int64_t)a->fields * a->dim, DCTR_E_DIM, "interacting_fwd: x_stride < fields*dim");
    DCTR_REQUIRE(!a->out || a->out_stride >= (int64_t)a->fields * dH, DCTR_E_DIM, "interacting_fwd: out_stride < fields*d*H");
    DCTR_REQUIRE((a->use_res == 0 || a->use_res == 1) && (a->scaling == 0 || a->scaling == 1), DCTR_E_ENUM,
                 "interacting_fwd: use_res / scaling must be 0 or 1");
    DCTR_REQUIRE((a->head_w == nullptr) == (a->logit == nullptr), DCTR_E_NULL, "interacting_fwd: head_w and logit go together");
    return DCTR_OK;
}

}  // namespace

extern "C" size_t dctr_interacting_workspace_bytes(const dctr_interacting_args_t* args) {
    if (ia_check(args) != DCTR_OK) return 0;
    IaPlan pl;
    ia_plan(args, &pl);
    return pl.route_bytes + pl.chain_bytes;
}

extern "C" int dctr_interacting_fwd(const dctr_interacting_args_t* a, void* stream) {
    int rc = ia_check(a);
    if (rc != DCTR_OK) return rc;
    if (a->batch == 0) return DCTR_OK;
    DCTR_REQUIRE(a->x && a->layers, DCTR_E_NULL, "interacting_fwd: null x / layers");
    DCTR_REQUIRE(a->out || a->logit, DCTR_E_NULL, "interacting_fwd: neither out nor head_w / logit");
    for (int l = 0; l < a->n_layers; ++l)
        DCTR_REQUIRE(a->layers[4 * l] && a->layers[4 * l + 1] && a->layers[4 * l + 2] && (!a->use_res || a->layers[4 * l + 3]),
                     DCTR_E_NULL, "interacting_fwd: layer %d: null weight", l);
    IaPlan pl;
    ia_plan(a, &pl);
    const size_t need = pl.route_bytes + pl.chain_bytes;
    if (need) DCTR_REQUIRE_WORKSPACE("interacting_fwd", "dctr_interacting_workspace_bytes", a->workspace, a->workspace_bytes, need);
    const int dH = a->att_embedding_size * a->head_num;
    float* chain = a->out ? a->out : (pl.chain_bytes ? (float*)((char*)a->workspace + pl.route_bytes) : nullptr);
    const int64_t chain_stride = a->out ? a->out_stride : (int64_t)a->fields * dH;
    const int64_t n_tiles = dctr_ceil_div(a->batch, pl.S);
    const size_t lds = pl.global ? 0 : (size_t)pl.tile_floats * sizeof(float);
    if (!pl.global) {
        static thread_local size_t granted[DCTR_MAX_DEVICES] = {0};
        hipError_t e = dctr_grant_lds((const void*)interacting_kernel<false>, lds, granted);
        DCTR_REQUIRE(e == hipSuccess, (int)e, "interacting_fwd: cannot raise dynamic LDS: %s", hipGetErrorString(e));
    }
    const int64_t grid = pl.global ? (n_tiles < pl.grid_max ? n_tiles : pl.grid_max) : (n_tiles < (1 << 24) ? n_tiles : (1 << 24));
    for (int l0 = 0; l0 < a->n_layers; l0 += IA_MAX_LAYERS) {
        const int nl = a->n_layers - l0 < IA_MAX_LAYERS ? a->n_layers - l0 : IA_MAX_LAYERS;
        const bool last = l0 + nl == a->n_layers;
        IaParams p = {};
        p.x = l0 == 0 ? a->x : chain;
        p.x_stride = l0 == 0 ? a->x_stride : chain_stride;
        p.batch = a->batch;
        p.F = a->fields;
        p.E = l0 == 0 ? a->dim : dH;
        p.n_layers = nl;
        p.d = a->att_embedding_size;
        p.H = a->head_num;
        p.use_res = a->use_res;
        p.scaling = a->scaling;
        p.sqrt_d = (float)sqrt((double)a->att_embedding_size);
        p.S = pl.S;
        p.ldx = pl.ldx;
        p.ldq = pl.ldq;
        p.tile_floats = pl.tile_floats;
        for (int l = 0; l < nl; ++l)
            for (int m = 0; m < 4; ++m) p.W[l][m] = a->layers[4 * (l0 + l) + m];
        p.out = last ? a->out : chain;
        p.out_stride = last ? a->out_stride : chain_stride;
        p.head_w = last ? a->head_w : nullptr;
        p.logit = last ? a->logit : nullptr;
        p.ws = pl.global ? (float*)a->workspace : nullptr;
        if (pl.global)
            DCTR_LAUNCH(interacting_kernel<true>, dim3((unsigned)grid), dim3(IA_THREADS), 0, (hipStream_t)stream, p);
        else
            DCTR_LAUNCH(interacting_kernel<false>, dim3((unsigned)grid), dim3(IA_THREADS), lds, (hipStream_t)stream, p);
        rc = dctr_launch_status("dctr_interacting_fwd");
        if (rc != DCTR_OK) return rc;
    }
    return DCTR_OK;
}
