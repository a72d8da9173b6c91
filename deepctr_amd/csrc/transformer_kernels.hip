// Transformer.call (reference deepctr/layers/sequence.py:523-635) x n_layers: BST's sequence block (models/sequence/bst.py:84-92) with
// PositionEncoding (sequence.py:683-689) and LayerNormalization (layers/normalization.py:34-43).
//
// Reference per layer: Xq = x + pe_q sqrt(E), Xk = keys + pe_k sqrt(E); Q = Xq Wq, K = Xk Wk, V = Xk Wv; per head the [T, T] scores
// Q_h K_h^T / sqrt(d), where(key mask, ., -2^32+1), the diagonal too with blinding, - row max, softmax, * query mask, P V; heads
// concatenated; + Xq; LayerNorm; relu(r fw1) fw2 + r; the same LayerNorm.  TensorFlow writes nine of those tensors to HBM per layer.
//
// Here one launch runs every layer.  A workgroup owns a tile of S samples; their [S*T, E] activations stay in LDS from the layer-0
// input to the last layer's output:
//   * Xq and Xk are formed from one read of x (A = x + pe_q, Bk = keys + pe_k; the tables arrive pre-scaled);
//   * Q, K, V on v_mfma_f32_16x16x4_f32 (mfma_tile.h: row tiles of 16 of the S*T rows, K padded to 16 with zeros, weights streamed
//     from L2 in their Keras layout) — exact fp32, k-ordered;
//   * attention: one thread per (sample, query position, head) walks the T keys twice — the row max, then exp(s - max), its sum and
//     the P V accumulation in registers — so no [T, T] score matrix exists anywhere.  Key mask, blinding, 1 / sqrt(d), the query mask,
//     1 / sum and the residual are in that pass, written over Xq.
//     Why not an MFMA Q K^T tile with an online softmax: at T <= 64 and d = E / H of 4 .. 8 a 16x16x4 tile spends K = d on 1 - 2 MFMA
//     steps per 256 scores and then needs the scores moved from the accumulator layout into a row-wise softmax and back into an A
//     operand through LDS; the attention is 4 T^2 E of the 22 T E^2 + 4 T^2 E per layer (22 % at T 50, E 32) and the thread-per-row walk
//     runs it on the fp32 VALU, in its own phase between the matrix phases, with no score traffic through LDS and no extra barriers.
//   * LayerNorm: one wave per row, two shuffles reductions (mean, then the biased variance of the centred row), a divide;
//   * feed-forward per 16-row tile: the [16, 4E] hidden slab of a wave lives in LDS (one slab per wave), never [S*T, 4E];
//   * output: [B, T, E] at the caller's strides (in place over the input is allowed: a tile reads its own samples before it writes
//     them), or the mean / sum over all T rows as [B, E].
// A sample too large for the LDS takes the same kernel with those buffers in a per-workgroup slice of the workspace (the "general
// route": S = 1, <= 256 persistent workgroups): nothing is refused for its size.
//
// Cost model, FLOP per sample and layer: 6 T E^2 projections + 4 T^2 E attention + 16 T E^2 feed-forward
//   (T 50, E 32: 307,200 + 320,000 + 819,200 = 1.45 MFLOP).
// LDS budget of a tile, floats: 2 pad16(S T) (pad16(E) + 4)  [Xq, Xk]  +  3 S T (E | 1)  [Q, K, V]  +  4 x 16 (pad16(4E) + 4)  [hidden
//   slabs]  +  2 S T  [masks].  S is the largest <= 16 that keeps a tile within 80 KiB (two workgroups per CU); a single sample may take
//   up to 160 KiB; beyond that the general route.  T 50, E 32, S 1: 2 x 64 x 36 + 4,952 + 8,448 + 100 = 18,108 floats = 70.7 KiB
//   (37.7 KiB of the sample + 33 KiB of slabs); S 2 would be 104 KiB -> S = 1.
#include <math.h>
#include "dctr_common.h"
#include "tile_route.h"
#include "mfma_tile.h"
#include "transformer_device.h"

namespace {

constexpr int TF_MAX_LAYERS = 16;               // layers per launch (more: launches chained through out / the workspace)

struct TfParams {
    const float* x;
    const float* keys;       // nullptr: the keys are the queries
    int64_t batch;
    int64_t x_stride, x_row_stride, k_stride, k_row_stride;
    int32_t T, E, d, H, n_layers;
    int32_t use_pe, use_res, use_ffn, use_ln, blinding, output_type;
    float sqrt_d, eps;
    int32_t S, ldx, ldq, ldh;
    int64_t tile_floats;
    const int32_t* q_len;
    const int32_t* k_len;
    const uint8_t* q_mask;
    const uint8_t* k_mask;
    const float* W[TF_MAX_LAYERS][TF_NW];
    float* out;
    int64_t out_stride, out_row_stride;
    uint8_t* mask_out;
    float* ws;               // general route only
    float* tape;             // training forward only: the inputs of layers >= 1, [n_layers - 1][B][T][E]
};

// LayerNormalization.call alone: one wave per row of x [rows, dim] (gamma / beta may be null: scale / center off)
__global__ __launch_bounds__(TF_THREADS) void layer_norm_kernel(const float* __restrict__ x, int64_t rows, int dim, int64_t x_stride,
                                                                const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                float eps, float* __restrict__ out, int64_t out_stride) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * TF_WAVES + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float* row = x + r * x_stride;
    float s = 0.f;
    for (int c = lane; c < dim; c += 64) s += row[c];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    const float mean = s / (float)dim;
    float v = 0.f;
    for (int c = lane; c < dim; c += 64) {
        const float t = row[c] - mean;
        v = fmaf(t, t, v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const float sd = sqrtf(v / (float)dim + eps);
    for (int c = lane; c < dim; c += 64) {
        float y = (row[c] - mean) / sd;
        if (gamma) y *= gamma[c];
        if (beta) y += beta[c];
        out[r * out_stride + c] = y;
    }
}

// TAPE: the training forward, which also writes the input of every layer past the first to p.tape
template <bool GLOBAL_WS, bool TAPE>
__global__ __launch_bounds__(TF_THREADS) void transformer_kernel(TfParams p) {
    extern __shared__ __attribute__((aligned(16))) float tf_lds[];
    float* A = GLOBAL_WS ? p.ws + (int64_t)blockIdx.x * p.tile_floats : tf_lds;
    const int S = p.S, T = p.T, E = p.E, d = p.d, H = p.H, ST = S * T, ldx = p.ldx, ldq = p.ldq, ldh = p.ldh;
    const int rows_pad = (ST + 15) & ~15;
    float* Bk = A + rows_pad * ldx;
    float* Qb = Bk + rows_pad * ldx;
    float* Kb = Qb + ST * ldq;
    float* Vb = Kb + ST * ldq;
    float* slabs = Qb + ((3 * ST * ldq + 3) & ~3);
    float* qm = slabs + TF_WAVES * 16 * ldh;
    float* km = qm + ST;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int RT = rows_pad >> 4, CT = (E + 15) >> 4, E4 = 4 * E, CTH = (E4 + 15) >> 4;
    const int KQ = ((E + 15) & ~15) >> 2, KQH = ((E4 + 15) & ~15) >> 2;
    const int64_t n_tiles = (p.batch + S - 1) / S;

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
                if (p.mask_out) p.mask_out[b * T + t] = k != 0.f ? 1 : 0;
            }
            qm[e] = q;
            km[e] = k;
        }
        // layer-0 input; zeros in the K padding, in the rows of samples past the batch and in the row padding
        for (int e = tid; e < rows_pad * ldx; e += TF_THREADS) {
            const int r = e / ldx, c = e - r * ldx;
            const int s = r / T, t = r - s * T;
            float v = 0.f, kv = 0.f;
            if (r < ST && s < nvalid && c < E) {
                v = p.x[(b0 + s) * p.x_stride + (int64_t)t * p.x_row_stride + c];
                if (p.keys) kv = p.keys[(b0 + s) * p.k_stride + (int64_t)t * p.k_row_stride + c];
            }
            A[e] = v;
            Bk[e] = kv;
        }
        __syncthreads();
        for (int l = 0; l < p.n_layers; ++l) {
            const float* const* W = p.W[l];
            // Xq = x + pe_q, Xk = keys + pe_k (the keys of a layer past the first are its queries)
            const bool own_keys = l == 0 && p.keys != nullptr;
            for (int e = tid; e < ST * ldx; e += TF_THREADS) {
                const int r = e / ldx, c = e - r * ldx;
                const float xv = A[e];
                if constexpr (TAPE) {
                    if (l > 0 && c < E && r / T < nvalid)
                        p.tape[(((int64_t)(l - 1) * p.batch + b0 + r / T) * T + r % T) * E + c] = xv;
                }
                float kv = own_keys ? Bk[e] : xv;
                float qv = xv;
                if (p.use_pe && c < E) {
                    const int t = r % T;
                    qv = xv + W[7][t * E + c];
                    kv = kv + W[8][t * E + c];
                }
                A[e] = qv;
                Bk[e] = kv;
            }
            __syncthreads();
            tf_project_qkv(A, Bk, Qb, Kb, Vb, W, RT, CT, ST, E, KQ, ldx, ldq);
            __syncthreads();
            tf_attention<false>(A, Qb, Kb, Vb, qm, km, nvalid, T, H, d, ldx, ldq, p.blinding, p.use_res, p.sqrt_d, nullptr);
            __syncthreads();
            if (p.use_ln) {
                tf_layer_norm(A, ST, ldx, E, W[5], W[6], p.eps);
                __syncthreads();
            }
            if (p.use_ffn) {
                if (p.use_res) {        // (without the residual the reference computes the feed-forward and drops it)
                    float* slab = slabs + wave * 16 * ldh;
                    for (int rt0 = 0; rt0 < RT; rt0 += TF_WAVES) {
                        const int rt = rt0 + wave;
                        if (rt < RT) {
                            for (int ct = 0; ct < CTH; ++ct) {
                                dctr::f32x4 acc[1] = {{0.f, 0.f, 0.f, 0.f}};
                                dctr::tile_gemm_kn<1>(A + rt * 16 * ldx, ldx, E, KQ, W[3], E4, ct * 16, acc);
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
                                        if (row0 + r < ST) A[(row0 + r) * ldx + col] += acc[0][r];
                                }
                            }
                        }
                        __syncthreads();
                    }
                }
                if (p.use_ln) {
                    tf_layer_norm(A, ST, ldx, E, W[5], W[6], p.eps);
                    __syncthreads();
                }
            }
        }
        if (p.output_type == DCTR_TRANSFORMER_OUT_NONE) {
            const int n = T * E;
            for (int e = tid; e < nvalid * n; e += TF_THREADS) {
                const int s = e / n, rem = e - s * n, t = rem / E, c = rem - t * E;
                p.out[(b0 + s) * p.out_stride + (int64_t)t * p.out_row_stride + c] = A[(s * T + t) * ldx + c];
            }
        } else {
            for (int e = tid; e < nvalid * E; e += TF_THREADS) {
                const int s = e / E, c = e - s * E;
                float acc = 0.f;
                for (int t = 0; t < T; ++t) acc += A[(s * T + t) * ldx + c];
                if (p.output_type == DCTR_TRANSFORMER_OUT_MEAN) acc = acc / (float)T;
                p.out[(b0 + s) * p.out_stride + c] = acc;
            }
        }
        __syncthreads();    // the buffers are reloaded for the next tile
    }
}

struct TfPlan {
    bool global;
    int S, ldx, ldq, ldh;
    int64_t tile_floats;
    int grid_max;
    size_t route_bytes;     // workspace of the general route (0 on the fused route)
    size_t chain_bytes;     // > 16 layers with a pooled output: the activations between launches
};

int64_t tf_tile_floats(int S, int T, int ldx, int ldq, int ldh) {
    const int64_t st = (int64_t)S * T;
    const int64_t v = 2 * ((st + 15) & ~(int64_t)15) * ldx + ((3 * st * ldq + 3) & ~(int64_t)3) + (int64_t)TF_WAVES * 16 * ldh + 2 * st;
    return (v + 3) & ~(int64_t)3;
}

void tf_plan(const dctr_transformer_args_t* a, TfPlan* pl) {
    const int T = a->seq_len, E = a->dim;
    pl->ldx = ((E + 15) & ~15) + 4;
    pl->ldq = E | 1;
    pl->ldh = a->use_feed_forward && a->use_res ? ((4 * E + 15) & ~15) + 4 : 0;
    pl->chain_bytes = 0;
    if (a->n_layers > TF_MAX_LAYERS && a->output_type != DCTR_TRANSFORMER_OUT_NONE)
        pl->chain_bytes = (size_t)(a->batch > 0 ? a->batch : 0) * T * E * sizeof(float);
    int S = TF_MAX_S;
    while (S > 1 && (size_t)tf_tile_floats(S, T, pl->ldx, pl->ldq, pl->ldh) * 4 > TF_LDS_TARGET) --S;
    const bool fits = (size_t)tf_tile_floats(S, T, pl->ldx, pl->ldq, pl->ldh) * 4 <= DCTR_LDS_MAX;
    pl->global = !fits || a->route == DCTR_TRANSFORMER_ROUTE_GENERAL;      // the general route takes one sample per tile
    pl->S = pl->global ? 1 : S;
    pl->tile_floats = tf_tile_floats(pl->S, T, pl->ldx, pl->ldq, pl->ldh);
    const dctr_tile_route r = pl->global ? dctr_workspace_slices((size_t)pl->tile_floats * 4) : dctr_tile_route{false, 0, 0};
    pl->grid_max = r.grid_max;
    pl->route_bytes = r.route_bytes;
}

int tf_check(const dctr_transformer_args_t* a) {
    DCTR_REQUIRE(a, DCTR_E_NULL, "transformer_fwd: null args");
    DCTR_REQUIRE(a->batch >= 0 && a->seq_len >= 1 && a->dim >= 1 && a->n_layers >= 1 && a->att_embedding_size >= 1 && a->head_num >= 1,
                 DCTR_E_DIM, "transformer_fwd: bad sizes");
    DCTR_REQUIRE((int64_t)a->att_embedding_size * a->head_num == a->dim, DCTR_E_DIM,
                 "transformer_fwd: att_embedding_size * head_num must equal dim, got %d * %d != %d", a->att_embedding_size, a->head_num,
                 a->dim);
    // a tile's buffers are indexed in 32 bits
    DCTR_REQUIRE(a->dim <= (1 << 22) && ((int64_t)a->seq_len + 16) * ((int64_t)a->dim + 20) * 5 + 64 * (4 * (int64_t)a->dim + 20) < 0x7fffffffLL,
                 DCTR_E_DIM, "transformer_fwd: one sample's buffers exceed 2^31 floats");
    DCTR_REQUIRE(a->q_row_stride >= a->dim && a->q_stride >= ((int64_t)a->seq_len - 1) * a->q_row_stride + a->dim, DCTR_E_DIM,
                 "transformer_fwd: query strides smaller than the [seq_len, dim] block");
    DCTR_REQUIRE(!a->keys || (a->k_row_stride >= a->dim && a->k_stride >= ((int64_t)a->seq_len - 1) * a->k_row_stride + a->dim), DCTR_E_DIM,
                 "transformer_fwd: key strides smaller than the [seq_len, dim] block");
    const uint32_t flags = (uint32_t)(a->use_positional_encoding | a->use_res | a->use_feed_forward | a->use_layer_norm | a->blinding);
    DCTR_REQUIRE(flags <= 1u, DCTR_E_ENUM, "transformer_fwd: the use_* flags and blinding must be 0 or 1");
    DCTR_REQUIRE(a->output_type >= DCTR_TRANSFORMER_OUT_NONE && a->output_type <= DCTR_TRANSFORMER_OUT_SUM, DCTR_E_ENUM,
                 "transformer_fwd: unknown output_type %d", a->output_type);
    DCTR_REQUIRE(a->route >= DCTR_TRANSFORMER_ROUTE_AUTO && a->route <= DCTR_TRANSFORMER_ROUTE_GENERAL, DCTR_E_ENUM,
                 "transformer_fwd: unknown route %d", a->route);
    DCTR_REQUIRE(!(a->query_lengths && a->query_mask), DCTR_E_ENUM, "transformer_fwd: query_lengths and query_mask are both given");
    DCTR_REQUIRE(!(a->key_lengths && a->key_mask), DCTR_E_ENUM, "transformer_fwd: key_lengths and key_mask are both given");
    if (a->output_type == DCTR_TRANSFORMER_OUT_NONE)
        DCTR_REQUIRE(!a->out || (a->out_row_stride >= a->dim && a->out_stride >= ((int64_t)a->seq_len - 1) * a->out_row_stride + a->dim),
                     DCTR_E_DIM, "transformer_fwd: out strides smaller than the [seq_len, dim] block");
    else
        DCTR_REQUIRE(!a->out || a->out_stride >= a->dim, DCTR_E_DIM, "transformer_fwd: out_stride < dim");
    TfPlan pl;
    tf_plan(a, &pl);
    DCTR_REQUIRE(a->route != DCTR_TRANSFORMER_ROUTE_FUSED || !pl.global, DCTR_E_UNSUPPORTED,
                 "transformer_fwd: one sample of seq_len %d, dim %d does not fit the fused route's LDS", a->seq_len, a->dim);
    return DCTR_OK;
}

}  // namespace

extern "C" size_t dctr_transformer_workspace_bytes(const dctr_transformer_args_t* args) {
    if (tf_check(args) != DCTR_OK) return 0;
    TfPlan pl;
    tf_plan(args, &pl);
    return pl.route_bytes + pl.chain_bytes;
}

extern "C" int dctr_transformer_route(const dctr_transformer_args_t* args) {
    int rc = tf_check(args);
    if (rc != DCTR_OK) return rc;
    TfPlan pl;
    tf_plan(args, &pl);
    return pl.global ? DCTR_TRANSFORMER_ROUTE_GENERAL : DCTR_TRANSFORMER_ROUTE_FUSED;
}

namespace {

// dctr_transformer_fwd (tape == nullptr) and dctr_transformer_train_fwd (the same kernel under its TAPE flag)
template <bool TAPE>
int tf_forward(const dctr_transformer_args_t* a, float* tape, void* stream) {
    int rc = DCTR_OK;
    DCTR_REQUIRE(a->queries && a->layers && a->out, DCTR_E_NULL, "transformer_fwd: null queries / layers / out");
    for (int l = 0; l < a->n_layers; ++l) {
        const float* const* w = a->layers + TF_NW * l;
        DCTR_REQUIRE(w[0] && w[1] && w[2], DCTR_E_NULL, "transformer_fwd: layer %d: null query / key / value", l);
        DCTR_REQUIRE(!(a->use_feed_forward && a->use_res) || (w[3] && w[4]), DCTR_E_NULL, "transformer_fwd: layer %d: null fw1 / fw2", l);
        DCTR_REQUIRE(!a->use_layer_norm || (w[5] && w[6]), DCTR_E_NULL, "transformer_fwd: layer %d: null ln_gamma / ln_beta", l);
        DCTR_REQUIRE(!a->use_positional_encoding || (w[7] && w[8]), DCTR_E_NULL, "transformer_fwd: layer %d: null pe_q / pe_k", l);
    }
    TfPlan pl;
    tf_plan(a, &pl);
    const size_t need = pl.route_bytes + pl.chain_bytes;
    if (need) DCTR_REQUIRE_WORKSPACE("transformer_fwd", "dctr_transformer_workspace_bytes", a->workspace, a->workspace_bytes, need);
    if (a->batch == 0) return DCTR_OK;
    const int T = a->seq_len, E = a->dim;
    const bool pooled = a->output_type != DCTR_TRANSFORMER_OUT_NONE;
    float* chain = !pooled ? a->out : (pl.chain_bytes ? (float*)((char*)a->workspace + pl.route_bytes) : nullptr);
    const int64_t chain_stride = !pooled ? a->out_stride : (int64_t)T * E;
    const int64_t chain_row = !pooled ? a->out_row_stride : E;
    const int64_t n_tiles = dctr_ceil_div(a->batch, pl.S);
    const size_t lds = pl.global ? 0 : (size_t)pl.tile_floats * sizeof(float);
    if (!pl.global) {
        static thread_local size_t granted[DCTR_MAX_DEVICES] = {0};
        hipError_t e = dctr_grant_lds((const void*)transformer_kernel<false, TAPE>, lds, granted);
        DCTR_REQUIRE(e == hipSuccess, (int)e, "transformer_fwd: cannot raise dynamic LDS: %s", hipGetErrorString(e));
    }
    const int64_t grid = pl.global ? (n_tiles < pl.grid_max ? n_tiles : pl.grid_max) : (n_tiles < (1 << 24) ? n_tiles : (1 << 24));
    for (int l0 = 0; l0 < a->n_layers; l0 += TF_MAX_LAYERS) {
        const int nl = a->n_layers - l0 < TF_MAX_LAYERS ? a->n_layers - l0 : TF_MAX_LAYERS;
        const bool first = l0 == 0, last = l0 + nl == a->n_layers;
        TfParams p = {};
        p.x = first ? a->queries : chain;
        p.x_stride = first ? a->q_stride : chain_stride;
        p.x_row_stride = first ? a->q_row_stride : chain_row;
        p.keys = first && a->keys && a->keys != a->queries ? a->keys : nullptr;
        p.k_stride = a->k_stride;
        p.k_row_stride = a->k_row_stride;
        p.batch = a->batch;
        p.T = T;
        p.E = E;
        p.d = a->att_embedding_size;
        p.H = a->head_num;
        p.n_layers = nl;
        p.use_pe = a->use_positional_encoding;
        p.use_res = a->use_res;
        p.use_ffn = a->use_feed_forward;
        p.use_ln = a->use_layer_norm;
        p.blinding = a->blinding;
        p.output_type = last ? a->output_type : DCTR_TRANSFORMER_OUT_NONE;
        p.sqrt_d = (float)sqrt((double)a->att_embedding_size);
        p.eps = a->ln_eps;
        p.S = pl.S;
        p.ldx = pl.ldx;
        p.ldq = pl.ldq;
        p.ldh = pl.ldh;
        p.tile_floats = pl.tile_floats;
        p.q_len = a->query_lengths;
        p.k_len = a->key_lengths;
        p.q_mask = a->query_mask;
        p.k_mask = a->key_mask;
        for (int l = 0; l < nl; ++l)
            for (int m = 0; m < TF_NW; ++m) p.W[l][m] = a->layers[TF_NW * (l0 + l) + m];
        p.out = last ? a->out : chain;
        p.out_stride = last ? a->out_stride : chain_stride;
        p.out_row_stride = last ? a->out_row_stride : chain_row;
        p.mask_out = first ? a->key_mask_out : nullptr;
        p.ws = pl.global ? (float*)a->workspace : nullptr;
        p.tape = tape;
        if (pl.global)
            DCTR_LAUNCH((transformer_kernel<true, TAPE>), dim3((unsigned)grid), dim3(TF_THREADS), 0, (hipStream_t)stream, p);
        else
            DCTR_LAUNCH((transformer_kernel<false, TAPE>), dim3((unsigned)grid), dim3(TF_THREADS), lds, (hipStream_t)stream, p);
        rc = dctr_launch_status(TAPE ? "dctr_transformer_train_fwd" : "dctr_transformer_fwd");
        if (rc != DCTR_OK) return rc;
    }
    return DCTR_OK;
}

}  // namespace

extern "C" int dctr_transformer_fwd(const dctr_transformer_args_t* a, void* stream) {
    int rc = tf_check(a);
    if (rc != DCTR_OK) return rc;
    return tf_forward<false>(a, nullptr, stream);
}

extern "C" size_t dctr_transformer_tape_bytes(const dctr_transformer_args_t* a) {
    if (tf_check(a) != DCTR_OK || a->n_layers > DCTR_TRANSFORMER_BWD_MAX_LAYERS) return 0;
    return (size_t)(a->n_layers - 1) * (size_t)a->batch * a->seq_len * a->dim * sizeof(float);
}

extern "C" int dctr_transformer_train_fwd(const dctr_transformer_train_args_t* t, void* stream) {
    DCTR_REQUIRE(t, DCTR_E_NULL, "transformer_train_fwd: null args");
    const dctr_transformer_args_t* a = &t->fwd;
    int rc = tf_check(a);
    if (rc != DCTR_OK) return rc;
    DCTR_REQUIRE(a->n_layers <= DCTR_TRANSFORMER_BWD_MAX_LAYERS, DCTR_E_UNSUPPORTED,
                 "transformer_train_fwd: %d layers, the tape and the backward take at most %d", a->n_layers, DCTR_TRANSFORMER_BWD_MAX_LAYERS);
    const size_t need = dctr_transformer_tape_bytes(a);
    DCTR_REQUIRE(!need || (t->tape && t->tape_bytes >= need), DCTR_E_NULL,
                 "transformer_train_fwd: the tape needs %zu bytes (dctr_transformer_tape_bytes)", need);
    return tf_forward<true>(a, (float*)t->tape, stream);
}

extern "C" int dctr_layer_norm_fwd(const float* x, int64_t rows, int32_t dim, int64_t x_stride, const float* gamma, const float* beta,
                                   float eps, float* out, int64_t out_stride, void* stream) {
    DCTR_REQUIRE(rows >= 0 && dim >= 1 && x_stride >= dim && out_stride >= dim, DCTR_E_DIM, "layer_norm_fwd: bad sizes");
    DCTR_REQUIRE(rows < ((int64_t)1 << 31) * TF_WAVES, DCTR_E_DIM, "layer_norm_fwd: too many rows for one launch");
    if (rows == 0) return DCTR_OK;
    DCTR_REQUIRE(x && out, DCTR_E_NULL, "layer_norm_fwd: null x / out");
    DCTR_LAUNCH(layer_norm_kernel, dim3((unsigned)dctr_ceil_div(rows, TF_WAVES)), dim3(TF_THREADS), 0, (hipStream_t)stream, x, rows, dim,
                x_stride, gamma, beta, eps, out, out_stride);
    return dctr_launch_status("dctr_layer_norm_fwd");
}
