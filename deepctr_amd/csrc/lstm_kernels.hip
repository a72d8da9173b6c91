// BiLSTM.call (reference deepctr/layers/sequence.py:318-428) over tf.keras.layers.LSTM as documented, and BiasEncoding.call (:706-757):
// DSIN's session-interest interaction (models/sequence/dsin.py:121-122) and its bias encoding (:156-157).
//
// Reference: two independent stacks of ``layers`` LSTMs; the forward stack walks t = 0 .. T-1, the backward stack t = T-1 .. 0 and
// every backward layer's output is put back into time order before it feeds the next one.  One step, gate order i | f | c~ | o:
//   z = x_t W + h U + b;   i, f, o = sigma(z_i, z_f, z_o);   g = tanh(z_c);   c' = f c + i g;   h' = o tanh(c');   h_0 = c_0 = 0
// with no mask and no lengths.  Layer l >= layers - res_layers adds its input to its output, in each stack; the stacks meet in
// the final merge (fw | bw | sum | mul | ave | concat | none).  Keras unrolls that into 2 * layers * T cells of ~10 kernels each.
//
// Here one launch runs both stacks.  A workgroup owns a tile of 16 samples (the M of v_mfma_f32_16x16x4_f32) and walks the stack
// layer by layer with the layer's whole [T, 16, u] input and output sequences of BOTH directions on chip; intermediate layers never
// reach HBM.  A step is ONE phase with one barrier: a work item is (direction, 16 units); its wave accumulates the unit's four gates
// in four independent accumulators over the column tiles j, u + j, 2u + j, 3u + j (K = [x_t | h], the accumulators start at the
// bias), so the lane that owns unit j of a sample holds i, f, g and o of it and updates c (in place, only it touches the element) and
// h without any exchange through LDS.  h is double-buffered: step t reads H[t & 1] and writes H[(t + 1) & 1].  Forward step t and
// backward step T-1-t run in the same phase and share the barrier; the backward row is stored at its own time position, which IS the
// reversal.  The merge reads two tiles that are on chip and writes the output once.
// x_t W is NOT hoisted out of the time loop: its [T, 16, 4u] result for both directions is four times a sequence tile (164 KiB at
// T = 5, u = 64) and would push the shapes DSIN uses out of the LDS; the step keeps it in the same MFMA chain instead.
// RESIDENT route: the current layer's W, U and b of both directions are copied into LDS at the start of the layer (row pitch chosen
// so that the k-slot groups of a B-operand read fall on different banks) when they fit the 160 KiB next to the tiles; STREAMED
// route: the same step code with the B operands read from global / L2; when even the tiles exceed the LDS they live in a
// per-workgroup slice of the workspace.  Nothing is refused for its size.
//
// Cost model per sample: T x 2 x 4u (D + u) MACs per layer (D = Din for layer 0, else u) against a serial chain of T phases.
#include <math.h>
#include <type_traits>
#include "dctr_common.h"
#include "tile_route.h"
#include "mfma_tile.h"
#include "lstm_device.h"

namespace {

constexpr int LSTM_THREADS = 256;
constexpr int LSTM_WAVES = LSTM_THREADS / 64;
constexpr int LSTM_ROWS = 16;                   // samples of a tile
constexpr int LSTM_MAX_LAYERS = DCTR_LSTM_MAX_LAYERS;
constexpr int LSTM_GRID_MAX = 2048;
constexpr int LSTM_NW = DCTR_LSTM_LAYER_PTRS;   // fw kernel, fw recurrent kernel, fw bias, bw kernel, bw recurrent kernel, bw bias

struct LstmParams {
    const float* x;
    int64_t batch, x_stride, x_row_stride;
    int32_t T, Din, u, n_layers, res_layers, merge, hard_sigmoid;
    int32_t ldx, ld, ldc, KQx, KQh, ldw0, ldw, ldwh;
    int64_t tile_floats;
    const float* W[LSTM_MAX_LAYERS][LSTM_NW];
    float* out;
    int64_t out_stride, out_row_stride;
    float* out_bw;
    int64_t out_bw_stride, out_bw_row_stride;
    float* ws;               // tiles of the streamed route when they exceed the LDS
};

// the training forward (dctr_bilstm_train_fwd): the input-dropout masks [B, D_l] of every LSTM and the tape of h_t and c_t
struct LstmTrainParams : LstmParams {
    const float* mask[LSTM_MAX_LAYERS][2];
    float* tape;
};

using dctr::lstm_gate;
using dctr::lstm_gemm4;

// TRAIN: the forward of a training step (never with GLOBAL_TILES): every LSTM's input is multiplied by its dropout mask where it
// enters x_t W (the residual adds the unmasked input), and h_t, c_t of every (layer, direction, step, sample) go to the tape
template <bool RESIDENT, bool GLOBAL_TILES, bool TRAIN = false>
__global__ __launch_bounds__(LSTM_THREADS) void bilstm_kernel(typename std::conditional<TRAIN, LstmTrainParams, LstmParams>::type p) {
    extern __shared__ __attribute__((aligned(16))) float lstm_lds[];
    typedef typename std::conditional<RESIDENT, int, int64_t>::type IDX;
    float* tiles = GLOBAL_TILES ? p.ws + (int64_t)blockIdx.x * p.tile_floats : lstm_lds;
    float* wl = lstm_lds + p.tile_floats;           // RESIDENT only
    const int T = p.T, Din = p.Din, u = p.u, L = p.n_layers, ldx = p.ldx, ld = p.ld, ldc = p.ldc;
    const int64_t xt = (int64_t)LSTM_ROWS * ldx, st = (int64_t)LSTM_ROWS * ld;          // one step of x / of a sequence tile
    // tiles: X0 [T], then the sequence sets [set][direction][T] (one set when L = 1: layer l reads set (l - 1) & 1, writes l & 1),
    // H [direction][2], C [direction]
    float* X0 = tiles;
    float* SEQ = X0 + T * xt;
    float* H = SEQ + (L > 1 ? 4 : 2) * T * st;
    float* C = H + 4 * st;
    // TRAIN: the two directions' mask tiles of the current layer, in the layout of its input tile (ones without a mask)
    const int64_t mkt = (int64_t)LSTM_ROWS * max(ldx, ld);
    float* MK = C + 2 * LSTM_ROWS * ldc;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, j = lane & 15;
    const int CT = (u + 15) >> 4;
    // a direction the merge never reads is not computed
    const int d0 = p.merge == DCTR_LSTM_MERGE_BW ? 1 : 0, nd = (p.merge == DCTR_LSTM_MERGE_FW || p.merge == DCTR_LSTM_MERGE_BW) ? 1 : 2;
    const int64_t n_tiles = (p.batch + LSTM_ROWS - 1) / LSTM_ROWS;
    // zeros in the K padding of every tile, once: nothing below writes a padding column
    for (int64_t e = tid; e < p.tile_floats; e += LSTM_THREADS) tiles[e] = 0.f;

    for (int64_t tl = blockIdx.x; tl < n_tiles; tl += gridDim.x) {
        const int64_t b0 = tl * LSTM_ROWS;
        const int nvalid = (int)min((int64_t)LSTM_ROWS, p.batch - b0);
        __syncthreads();        // the zero fill; the previous tile's merge is done with the tiles
        const int64_t n_x = (int64_t)T * LSTM_ROWS * Din;
        for (int64_t e = tid; e < n_x; e += LSTM_THREADS) {
            const int t = (int)(e / (LSTM_ROWS * Din)), rem = (int)(e - (int64_t)t * (LSTM_ROWS * Din));
            const int row = rem / Din, c = rem - row * Din;
            X0[t * xt + row * ldx + c] = row < nvalid ? p.x[(b0 + row) * p.x_stride + (int64_t)t * p.x_row_stride + c] : 0.f;
        }
        for (int l = 0; l < L; ++l) {
            const int D = l ? u : Din, KQa = l ? p.KQh : p.KQx, lda = l ? ld : ldx;
            const int64_t at = l ? st : xt;
            const int ldwx = RESIDENT ? (l ? p.ldw : p.ldw0) : 4 * u, ldwh = RESIDENT ? p.ldwh : 4 * u;
            const int dir_floats = RESIDENT ? D * ldwx + u * ldwh + 4 * u : 0;      // (resident sizes fit the LDS, so 32 bits)
            const bool res = l >= L - p.res_layers;
            if (RESIDENT) {         // (the barrier behind the previous layer's last step released its weights)
                // rows of 4u floats: one 16-byte load feeds four LDS stores (the pitch need not be a multiple of 4)
                for (int d = d0; d < d0 + nd; ++d) {
                    float* dst = wl + d * dir_floats;
                    for (int m = 0; m < 2; ++m) {
                        const float4* sw = reinterpret_cast<const float4*>(p.W[l][3 * d + m]);
                        const int rows = m ? u : D, pitch = m ? ldwh : ldwx;
                        for (int e = tid; e < rows * u; e += LSTM_THREADS) {
                            const int row = e / u, c = 4 * (e - row * u);
                            const float4 v = sw[e];
                            float* o = dst + row * pitch + c;
                            o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
                        }
                        dst += rows * pitch;
                    }
                    const float* sb = p.W[l][3 * d + 2];
                    for (int e = tid; e < 4 * u; e += LSTM_THREADS) dst[e] = sb[e];
                }
            }
            if constexpr (TRAIN) {
                for (int d = d0; d < d0 + nd; ++d) {
                    const float* mk = p.mask[l][d];
                    for (int e = tid; e < LSTM_ROWS * D; e += LSTM_THREADS) {
                        const int row = e / D, c = e - row * D;
                        MK[d * mkt + row * lda + c] = !mk ? 1.f : row < nvalid ? mk[(b0 + row) * D + c] : 0.f;
                    }
                }
            }
            __syncthreads();                // x / the previous layer's sequences / the weights are in place
            for (int t = 0; t < T; ++t) {
                for (int item = wave; item < nd * CT; item += LSTM_WAVES) {
                    const int d = d0 + item / CT, ct = item % CT;
                    const int td = d ? T - 1 - t : t;
                    const float* in = (l ? SEQ + (((l - 1) & 1) * 2 + d) * T * st : X0) + td * at;
                    float* outp = SEQ + ((l & 1) * 2 + d) * T * st + td * st;
                    const float* Hc = H + (d * 2 + (t & 1)) * st;
                    float* Hn = H + (d * 2 + ((t + 1) & 1)) * st;
                    const float* Wx = RESIDENT ? wl + d * dir_floats : p.W[l][3 * d];
                    const float* Wh = RESIDENT ? Wx + D * ldwx : p.W[l][3 * d + 1];
                    const float* bv = RESIDENT ? Wh + u * ldwh : p.W[l][3 * d + 2];
                    const int col = ct * 16 + j, colc = min(col, u - 1);
                    dctr::f32x4 acc[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float b = bv[q * u + colc];
                        acc[q] = dctr::f32x4{b, b, b, b};
                    }
                    if constexpr (TRAIN)
                        lstm_gemm4<IDX, true>(in, lda, D, KQa, Wx, ldwx, u, colc, acc, MK + d * mkt);
                    else
                        lstm_gemm4<IDX>(in, lda, D, KQa, Wx, ldwx, u, colc, acc);
                    if (t) lstm_gemm4<IDX>(Hc, ld, u, p.KQh, Wh, ldwh, u, colc, acc);      // h_0 = 0
                    if (col < u) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int row = 4 * g + r;
                            const float ig = lstm_gate(acc[0][r], p.hard_sigmoid), fg = lstm_gate(acc[1][r], p.hard_sigmoid);
                            const float og = lstm_gate(acc[3][r], p.hard_sigmoid), gg = dctr::tanh_fast(acc[2][r]);
                            float* cp = C + (d * LSTM_ROWS + row) * ldc + col;
                            const float c = fmaf(fg, t ? *cp : 0.f, ig * gg);                // c_0 = 0
                            *cp = c;
                            const float h = og * dctr::tanh_fast(c);
                            Hn[row * ld + col] = h;
                            outp[row * ld + col] = res ? h + in[row * lda + col] : h;
                            if constexpr (TRAIN) {
                                if (row < nvalid) {
                                    float* tp = p.tape + ((((int64_t)l * 2 + d) * T + td) * 2 * p.batch + b0 + row) * u + col;
                                    tp[0] = h;
                                    tp[p.batch * u] = c;
                                }
                            }
                        }
                    }
                }
                __syncthreads();
            }
        }
        // the merge: both stacks' last sequences are on chip
        const float* F = SEQ + (((L - 1) & 1) * 2) * T * st;
        const float* Bw = F + T * st;
        const int64_t n_out = (int64_t)nvalid * T * u;
        for (int64_t e = tid; e < n_out; e += LSTM_THREADS) {
            const int row = (int)(e / ((int64_t)T * u));
            const int rem = (int)(e - (int64_t)row * T * u);
            const int t = rem / u, c = rem - t * u;
            const int64_t s = t * st + row * ld + c;
            float* o = p.out + (b0 + row) * p.out_stride + (int64_t)t * p.out_row_stride + c;
            switch (p.merge) {
                case DCTR_LSTM_MERGE_FW: *o = F[s]; break;
                case DCTR_LSTM_MERGE_BW: *o = Bw[s]; break;
                case DCTR_LSTM_MERGE_SUM: *o = F[s] + Bw[s]; break;
                case DCTR_LSTM_MERGE_MUL: *o = F[s] * Bw[s]; break;
                case DCTR_LSTM_MERGE_AVE: *o = (F[s] + Bw[s]) / 2.f; break;
                case DCTR_LSTM_MERGE_CONCAT: o[0] = F[s]; o[u] = Bw[s]; break;
                default:
                    *o = F[s];
                    p.out_bw[(b0 + row) * p.out_bw_stride + (int64_t)t * p.out_bw_row_stride + c] = Bw[s];
            }
        }
    }
}

struct LstmPlan {
    bool resident, global_tiles;
    int ldx, ld, ldc, KQx, KQh, ldw0, ldw, ldwh;
    int64_t tile_floats;
    size_t lds_bytes;
    int grid_max;
    size_t ws_bytes;
};

void lstm_plan(const dctr_lstm_args_t* a, LstmPlan* pl, bool train = false) {
    const int64_t T = a->seq_len, Din = a->in_dim, u = a->units, L = a->n_layers;
    const dctr::LstmPitch lp = dctr::lstm_pitches(Din, u);
    pl->ldx = lp.ldx;
    pl->ld = lp.ld;
    pl->ldc = lp.ldc;
    pl->KQx = lp.KQx;
    pl->KQh = lp.KQh;
    pl->ldw0 = lp.ldw0;
    pl->ldw = lp.ldw;
    pl->ldwh = lp.ldwh;
    const int64_t xt = (int64_t)LSTM_ROWS * pl->ldx, st = (int64_t)LSTM_ROWS * pl->ld;
    // (the training forward's two mask tiles behind the cell states)
    pl->tile_floats = (T * xt + (L > 1 ? 4 : 2) * T * st + 4 * st + 2 * (int64_t)LSTM_ROWS * pl->ldc + (train ? 2 * (xt > st ? xt : st) : 0) + 3) &
                      ~(int64_t)3;
    // the widest layer's W, U and b of both directions
    const int64_t w0 = Din * pl->ldw0 + u * pl->ldwh + 4 * u, w1 = u * pl->ldw + u * pl->ldwh + 4 * u;
    const int64_t w_floats = 2 * (L > 1 && w1 > w0 ? w1 : w0);
    const size_t tiles_bytes = (size_t)pl->tile_floats * 4;
    const size_t res_bytes = tiles_bytes + (size_t)w_floats * 4;
    const bool res_fits = res_bytes <= DCTR_LDS_MAX;
    pl->resident = res_fits && (a->route == DCTR_LSTM_ROUTE_AUTO || a->route == DCTR_LSTM_ROUTE_RESIDENT);
    pl->global_tiles = !pl->resident && (tiles_bytes > DCTR_LDS_MAX || a->route == DCTR_LSTM_ROUTE_WORKSPACE);
    pl->lds_bytes = pl->resident ? res_bytes : pl->global_tiles ? 0 : tiles_bytes;
    pl->grid_max = LSTM_GRID_MAX;
    pl->ws_bytes = 0;
    if (pl->global_tiles) {
        const dctr_tile_route r = dctr_workspace_slices(tiles_bytes);
        pl->grid_max = r.grid_max;
        pl->ws_bytes = r.route_bytes;
    }
}

bool lstm_resident_fits(const dctr_lstm_args_t* a) {
    dctr_lstm_args_t b = *a;
    b.route = DCTR_LSTM_ROUTE_AUTO;
    LstmPlan pl;
    lstm_plan(&b, &pl);
    return pl.resident;
}

int lstm_check(const dctr_lstm_args_t* a) {
    DCTR_REQUIRE(a, DCTR_E_NULL, "bilstm_fwd: null args");
    DCTR_REQUIRE(a->batch >= 0 && a->seq_len >= 1 && a->in_dim >= 1 && a->units >= 1, DCTR_E_DIM, "bilstm_fwd: bad sizes");
    DCTR_REQUIRE(a->n_layers >= 1 && a->n_layers <= LSTM_MAX_LAYERS, DCTR_E_DIM, "bilstm_fwd: n_layers must be 1..%d, got %d", LSTM_MAX_LAYERS,
                 a->n_layers);
    DCTR_REQUIRE(a->res_layers >= 0, DCTR_E_DIM, "bilstm_fwd: res_layers < 0");
    // a tile's rows are indexed in 32 bits
    DCTR_REQUIRE(a->units <= (1 << 20) && a->in_dim <= (1 << 20) && a->seq_len <= (1 << 20), DCTR_E_DIM,
                 "bilstm_fwd: seq_len / in_dim / units exceed 2^20");
    DCTR_REQUIRE(a->res_layers < a->n_layers || a->in_dim == a->units, DCTR_E_DIM,
                 "bilstm_fwd: a residual over layer 0 needs in_dim == units, got %d and %d", a->in_dim, a->units);
    DCTR_REQUIRE(a->merge_mode >= DCTR_LSTM_MERGE_FW && a->merge_mode <= DCTR_LSTM_MERGE_NONE, DCTR_E_ENUM, "bilstm_fwd: unknown merge_mode %d",
                 a->merge_mode);
    DCTR_REQUIRE((uint32_t)a->recurrent_activation <= 1u, DCTR_E_ENUM, "bilstm_fwd: unknown recurrent_activation %d", a->recurrent_activation);
    DCTR_REQUIRE(a->route >= DCTR_LSTM_ROUTE_AUTO && a->route <= DCTR_LSTM_ROUTE_WORKSPACE, DCTR_E_ENUM, "bilstm_fwd: unknown route %d", a->route);
    DCTR_REQUIRE(a->x_row_stride >= a->in_dim && a->x_stride >= ((int64_t)a->seq_len - 1) * a->x_row_stride + a->in_dim, DCTR_E_DIM,
                 "bilstm_fwd: x strides smaller than the [seq_len, in_dim] block");
    const int64_t w = a->merge_mode == DCTR_LSTM_MERGE_CONCAT ? 2 * (int64_t)a->units : a->units;
    DCTR_REQUIRE(a->out_row_stride >= w && a->out_stride >= ((int64_t)a->seq_len - 1) * a->out_row_stride + w, DCTR_E_DIM,
                 "bilstm_fwd: out strides smaller than the [seq_len, %lld] block", (long long)w);
    if (a->merge_mode == DCTR_LSTM_MERGE_NONE)
        DCTR_REQUIRE(a->out_bw_row_stride >= a->units && a->out_bw_stride >= ((int64_t)a->seq_len - 1) * a->out_bw_row_stride + a->units,
                     DCTR_E_DIM, "bilstm_fwd: out_bw strides smaller than the [seq_len, units] block");
    DCTR_REQUIRE(a->route != DCTR_LSTM_ROUTE_RESIDENT || lstm_resident_fits(a), DCTR_E_UNSUPPORTED,
                 "bilstm_fwd: a layer's kernels of %d units over %d steps do not fit the resident route's LDS", a->units, a->seq_len);
    return DCTR_OK;
}

void lstm_fill(const dctr_lstm_args_t* a, const LstmPlan& pl, LstmParams* p) {
    p->x = a->x;
    p->batch = a->batch;
    p->x_stride = a->x_stride;
    p->x_row_stride = a->x_row_stride;
    p->T = a->seq_len;
    p->Din = a->in_dim;
    p->u = a->units;
    p->n_layers = a->n_layers;
    p->res_layers = a->res_layers < a->n_layers ? a->res_layers : a->n_layers;
    p->merge = a->merge_mode;
    p->hard_sigmoid = a->recurrent_activation;
    p->ldx = pl.ldx;
    p->ld = pl.ld;
    p->ldc = pl.ldc;
    p->KQx = pl.KQx;
    p->KQh = pl.KQh;
    p->ldw0 = pl.ldw0;
    p->ldw = pl.ldw;
    p->ldwh = pl.ldwh;
    p->tile_floats = pl.tile_floats;
    for (int l = 0; l < a->n_layers; ++l)
        for (int m = 0; m < LSTM_NW; ++m) p->W[l][m] = a->layers[LSTM_NW * l + m];
    p->out = a->out;
    p->out_stride = a->out_stride;
    p->out_row_stride = a->out_row_stride;
    p->out_bw = a->out_bw;
    p->out_bw_stride = a->out_bw_stride;
    p->out_bw_row_stride = a->out_bw_row_stride;
    p->ws = pl.global_tiles ? (float*)a->workspace : nullptr;
}

__global__ void bias_encoding_kernel(float* x, int64_t n, int32_t S, int32_t T, int32_t E, int64_t sb, int64_t ss, int64_t st, const float* sess,
                                     const float* seq, const float* item) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int e = (int)(i % E);
        const int64_t r = i / E;
        const int t = (int)(r % T);
        const int64_t r2 = r / T;
        const int s = (int)(r2 % S);
        const int64_t b = r2 / S;
        x[b * sb + s * ss + t * st + e] += item[e] + seq[t] + sess[s];
    }
}

}  // namespace

extern "C" size_t dctr_bilstm_workspace_bytes(const dctr_lstm_args_t* args) {
    if (lstm_check(args) != DCTR_OK) return 0;
    LstmPlan pl;
    lstm_plan(args, &pl);
    return pl.ws_bytes;
}

extern "C" int dctr_bilstm_route(const dctr_lstm_args_t* args) {
    int rc = lstm_check(args);
    if (rc != DCTR_OK) return rc;
    LstmPlan pl;
    lstm_plan(args, &pl);
    return pl.resident ? DCTR_LSTM_ROUTE_RESIDENT : DCTR_LSTM_ROUTE_STREAMED;
}

extern "C" int dctr_bilstm_fwd(const dctr_lstm_args_t* a, void* stream) {
    int rc = lstm_check(a);
    if (rc != DCTR_OK) return rc;
    DCTR_REQUIRE(a->x && a->layers && a->out, DCTR_E_NULL, "bilstm_fwd: null x / layers / out");
    DCTR_REQUIRE(a->merge_mode != DCTR_LSTM_MERGE_NONE || a->out_bw, DCTR_E_NULL, "bilstm_fwd: merge_mode none needs out_bw");
    for (int l = 0; l < a->n_layers; ++l)
        for (int m = 0; m < LSTM_NW; ++m)
            DCTR_REQUIRE(a->layers[LSTM_NW * l + m], DCTR_E_NULL, "bilstm_fwd: layer %d: null kernel / recurrent kernel / bias", l);
    LstmPlan pl;
    lstm_plan(a, &pl);
    if (pl.resident)        // the copy into LDS reads the kernels 16 bytes at a time
        for (int l = 0; l < a->n_layers; ++l)
            for (int m = 0; m < LSTM_NW; ++m)
                DCTR_REQUIRE(m % 3 == 2 || dctr_aligned16(a->layers[LSTM_NW * l + m]), DCTR_E_ALIGN,
                             "bilstm_fwd: layer %d: kernel / recurrent kernel not 16-B aligned", l);
    if (pl.ws_bytes)
        DCTR_REQUIRE_WORKSPACE("bilstm_fwd", "dctr_bilstm_workspace_bytes", a->workspace, a->workspace_bytes, pl.ws_bytes);
    if (a->batch == 0) return DCTR_OK;
    LstmParams p = {};
    lstm_fill(a, pl, &p);
    const int64_t n_tiles = dctr_ceil_div(a->batch, LSTM_ROWS);
    const unsigned grid = (unsigned)(n_tiles < pl.grid_max ? n_tiles : pl.grid_max);
    if (pl.resident) {
        static thread_local size_t granted[DCTR_MAX_DEVICES] = {0};
        hipError_t e = dctr_grant_lds((const void*)bilstm_kernel<true, false>, pl.lds_bytes, granted);
        DCTR_REQUIRE(e == hipSuccess, (int)e, "bilstm_fwd: cannot raise dynamic LDS: %s", hipGetErrorString(e));
        DCTR_LAUNCH((bilstm_kernel<true, false>), dim3(grid), dim3(LSTM_THREADS), pl.lds_bytes, (hipStream_t)stream, p);
    } else if (!pl.global_tiles) {
        static thread_local size_t granted[DCTR_MAX_DEVICES] = {0};
        hipError_t e = dctr_grant_lds((const void*)bilstm_kernel<false, false>, pl.lds_bytes, granted);
        DCTR_REQUIRE(e == hipSuccess, (int)e, "bilstm_fwd: cannot raise dynamic LDS: %s", hipGetErrorString(e));
        DCTR_LAUNCH((bilstm_kernel<false, false>), dim3(grid), dim3(LSTM_THREADS), pl.lds_bytes, (hipStream_t)stream, p);
    } else {
        DCTR_LAUNCH((bilstm_kernel<false, true>), dim3(grid), dim3(LSTM_THREADS), pl.lds_bytes, (hipStream_t)stream, p);
    }
    return dctr_launch_status("dctr_bilstm_fwd");
}

extern "C" size_t dctr_bilstm_tape_bytes(const dctr_lstm_args_t* a) {
    if (lstm_check(a) != DCTR_OK) return 0;
    return (size_t)a->n_layers * 2 * (size_t)a->seq_len * 2 * (size_t)a->batch * (size_t)a->units * sizeof(float);
}

// (lstm_bwd_kernels.hip: the backward's arguments pass the forward's checks first, and it asks whether the training forward takes a
// shape before it does: it reads the tape only that forward writes)
int dctr_lstm_check_args(const dctr_lstm_args_t* a) { return lstm_check(a); }

bool dctr_lstm_train_fwd_fits(const dctr_lstm_args_t* a) {
    if (a->route == DCTR_LSTM_ROUTE_WORKSPACE) return false;
    LstmPlan pl;
    lstm_plan(a, &pl, true);
    return !pl.global_tiles;
}

extern "C" int dctr_bilstm_train_fwd(const dctr_lstm_train_args_t* t, void* stream) {
    DCTR_REQUIRE(t, DCTR_E_NULL, "bilstm_train_fwd: null args");
    const dctr_lstm_args_t* a = &t->fwd;
    int rc = lstm_check(a);
    if (rc != DCTR_OK) return rc;
    DCTR_REQUIRE(dctr_lstm_train_fwd_fits(a), DCTR_E_UNSUPPORTED,
                 "bilstm_train_fwd: the tiles of %d units over %d steps and %d layer(s) do not fit the LDS (no workspace route)", a->units,
                 a->seq_len, a->n_layers);
    DCTR_REQUIRE(a->x && a->layers && a->out, DCTR_E_NULL, "bilstm_train_fwd: null x / layers / out");
    DCTR_REQUIRE(a->merge_mode != DCTR_LSTM_MERGE_NONE || a->out_bw, DCTR_E_NULL, "bilstm_train_fwd: merge_mode none needs out_bw");
    for (int l = 0; l < a->n_layers; ++l)
        for (int m = 0; m < LSTM_NW; ++m)
            DCTR_REQUIRE(a->layers[LSTM_NW * l + m], DCTR_E_NULL, "bilstm_train_fwd: layer %d: null kernel / recurrent kernel / bias", l);
    LstmPlan pl;
    lstm_plan(a, &pl, true);
    DCTR_REQUIRE(a->route != DCTR_LSTM_ROUTE_RESIDENT || pl.resident, DCTR_E_UNSUPPORTED,
                 "bilstm_train_fwd: a layer's kernels of %d units over %d steps do not fit the resident route's LDS", a->units, a->seq_len);
    if (pl.resident)
        for (int l = 0; l < a->n_layers; ++l)
            for (int m = 0; m < LSTM_NW; ++m)
                DCTR_REQUIRE(m % 3 == 2 || dctr_aligned16(a->layers[LSTM_NW * l + m]), DCTR_E_ALIGN,
                             "bilstm_train_fwd: layer %d: kernel / recurrent kernel not 16-B aligned", l);
    DCTR_REQUIRE(a->batch == 0 || (t->tape && t->tape_bytes >= dctr_bilstm_tape_bytes(a)), DCTR_E_NULL,
                 "bilstm_train_fwd: needs a tape of dctr_bilstm_tape_bytes() bytes");
    if (a->batch == 0) return DCTR_OK;
    LstmTrainParams p = {};
    lstm_fill(a, pl, &p);
    for (int l = 0; l < a->n_layers; ++l)
        for (int d = 0; d < 2; ++d) p.mask[l][d] = t->masks ? t->masks[2 * l + d] : nullptr;
    p.tape = (float*)t->tape;
    const int64_t n_tiles = dctr_ceil_div(a->batch, LSTM_ROWS);
    const unsigned grid = (unsigned)(n_tiles < pl.grid_max ? n_tiles : pl.grid_max);
    if (pl.resident) {
        static thread_local size_t granted[DCTR_MAX_DEVICES] = {0};
        hipError_t e = dctr_grant_lds((const void*)bilstm_kernel<true, false, true>, pl.lds_bytes, granted);
        DCTR_REQUIRE(e == hipSuccess, (int)e, "bilstm_train_fwd: cannot raise dynamic LDS: %s", hipGetErrorString(e));
        DCTR_LAUNCH((bilstm_kernel<true, false, true>), dim3(grid), dim3(LSTM_THREADS), pl.lds_bytes, (hipStream_t)stream, p);
    } else {
        static thread_local size_t granted[DCTR_MAX_DEVICES] = {0};
        hipError_t e = dctr_grant_lds((const void*)bilstm_kernel<false, false, true>, pl.lds_bytes, granted);
        DCTR_REQUIRE(e == hipSuccess, (int)e, "bilstm_train_fwd: cannot raise dynamic LDS: %s", hipGetErrorString(e));
        DCTR_LAUNCH((bilstm_kernel<false, false, true>), dim3(grid), dim3(LSTM_THREADS), pl.lds_bytes, (hipStream_t)stream, p);
    }
    return dctr_launch_status("dctr_bilstm_train_fwd");
}

extern "C" int dctr_bias_encoding_fwd(float* x, int64_t batch, int32_t sess, int32_t seq_len, int32_t dim, int64_t x_stride, int64_t sess_stride,
                                      int64_t row_stride, const float* sess_bias, const float* seq_bias, const float* item_bias, void* stream) {
    DCTR_REQUIRE(batch >= 0 && sess >= 1 && seq_len >= 1 && dim >= 1, DCTR_E_DIM, "bias_encoding_fwd: bad sizes");
    DCTR_REQUIRE(row_stride >= dim && sess_stride >= ((int64_t)seq_len - 1) * row_stride + dim &&
                     x_stride >= ((int64_t)sess - 1) * sess_stride + ((int64_t)seq_len - 1) * row_stride + dim,
                 DCTR_E_DIM, "bias_encoding_fwd: strides smaller than the [sess, seq_len, dim] block");
    if (batch == 0) return DCTR_OK;
    DCTR_REQUIRE(x && sess_bias && seq_bias && item_bias, DCTR_E_NULL, "bias_encoding_fwd: null x / sess_bias / seq_bias / item_bias");
    const int64_t n = batch * sess * seq_len * dim;
    const int64_t blocks = dctr_ceil_div(n, 256);
    DCTR_LAUNCH(bias_encoding_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, (hipStream_t)stream, x, n, sess, seq_len, dim,
                x_stride, sess_stride, row_stride, sess_bias, seq_bias, item_bias);
    return dctr_launch_status("dctr_bias_encoding_fwd");
}
