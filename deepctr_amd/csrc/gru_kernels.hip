// DynamicGRU.call (reference deepctr/layers/sequence.py:760-815) over tf's GRUCell and the attention-gated cells of
// deepctr/contrib/utils.py (QAAttGRUCell :208-261 = AGRU, VecAttGRUCell :327-378 = AUGRU), under the sequence_length rule of
// dynamic_rnn (contrib/rnn_v2.py:1324-1401): DIEN's interest extractor and interest evolution (models/sequence/dien.py:66-109).
//
// Reference per step, with inputs and units of one width E:  [r | u] = sigmoid([x_t | h] Wg + bg);  c = tanh([x_t | r * h] Wc + bc);
//   GRU   h' = u h + (1 - u) c;    AGRU  h' = (1 - a) h + a c;    AUGRU  u <- (1 - a) u, then the GRU form;
// at t >= length the state is copied through and the emitted row is zero.  TensorFlow runs that as a while_loop of ~20 kernels per
// step and writes every intermediate to HBM.
//
// Here one launch runs the whole time loop.  A workgroup owns a tile of 16 samples (the M of v_mfma_f32_16x16x4_f32); per layer the
// state tile H, the r * h tile and the update gates stay in LDS for all T steps, x_t is double-buffered in LDS and fetched one step
// ahead (the loads are issued before the gate GEMM, their LDS stores after it), attention scores of a step are fetched the same way.
// A step of a layer is two phases with one barrier each:
//   1. gates: [16, 2E] = X Wg[:E] + H Wg[E:] on the matrix cores (16-column tiles over the four waves, K split x | h so that x_t needs
//      no copy next to h), sigmoid in the accumulator layout, r * h and u written to LDS;
//   2. candidate: [16, E] = X Wc[:E] + (r * h) Wc[E:], tanh, the cell's state update for the rows with t < length, in place over H by
//      the lane that owns the element, and the output row (zero past the length) straight to HBM.
// With n_layers = 2 (gru_type "GRU": gru1 -> gru2) layer 2's X at step t IS layer 1's state tile after its step t: layer 1's [B, T, E]
// never exists.  A tile loops to its own longest sample and zero-fills the rest.
// RESIDENT route: Wg, Wc and the biases of every layer are copied into LDS once per workgroup (row pitch chosen so that the four k-slot
// groups of a B-operand read fall on different banks) when they fit the 160 KiB next to the tiles; STREAMED route: the same step code
// with the B operands read from global / L2 each step; when even the tiles exceed the LDS (E >= 497) they live in a per-workgroup
// slice of the workspace.  Nothing is refused for its size.
//
// Cost model per sample: T x 6 E^2 MACs per layer (4 E^2 gates + 2 E^2 candidate) against a serial chain of 2 T dependent phases.
#include <math.h>
#include <type_traits>
#include "dctr_common.h"
#include "tile_route.h"
#include "mfma_tile.h"
#include "gru_device.h"

namespace {

using dctr::gru_gemm;
using dctr::gru_pitch;

constexpr int GRU_THREADS = 256;
constexpr int GRU_WAVES = GRU_THREADS / 64;
constexpr int GRU_ROWS = 16;                    // samples of a tile
constexpr int GRU_MAX_LAYERS = 2;
constexpr int GRU_XREG = 4;                     // x_{t+1} elements a thread holds in registers across the gate phase (E <= 64 entirely)
constexpr int GRU_GRID_MAX = 2048;
constexpr int GRU_NW = DCTR_GRU_LAYER_PTRS;     // gate kernel, gate bias, candidate kernel, candidate bias

struct GruParams {
    const float* x;
    int64_t batch, x_stride, x_row_stride;
    const int32_t* len;
    const float* att;
    int64_t att_stride;
    int32_t T, E, n_layers, cell, scale_input, return_sequence;
    int32_t ld, ldu, KQ, ldwg, ldwc;
    int64_t tile_floats;
    const float* W[GRU_MAX_LAYERS][GRU_NW];
    float* out;
    int64_t out_stride, out_row_stride;
    float* ws;               // tiles of the streamed route when they exceed the LDS
};

// phase 1 of a layer's step: r * h -> RH, u -> U
template <typename IDX>
__device__ __forceinline__ void gru_gates(const float* X, const float* H, float* RH, float* U, const float* Wg, const float* bg, int ldw, int ld,
                                          int ldu, int E, int KQ) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, j = lane & 15;
    const int N = 2 * E, CT = (N + 15) >> 4;
    for (int ct = wave; ct < CT; ct += GRU_WAVES) {
        const dctr::f32x4 acc = gru_gemm<IDX>(X, H, ld, E, KQ, Wg, ldw, N, ct * 16);
        const int col = ct * 16 + j;
        if (col < N) {
            const float b = bg[col];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 4 * g + r;
                const float v = dctr::sigmoidf_(acc[r] + b);
                if (col < E)
                    RH[row * ld + col] = v * H[row * ld + col];
                else
                    U[row * ldu + col - E] = v;
            }
        }
    }
}

// phase 2: the candidate and the cell's update of the rows with t < length, in place over H; the emitted row goes to ``out`` (may be null)
template <typename IDX>
__device__ __forceinline__ void gru_candidate(const float* X, const float* RH, float* H, const float* U, const float* Wc, const float* bc, int ldw,
                                              int ld, int ldu, int E, int KQ, int cell, const float (&a)[4], const int* lens, int t, int nvalid,
                                              float* out, int64_t out_stride) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, j = lane & 15;
    const int CT = (E + 15) >> 4;
    for (int ct = wave; ct < CT; ct += GRU_WAVES) {
        const dctr::f32x4 acc = gru_gemm<IDX>(X, RH, ld, E, KQ, Wc, ldw, E, ct * 16);
        const int col = ct * 16 + j;
        if (col < E) {
            const float b = bc[col];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 4 * g + r;
                const float c = dctr::tanh_fast(acc[r] + b);
                const float h = H[row * ld + col];
                float u = U[row * ldu + col];
                float hn;
                if (cell == DCTR_GRU_CELL_AGRU) {
                    hn = (1.f - a[r]) * h + a[r] * c;
                } else {
                    if (cell == DCTR_GRU_CELL_AUGRU) u = (1.f - a[r]) * u;
                    hn = u * h + (1.f - u) * c;
                }
                const bool live = t < lens[row];
                if (live) H[row * ld + col] = hn;
                if (out && row < nvalid) out[row * out_stride + col] = live ? hn : 0.f;
            }
        }
    }
}

template <bool RESIDENT, bool GLOBAL_TILES>
__global__ __launch_bounds__(GRU_THREADS) void gru_kernel(GruParams p) {
    extern __shared__ __attribute__((aligned(16))) float gru_lds[];
    typedef typename std::conditional<RESIDENT, int, int64_t>::type IDX;
    int* lens = reinterpret_cast<int*>(gru_lds);
    float* tiles = GLOBAL_TILES ? p.ws + (int64_t)blockIdx.x * p.tile_floats : gru_lds + GRU_ROWS;
    const int E = p.E, T = p.T, ld = p.ld, ldu = p.ldu, KQ = p.KQ, L = p.n_layers;
    const int tile = GRU_ROWS * ld;
    // tiles: X[2], then per layer H, RH, U
    float* Xb = tiles;
    float* Lb = tiles + 2 * tile;
    const int layer_floats = 2 * tile + GRU_ROWS * ldu;
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4;
    const int ldwg = RESIDENT ? p.ldwg : 2 * E, ldwc = RESIDENT ? p.ldwc : E;
    const int w_floats = 2 * E * ldwg + 2 * E * ldwc + 3 * E;
    float* wl = gru_lds + GRU_ROWS + p.tile_floats;
    if (RESIDENT) {
        for (int l = 0; l < L; ++l) {
            float* d = wl + l * w_floats;
            for (int e = tid; e < 2 * E * 2 * E; e += GRU_THREADS) d[(e / (2 * E)) * ldwg + e % (2 * E)] = p.W[l][0][e];
            d += 2 * E * ldwg;
            for (int e = tid; e < 2 * E * E; e += GRU_THREADS) d[(e / E) * ldwc + e % E] = p.W[l][2][e];
            d += 2 * E * ldwc;
            for (int e = tid; e < 2 * E; e += GRU_THREADS) d[e] = p.W[l][1][e];
            for (int e = tid; e < E; e += GRU_THREADS) d[2 * E + e] = p.W[l][3][e];
        }
    }
    const int64_t n_tiles = (p.batch + GRU_ROWS - 1) / GRU_ROWS;
    const int n_x = GRU_ROWS * E;
    // the x elements this thread fetches one step ahead: (row, column) fixed for the whole launch
    int xrow[GRU_XREG], xcol[GRU_XREG];
#pragma unroll
    for (int i = 0; i < GRU_XREG; ++i) {
        const int e = tid + i * GRU_THREADS;
        xrow[i] = e < n_x ? e / E : GRU_ROWS;
        xcol[i] = e < n_x ? e % E : 0;
    }

    for (int64_t tl = blockIdx.x; tl < n_tiles; tl += gridDim.x) {
        const int64_t b0 = tl * GRU_ROWS;
        const int nvalid = (int)min((int64_t)GRU_ROWS, p.batch - b0);
        __syncthreads();        // the previous tile is done with lens and the tiles
        if (tid < GRU_ROWS) lens[tid] = tid < nvalid ? min(max(p.len[b0 + tid], 0), T) : 0;
        // h_0 = 0, zeros in the K padding
        for (int e = tid; e < 2 * tile + L * layer_floats; e += GRU_THREADS) tiles[e] = 0.f;
        __syncthreads();
        int t_max = 0;
#pragma unroll
        for (int r = 0; r < GRU_ROWS; ++r) t_max = max(t_max, lens[r]);
        if (t_max > 0) {
            for (int e = tid; e < n_x; e += GRU_THREADS) {
                const int row = e / E, c = e - row * E;
                float v = 0.f;
                if (row < nvalid) {
                    v = p.x[(b0 + row) * p.x_stride + c];
                    if (p.scale_input) v *= p.att[(b0 + row) * p.att_stride];
                }
                Xb[row * ld + c] = v;
            }
        }
        __syncthreads();
        for (int t = 0; t < t_max; ++t) {
            const float* X = Xb + (t & 1) * tile;
            float* Xn = Xb + ((t + 1) & 1) * tile;
            const bool more = t + 1 < t_max;
            // x_{t+1} and this step's scores: issued here, consumed behind the gate GEMM
            float xr[GRU_XREG];
#pragma unroll
            for (int i = 0; i < GRU_XREG; ++i) {
                xr[i] = 0.f;
                if (more && xrow[i] < nvalid) {
                    xr[i] = p.x[(b0 + xrow[i]) * p.x_stride + (int64_t)(t + 1) * p.x_row_stride + xcol[i]];
                    if (p.scale_input) xr[i] *= p.att[(b0 + xrow[i]) * p.att_stride + t + 1];
                }
            }
            float a[4] = {0.f, 0.f, 0.f, 0.f};
            if (p.cell != DCTR_GRU_CELL_GRU) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (4 * g + r < nvalid) a[r] = p.att[(b0 + 4 * g + r) * p.att_stride + t];
            }
#pragma unroll
            for (int l = 0; l < GRU_MAX_LAYERS; ++l) {
                if (l < L) {
                    float* H = Lb + l * layer_floats;
                    float* RH = H + tile;
                    float* U = RH + tile;
                    const float* Xl = l == 0 ? X : Lb;             // layer 2 reads layer 1's state tile after its step t
                    const float* Wg = RESIDENT ? wl + l * w_floats : p.W[l][0];
                    const float* Wc = RESIDENT ? Wg + 2 * E * ldwg : p.W[l][2];
                    const float* bg = RESIDENT ? Wc + 2 * E * ldwc : p.W[l][1];
                    const float* bc = RESIDENT ? bg + 2 * E : p.W[l][3];
                    gru_gates<IDX>(Xl, H, RH, U, Wg, bg, ldwg, ld, ldu, E, KQ);
                    if (l == 0 && more) {
#pragma unroll
                        for (int i = 0; i < GRU_XREG; ++i) {
                            if (xrow[i] < GRU_ROWS) Xn[xrow[i] * ld + xcol[i]] = xr[i];
                        }
                        for (int e = tid + GRU_XREG * GRU_THREADS; e < n_x; e += GRU_THREADS) {
                            const int row = e / E, c = e - row * E;
                            float v = 0.f;
                            if (row < nvalid) {
                                v = p.x[(b0 + row) * p.x_stride + (int64_t)(t + 1) * p.x_row_stride + c];
                                if (p.scale_input) v *= p.att[(b0 + row) * p.att_stride + t + 1];
                            }
                            Xn[row * ld + c] = v;
                        }
                    }
                    __syncthreads();
                    const bool emit = p.return_sequence && l == L - 1;
                    gru_candidate<IDX>(Xl, RH, H, U, Wc, bc, ldwc, ld, ldu, E, KQ, p.cell, a, lens, t, nvalid,
                                       emit ? p.out + b0 * p.out_stride + (int64_t)t * p.out_row_stride : nullptr, p.out_stride);
                    __syncthreads();
                }
            }
        }
        const float* Hl = Lb + (L - 1) * layer_floats;
        if (p.return_sequence) {            // rows past the tile's longest sample
            const int64_t n = (int64_t)(T - t_max) * E;
            for (int64_t e = tid; e < nvalid * n; e += GRU_THREADS) {
                const int row = (int)(e / n);
                const int64_t rem = e - row * n;
                const int t = t_max + (int)(rem / E), c = (int)(rem % E);
                p.out[(b0 + row) * p.out_stride + (int64_t)t * p.out_row_stride + c] = 0.f;
            }
        } else {
            for (int e = tid; e < nvalid * E; e += GRU_THREADS) {
                const int row = e / E, c = e - row * E;
                p.out[(b0 + row) * p.out_stride + c] = Hl[row * ld + c];
            }
        }
    }
}

struct GruPlan {
    bool resident, global_tiles;
    int ld, ldu, KQ, ldwg, ldwc;
    int64_t tile_floats;
    size_t lds_bytes;
    int grid_max;
    size_t ws_bytes;
};

void gru_plan(const dctr_gru_args_t* a, GruPlan* pl) {
    const int E = a->dim, L = a->n_layers;
    pl->ld = ((E + 15) & ~15) + 4;
    pl->ldu = E | 1;
    pl->KQ = ((E + 15) & ~15) >> 2;
    pl->ldwg = gru_pitch(2 * E, pl->KQ);
    pl->ldwc = gru_pitch(E, pl->KQ);
    const int64_t tile = (int64_t)GRU_ROWS * pl->ld;
    pl->tile_floats = (2 * tile + L * (2 * tile + (int64_t)GRU_ROWS * pl->ldu) + 3) & ~(int64_t)3;
    const int64_t w_floats = (int64_t)L * (2 * (int64_t)E * pl->ldwg + 2 * (int64_t)E * pl->ldwc + 3 * (int64_t)E);
    const size_t tiles_bytes = (size_t)(GRU_ROWS + pl->tile_floats) * 4;
    const size_t res_bytes = tiles_bytes + (size_t)w_floats * 4;
    const bool res_fits = res_bytes <= DCTR_LDS_MAX;
    pl->resident = res_fits && a->route != DCTR_GRU_ROUTE_STREAMED;
    pl->global_tiles = !pl->resident && tiles_bytes > DCTR_LDS_MAX;
    pl->lds_bytes = pl->resident ? res_bytes : pl->global_tiles ? (size_t)GRU_ROWS * 4 : tiles_bytes;
    pl->grid_max = GRU_GRID_MAX;
    pl->ws_bytes = 0;
    if (pl->global_tiles) {
        const dctr_tile_route r = dctr_workspace_slices((size_t)pl->tile_floats * 4);
        pl->grid_max = r.grid_max;
        pl->ws_bytes = r.route_bytes;
    }
}

bool gru_resident_fits(const dctr_gru_args_t* a) {
    dctr_gru_args_t b = *a;
    b.route = DCTR_GRU_ROUTE_AUTO;
    GruPlan pl;
    gru_plan(&b, &pl);
    return pl.resident;
}

int gru_check(const dctr_gru_args_t* a) {
    DCTR_REQUIRE(a, DCTR_E_NULL, "gru_fwd: null args");
    DCTR_REQUIRE(a->batch >= 0 && a->seq_len >= 1 && a->dim >= 1, DCTR_E_DIM, "gru_fwd: bad sizes");
    DCTR_REQUIRE(a->n_layers >= 1 && a->n_layers <= GRU_MAX_LAYERS, DCTR_E_DIM, "gru_fwd: n_layers must be 1 or 2, got %d", a->n_layers);
    // a tile's buffers are indexed in 32 bits
    DCTR_REQUIRE(a->dim <= (1 << 20), DCTR_E_DIM, "gru_fwd: dim %d exceeds 2^20", a->dim);
    DCTR_REQUIRE(a->cell >= DCTR_GRU_CELL_GRU && a->cell <= DCTR_GRU_CELL_AUGRU, DCTR_E_ENUM, "gru_fwd: unknown cell %d", a->cell);
    DCTR_REQUIRE(a->n_layers == 1 || a->cell == DCTR_GRU_CELL_GRU, DCTR_E_ENUM, "gru_fwd: two layers take the plain GRU cell only");
    DCTR_REQUIRE((uint32_t)(a->scale_input | a->return_sequence) <= 1u, DCTR_E_ENUM, "gru_fwd: scale_input and return_sequence must be 0 or 1");
    DCTR_REQUIRE(a->route >= DCTR_GRU_ROUTE_AUTO && a->route <= DCTR_GRU_ROUTE_STREAMED, DCTR_E_ENUM, "gru_fwd: unknown route %d", a->route);
    DCTR_REQUIRE(a->x_row_stride >= a->dim && a->x_stride >= ((int64_t)a->seq_len - 1) * a->x_row_stride + a->dim, DCTR_E_DIM,
                 "gru_fwd: x strides smaller than the [seq_len, dim] block");
    if (a->return_sequence)
        DCTR_REQUIRE(a->out_row_stride >= a->dim && a->out_stride >= ((int64_t)a->seq_len - 1) * a->out_row_stride + a->dim, DCTR_E_DIM,
                     "gru_fwd: out strides smaller than the [seq_len, dim] block");
    else
        DCTR_REQUIRE(a->out_stride >= a->dim, DCTR_E_DIM, "gru_fwd: out_stride < dim");
    if (a->cell != DCTR_GRU_CELL_GRU || a->scale_input)
        DCTR_REQUIRE(a->att_stride >= a->seq_len, DCTR_E_DIM, "gru_fwd: att_stride < seq_len");
    DCTR_REQUIRE(a->route != DCTR_GRU_ROUTE_RESIDENT || gru_resident_fits(a), DCTR_E_UNSUPPORTED,
                 "gru_fwd: the weights of %d layer(s) of dim %d do not fit the resident route's LDS", a->n_layers, a->dim);
    return DCTR_OK;
}

}  // namespace

extern "C" size_t dctr_gru_workspace_bytes(const dctr_gru_args_t* args) {
    if (gru_check(args) != DCTR_OK) return 0;
    GruPlan pl;
    gru_plan(args, &pl);
    return pl.ws_bytes;
}

extern "C" int dctr_gru_route(const dctr_gru_args_t* args) {
    int rc = gru_check(args);
    if (rc != DCTR_OK) return rc;
    GruPlan pl;
    gru_plan(args, &pl);
    return pl.resident ? DCTR_GRU_ROUTE_RESIDENT : DCTR_GRU_ROUTE_STREAMED;
}

extern "C" int dctr_gru_fwd(const dctr_gru_args_t* a, void* stream) {
    int rc = gru_check(a);
    if (rc != DCTR_OK) return rc;
    DCTR_REQUIRE(a->x && a->lengths && a->layers && a->out, DCTR_E_NULL, "gru_fwd: null x / lengths / layers / out");
    DCTR_REQUIRE(!(a->cell != DCTR_GRU_CELL_GRU || a->scale_input) || a->att_scores, DCTR_E_NULL,
                 "gru_fwd: the attention-gated cells and scale_input need att_scores");
    for (int l = 0; l < a->n_layers; ++l)
        for (int m = 0; m < GRU_NW; ++m)
            DCTR_REQUIRE(a->layers[GRU_NW * l + m], DCTR_E_NULL, "gru_fwd: layer %d: null gate / candidate kernel or bias", l);
    GruPlan pl;
    gru_plan(a, &pl);
    if (pl.ws_bytes) DCTR_REQUIRE_WORKSPACE("gru_fwd", "dctr_gru_workspace_bytes", a->workspace, a->workspace_bytes, pl.ws_bytes);
    if (a->batch == 0) return DCTR_OK;
    GruParams p = {};
    p.x = a->x;
    p.batch = a->batch;
    p.x_stride = a->x_stride;
    p.x_row_stride = a->x_row_stride;
    p.len = a->lengths;
    p.att = a->att_scores;
    p.att_stride = a->att_stride;
    p.T = a->seq_len;
    p.E = a->dim;
    p.n_layers = a->n_layers;
    p.cell = a->cell;
    p.scale_input = a->scale_input;
    p.return_sequence = a->return_sequence;
    p.ld = pl.ld;
    p.ldu = pl.ldu;
    p.KQ = pl.KQ;
    p.ldwg = pl.ldwg;
    p.ldwc = pl.ldwc;
    p.tile_floats = pl.tile_floats;
    for (int l = 0; l < a->n_layers; ++l)
        for (int m = 0; m < GRU_NW; ++m) p.W[l][m] = a->layers[GRU_NW * l + m];
    p.out = a->out;
    p.out_stride = a->out_stride;
    p.out_row_stride = a->out_row_stride;
    p.ws = pl.global_tiles ? (float*)a->workspace : nullptr;
    const int64_t n_tiles = dctr_ceil_div(a->batch, GRU_ROWS);
    const unsigned grid = (unsigned)(n_tiles < pl.grid_max ? n_tiles : pl.grid_max);
    if (pl.resident) {
        static thread_local size_t granted[DCTR_MAX_DEVICES] = {0};
        hipError_t e = dctr_grant_lds((const void*)gru_kernel<true, false>, pl.lds_bytes, granted);
        DCTR_REQUIRE(e == hipSuccess, (int)e, "gru_fwd: cannot raise dynamic LDS: %s", hipGetErrorString(e));
        DCTR_LAUNCH((gru_kernel<true, false>), dim3(grid), dim3(GRU_THREADS), pl.lds_bytes, (hipStream_t)stream, p);
    } else if (!pl.global_tiles) {
        static thread_local size_t granted[DCTR_MAX_DEVICES] = {0};
        hipError_t e = dctr_grant_lds((const void*)gru_kernel<false, false>, pl.lds_bytes, granted);
        DCTR_REQUIRE(e == hipSuccess, (int)e, "gru_fwd: cannot raise dynamic LDS: %s", hipGetErrorString(e));
        DCTR_LAUNCH((gru_kernel<false, false>), dim3(grid), dim3(GRU_THREADS), pl.lds_bytes, (hipStream_t)stream, p);
    } else {
        DCTR_LAUNCH((gru_kernel<false, true>), dim3(grid), dim3(GRU_THREADS), pl.lds_bytes, (hipStream_t)stream, p);
    }
    return dctr_launch_status("dctr_gru_fwd");
}
