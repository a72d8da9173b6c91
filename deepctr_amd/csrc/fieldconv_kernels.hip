// The convolution along the field axis of the [B, F, E] embedding block that CCPM (reference deepctr/models/ccpm.py:62-70) and
// FGCNNLayer (deepctr/layers/interaction.py:937-1064) share, with the pooling that follows it, and KMaxPooling
// (deepctr/layers/sequence.py:818-874) on its own.
//
// Reference, per stage: Conv2D(filters, (w, 1), padding='same', activation='tanh', use_bias=True) over [B, rows, E, C_in], then
// KMaxPooling(k, axis=1) (tf.nn.top_k(sorted=True): the k largest in DESCENDING order of value) or MaxPooling2D((p, 1)) ('valid',
// stride p: rows // p output rows).  keras runs a pad, a conv, a tanh and a pool per stage, each a round trip through HBM.
//   y[b, r, e, co] = tanh(bias[co] + sum_{d, ci} xpad[b, r + d, e, ci] K[d, ci, co]),  (w - 1) / 2 zero rows before the first field
// (a cross-correlation: K is not flipped).
//
// Here one launch runs the whole stack.  The embedding columns e of a sample never meet in it, so the unit of work is a COLUMN
// (b, e): a workgroup owns 16 G of them and keeps two maps per column on chip,
//   A [column][(rows + w - 1) C_in]   the stage's input with its 'same' padding rows, channel-last: the w x C_in window of output
//                                     row r is the CONTIGUOUS run of K = w C_in floats from r C_in
//   B [column][rows C_out]            the stage's convolution, before its pooling.
// A conv item is (16 columns, row r, 16 output channels): M = the 16 columns at field position r, K over (d, ci), N a slice of
// C_out, on v_mfma_f32_16x16x4_f32 (exact fp32 products), the accumulators starting at the bias; k-slot g of MFMA s takes
// k = 4 s + g.  The items of a stage go round the four waves.  The column pitches are 2 (A) and 4 (B) mod 32 floats, which puts the
// 32 lanes of a half-wave ds_read_b32 / ds_write_b32 on 32 banks, and a kernel's row pitch in LDS is 16 mod 32 for the same reason.
// The pooling reads B and writes the next stage's A (its padding rows are zeroed beside it), the requested per-stage outputs and,
// after the last stage, the output, all channel-last [rows, E, C] = what Flatten sees.  k-max is rank counting: element i goes to
// position #{j : v_j > v_i} + #{j < i : v_j = v_i} when that is < k, so the result is the sorted multiset, bit for bit, with no
// exchange between lanes.
// RESIDENT route: every stage's kernel and bias stay in LDS for the workgroup's life; AUTO takes it while maps and kernels fit
// 64 KiB (two workgroups per CU), a forced RESIDENT holds up to 160 KiB.  STREAMED: the same step code with the B operands read from
// global / L2.  WORKSPACE: streamed, with the maps in a per-workgroup slice of a workspace (taken when even 16 columns' maps exceed
// the LDS).  Nothing is refused for its size.
//
// Cost model per sample: E x sum_stages rows w C_in C_out MACs.
#include <math.h>
#include "dctr_common.h"
#include "tile_route.h"
#include "mfma_tile.h"

namespace {

constexpr int FC_THREADS = 256;
constexpr int FC_WAVES = FC_THREADS / 64;
constexpr int FC_MAX = DCTR_FIELDCONV_MAX_STAGES;
constexpr size_t FC_LDS_TARGET = 64 * 1024;     // two workgroups per CU while the shapes allow
constexpr int FC_GRID_MAX = 2048;
constexpr int64_t FC_DIM_MAX = 1 << 20;
constexpr int64_t FC_COL_MAX = (int64_t)1 << 26;        // floats of one column's maps: 32-bit offsets inside a tile

struct FcStage {
    int32_t w, cin, cout, pool, parg, rin, rout, K, K4, ldw, woff, pb;
    const float* kern;
    const float* bias;
    float* sout;
    int64_t sout_stride;
};

struct FcParams {
    const float* x;
    int64_t x_stride, x_offset, n_cols;
    int32_t F, E, C0, L, G, lda, ldb;
    int64_t tile_floats;
    FcStage st[FC_MAX];
    float* out;
    int64_t out_stride, out_offset;
    float* ws;
};

template <bool RESIDENT, bool GLOBAL_TILES>
__global__ __launch_bounds__(FC_THREADS) void fieldconv_kernel(FcParams p) {
    extern __shared__ __attribute__((aligned(16))) float fc_lds[];
    float* tiles = GLOBAL_TILES ? p.ws + (int64_t)blockIdx.x * p.tile_floats : fc_lds;
    float* wl = fc_lds + p.tile_floats;             // RESIDENT only
    const int cols = 16 * p.G, lda = p.lda, ldb = p.ldb, E = p.E, L = p.L;
    float* A = tiles;
    float* Bm = tiles + cols * lda;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, j = lane & 15;

    if (RESIDENT) {     // rows >= K and columns >= C_out of a kernel's image are zero
        for (int s = 0; s < L; ++s) {
            const FcStage& st = p.st[s];
            float* dst = wl + st.woff;
            const int n = st.K4 * st.ldw, cpad = (st.cout + 15) & ~15;
            for (int e = tid; e < n; e += FC_THREADS) {
                const int k = e / st.ldw, c = e - k * st.ldw;
                dst[e] = (k < st.K && c < st.cout) ? st.kern[k * st.cout + c] : 0.f;
            }
            for (int e = tid; e < cpad; e += FC_THREADS) dst[n + e] = e < st.cout ? st.bias[e] : 0.f;
        }
    }
    const int64_t n_tiles = (p.n_cols + cols - 1) / cols;
    for (int64_t tl = blockIdx.x; tl < n_tiles; tl += gridDim.x) {
        const int64_t q0 = tl * cols;
        const int64_t b0 = q0 / E;
        const int e0 = (int)(q0 - b0 * E);
        const int nvalid = (int)min((int64_t)cols, p.n_cols - q0);
        __syncthreads();            // the kernels' images; the previous tile's pooling is done with the maps
        {   // stage 0's input with its padding rows (and the 3 floats the last k-slots of a window may touch)
            const FcStage& st = p.st[0];
            const int C0 = p.C0, data = (p.F + st.w - 1) * C0, ext = data + 3;
            for (int e = tid; e < cols * ext; e += FC_THREADS) {
                const int pos = e / cols, col = e - pos * cols;
                float v = 0.f;
                if (pos < data && col < nvalid) {
                    const int prow = pos / C0, c = pos - prow * C0, row = prow - st.pb;
                    if (row >= 0 && row < p.F) {
                        const int t = e0 + col, bb = t / E, ee = t - bb * E;
                        v = p.x[(b0 + bb) * p.x_stride + p.x_offset + ((int64_t)row * E + ee) * C0 + c];
                    }
                }
                A[col * lda + pos] = v;
            }
        }
        __syncthreads();
        for (int s = 0; s < L; ++s) {
            const FcStage& st = p.st[s];
            const int cin = st.cin, cout = st.cout, rin = st.rin, rout = st.rout, K = st.K;
            const int NT = (cout + 15) >> 4, items = p.G * rin * NT, ksteps = st.K4 >> 2;
            const float* Wl = wl + st.woff;
            for (int item = wave; item < items; item += FC_WAVES) {
                const int nt = item % NT, rest = item / NT;
                const int r = rest % rin, grp = rest / rin;
                const int co = nt * 16 + j, coc = min(co, cout - 1);
                const float* arow = A + (grp * 16 + j) * lda + r * cin;
                const float bv = RESIDENT ? Wl[st.K4 * st.ldw + co] : st.bias[coc];
                dctr::f32x4 acc = {bv, bv, bv, bv};
                for (int ks = 0; ks < ksteps; ++ks) {
                    const int k = 4 * ks + g;
                    const float av = arow[k];           // (in bounds: the 3 floats behind a column's padded map)
                    const float a = k < K ? av : 0.f;
                    // (k >= K: the resident image holds zeros there; the streamed load is clamped, so its value is dropped too)
                    const float bw = RESIDENT ? Wl[k * st.ldw + co] : st.kern[(int64_t)min(k, K - 1) * cout + coc];
                    const float b = (RESIDENT || k < K) ? bw : 0.f;
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
                }
                if (co < cout) {
#pragma unroll
                    for (int r4 = 0; r4 < 4; ++r4)
                        Bm[(grp * 16 + 4 * g + r4) * ldb + r * cout + co] = dctr::tanh_fast(acc[r4]);
                }
            }
            __syncthreads();
            const bool last = s == L - 1;
            const int pbn = last ? 0 : p.st[s + 1].pb;
            const int extn = last ? 0 : (rout + p.st[s + 1].w - 1) * cout + 3;
            if (!last) {        // the next stage's padding rows
                const int npad = extn - rout * cout, head = pbn * cout;
                for (int e = tid; e < cols * npad; e += FC_THREADS) {
                    const int z = e / cols, col = e - z * cols;
                    A[col * lda + (z < head ? z : z + rout * cout)] = 0.f;
                }
            }
            const int nsrc = st.pool == DCTR_FIELDCONV_POOL_KMAX ? rin : rout;
            for (int e = tid; e < cols * nsrc * cout; e += FC_THREADS) {
                const int c = e % cout, t = e / cout;
                const int i = t % nsrc, col = t / nsrc;
                const float* src = Bm + col * ldb + c;
                float v;
                int ro;
                if (st.pool == DCTR_FIELDCONV_POOL_KMAX) {
                    v = src[i * cout];
                    int rank = 0;
                    for (int jj = 0; jj < rin; ++jj) {
                        const float u = src[jj * cout];
                        rank += (u > v || (u == v && jj < i)) ? 1 : 0;
                    }
                    if (rank >= st.parg) continue;
                    ro = rank;
                } else {
                    v = src[i * st.parg * cout];
                    for (int d = 1; d < st.parg; ++d) v = fmaxf(v, src[(i * st.parg + d) * cout]);
                    ro = i;
                }
                if (!last) A[col * lda + (pbn + ro) * cout + c] = v;
                if (col < nvalid) {
                    const int tt = e0 + col, bb = tt / E, ee = tt - bb * E;
                    const int64_t o = ((int64_t)ro * E + ee) * cout + c;
                    if (st.sout) st.sout[(b0 + bb) * st.sout_stride + o] = v;
                    if (last) p.out[(b0 + bb) * p.out_stride + p.out_offset + o] = v;
                }
            }
            __syncthreads();
        }
    }
}

struct FcPlan {
    bool resident, global_tiles;
    int G, lda, ldb, L;
    int rin[FC_MAX], rout[FC_MAX], cin[FC_MAX], ldw[FC_MAX], woff[FC_MAX], K4[FC_MAX];
    int64_t tile_floats, w_floats;
    size_t lds_bytes, ws_bytes;
    int grid_max;
};

int fc_pitch(int64_t n, int rem) {        // >= n and = rem (mod 32)
    return (int)(n + ((rem - n) % 32 + 32) % 32);
}

int fc_check(const dctr_fieldconv_args_t* a) {
    DCTR_REQUIRE(a, DCTR_E_NULL, "fieldconv_fwd: null args");
    DCTR_REQUIRE(a->batch >= 0 && a->fields >= 1 && a->dim >= 1 && a->in_channels >= 1, DCTR_E_DIM, "fieldconv_fwd: bad sizes");
    DCTR_REQUIRE(a->fields <= FC_DIM_MAX && a->dim <= FC_DIM_MAX && a->in_channels <= FC_DIM_MAX, DCTR_E_DIM,
                 "fieldconv_fwd: fields / dim / in_channels exceed 2^20");
    DCTR_REQUIRE(a->n_stages >= 1 && a->n_stages <= FC_MAX, DCTR_E_DIM, "fieldconv_fwd: n_stages must be 1..%d, got %d", FC_MAX, a->n_stages);
    DCTR_REQUIRE(a->widths && a->channels && a->pool_kinds && a->pool_args, DCTR_E_NULL, "fieldconv_fwd: null widths / channels / pool_kinds / pool_args");
    DCTR_REQUIRE(a->route >= DCTR_FIELDCONV_ROUTE_AUTO && a->route <= DCTR_FIELDCONV_ROUTE_WORKSPACE, DCTR_E_ENUM, "fieldconv_fwd: unknown route %d",
                 a->route);
    int64_t rows = a->fields, cin = a->in_channels;
    for (int s = 0; s < a->n_stages; ++s) {
        const int64_t w = a->widths[s], c = a->channels[s], arg = a->pool_args[s];
        DCTR_REQUIRE(w >= 1 && c >= 1 && w <= FC_DIM_MAX && c <= FC_DIM_MAX, DCTR_E_DIM, "fieldconv_fwd: stage %d: width %lld / channels %lld outside 1..2^20",
                     s, (long long)w, (long long)c);
        DCTR_REQUIRE(a->pool_kinds[s] == DCTR_FIELDCONV_POOL_KMAX || a->pool_kinds[s] == DCTR_FIELDCONV_POOL_MAX, DCTR_E_ENUM,
                     "fieldconv_fwd: stage %d: unknown pooling %d", s, a->pool_kinds[s]);
        DCTR_REQUIRE(arg >= 1 && arg <= rows, DCTR_E_DIM, "fieldconv_fwd: stage %d: k / pooling width %lld outside 1..%lld rows", s, (long long)arg,
                     (long long)rows);
        DCTR_REQUIRE((rows + w - 1) * cin + 3 + rows * c + 64 <= FC_COL_MAX, DCTR_E_DIM, "fieldconv_fwd: stage %d: a column's maps exceed 2^26 floats", s);
        DCTR_REQUIRE(w * cin <= ((int64_t)1 << 30) / 4 && w * cin * ((c + 31) / 16 * 16 + 16) <= ((int64_t)1 << 30), DCTR_E_DIM,
                     "fieldconv_fwd: stage %d: kernel of %lld x %lld x %lld too large", s, (long long)w, (long long)cin, (long long)c);
        rows = a->pool_kinds[s] == DCTR_FIELDCONV_POOL_KMAX ? arg : rows / arg;
        cin = c;
    }
    const int64_t in_w = (int64_t)a->fields * a->dim * a->in_channels, out_w = rows * a->dim * cin;
    DCTR_REQUIRE(a->x_offset >= 0 && a->x_stride >= a->x_offset + in_w, DCTR_E_DIM, "fieldconv_fwd: x_stride smaller than x_offset + the %lld inputs of a sample",
                 (long long)in_w);
    DCTR_REQUIRE(a->out_offset >= 0 && a->out_stride >= a->out_offset + out_w, DCTR_E_DIM,
                 "fieldconv_fwd: out_stride smaller than out_offset + the %lld outputs of a sample", (long long)out_w);
    return DCTR_OK;
}

void fc_plan(const dctr_fieldconv_args_t* a, FcPlan* pl) {
    const int L = a->n_stages;
    pl->L = L;
    int64_t rows = a->fields, cin = a->in_channels, ea = 0, eb = 0, wf = 0;
    for (int s = 0; s < L; ++s) {
        const int64_t w = a->widths[s], c = a->channels[s], K = w * cin, K4 = (K + 3) & ~(int64_t)3, cpad = (c + 15) & ~(int64_t)15;
        pl->rin[s] = (int)rows;
        pl->cin[s] = (int)cin;
        pl->K4[s] = (int)K4;
        pl->ldw[s] = fc_pitch(cpad, 16);
        pl->woff[s] = (int)wf;
        wf += K4 * pl->ldw[s] + cpad;
        const int64_t xa = (rows + w - 1) * cin + 3, xb = rows * c;
        ea = xa > ea ? xa : ea;
        eb = xb > eb ? xb : eb;
        rows = a->pool_kinds[s] == DCTR_FIELDCONV_POOL_KMAX ? a->pool_args[s] : rows / a->pool_args[s];
        pl->rout[s] = (int)rows;
        cin = c;
    }
    pl->lda = fc_pitch(ea, 2);
    pl->ldb = fc_pitch(eb, 4);
    pl->w_floats = wf;
    const size_t col_bytes = (size_t)(pl->lda + pl->ldb) * 4, w_bytes = (size_t)wf * 4;
    const bool may_res = a->route == DCTR_FIELDCONV_ROUTE_AUTO || a->route == DCTR_FIELDCONV_ROUTE_RESIDENT;
    // AUTO keeps the kernels in LDS only while that costs no occupancy (maps and kernels within the two-workgroup budget): past it
    // a CU holds one resident workgroup, one wave per SIMD, against two or three streamed ones (the measured times: DESIGN.md 4.19)
    const size_t res_bytes = 16 * col_bytes + w_bytes;
    pl->resident = may_res && res_bytes <= (a->route == DCTR_FIELDCONV_ROUTE_RESIDENT ? DCTR_LDS_MAX : FC_LDS_TARGET);
    pl->global_tiles = !pl->resident && (16 * col_bytes > DCTR_LDS_MAX || a->route == DCTR_FIELDCONV_ROUTE_WORKSPACE);
    const size_t fixed = pl->resident ? w_bytes : 0;
    pl->G = 1;
    if (!pl->global_tiles)
        for (int G = 4; G > 1; G >>= 1)
            if (16 * G * col_bytes + fixed <= FC_LDS_TARGET) {
                pl->G = G;
                break;
            }
    pl->tile_floats = (int64_t)16 * pl->G * (pl->lda + pl->ldb);
    const size_t tiles_bytes = (size_t)pl->tile_floats * 4;
    pl->lds_bytes = pl->global_tiles ? 0 : tiles_bytes + fixed;
    pl->grid_max = FC_GRID_MAX;
    pl->ws_bytes = 0;
    if (pl->global_tiles) {
        const dctr_tile_route r = dctr_workspace_slices(tiles_bytes);
        pl->grid_max = r.grid_max;
        pl->ws_bytes = r.route_bytes;
    }
}

int fc_check_route(const dctr_fieldconv_args_t* a) {
    int rc = fc_check(a);
    if (rc != DCTR_OK) return rc;
    if (a->route == DCTR_FIELDCONV_ROUTE_RESIDENT) {
        FcPlan pl;
        fc_plan(a, &pl);
        DCTR_REQUIRE(pl.resident, DCTR_E_UNSUPPORTED, "fieldconv_fwd: 16 columns' maps and the %d stages' kernels do not fit the resident route's LDS",
                     a->n_stages);
    }
    return DCTR_OK;
}

__global__ void kmax_pool_kernel(const float* x, int64_t total, int32_t n, int64_t inner, int32_t k, float* y) {
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t in = idx % inner, t = idx / inner;
        const int i = (int)(t % n);
        const int64_t o = t / n;
        const float* src = x + o * n * inner + in;
        const float v = src[i * inner];
        int rank = 0;
        for (int jj = 0; jj < n; ++jj) {
            const float u = src[jj * inner];
            rank += (u > v || (u == v && jj < i)) ? 1 : 0;
        }
        if (rank < k) y[(o * k + rank) * inner + in] = v;
    }
}

}  // namespace

extern "C" size_t dctr_fieldconv_workspace_bytes(const dctr_fieldconv_args_t* args) {
    if (fc_check_route(args) != DCTR_OK) return 0;
    FcPlan pl;
    fc_plan(args, &pl);
    return pl.ws_bytes;
}

extern "C" int dctr_fieldconv_route(const dctr_fieldconv_args_t* args) {
    int rc = fc_check_route(args);
    if (rc != DCTR_OK) return rc;
    FcPlan pl;
    fc_plan(args, &pl);
    return pl.resident ? DCTR_FIELDCONV_ROUTE_RESIDENT : DCTR_FIELDCONV_ROUTE_STREAMED;
}

extern "C" int dctr_fieldconv_fwd(const dctr_fieldconv_args_t* a, void* stream) {
    int rc = fc_check_route(a);
    if (rc != DCTR_OK) return rc;
    DCTR_REQUIRE(a->x && a->kernels && a->biases && a->out, DCTR_E_NULL, "fieldconv_fwd: null x / kernels / biases / out");
    for (int s = 0; s < a->n_stages; ++s)
        DCTR_REQUIRE(a->kernels[s] && a->biases[s], DCTR_E_NULL, "fieldconv_fwd: stage %d: null kernel / bias", s);
    FcPlan pl;
    fc_plan(a, &pl);
    for (int s = 0; s < a->n_stages && a->stage_outs; ++s)
        if (a->stage_outs[s])
            DCTR_REQUIRE(a->stage_out_strides && a->stage_out_strides[s] >= (int64_t)pl.rout[s] * a->dim * a->channels[s], DCTR_E_DIM,
                         "fieldconv_fwd: stage %d: stage_out stride smaller than its [%d, %d, %d] map", s, pl.rout[s], a->dim, a->channels[s]);
    if (pl.ws_bytes)
        DCTR_REQUIRE_WORKSPACE("fieldconv_fwd", "dctr_fieldconv_workspace_bytes", a->workspace, a->workspace_bytes, pl.ws_bytes);
    if (a->batch == 0) return DCTR_OK;
    FcParams p = {};
    p.x = a->x;
    p.x_stride = a->x_stride;
    p.x_offset = a->x_offset;
    p.n_cols = a->batch * a->dim;
    p.F = a->fields;
    p.E = a->dim;
    p.C0 = a->in_channels;
    p.L = a->n_stages;
    p.G = pl.G;
    p.lda = pl.lda;
    p.ldb = pl.ldb;
    p.tile_floats = pl.tile_floats;
    for (int s = 0; s < a->n_stages; ++s) {
        FcStage& st = p.st[s];
        st.w = a->widths[s];
        st.cin = pl.cin[s];
        st.cout = a->channels[s];
        st.pool = a->pool_kinds[s];
        st.parg = a->pool_args[s];
        st.rin = pl.rin[s];
        st.rout = pl.rout[s];
        st.K = st.w * st.cin;
        st.K4 = pl.K4[s];
        st.ldw = pl.ldw[s];
        st.woff = pl.woff[s];
        st.pb = (st.w - 1) / 2;
        st.kern = a->kernels[s];
        st.bias = a->biases[s];
        st.sout = a->stage_outs ? a->stage_outs[s] : nullptr;
        st.sout_stride = st.sout ? a->stage_out_strides[s] : 0;
    }
    p.out = a->out;
    p.out_stride = a->out_stride;
    p.out_offset = a->out_offset;
    p.ws = pl.global_tiles ? (float*)a->workspace : nullptr;
    const int64_t n_tiles = dctr_ceil_div(p.n_cols, 16 * pl.G);
    unsigned grid = (unsigned)(n_tiles < pl.grid_max ? n_tiles : pl.grid_max);
    if (pl.resident) {
        // a workgroup copies every stage's kernel into LDS once and then walks its tiles: no more workgroups than the CUs hold at a time
        const int64_t held = (int64_t)dctr_n_cus() * (int64_t)(DCTR_LDS_MAX / pl.lds_bytes);
        if (grid > held) grid = (unsigned)held;
        static thread_local size_t granted[DCTR_MAX_DEVICES] = {0};
        hipError_t e = dctr_grant_lds((const void*)fieldconv_kernel<true, false>, pl.lds_bytes, granted);
        DCTR_REQUIRE(e == hipSuccess, (int)e, "fieldconv_fwd: cannot raise dynamic LDS: %s", hipGetErrorString(e));
        DCTR_LAUNCH((fieldconv_kernel<true, false>), dim3(grid), dim3(FC_THREADS), pl.lds_bytes, (hipStream_t)stream, p);
    } else if (!pl.global_tiles) {
        static thread_local size_t granted[DCTR_MAX_DEVICES] = {0};
        hipError_t e = dctr_grant_lds((const void*)fieldconv_kernel<false, false>, pl.lds_bytes, granted);
        DCTR_REQUIRE(e == hipSuccess, (int)e, "fieldconv_fwd: cannot raise dynamic LDS: %s", hipGetErrorString(e));
        DCTR_LAUNCH((fieldconv_kernel<false, false>), dim3(grid), dim3(FC_THREADS), pl.lds_bytes, (hipStream_t)stream, p);
    } else {
        DCTR_LAUNCH((fieldconv_kernel<false, true>), dim3(grid), dim3(FC_THREADS), 0, (hipStream_t)stream, p);
    }
    return dctr_launch_status("dctr_fieldconv_fwd");
}

extern "C" int dctr_kmax_pool_fwd(const float* x, int64_t outer, int32_t n, int64_t inner, int32_t k, float* y, void* stream) {
    DCTR_REQUIRE(outer >= 0 && n >= 1 && inner >= 0, DCTR_E_DIM, "kmax_pool_fwd: bad sizes");
    DCTR_REQUIRE(k >= 1 && k <= n, DCTR_E_DIM, "kmax_pool_fwd: k must be 1..%d, got %d", n, k);
    if (outer == 0 || inner == 0) return DCTR_OK;
    DCTR_REQUIRE(x && y, DCTR_E_NULL, "kmax_pool_fwd: null x / y");
    const int64_t total = outer * n * inner, blocks = dctr_ceil_div(total, 256);
    DCTR_LAUNCH(kmax_pool_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, (hipStream_t)stream, x, total, n, inner, k, y);
    return dctr_launch_status("dctr_kmax_pool_fwd");
}
