// Backward of the input-aware FM (include/dctr.h: dctr_ifm_bwd), from the forward's saved m and d_out to dx, dterms, dm' (dmprime),
// dact_s = dm' kernel_s^T and dkernel_s = act_s^T dm'.  Three kinds of launch on the caller's stream:
//
//   row pass     one wave per sample, the forward epilogue's lane mapping: the 64 lanes split into G = 64 / dp groups of dp = pow2(d)
//                lanes, group g walks the fields g, g + G, ... with a lane per embedding column.  Walk 1 forms S[c] (the groups meet in
//                xor-shuffles), walk 2 writes dx and reduces dm[f] over the group's lanes (over the column blocks too when d > 64) into
//                the wave's LDS row of F floats; then a lane per field: dterms, one wave sum of m[h] dm[h] for the softmax, dm'.
//   dact pass    a wave owns 16 samples: dact[16, K] = dm'[16, F] . kernel^T on v_mfma_f32_16x16x4_f32; the dm' tile goes through LDS in
//                chunks of 64 columns at the forward's pitch of 68, kernel^T comes straight from L2 (lane j reads row n0 + 16 c + j of
//                the [K, F] kernel at four consecutive f: the whole kernel is a few hundred KiB, every wave of the grid reads the same
//                bytes, and staging it would put a second barrier pair into every 64-column pass for a tile read once); 64 output
//                columns (four accumulator tiles) per pass.
//   dkernel pass workgroup (kb, s): the [64, F] block kb of act^T . dm' over batch slice s, the batch as the MFMA's k dimension, a wave
//                per 16 kernel rows, F walked in blocks of at most 256 columns (16 accumulator tiles in registers); the block goes to
//                partials[s]; a last launch adds the S partials of every element in the order s = 0 .. S-1.  No atomics.
#include "ifm_device.h"

namespace {

using namespace dctr_ifm;

constexpr int IFM_BWD_FB = 256;                   // dkernel: columns of F per pass (16 accumulator tiles)
constexpr int IFM_BWD_WGS = 2 * 256;              // dkernel, slices = 0: about two workgroups per CU of a 256-CU part

struct IfmBwdRow {
    int64_t batch;
    int32_t F, d, dp, softmax;
    const float* x;
    int64_t x_stride;
    const float* m;
    int64_t m_stride;
    const float* t;
    int64_t t_stride;
    const float* g;
    float* dx;
    int64_t dx_stride;
    float* dt;
    int64_t dt_stride;
    float* dmp;                      // dm' [B, dmp_stride]: dmprime or the workspace region; NULL: not formed
    int64_t dmp_stride;
};

// one sample by one wave; every wave of the workgroup runs the same trip counts (the barriers are workgroup-wide), a wave past the
// batch loads zeros and stores nothing
__global__ void __launch_bounds__(IFM_THREADS) ifm_bwd_row_kernel(IfmBwdRow p) {
    extern __shared__ __align__(16) float ifm_bwd_smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    const int64_t b = (int64_t)blockIdx.x * n_waves + wave;
    const bool live = b < p.batch;
    const int64_t bb = live ? b : 0;
    const int F = p.F, d = p.d, dp = p.dp;
    float* dm_row = ifm_bwd_smem + (size_t)wave * F;
    const int G = 64 / dp, grp = lane / dp, c = lane - grp * dp;
    const float* xr = p.x + bb * p.x_stride;
    const float* mr = p.m + bb * p.m_stride;
    const float g = live ? p.g[bb] : 0.f;
    const bool want_dm = p.dmp != nullptr;
    if (p.dx || want_dm) {
        for (int cb = 0; cb < d; cb += 64) {
            const int cc = cb + c;
            const bool on = live && cc < d;
            float s = 0.f;
            for (int f0 = 0; f0 < F; f0 += G) {
                const int f = f0 + grp;
                if (on && f < F) s = fmaf(mr[f], xr[(int64_t)f * d + cc], s);
            }
            for (int o = dp; o < 64; o <<= 1) s += __shfl_xor(s, o, 64);
            for (int f0 = 0; f0 < F; f0 += G) {
                const int f = f0 + grp;
                const bool in = on && f < F;
                const float e = in ? xr[(int64_t)f * d + cc] : 0.f;
                const float mf = in ? mr[f] : 0.f;
                const float u = in ? s - mf * e : 0.f;
                if (in && p.dx) p.dx[b * p.dx_stride + (int64_t)f * d + cc] = g * mf * u;
                if (want_dm) {
                    float r = e * u;
                    for (int o = 1; o < dp; o <<= 1) r += __shfl_xor(r, o, 64);
                    if (c == 0 && f < F) dm_row[f] = cb == 0 ? r : dm_row[f] + r;
                }
            }
        }
    }
    __syncthreads();
    float corr = 0.f;
    if (want_dm && p.softmax) {
        float a = 0.f;
        for (int f = lane; f < F; f += 64) {
            const float dmf = dm_row[f] + (p.t && live ? p.t[bb * p.t_stride + f] : 0.f);
            a = fmaf(live ? mr[f] : 0.f, dmf, a);
        }
        corr = ifm_wave_sum(a) / (float)F;
    }
    if (!live) return;
    for (int f = lane; f < F; f += 64) {
        const float mf = mr[f];
        if (p.dt) p.dt[b * p.dt_stride + f] = g * mf;
        if (want_dm) {
            const float dmf = dm_row[f] + (p.t ? p.t[b * p.t_stride + f] : 0.f);
            p.dmp[b * p.dmp_stride + f] = p.softmax ? g * mf * (dmf - corr) : g * dmf;
        }
    }
}

struct IfmBwdAct {
    int64_t batch;
    int32_t F, K;
    const float* dmp;
    int64_t dmp_stride;
    const float* kernel;             // [K, F]
    float* dact;
    int64_t dact_stride;
};

// dact[16, K] of a wave's 16 samples.  Uniform trip counts over the workgroup; samples past the batch enter as zeros.
__global__ void __launch_bounds__(IFM_THREADS) ifm_bwd_dact_kernel(IfmBwdAct p) {
    extern __shared__ __align__(16) float ifm_bwd_smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    const int g = lane >> 4, j = lane & 15;
    const int64_t row0 = ((int64_t)blockIdx.x * n_waves + wave) * IFM_ROWS;
    float* a_lds = ifm_bwd_smem + wave * IFM_ROWS * IFM_APITCH;
    const int F = p.F, K = p.K;
    const bool one_chunk = F <= IFM_KC;          // the dm' tile is staged once and serves every pass over K
    for (int n0 = 0; n0 < K; n0 += 64) {
        f32x4 acc[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
        const float* krow[4];
        bool kon[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int n = n0 + 16 * c + j;
            kon[c] = n < K;
            krow[c] = p.kernel + (int64_t)(kon[c] ? n : 0) * F;
        }
        for (int f0 = 0; f0 < F; f0 += IFM_KC) {
            if (!one_chunk || n0 == 0) {
                __syncthreads();                 // the previous chunk's operand reads are done
#pragma unroll 2
                for (int r = 0; r < IFM_ROWS; ++r) {
                    const int64_t b = row0 + r;
                    const int f = f0 + lane;
                    a_lds[r * IFM_APITCH + lane] = (b < p.batch && f < F) ? p.dmp[b * p.dmp_stride + f] : 0.f;
                }
                __syncthreads();
            }
            const int steps = (min(IFM_KC, F - f0) + 3) >> 2;
            for (int kk = 0; kk < steps; ++kk) {
                const int f = f0 + 4 * kk + g;
                const float av = a_lds[j * IFM_APITCH + 4 * kk + g];
                float bv[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) bv[c] = (kon[c] && f < F) ? krow[c][f] : 0.f;
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[c], acc[c], 0, 0, 0);
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int n = n0 + 16 * c + j;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t b = row0 + 4 * g + r;
                if (n < K && b < p.batch) p.dact[b * p.dact_stride + n] = acc[c][r];
            }
        }
    }
}

struct IfmBwdKer {
    int64_t batch, slice_rows;       // slice s: samples [s * slice_rows, (s + 1) * slice_rows) below batch
    int32_t F, n_kb;                 // n_kb: 64-row blocks over the wanted sources
    int32_t kb0[2], K[2];            // per wanted source: its first block, its K
    const float* act[2];
    int64_t act_stride[2];
    const float* dmp;
    int64_t dmp_stride;
    float* partials;                 // [S][n_kb][64][F]
};

// NT accumulator tiles of 16 columns: the block's rows 16 * wave .. + 16 against columns [f0, f0 + 16 NT) of dm'
template <int NT>
__device__ __forceinline__ void ifm_bwd_dkernel_block(const IfmBwdKer& p, const float* act, int64_t act_stride, int K, int k0, int f0,
                                                      int64_t b_lo, int64_t b_hi, float* dst) {
    const int lane = threadIdx.x & 63, g = lane >> 4, j = lane & 15;
    const int F = p.F;
    f32x4 acc[NT];
#pragma unroll
    for (int c = 0; c < NT; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int k = k0 + j;
    const bool kon = k < K;
    const float* acol = act + (kon ? k : 0);
    bool fon[NT];
    int fcol[NT];
#pragma unroll
    for (int c = 0; c < NT; ++c) {
        const int f = f0 + 16 * c + j;
        fon[c] = f < F;
        fcol[c] = fon[c] ? f : 0;
    }
    constexpr int U = NT <= 4 ? 4 : 2;           // k-steps in flight: their loads are issued before the first MFMA
    for (int64_t b0 = b_lo; b0 < b_hi; b0 += 4 * U) {
        float av[U], bv[U][NT];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t b = b0 + 4 * u + g;
            const bool bon = b < b_hi;
            const int64_t br = bon ? b : b_lo;
            av[u] = (bon && kon) ? acol[br * act_stride] : 0.f;
            const float* drow = p.dmp + br * p.dmp_stride;
#pragma unroll
            for (int c = 0; c < NT; ++c) bv[u][c] = (bon && fon[c]) ? drow[fcol[c]] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int c = 0; c < NT; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], bv[u][c], acc[c], 0, 0, 0);
        }
    }
#pragma unroll
    for (int c = 0; c < NT; ++c) {
        const int f = f0 + 16 * c + j;
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (f < F) dst[(int64_t)(4 * g + r) * F + f] = acc[c][r];      // (rows past K hold zeros: the partials carry whole blocks)
    }
}

__global__ void __launch_bounds__(IFM_THREADS) ifm_bwd_dkernel_kernel(IfmBwdKer p) {
    const int wave = threadIdx.x >> 6;
    const int kb = blockIdx.x, s = blockIdx.y;
    const int src = (p.kb0[1] >= 0 && kb >= p.kb0[1]) ? 1 : 0;
    const int k0 = (kb - p.kb0[src]) * 64 + 16 * wave;
    const int64_t b_lo = min((int64_t)s * p.slice_rows, p.batch), b_hi = min(b_lo + p.slice_rows, p.batch);
    const int F = p.F;
    float* dst = p.partials + (((int64_t)s * p.n_kb + kb) * 64 + 16 * wave) * F;
    for (int f0 = 0; f0 < F; f0 += IFM_BWD_FB) {
        const int tiles = (min(IFM_BWD_FB, F - f0) + 15) >> 4;
#define IFM_BWD_BLOCK(NT) ifm_bwd_dkernel_block<NT>(p, p.act[src], p.act_stride[src], p.K[src], k0, f0, b_lo, b_hi, dst)
        if (tiles <= 1) IFM_BWD_BLOCK(1);
        else if (tiles <= 2) IFM_BWD_BLOCK(2);
        else if (tiles <= 3) IFM_BWD_BLOCK(3);
        else if (tiles <= 4) IFM_BWD_BLOCK(4);
        else if (tiles <= 8) IFM_BWD_BLOCK(8);
        else IFM_BWD_BLOCK(16);
#undef IFM_BWD_BLOCK
    }
}

struct IfmBwdSum {
    int32_t F, n_kb, S, n;           // n: wanted sources
    int32_t kb0[2], K[2];
    const float* partials;
    float* dkernel[2];
    int64_t dkernel_stride[2];
};

// element (k, f) of a wanted dkernel: its S partials added in the order 0 .. S-1
__global__ void __launch_bounds__(IFM_THREADS) ifm_bwd_sum_kernel(IfmBwdSum p) {
    int64_t i = (int64_t)blockIdx.x * IFM_THREADS + threadIdx.x;
    const int64_t n0 = (int64_t)p.K[0] * p.F;
    int src = 0;
    if (i >= n0) {
        if (p.n < 2) return;
        i -= n0;
        src = 1;
        if (i >= (int64_t)p.K[1] * p.F) return;
    }
    const int k = (int)(i / p.F), f = (int)(i - (int64_t)k * p.F);
    const int64_t slice = (int64_t)p.n_kb * 64 * p.F;
    const float* src_p = p.partials + ((int64_t)p.kb0[src] * 64 + k) * p.F + f;
    float v = 0.f;
    for (int s = 0; s < p.S; ++s) v += src_p[s * slice];
    p.dkernel[src][k * p.dkernel_stride[src] + f] = v;
}

struct IfmBwdPlan {
    bool want_dact, want_dkernel, dm_in_ws;
    int n_kb, S;
    int64_t slice_rows;
    size_t dm_bytes, partial_bytes, ws_bytes;
    size_t row_lds;                  // one wave's row
};

int ifm_bwd_check(const dctr_ifm_bwd_args_t* a) {
    DCTR_REQUIRE(a, DCTR_E_NULL, "ifm_bwd: null args");
    DCTR_REQUIRE(a->n_fields >= 1 && a->dim >= 1, DCTR_E_DIM, "ifm_bwd: n_fields = %d, dim = %d", a->n_fields, a->dim);
    DCTR_REQUIRE(a->batch >= 0, DCTR_E_DIM, "ifm_bwd: negative batch");
    const int64_t F = a->n_fields, Fd = F * a->dim;
    DCTR_REQUIRE(Fd < (1LL << 27), DCTR_E_DIM, "ifm_bwd: n_fields * dim = %lld exceeds 2^27", (long long)Fd);
    DCTR_REQUIRE(a->x_stride >= Fd, DCTR_E_DIM, "ifm_bwd: x_stride %lld < n_fields * dim = %lld", (long long)a->x_stride, (long long)Fd);
    DCTR_REQUIRE(a->factor_stride >= F, DCTR_E_DIM, "ifm_bwd: factor_stride %lld < n_fields = %d", (long long)a->factor_stride, a->n_fields);
    DCTR_REQUIRE(!a->terms || a->terms_stride >= F, DCTR_E_DIM, "ifm_bwd: terms_stride %lld < n_fields = %d", (long long)a->terms_stride,
                 a->n_fields);
    DCTR_REQUIRE(a->n_src >= 0 && a->n_src <= 2, DCTR_E_DIM, "ifm_bwd: n_src = %d: 0, 1 or 2 factor sources", a->n_src);
    for (int s = 0; s < a->n_src; ++s) {
        DCTR_REQUIRE(a->src[s].K >= 1, DCTR_E_DIM, "ifm_bwd: source %d: K = %d", s, a->src[s].K);
        DCTR_REQUIRE(a->src[s].act_stride >= a->src[s].K, DCTR_E_DIM, "ifm_bwd: source %d: act_stride %lld < K = %d", s,
                     (long long)a->src[s].act_stride, a->src[s].K);
        DCTR_REQUIRE(!a->dact[s] || a->dact_stride[s] >= a->src[s].K, DCTR_E_DIM, "ifm_bwd: source %d: dact_stride %lld < K = %d", s,
                     (long long)a->dact_stride[s], a->src[s].K);
        DCTR_REQUIRE(!a->dkernel[s] || a->dkernel_stride[s] >= F, DCTR_E_DIM, "ifm_bwd: source %d: dkernel_stride %lld < n_fields = %d", s,
                     (long long)a->dkernel_stride[s], a->n_fields);
    }
    DCTR_REQUIRE(!a->dx || a->dx_stride >= Fd, DCTR_E_DIM, "ifm_bwd: dx_stride %lld < n_fields * dim = %lld", (long long)a->dx_stride,
                 (long long)Fd);
    DCTR_REQUIRE(!a->dterms || a->dterms_stride >= F, DCTR_E_DIM, "ifm_bwd: dterms_stride %lld < n_fields = %d",
                 (long long)a->dterms_stride, a->n_fields);
    DCTR_REQUIRE(!a->dmprime || a->dmprime_stride >= F, DCTR_E_DIM, "ifm_bwd: dmprime_stride %lld < n_fields = %d",
                 (long long)a->dmprime_stride, a->n_fields);
    DCTR_REQUIRE(a->slices >= 0 && a->slices <= DCTR_GLOBAL_WGS, DCTR_E_DIM, "ifm_bwd: slices = %d: 0 (the library's choice) or 1 .. %d",
                 a->slices, DCTR_GLOBAL_WGS);
    return DCTR_OK;
}

bool ifm_bwd_fits(const dctr_ifm_bwd_args_t* a) { return ((size_t)a->n_fields + 15) / 16 * 16 * 4 <= DCTR_LDS_MAX; }

void ifm_bwd_plan(const dctr_ifm_bwd_args_t* a, IfmBwdPlan* pl) {
    const size_t F = (size_t)a->n_fields;
    pl->want_dact = pl->want_dkernel = false;
    pl->n_kb = 0;
    for (int s = 0; s < a->n_src; ++s) {
        pl->want_dact |= a->dact[s] != nullptr;
        if (a->dkernel[s]) {
            pl->want_dkernel = true;
            pl->n_kb += (a->src[s].K + 63) / 64;
        }
    }
    pl->dm_in_ws = (pl->want_dact || pl->want_dkernel) && !a->dmprime;
    pl->dm_bytes = pl->dm_in_ws ? ((size_t)a->batch * F * 4 + 15) & ~(size_t)15 : 0;
    pl->S = 0;
    pl->slice_rows = 0;
    pl->partial_bytes = 0;
    if (pl->want_dkernel) {
        const size_t slice_bytes = (size_t)pl->n_kb * 64 * F * 4;
        int64_t S = a->slices;
        if (S == 0) {
            S = dctr_ceil_div(IFM_BWD_WGS, pl->n_kb);
            const int64_t by_rows = dctr_ceil_div(a->batch, 64);
            if (S > by_rows) S = by_rows;
            if (S > DCTR_GLOBAL_WGS) S = DCTR_GLOBAL_WGS;
            const int64_t by_bytes = (int64_t)(DCTR_GLOBAL_MAX / slice_bytes);
            if (S > by_bytes) S = by_bytes;
            if (S < 1) S = 1;
        }
        pl->S = (int)S;
        pl->slice_rows = (dctr_ceil_div(a->batch, S) + 3) / 4 * 4;
        if (pl->slice_rows < 4) pl->slice_rows = 4;
        pl->partial_bytes = slice_bytes * (size_t)S;
    }
    pl->ws_bytes = pl->dm_bytes + pl->partial_bytes;
    pl->row_lds = F * 4;
}

}  // namespace

extern "C" int dctr_ifm_bwd_supported(const dctr_ifm_bwd_args_t* args) {
    if (!args || args->n_fields < 1 || args->dim < 1 || (int64_t)args->n_fields * args->dim >= (1LL << 27)) return 0;
    return ifm_bwd_fits(args) ? 1 : 0;
}

extern "C" size_t dctr_ifm_bwd_workspace_bytes(const dctr_ifm_bwd_args_t* args) {
    if (!args || ifm_bwd_check(args) != DCTR_OK || !ifm_bwd_fits(args)) return 0;
    IfmBwdPlan pl;
    ifm_bwd_plan(args, &pl);
    return pl.ws_bytes;
}

extern "C" int dctr_ifm_bwd(const dctr_ifm_bwd_args_t* a, void* stream) {
    int rc = ifm_bwd_check(a);
    if (rc != DCTR_OK) return rc;
    DCTR_REQUIRE(ifm_bwd_fits(a), DCTR_E_UNSUPPORTED, "ifm_bwd: a row of %d fields exceeds the LDS (dctr_ifm_bwd_supported)", a->n_fields);
    DCTR_REQUIRE(a->x && a->factor && a->d_out, DCTR_E_NULL, "ifm_bwd: null x / factor / d_out");
    IfmBwdPlan pl;
    ifm_bwd_plan(a, &pl);
    for (int s = 0; s < a->n_src; ++s) {
        DCTR_REQUIRE(!a->dact[s] || a->src[s].kernel, DCTR_E_NULL, "ifm_bwd: source %d: dact without the kernel", s);
        DCTR_REQUIRE(!a->dkernel[s] || a->src[s].act, DCTR_E_NULL, "ifm_bwd: source %d: dkernel without act", s);
    }
    if (pl.ws_bytes) DCTR_REQUIRE_WORKSPACE("ifm_bwd", "dctr_ifm_bwd_workspace_bytes", a->workspace, a->workspace_bytes, pl.ws_bytes);
    if (a->batch == 0) {
        // (an empty batch: the sums over it are zeros — one sum launch over no slices)
        if (!pl.want_dkernel) return DCTR_OK;
    }
    const hipStream_t st = (hipStream_t)stream;
    const int F = a->n_fields;
    float* dm_ws = pl.dm_in_ws ? (float*)a->workspace : nullptr;
    float* partials = pl.want_dkernel ? (float*)((char*)a->workspace + pl.dm_bytes) : nullptr;
    const float* dmp = a->dmprime ? a->dmprime : dm_ws;
    const int64_t dmp_stride = a->dmprime ? a->dmprime_stride : F;
    if (a->batch > 0 && (a->dx || a->dterms || dmp)) {
        IfmBwdRow p = {};
        p.batch = a->batch;
        p.F = F;
        p.d = a->dim;
        p.dp = ifm_group_lanes(a->dim);
        p.softmax = a->softmax ? 1 : 0;
        p.x = a->x;
        p.x_stride = a->x_stride;
        p.m = a->factor;
        p.m_stride = a->factor_stride;
        p.t = a->terms;
        p.t_stride = a->terms_stride;
        p.g = a->d_out;
        p.dx = a->dx;
        p.dx_stride = a->dx_stride;
        p.dt = a->dterms;
        p.dt_stride = a->dterms_stride;
        p.dmp = a->dmprime ? a->dmprime : dm_ws;
        p.dmp_stride = dmp_stride;
        // four waves, a sample each; one wave where four rows do not fit the LDS or four-wave groups would leave CUs idle
        const bool small = 4 * pl.row_lds > DCTR_LDS_MAX || dctr_ceil_div(a->batch, 4) < (int64_t)IFM_SMALL_WG_BELOW * dctr_n_cus();
        const int n_waves = small ? 1 : 4;
        const size_t lds = pl.row_lds * n_waves;
        static thread_local size_t granted[DCTR_MAX_DEVICES] = {0};
        if (lds > 48 * 1024) {
            hipError_t e = dctr_grant_lds((const void*)ifm_bwd_row_kernel, lds, granted);
            DCTR_REQUIRE(e == hipSuccess, (int)e, "ifm_bwd: cannot raise dynamic LDS: %s", hipGetErrorString(e));
        }
        const dim3 grid((unsigned)dctr_ceil_div(a->batch, (int64_t)n_waves)), block(64 * n_waves);
        DCTR_LAUNCH(ifm_bwd_row_kernel, grid, block, lds, st, p);
        rc = dctr_launch_status("dctr_ifm_bwd (row pass)");
        if (rc != DCTR_OK) return rc;
    }
    if (a->batch > 0) {
        const bool small = dctr_ceil_div(a->batch, (int64_t)IFM_WG_ROWS) < (int64_t)IFM_SMALL_WG_BELOW * dctr_n_cus();
        const int n_waves = small ? 1 : 4;
        for (int s = 0; s < a->n_src; ++s) {
            if (!a->dact[s]) continue;
            IfmBwdAct p = {};
            p.batch = a->batch;
            p.F = F;
            p.K = a->src[s].K;
            p.dmp = dmp;
            p.dmp_stride = dmp_stride;
            p.kernel = a->src[s].kernel;
            p.dact = a->dact[s];
            p.dact_stride = a->dact_stride[s];
            const dim3 grid((unsigned)dctr_ceil_div(a->batch, (int64_t)IFM_ROWS * n_waves)), block(64 * n_waves);
            DCTR_LAUNCH(ifm_bwd_dact_kernel, grid, block, (size_t)n_waves * IFM_ROWS * IFM_APITCH * 4, st, p);
            rc = dctr_launch_status("dctr_ifm_bwd (dact pass)");
            if (rc != DCTR_OK) return rc;
        }
    }
    if (pl.want_dkernel) {
        IfmBwdKer p = {};
        IfmBwdSum q = {};
        p.batch = a->batch;
        p.slice_rows = pl.slice_rows;
        p.F = q.F = F;
        p.n_kb = q.n_kb = pl.n_kb;
        p.dmp = dmp;
        p.dmp_stride = dmp_stride;
        p.partials = partials;
        q.partials = partials;
        q.S = a->batch > 0 ? pl.S : 0;
        p.kb0[1] = q.kb0[1] = -1;
        int n = 0, kb = 0;
        int64_t elems = 0;
        for (int s = 0; s < a->n_src; ++s) {
            if (!a->dkernel[s]) continue;
            p.kb0[n] = q.kb0[n] = kb;
            p.K[n] = q.K[n] = a->src[s].K;
            p.act[n] = a->src[s].act;
            p.act_stride[n] = a->src[s].act_stride;
            q.dkernel[n] = a->dkernel[s];
            q.dkernel_stride[n] = a->dkernel_stride[s];
            kb += (a->src[s].K + 63) / 64;
            elems += (int64_t)a->src[s].K * F;
            ++n;
        }
        q.n = n;
        if (a->batch > 0) {
            const dim3 grid((unsigned)pl.n_kb, (unsigned)pl.S), block(IFM_THREADS);
            DCTR_LAUNCH(ifm_bwd_dkernel_kernel, grid, block, 0, st, p);
            rc = dctr_launch_status("dctr_ifm_bwd (dkernel pass)");
            if (rc != DCTR_OK) return rc;
        }
        const dim3 grid((unsigned)dctr_ceil_div(elems, (int64_t)IFM_THREADS)), block(IFM_THREADS);
        DCTR_LAUNCH(ifm_bwd_sum_kernel, grid, block, 0, st, q);
    }
    return dctr_launch_status("dctr_ifm_bwd");
}
