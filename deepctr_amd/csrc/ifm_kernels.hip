// IFM / DIFM (reference deepctr/models/ifm.py:55-72, difm.py:59-80): from the inputs of the input-aware factor to the probability.
//
// Per sample b, F fields of one embedding_dim d:
//     m'[f] = mprime[b, f] + sum over the sources s of act_s[b, :] . kernel_s[:, f]          (0, 1 or 2 sources; mprime optional)
//     m[f]  = softmax ? F * exp(m'[f] - max m') / sum_f exp(m'[f] - max m') : m'[f]
//     fm    = 0.5 * sum_c ((sum_f m[f] e[f, c])^2 - sum_f (m[f] e[f, c])^2)                   e = the leading F*d columns of x
//     lin   = sum_k m[k] * lin_k                 lin_k gathered from a 1-wide table by id, or read from a pre-pooled [B] vector
//     out   = act(fm + lin + sum_i add_i[b] + *global_bias)
//
// A wave takes 16 samples; four waves form a workgroup (one wave per workgroup at batches that would otherwise leave CUs idle — the
// waves share nothing but the barriers, so the arithmetic is the same).  Projection: the wave's [16, K] slice of a source goes through LDS in
// chunks of 64 columns (coalesced loads, conflict-free operand reads), the Keras-layout kernel comes straight from L2 in the MFMA's
// operand layout (16 consecutive columns of 4 rows), and v_mfma_f32_16x16x4_f32 keeps the product in exact fp32; 64 output columns
// (four accumulator tiles) per pass over K.  The [16, F] tile of m' then waits in LDS (route LDS), or is written to the workspace and
// read back by a second launch of the same epilogue (route WORKSPACE: more fields than the LDS holds, or forced) — the same
// instructions on the same values in the same order, hence the same bits.  Epilogue: one wave per sample; the lanes split into 64 / dp
// groups of dp = pow2(d) lanes, group g walks the fields g, g + G, ... with a lane per embedding column, so a wave reads 256
// contiguous bytes of the row per step; the groups meet in xor-shuffles.  m is formed where it is used and reaches HBM only through
// factor_out.  An id outside [0, vocab) raises DCTR_STATUS_INDEX_OOR and contributes zero; nothing outside the tables is read.
#include "ifm_device.h"

namespace {

using namespace dctr_ifm;

enum { IFM_FUSED = 0, IFM_PROJECT = 1, IFM_EPILOGUE = 2 };

struct IfmParams {
    dctr_ifm_src_t src[2];
    int32_t n_src;
    int64_t batch;
    int32_t F, d, dp, Fpad;          // dp: power of two >= min(d, 64); Fpad: F rounded up to 16
    const float* x;
    int64_t x_stride;
    const float* mprime;             // [B, mprime_stride] or NULL
    int64_t mprime_stride;
    float* ws;                       // IFM_PROJECT: destination [B, F]
    const dctr_ifm_lin_t* lin;
    int32_t n_lin, n_add, softmax, sigmoid_out;
    const float* add[4];
    const float* global_bias;
    float* out;
    float* factor_out;
    int64_t factor_stride;
    int32_t* status;
};

// m' of the wave's 16 samples: columns [0, F) to dst (LDS tile or workspace rows), row pitch dst_pitch.  Every wave of the workgroup
// runs the same trip counts (the barriers are workgroup-wide); samples past the batch enter as zeros and are not stored to global.
template <bool TO_GLOBAL>
__device__ __forceinline__ void ifm_project(const IfmParams& p, float* a_lds, float* dst, int64_t dst_pitch, int64_t row0) {
    const int lane = threadIdx.x & 63, g = lane >> 4, j = lane & 15;
    const int F = p.F;
    for (int n0 = 0; n0 < p.Fpad; n0 += 64) {
        f32x4 acc[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t b = row0 + 4 * g + r;
                const int n = n0 + 16 * c + j;
                acc[c][r] = (p.mprime && b < p.batch && n < F) ? p.mprime[b * p.mprime_stride + n] : 0.f;
            }
        }
        for (int s = 0; s < p.n_src; ++s) {
            const dctr_ifm_src_t sd = p.src[s];
            for (int k0 = 0; k0 < sd.K; k0 += IFM_KC) {
                __syncthreads();                 // the previous chunk's operand reads are done
#pragma unroll 2
                for (int r = 0; r < IFM_ROWS; ++r) {
                    const int64_t b = row0 + r;
                    const int k = k0 + lane;
                    a_lds[r * IFM_APITCH + lane] = (b < p.batch && k < sd.K) ? sd.act[b * sd.act_stride + k] : 0.f;
                }
                __syncthreads();
#pragma unroll
                for (int kk = 0; kk < IFM_KC / 4; ++kk) {
                    const int k = k0 + 4 * kk + g;           // (k-steps past K multiply zeros: no early exit, the 16 steps stay one block)
                    const float av = a_lds[j * IFM_APITCH + 4 * kk + g];
                    float bv[4];
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const int n = n0 + 16 * c + j;
                        bv[c] = (k < sd.K && n < F) ? sd.kernel[(int64_t)k * F + n] : 0.f;
                    }
#pragma unroll
                    for (int c = 0; c < 4; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[c], acc[c], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int n = n0 + 16 * c + j;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 4 * g + r;
                if (TO_GLOBAL) {
                    if (n < F && row0 + row < p.batch) dst[(row0 + row) * dst_pitch + n] = acc[c][r];
                } else {
                    if (n < p.Fpad) dst[row * dst_pitch + n] = acc[c][r];
                }
            }
        }
    }
}

// one sample by one wave; mp: the sample's F values of m' (LDS or global)
__device__ __forceinline__ void ifm_epilogue_row(const IfmParams& p, const float* mp, int64_t b) {
    const int lane = threadIdx.x & 63;
    const int F = p.F, d = p.d, dp = p.dp;
    float mx = 0.f, sc = 1.f;
    if (p.softmax) {
        float v = -INFINITY;
        for (int f = lane; f < F; f += 64) v = fmaxf(v, mp[f]);
        mx = ifm_wave_max(v);
        float s = 0.f;
        for (int f = lane; f < F; f += 64) s += expf(mp[f] - mx);
        sc = 1.f / ifm_wave_sum(s);
    }
    const float nf = (float)F;
#define IFM_FACTOR(f) (p.softmax ? nf * (expf(mp[(f)] - mx) * sc) : mp[(f)])
    if (p.factor_out)
        for (int f = lane; f < F; f += 64) p.factor_out[b * p.factor_stride + f] = IFM_FACTOR(f);
    // ---- FM over the refined embeddings ------------------------------------------------------------------------------------------
    const int G = 64 / dp, grp = lane / dp, c = lane - grp * dp;
    const float* xr = p.x + b * p.x_stride;
    float fm = 0.f;
    for (int cb = 0; cb < d; cb += 64) {
        const int cc = cb + c;
        const bool on = cc < d;
        float s = 0.f, q = 0.f;
        for (int f = grp; f < F; f += G) {
            const float v = on ? IFM_FACTOR(f) * xr[(int64_t)f * d + cc] : 0.f;
            s += v;
            q = fmaf(v, v, q);
        }
        for (int o = dp; o < 64; o <<= 1) {
            s += __shfl_xor(s, o, 64);
            q += __shfl_xor(q, o, 64);
        }
        if (grp == 0 && on) fm += s * s - q;
    }
    fm = 0.5f * ifm_wave_sum(fm);
    // ---- the refined first-order terms, by position ------------------------------------------------------------------------------
    float lin = 0.f;
    for (int k = lane; k < p.n_lin; k += 64) {
        const dctr_ifm_lin_t ld = p.lin[k];
        float w = 0.f;
        if (ld.vec) {
            w = ld.vec[b * ld.vec_stride];
        } else {
            const int64_t r = ld.ids_is_i64 ? ((const int64_t*)ld.ids)[b * ld.ids_stride] : (int64_t)((const int32_t*)ld.ids)[b * ld.ids_stride];
            if (r >= 0 && r < ld.vocab)
                w = ld.table[r];
            else if (p.status)
                atomicOr(p.status, DCTR_STATUS_INDEX_OOR);
        }
        lin = fmaf(IFM_FACTOR(k), w, lin);
    }
#undef IFM_FACTOR
    lin = ifm_wave_sum(lin);
    if (lane == 0) {
        float logit = fm + lin;
        for (int i = 0; i < p.n_add; ++i) logit += p.add[i][b];
        if (p.global_bias) logit += *p.global_bias;
        p.out[b] = p.sigmoid_out ? 1.f / (1.f + expf(-logit)) : logit;
    }
}

template <int MODE>
__global__ void __launch_bounds__(IFM_THREADS) ifm_kernel(IfmParams p) {
    extern __shared__ __align__(16) float ifm_smem[];
    const int wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;        // 4 waves, or 1 where the batch would leave CUs idle
    const int64_t row0 = ((int64_t)blockIdx.x * n_waves + wave) * IFM_ROWS;
    const int tpitch = p.Fpad + 4;          // bank = 16 * (row / 4) + column: an accumulator store hits 64 banks
    const bool project = MODE != IFM_EPILOGUE && (p.n_src > 0 || MODE == IFM_PROJECT);
    float* a_lds = ifm_smem + wave * IFM_ROWS * IFM_APITCH;
    float* tile = ifm_smem + n_waves * IFM_ROWS * IFM_APITCH + (size_t)wave * IFM_ROWS * tpitch;
    if (MODE == IFM_PROJECT) {
        ifm_project<true>(p, a_lds, p.ws, p.F, row0);
        return;
    }
    if (project) {
        ifm_project<false>(p, a_lds, tile, tpitch, row0);
        __syncthreads();
    }
    for (int r = 0; r < IFM_ROWS; ++r) {
        const int64_t b = row0 + r;
        if (b >= p.batch) break;
        const float* mp = project ? tile + r * tpitch : p.mprime + b * p.mprime_stride;
        ifm_epilogue_row(p, mp, b);
    }
}

struct IfmPlan {
    bool workspace;        // m' goes through HBM
    size_t lds, lds_project;
    size_t ws_bytes;
};

int ifm_check(const dctr_ifm_args_t* a) {
    DCTR_REQUIRE(a, DCTR_E_NULL, "ifm_fwd: null args");
    DCTR_REQUIRE(a->n_fields >= 1 && a->dim >= 1, DCTR_E_DIM, "ifm_fwd: n_fields = %d, dim = %d", a->n_fields, a->dim);
    DCTR_REQUIRE(a->batch >= 0, DCTR_E_DIM, "ifm_fwd: negative batch");
    DCTR_REQUIRE((int64_t)a->n_fields * a->dim < (1LL << 27), DCTR_E_DIM, "ifm_fwd: n_fields * dim = %lld exceeds 2^27",
                 (long long)a->n_fields * a->dim);
    DCTR_REQUIRE(a->x_stride >= (int64_t)a->n_fields * a->dim, DCTR_E_DIM, "ifm_fwd: x_stride %lld < n_fields * dim = %lld",
                 (long long)a->x_stride, (long long)a->n_fields * a->dim);
    DCTR_REQUIRE(a->n_src >= 0 && a->n_src <= 2, DCTR_E_DIM, "ifm_fwd: n_src = %d: 0, 1 or 2 factor sources", a->n_src);
    for (int s = 0; s < a->n_src; ++s) {
        DCTR_REQUIRE(a->src[s].K >= 1, DCTR_E_DIM, "ifm_fwd: source %d: K = %d", s, a->src[s].K);
        DCTR_REQUIRE(a->src[s].act_stride >= a->src[s].K, DCTR_E_DIM, "ifm_fwd: source %d: act_stride %lld < K = %d", s,
                     (long long)a->src[s].act_stride, a->src[s].K);
    }
    DCTR_REQUIRE(a->n_src > 0 || a->mprime_stride >= a->n_fields, DCTR_E_DIM,
                 "ifm_fwd: no factor source: mprime [B, n_fields] is required with mprime_stride >= %d", a->n_fields);
    DCTR_REQUIRE(a->n_lin == 0 || a->n_lin == a->n_fields, DCTR_E_DIM,
                 "ifm_fwd: n_lin = %d: the factor refines the first-order terms by position, 0 or n_fields = %d of them", a->n_lin,
                 a->n_fields);
    DCTR_REQUIRE(a->n_add >= 0 && a->n_add <= 4, DCTR_E_DIM, "ifm_fwd: n_add = %d: at most 4", a->n_add);
    DCTR_REQUIRE(a->route == DCTR_IFM_ROUTE_AUTO || a->route == DCTR_IFM_ROUTE_WORKSPACE, DCTR_E_ENUM, "ifm_fwd: unknown route %d",
                 a->route);
    return DCTR_OK;
}

void ifm_plan(const dctr_ifm_args_t* a, IfmPlan* pl) {
    const size_t Fpad = ((size_t)a->n_fields + 15) / 16 * 16;
    pl->lds_project = (size_t)4 * IFM_ROWS * IFM_APITCH * 4;
    pl->lds = a->n_src > 0 ? pl->lds_project + (size_t)4 * IFM_ROWS * (Fpad + 4) * 4 : 0;
    pl->workspace = a->n_src > 0 && (a->route == DCTR_IFM_ROUTE_WORKSPACE || pl->lds > DCTR_LDS_MAX);
    pl->ws_bytes = pl->workspace ? ((size_t)a->batch * (size_t)a->n_fields * 4 + 15) & ~(size_t)15 : 0;
}

}  // namespace

extern "C" size_t dctr_ifm_workspace_bytes(const dctr_ifm_args_t* args) {
    if (ifm_check(args) != DCTR_OK) return 0;
    IfmPlan pl;
    ifm_plan(args, &pl);
    return pl.ws_bytes;
}

extern "C" int dctr_ifm_route(const dctr_ifm_args_t* args) {
    int rc = ifm_check(args);
    if (rc != DCTR_OK) return rc;
    IfmPlan pl;
    ifm_plan(args, &pl);
    return pl.workspace ? DCTR_IFM_ROUTE_WORKSPACE : DCTR_IFM_ROUTE_LDS;
}

extern "C" int dctr_ifm_fwd(const dctr_ifm_args_t* a, void* stream) {
    int rc = ifm_check(a);
    if (rc != DCTR_OK) return rc;
    DCTR_REQUIRE(a->x && a->out, DCTR_E_NULL, "ifm_fwd: null x / out");
    DCTR_REQUIRE(a->n_src > 0 || a->mprime, DCTR_E_NULL, "ifm_fwd: neither a factor source nor mprime");
    DCTR_REQUIRE(!a->mprime || a->mprime_stride >= a->n_fields, DCTR_E_DIM, "ifm_fwd: mprime_stride %lld < n_fields = %d",
                 (long long)a->mprime_stride, a->n_fields);
    for (int s = 0; s < a->n_src; ++s)
        DCTR_REQUIRE(a->src[s].act && a->src[s].kernel, DCTR_E_NULL, "ifm_fwd: source %d: null act / kernel", s);
    DCTR_REQUIRE(a->n_lin == 0 || a->lin, DCTR_E_NULL, "ifm_fwd: n_lin = %d without descriptors", a->n_lin);
    for (int i = 0; i < a->n_add; ++i) DCTR_REQUIRE(a->add[i], DCTR_E_NULL, "ifm_fwd: add[%d] is null", i);
    DCTR_REQUIRE(!a->factor_out || a->factor_stride >= a->n_fields, DCTR_E_DIM, "ifm_fwd: factor_stride %lld < n_fields = %d",
                 (long long)a->factor_stride, a->n_fields);
    IfmPlan pl;
    ifm_plan(a, &pl);
    if (pl.workspace) {
        DCTR_REQUIRE(a->workspace, DCTR_E_NULL, "ifm_fwd: %d fields on the workspace route: %zu bytes of workspace are required",
                     a->n_fields, pl.ws_bytes);
        DCTR_REQUIRE(dctr_aligned16(a->workspace), DCTR_E_ALIGN, "ifm_fwd: workspace not 16-B aligned");
        DCTR_REQUIRE(a->workspace_bytes >= pl.ws_bytes, DCTR_E_DIM, "ifm_fwd: workspace of %zu bytes, %zu needed", a->workspace_bytes,
                     pl.ws_bytes);
    }
    if (a->batch == 0) return DCTR_OK;
    IfmParams p = {};
    p.n_src = a->n_src;
    for (int s = 0; s < a->n_src; ++s) p.src[s] = a->src[s];
    p.batch = a->batch;
    p.F = a->n_fields;
    p.d = a->dim;
    p.dp = ifm_group_lanes(a->dim);
    p.Fpad = (a->n_fields + 15) / 16 * 16;
    p.x = a->x;
    p.x_stride = a->x_stride;
    p.mprime = a->mprime;
    p.mprime_stride = a->mprime_stride;
    p.lin = a->lin;
    p.n_lin = a->n_lin;
    p.n_add = a->n_add;
    for (int i = 0; i < a->n_add; ++i) p.add[i] = a->add[i];
    p.softmax = a->softmax ? 1 : 0;
    p.sigmoid_out = a->sigmoid_out ? 1 : 0;
    p.global_bias = a->global_bias;
    p.out = a->out;
    p.factor_out = a->factor_out;
    p.factor_stride = a->factor_stride;
    p.status = a->status;
    const hipStream_t st = (hipStream_t)stream;
    // four waves per workgroup share nothing but the barriers; where that leaves CUs without work, a wave per workgroup (same arithmetic)
    const bool small = dctr_ceil_div(a->batch, (int64_t)IFM_WG_ROWS) < (int64_t)IFM_SMALL_WG_BELOW * dctr_n_cus();
    const int n_waves = small ? 1 : 4;
    const dim3 grid((unsigned)dctr_ceil_div(a->batch, (int64_t)IFM_ROWS * n_waves)), block(64 * n_waves);
    const size_t lds_fused = pl.lds / 4 * n_waves, lds_project = pl.lds_project / 4 * n_waves;
    static thread_local size_t granted[DCTR_MAX_DEVICES] = {0};
    if (pl.workspace) {
        p.ws = (float*)a->workspace;
        DCTR_LAUNCH((ifm_kernel<IFM_PROJECT>), grid, block, lds_project, st, p);
        rc = dctr_launch_status("dctr_ifm_fwd (projection)");
        if (rc != DCTR_OK) return rc;
        p.mprime = p.ws;
        p.mprime_stride = a->n_fields;
        p.n_src = 0;
        DCTR_LAUNCH((ifm_kernel<IFM_EPILOGUE>), grid, block, 0, st, p);
    } else if (a->n_src > 0) {
        hipError_t e = dctr_grant_lds((const void*)ifm_kernel<IFM_FUSED>, pl.lds, granted);
        DCTR_REQUIRE(e == hipSuccess, (int)e, "ifm_fwd: cannot raise dynamic LDS: %s", hipGetErrorString(e));
        DCTR_LAUNCH((ifm_kernel<IFM_FUSED>), grid, block, lds_fused, st, p);
    } else {
        DCTR_LAUNCH((ifm_kernel<IFM_EPILOGUE>), grid, block, 0, st, p);
    }
    return dctr_launch_status("dctr_ifm_fwd");
}
