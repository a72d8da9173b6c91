// Backward of ONN's pair products (ffm_kernels.hip, without scale / shift and without dense columns), one launch from the ids and the
// output gradient to the gradients of the fused tables.  The forward saves nothing: ids and rows are loaded again.
//
// Per sample b and pair p = (i < j, itertools.combinations order), g = d_out[b]:
//     d row_i[slot j = j - 1][e] += g[p*d + e] * row_j[slot i = i][e]
//     d row_j[slot i = i][e]     += g[p*d + e] * row_i[slot j = j - 1][e]          (reduce_sum: g[p])
// so the gradient of one (sample, field f) is ONE contiguous run of R = (F-1)*d floats: slot k <- partner i = k (k < f) or k + 1, the
// pair of (f, i), and the partner's slot towards f.  Nothing is summed inside a sample: every element is one fp32 product.
//
// LDS route: a workgroup walks tiles of S samples.  Phase 0 resolves per (sample, field) the source row and the destination row (id
// load, range check, pre-pooled fields: row = sample index; a frozen field or an id out of range: no destination); phase 1 gathers the
// S*F whole rows into LDS as the forward does (16-B loads when d % 4 == 0); phase 2 walks the tile's S*F*R gradient elements in order,
// one dword per lane: a wave-instruction covers 256 contiguous bytes of a gradient row (or the end of one row and the start of the
// next), the shape at which global float atomics run at the chip-wide rate.  Table fields leave through unsafeAtomicAdd into the dense
// gradient table, pre-pooled fields through plain stores (one owner per element).  ffm_kernels.hip's phases 0 and 1 are restated here,
// not shared: phase 0 resolves a second address per row, and the forward stays the code it was.
// Direct route (rows past the LDS, or forced): phase 0 keeps the row indices only; every lane reads its partner element from global
// memory through the field descriptors.  Same arithmetic, same destinations.
// Ids that repeat inside a tile are not merged before the atomics (DESIGN.md §4.11 has the measurement on skewed ids).
#include <stdint.h>
#include "dctr_common.h"
#include "tile_route.h"

namespace {

constexpr int FFB_THREADS = 256;
constexpr size_t FFB_TILE_BUDGET = 40 * 1024;    // target bytes of a tile's rows: >= 3 workgroups per CU, as the forward
constexpr int FFB_S_MAX = 32;
constexpr int FFB_S_DIRECT = 8;

struct FfmBwdParams {
    const dctr_ffm_field_t* fields;
    const dctr_ffm_grad_t* grads;
    int64_t batch;
    int32_t F, d, R, S;          // R = (F-1)*d floats per fused row; S samples per tile
    int32_t reduce, pad_;
    const float* g;              // d_out, already advanced by d_out_offset
    int64_t g_stride;
    int32_t* status;
    int64_t n_tiles;
};

// bytes of a workgroup's dynamic LDS: LDS route = source rows [S*F] + destinations [S*F] (8 B each) + the tile; direct = row indices
inline size_t ffb_lds_bytes(int F, int d, int S, bool direct) {
    const size_t SF = (size_t)S * F;
    return direct ? SF * 8 : SF * 16 + SF * (size_t)(F - 1) * d * 4;
}

// the pair index of fields a != b
__device__ __forceinline__ int ffb_pair(int a, int b, int F) {
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    return (int)((int64_t)lo * (2 * F - lo - 1) / 2) + hi - lo - 1;
}

template <bool DIRECT, bool VEC>
__global__ void __launch_bounds__(FFB_THREADS) ffm_bwd_kernel(FfmBwdParams p) {
    extern __shared__ __align__(16) unsigned char ffb_smem[];
    const int F = p.F, d = p.d, R = p.R, S = p.S;
    const int SF = S * F;
    // LDS route: src[SF] | dst[SF] (bit 0 set: plain stores) | tile[SF * R]; direct route: ridx[SF]
    const float** src = reinterpret_cast<const float**>(ffb_smem);
    uintptr_t* dst = reinterpret_cast<uintptr_t*>(ffb_smem + (size_t)SF * 8);
    float* tile = reinterpret_cast<float*>(ffb_smem + (size_t)SF * 16);
    int64_t* ridx = reinterpret_cast<int64_t*>(ffb_smem);
    const int tid = threadIdx.x;

    for (int64_t t = blockIdx.x; t < p.n_tiles; t += gridDim.x) {
        const int64_t b0 = t * S;
        const int nvalid = (int)((p.batch - b0) < S ? (p.batch - b0) : S);
        __syncthreads();        // the previous tile's readers are done with the addresses and the tile
        // ---- phase 0: source and destination rows ------------------------------------------------------------------------------
        for (int sf = tid; sf < SF; sf += FFB_THREADS) {
            const int s = sf / F, f = sf - s * F;
            int64_t r = -1;
            const float* sp = nullptr;
            uintptr_t dp = 0;
            if (s < nvalid) {
                const dctr_ffm_field_t fd = p.fields[f];
                const int64_t b = b0 + s;
                r = b;
                if (!fd.identity)
                    r = fd.ids_is_i64 ? ((const int64_t*)fd.ids)[b * fd.ids_stride] : (int64_t)((const int32_t*)fd.ids)[b * fd.ids_stride];
                if (r >= 0 && r < fd.vocab) {
                    if (!DIRECT) {
                        sp = fd.rows + r * fd.row_pitch;
                        const dctr_ffm_grad_t gd = p.grads[f];
                        if (gd.grad) dp = reinterpret_cast<uintptr_t>(gd.grad + r * gd.row_stride) | (fd.identity ? 1u : 0u);
                    }
                } else {
                    r = -1;
                    if (p.status) atomicOr(p.status, DCTR_STATUS_INDEX_OOR);
                }
            }
            if (DIRECT) {
                ridx[sf] = r;
            } else {
                src[sf] = sp;
                dst[sf] = dp;
            }
        }
        __syncthreads();
        // ---- phase 1 (LDS route): the S*F whole rows into the tile, an id out of range as zeros ---------------------------------
        if (!DIRECT) {
            if (VEC) {
                const int C = R >> 2, n = nvalid * F * C;
                for (int base = tid; base < n; base += 4 * FFB_THREADS) {
                    float4 v[4];
                    int at[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int idx = base + u * FFB_THREADS;
                        at[u] = -1;
                        v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                        if (idx < n) {
                            const int sf = idx / C, c = idx - sf * C;
                            at[u] = sf * R + 4 * c;
                            const float* q = src[sf];
                            if (q) {
                                q += 4 * c;
                                if ((reinterpret_cast<uintptr_t>(q) & 15u) == 0)
                                    v[u] = *reinterpret_cast<const float4*>(q);
                                else
                                    v[u] = make_float4(q[0], q[1], q[2], q[3]);
                            }
                        }
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (at[u] >= 0) *reinterpret_cast<float4*>(tile + at[u]) = v[u];
                }
            } else {
                const int n = nvalid * F * R;
                for (int idx = tid; idx < n; idx += FFB_THREADS) {
                    const int sf = idx / R, c = idx - sf * R;
                    const float* q = src[sf];
                    tile[idx] = q ? q[c] : 0.f;
                }
            }
            __syncthreads();
        }
        // ---- phase 2: the gradient rows, element by element in memory order: one dword per lane ---------------------------------
        const int n = nvalid * F * R;           // (the plan keeps S*F*R below 2^30 on both routes)
        for (int idx = tid; idx < n; idx += FFB_THREADS) {
            const int sf = idx / R, c = idx - sf * R;
            const int s = sf / F, f = sf - s * F;
            float* out;
            bool store;
            if (DIRECT) {
                const int64_t r = ridx[sf];
                if (r < 0) continue;
                const dctr_ffm_grad_t gd = p.grads[f];
                if (!gd.grad) continue;
                out = gd.grad + r * gd.row_stride + c;
                store = p.fields[f].identity != 0;
            } else {
                const uintptr_t dp = dst[sf];
                if (!dp) continue;
                out = reinterpret_cast<float*>(dp & ~(uintptr_t)1) + c;
                store = (dp & 1u) != 0;
            }
            const int k = c / d, e = c - k * d;
            const int i = k < f ? k : k + 1;                    // the partner of slot k
            const int pr = ffb_pair(f, i, F);
            const int at = (f < i ? f : f - 1) * d + e;         // the partner's slot towards f
            const float gv = p.g[(b0 + s) * p.g_stride + (p.reduce ? pr : pr * d + e)];
            float pv = 0.f;
            if (DIRECT) {
                const int64_t ri = ridx[s * F + i];
                if (ri >= 0) {
                    const dctr_ffm_field_t fi = p.fields[i];
                    pv = fi.rows[ri * fi.row_pitch + at];
                }
            } else {
                pv = tile[(size_t)(s * F + i) * R + at];
            }
            const float v = __fmul_rn(gv, pv);
            if (store)
                *out = v;
            else
                unsafeAtomicAdd(out, v);
        }
    }
}

struct FfbPlan {
    bool direct;
    int S;
    size_t lds;
};

// the shape checks: what dctr_ffm_bwd_route answers without looking at a pointer
int ffb_check(const dctr_ffm_bwd_args_t* a) {
    DCTR_REQUIRE(a, DCTR_E_NULL, "ffm_bwd: null args");
    const dctr_ffm_args_t* w = &a->fwd;
    DCTR_REQUIRE(w->n_fields >= 2, DCTR_E_DIM, "ffm_bwd: n_fields = %d: a field pair needs at least 2 fields", w->n_fields);
    DCTR_REQUIRE(w->dim >= 1, DCTR_E_DIM, "ffm_bwd: dim = %d", w->dim);
    DCTR_REQUIRE(w->batch >= 0 && a->d_out_offset >= 0 && a->max_blocks >= 0, DCTR_E_DIM, "ffm_bwd: negative size");
    DCTR_REQUIRE(w->route == DCTR_FFM_ROUTE_AUTO || w->route == DCTR_FFM_ROUTE_DIRECT, DCTR_E_ENUM, "ffm_bwd: unknown route %d", w->route);
    const int64_t F = w->n_fields, d = w->dim, P = F * (F - 1) / 2;
    DCTR_REQUIRE(F <= 65535 && (F - 1) * d < (1LL << 27) && P * d < (1LL << 27), DCTR_E_DIM,
                 "ffm_bwd: n_fields = %d, dim = %d: a row of the output exceeds 2^27 floats", w->n_fields, w->dim);
    DCTR_REQUIRE(w->n_dense == 0, DCTR_E_UNSUPPORTED, "ffm_bwd: n_dense = %d: the dense columns' gradient stays with the caller", w->n_dense);
    return DCTR_OK;
}

void ffb_plan(const dctr_ffm_bwd_args_t* a, FfbPlan* pl) {
    const int F = a->fwd.n_fields, d = a->fwd.dim;
    const size_t per_sample = (size_t)F * (F - 1) * d * 4;
    pl->direct = a->fwd.route == DCTR_FFM_ROUTE_DIRECT || ffb_lds_bytes(F, d, 1, false) > DCTR_LDS_MAX;
    if (pl->direct) {
        int S = FFB_S_DIRECT;       // (per_sample < 2^30 bytes: the kernel's element index stays inside 32 bits)
        while (S > 1 && (ffb_lds_bytes(F, d, S, true) > DCTR_LDS_MAX / 4 || (size_t)S * per_sample >= ((size_t)1 << 32))) S >>= 1;
        pl->S = S;
        pl->lds = ffb_lds_bytes(F, d, S, true);
        return;
    }
    int64_t S = (int64_t)(FFB_TILE_BUDGET / per_sample);
    S = S < 1 ? 1 : S > FFB_S_MAX ? FFB_S_MAX : S;
    if (a->fwd.batch > 0 && S > a->fwd.batch) S = a->fwd.batch;
    while (S > 1 && ffb_lds_bytes(F, d, (int)S, false) > DCTR_LDS_MAX) --S;
    pl->S = (int)S;
    pl->lds = ffb_lds_bytes(F, d, (int)S, false);
}

}  // namespace

extern "C" size_t dctr_ffm_bwd_workspace_bytes(const dctr_ffm_bwd_args_t* args) {
    (void)args;
    return 0;       // both routes keep their state on chip
}

extern "C" int dctr_ffm_bwd_route(const dctr_ffm_bwd_args_t* args) {
    int rc = ffb_check(args);
    if (rc != DCTR_OK) return rc;
    FfbPlan pl;
    ffb_plan(args, &pl);
    DCTR_REQUIRE(pl.lds <= DCTR_LDS_MAX, DCTR_E_DIM, "ffm_bwd: %d fields: the row table alone exceeds the LDS", args->fwd.n_fields);
    return pl.direct ? DCTR_FFM_ROUTE_DIRECT : DCTR_FFM_ROUTE_LDS;
}

extern "C" int dctr_ffm_bwd(const dctr_ffm_bwd_args_t* a, void* stream) {
    int rc = ffb_check(a);
    if (rc != DCTR_OK) return rc;
    const dctr_ffm_args_t* w = &a->fwd;
    DCTR_REQUIRE(!w->scale && !w->shift, DCTR_E_UNSUPPORTED, "ffm_bwd: scale / shift: the BatchNormalization's backward stays with the caller");
    DCTR_REQUIRE(w->fields && a->d_out && a->grads, DCTR_E_NULL, "ffm_bwd: null fields / d_out / grads");
    const int64_t F = w->n_fields, d = w->dim, P = F * (F - 1) / 2;
    const int64_t W = w->reduce_sum ? P : P * d;
    DCTR_REQUIRE(a->d_out_stride >= a->d_out_offset + W, DCTR_E_DIM, "ffm_bwd: d_out_stride %lld < d_out_offset + width = %lld",
                 (long long)a->d_out_stride, (long long)(a->d_out_offset + W));
    DCTR_REQUIRE(!a->workspace || dctr_aligned16(a->workspace), DCTR_E_ALIGN, "ffm_bwd: workspace not 16-B aligned");
    FfbPlan pl;
    ffb_plan(a, &pl);
    DCTR_REQUIRE(pl.lds <= DCTR_LDS_MAX, DCTR_E_DIM, "ffm_bwd: %d fields: the row table alone exceeds the LDS", w->n_fields);
    if (w->batch == 0) return DCTR_OK;
    FfmBwdParams p = {};
    p.fields = w->fields;
    p.grads = a->grads;
    p.batch = w->batch;
    p.F = (int32_t)F;
    p.d = (int32_t)d;
    p.R = (int32_t)((F - 1) * d);
    p.S = pl.S;
    p.reduce = w->reduce_sum ? 1 : 0;
    p.g = a->d_out + a->d_out_offset;
    p.g_stride = a->d_out_stride;
    p.status = w->status;
    p.n_tiles = dctr_ceil_div(w->batch, (int64_t)pl.S);
    const bool vec = d % 4 == 0;
    size_t per_cu = DCTR_LDS_MAX / (pl.lds > 1024 ? pl.lds : 1024);
    per_cu = per_cu < 1 ? 1 : per_cu > 8 ? 8 : per_cu;
    const int64_t cap = (int64_t)dctr_n_cus() * (int64_t)per_cu;
    int64_t grid = p.n_tiles < cap ? p.n_tiles : cap;
    if (a->max_blocks > 0 && grid > a->max_blocks) grid = a->max_blocks;
    const hipStream_t st = (hipStream_t)stream;
    static thread_local size_t granted[4][DCTR_MAX_DEVICES] = {{0}};
    const int which = (pl.direct ? 2 : 0) + (vec ? 1 : 0);
    const void* fn = which == 0   ? (const void*)ffm_bwd_kernel<false, false>
                     : which == 1 ? (const void*)ffm_bwd_kernel<false, true>
                     : which == 2 ? (const void*)ffm_bwd_kernel<true, false>
                                  : (const void*)ffm_bwd_kernel<true, true>;
    hipError_t e = dctr_grant_lds(fn, pl.lds, granted[which]);
    DCTR_REQUIRE(e == hipSuccess, (int)e, "ffm_bwd: cannot raise dynamic LDS: %s", hipGetErrorString(e));
    switch (which) {
        case 0: DCTR_LAUNCH((ffm_bwd_kernel<false, false>), dim3((unsigned)grid), dim3(FFB_THREADS), pl.lds, st, p); break;
        case 1: DCTR_LAUNCH((ffm_bwd_kernel<false, true>), dim3((unsigned)grid), dim3(FFB_THREADS), pl.lds, st, p); break;
        case 2: DCTR_LAUNCH((ffm_bwd_kernel<true, false>), dim3((unsigned)grid), dim3(FFB_THREADS), pl.lds, st, p); break;
        default: DCTR_LAUNCH((ffm_bwd_kernel<true, true>), dim3((unsigned)grid), dim3(FFB_THREADS), pl.lds, st, p); break;
    }
    return dctr_launch_status("dctr_ffm_bwd");
}
