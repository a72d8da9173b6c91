// ONN's sparse path (reference deepctr/models/onn.py:59-99): field-aware embeddings gathered and multiplied pair by pair, one launch
// from the ids to the model's whole DNN-input row.
//
// Feature j owns ONE fused table [V_j, F-1, d]: row r holds the embeddings of id r towards every partner field, slot k = partner i in
// field order with j itself skipped (slot(i) = i for i < j, i - 1 for i > j).  Per sample and pair (i < j, itertools.combinations order)
//     out[p, e] = row_i[slot j = j - 1][e] * row_j[slot i = i][e]            (reduce_sum: summed over e into one scalar)
// then the inference form of BatchNormalization (scale / shift per output column), then the dense values behind the P*d (or P) columns.
//
// LDS route: a workgroup walks tiles of S samples.  Phase 0 resolves the S*F row addresses (id load, range check, pre-pooled fields:
// row = sample index) into LDS; phase 1 gathers the S*F whole rows — contiguous (F-1)*d*4 bytes each — with 16-B loads, four in flight
// per lane, into an LDS tile, so every table byte crosses the memory system once and coalesced; phase 2 forms each output element from
// two LDS reads (16 B per lane when d % 4 == 0) and stores contiguous runs of the output row.  S comes from an LDS budget that keeps
// several workgroups per CU, whose phases overlap each other (one tile's gather under another's products).
// Direct route: samples whose rows exceed the LDS (and the comparison point): the same phase 0, then every lane reads its two operands
// from global memory through the resolved row addresses; L2 serves the re-use of a row's lines.  Same arithmetic, same bits.
// An id outside [0, vocab) raises DCTR_STATUS_INDEX_OOR and contributes a row of zeros: nothing outside the tables is read.
#include <math.h>
#include <stdint.h>
#include "dctr_common.h"
#include "tile_route.h"

namespace {

constexpr int FFM_THREADS = 256;
constexpr size_t FFM_TILE_BUDGET = 40 * 1024;    // target bytes of a tile: >= 3 workgroups per CU
constexpr int FFM_S_MAX = 32;
constexpr int FFM_S_DIRECT = 8;

struct FfmParams {
    const dctr_ffm_field_t* fields;
    int64_t batch;
    int32_t F, d, R, S;          // R = (F-1)*d floats per fused row; S samples per tile
    int32_t P, W;                // pairs; output columns of the pair block (P*d or P)
    int32_t reduce, n_dense;
    const float* scale;
    const float* shift;
    const float* dense;
    int64_t dense_stride;
    float* out;                  // already advanced by out_offset
    int64_t out_stride;
    int32_t* status;
    int64_t n_tiles;
};

// offsets (bytes) inside a workgroup's dynamic LDS
struct FfmLayout {
    size_t rowptr, pairs, tile, total;
};

inline FfmLayout ffm_layout(int F, int d, int S, bool direct) {
    FfmLayout l;
    const size_t R = (size_t)(F - 1) * d, P = (size_t)F * (F - 1) / 2;
    l.rowptr = 0;
    l.pairs = (size_t)S * F * 8;
    l.tile = (l.pairs + (direct ? 0 : P * 4) + 15) & ~(size_t)15;
    l.total = l.tile + (direct ? 0 : (size_t)S * F * R * 4);
    return l;
}

// pair index p -> (i, j), i < j, itertools.combinations order: pairs before row i = i (2F - i - 1) / 2
__device__ inline void ffm_pair_of(int p, int F, int& i, int& j) {
    const double b = 2.0 * F - 1.0;
    int g = (int)((b - sqrt(b * b - 8.0 * (double)p)) * 0.5);
    g = g < 0 ? 0 : (g > F - 2 ? F - 2 : g);
    while (g > 0 && (int64_t)g * (2 * F - g - 1) / 2 > p) --g;
    while (g < F - 2 && (int64_t)(g + 1) * (2 * F - g - 2) / 2 <= p) ++g;
    i = g;
    j = p - (int)((int64_t)g * (2 * F - g - 1) / 2) + g + 1;
}

// one output element: the fp32 product, then (scale != NULL) one fma — the same two roundings on both routes
__device__ inline float ffm_finish(float v, const float* scale, const float* shift, int o) {
    return scale ? fmaf(v, scale[o], shift[o]) : v;
}

template <bool DIRECT, bool VEC>
__global__ void __launch_bounds__(FFM_THREADS) ffm_kernel(FfmParams p) {
    extern __shared__ __align__(16) unsigned char ffm_smem[];
    const int F = p.F, d = p.d, R = p.R, S = p.S;
    const size_t pairs_off = (size_t)S * F * 8;
    const float** rowptr = reinterpret_cast<const float**>(ffm_smem);
    uint32_t* pairs = reinterpret_cast<uint32_t*>(ffm_smem + pairs_off);
    const size_t tile_off = (pairs_off + (DIRECT ? 0 : (size_t)p.P * 4) + 15) & ~(size_t)15;
    float* tile = reinterpret_cast<float*>(ffm_smem + tile_off);
    const int tid = threadIdx.x;

    if (!DIRECT) {
        // the pair table, once per workgroup: thread t fills row i = t, t + 256, ...
        for (int i = tid; i < F - 1; i += FFM_THREADS) {
            const int base = (int)((int64_t)i * (2 * F - i - 1) / 2);
            for (int j = i + 1; j < F; ++j) pairs[base + j - i - 1] = ((uint32_t)i << 16) | (uint32_t)j;
        }
    }

    for (int64_t t = blockIdx.x; t < p.n_tiles; t += gridDim.x) {
        const int64_t b0 = t * S;
        const int nvalid = (int)((p.batch - b0) < S ? (p.batch - b0) : S);
        __syncthreads();        // the previous tile's readers are done with rowptr / tile (and the pair table is written)
        // ---- phase 0: row addresses --------------------------------------------------------------------------------------------
        for (int sf = tid; sf < S * F; sf += FFM_THREADS) {
            const int s = sf / F, f = sf - s * F;
            const float* ptr = nullptr;
            if (s < nvalid) {
                const dctr_ffm_field_t fd = p.fields[f];
                const int64_t b = b0 + s;
                int64_t r = b;
                if (!fd.identity)
                    r = fd.ids_is_i64 ? ((const int64_t*)fd.ids)[b * fd.ids_stride] : (int64_t)((const int32_t*)fd.ids)[b * fd.ids_stride];
                if (r >= 0 && r < fd.vocab)
                    ptr = fd.rows + r * fd.row_pitch;
                else if (p.status)
                    atomicOr(p.status, DCTR_STATUS_INDEX_OOR);
            }
            rowptr[sf] = ptr;
        }
        __syncthreads();
        // ---- phase 1 (LDS route): the S*F whole rows into the tile -------------------------------------------------------------
        if (!DIRECT) {
            if (VEC) {
                const int C = R >> 2, n = nvalid * F * C;
                for (int base = tid; base < n; base += 4 * FFM_THREADS) {
                    float4 v[4];
                    int dst[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int idx = base + u * FFM_THREADS;
                        dst[u] = -1;
                        v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                        if (idx < n) {
                            const int sf = idx / C, c = idx - sf * C;
                            dst[u] = sf * R + 4 * c;
                            const float* src = rowptr[sf];
                            if (src) {
                                src += 4 * c;
                                if ((reinterpret_cast<uintptr_t>(src) & 15u) == 0)
                                    v[u] = *reinterpret_cast<const float4*>(src);
                                else
                                    v[u] = make_float4(src[0], src[1], src[2], src[3]);
                            }
                        }
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (dst[u] >= 0) *reinterpret_cast<float4*>(tile + dst[u]) = v[u];
                }
            } else {
                const int n = nvalid * F * R;
                for (int idx = tid; idx < n; idx += FFM_THREADS) {
                    const int sf = idx / R, c = idx - sf * R;
                    const float* src = rowptr[sf];
                    tile[idx] = src ? src[c] : 0.f;
                }
            }
            __syncthreads();
        }
        // ---- phase 2: products -------------------------------------------------------------------------------------------------
        if (p.reduce) {
            const int n = nvalid * p.P;
            for (int idx = tid; idx < n; idx += FFM_THREADS) {
                const int s = idx / p.P, pr = idx - s * p.P;
                int i, j;
                if (DIRECT) {
                    ffm_pair_of(pr, F, i, j);
                } else {
                    const uint32_t ij = pairs[pr];
                    i = (int)(ij >> 16);
                    j = (int)(ij & 0xffffu);
                }
                float acc = 0.f;
                if (DIRECT) {
                    const float* a = rowptr[s * F + i];
                    const float* b = rowptr[s * F + j];
                    if (a && b) {
                        a += (size_t)(j - 1) * d;
                        b += (size_t)i * d;
                        for (int e = 0; e < d; ++e) acc = fmaf(a[e], b[e], acc);
                    }
                } else {
                    const float* a = tile + (size_t)(s * F + i) * R + (size_t)(j - 1) * d;
                    const float* b = tile + (size_t)(s * F + j) * R + (size_t)i * d;
                    for (int e = 0; e < d; ++e) acc = fmaf(a[e], b[e], acc);
                }
                p.out[(b0 + s) * p.out_stride + pr] = ffm_finish(acc, p.scale, p.shift, pr);
            }
        } else if (VEC) {
            const int n4 = p.W >> 2, dq = d >> 2, n = nvalid * n4;
            for (int idx = tid; idx < n; idx += FFM_THREADS) {
                const int s = idx / n4, o4 = idx - s * n4;
                const int pr = o4 / dq, e = (o4 - pr * dq) << 2, o = o4 << 2;
                int i, j;
                if (DIRECT) {
                    ffm_pair_of(pr, F, i, j);
                } else {
                    const uint32_t ij = pairs[pr];
                    i = (int)(ij >> 16);
                    j = (int)(ij & 0xffffu);
                }
                float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
                if (DIRECT) {
                    const float* pa = rowptr[s * F + i];
                    const float* pb = rowptr[s * F + j];
                    if (pa) {
                        pa += (size_t)(j - 1) * d + e;
                        a = (reinterpret_cast<uintptr_t>(pa) & 15u) == 0 ? *reinterpret_cast<const float4*>(pa)
                                                                          : make_float4(pa[0], pa[1], pa[2], pa[3]);
                    }
                    if (pb) {
                        pb += (size_t)i * d + e;
                        b = (reinterpret_cast<uintptr_t>(pb) & 15u) == 0 ? *reinterpret_cast<const float4*>(pb)
                                                                          : make_float4(pb[0], pb[1], pb[2], pb[3]);
                    }
                } else {
                    a = *reinterpret_cast<const float4*>(tile + (size_t)(s * F + i) * R + (size_t)(j - 1) * d + e);
                    b = *reinterpret_cast<const float4*>(tile + (size_t)(s * F + j) * R + (size_t)i * d + e);
                }
                float4 r;
                r.x = ffm_finish(__fmul_rn(a.x, b.x), p.scale, p.shift, o);
                r.y = ffm_finish(__fmul_rn(a.y, b.y), p.scale, p.shift, o + 1);
                r.z = ffm_finish(__fmul_rn(a.z, b.z), p.scale, p.shift, o + 2);
                r.w = ffm_finish(__fmul_rn(a.w, b.w), p.scale, p.shift, o + 3);
                float* dst = p.out + (b0 + s) * p.out_stride + o;
                if ((reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
                    *reinterpret_cast<float4*>(dst) = r;
                } else {
                    dst[0] = r.x;
                    dst[1] = r.y;
                    dst[2] = r.z;
                    dst[3] = r.w;
                }
            }
        } else {
            const int n = nvalid * p.W;
            for (int idx = tid; idx < n; idx += FFM_THREADS) {
                const int s = idx / p.W, o = idx - s * p.W;
                const int pr = o / d, e = o - pr * d;
                int i, j;
                if (DIRECT) {
                    ffm_pair_of(pr, F, i, j);
                } else {
                    const uint32_t ij = pairs[pr];
                    i = (int)(ij >> 16);
                    j = (int)(ij & 0xffffu);
                }
                float a = 0.f, b = 0.f;
                if (DIRECT) {
                    const float* pa = rowptr[s * F + i];
                    const float* pb = rowptr[s * F + j];
                    if (pa) a = pa[(size_t)(j - 1) * d + e];
                    if (pb) b = pb[(size_t)i * d + e];
                } else {
                    a = tile[(size_t)(s * F + i) * R + (size_t)(j - 1) * d + e];
                    b = tile[(size_t)(s * F + j) * R + (size_t)i * d + e];
                }
                p.out[(b0 + s) * p.out_stride + o] = ffm_finish(__fmul_rn(a, b), p.scale, p.shift, o);
            }
        }
        // ---- the dense values behind the pair block ----------------------------------------------------------------------------
        if (p.n_dense > 0) {
            const int n = nvalid * p.n_dense;
            for (int idx = tid; idx < n; idx += FFM_THREADS) {
                const int s = idx / p.n_dense, k = idx - s * p.n_dense;
                p.out[(b0 + s) * p.out_stride + p.W + k] = p.dense[(b0 + s) * p.dense_stride + k];
            }
        }
    }
}

struct FfmPlan {
    bool direct;
    int S;
    size_t lds;
};

int ffm_check(const dctr_ffm_args_t* a) {
    DCTR_REQUIRE(a, DCTR_E_NULL, "ffm_fwd: null args");
    DCTR_REQUIRE(a->n_fields >= 2, DCTR_E_DIM, "ffm_fwd: n_fields = %d: a field pair needs at least 2 fields", a->n_fields);
    DCTR_REQUIRE(a->dim >= 1, DCTR_E_DIM, "ffm_fwd: dim = %d", a->dim);
    DCTR_REQUIRE(a->batch >= 0 && a->n_dense >= 0 && a->out_offset >= 0, DCTR_E_DIM, "ffm_fwd: negative size");
    DCTR_REQUIRE(a->route == DCTR_FFM_ROUTE_AUTO || a->route == DCTR_FFM_ROUTE_DIRECT, DCTR_E_ENUM, "ffm_fwd: unknown route %d", a->route);
    const int64_t F = a->n_fields, d = a->dim, P = F * (F - 1) / 2;
    // pair table entries are 16 + 16 bits; rows and output rows are indexed in 32 bits
    DCTR_REQUIRE(F <= 65535 && (F - 1) * d < (1LL << 27) && P * d < (1LL << 27), DCTR_E_DIM,
                 "ffm_fwd: n_fields = %d, dim = %d: a row of the output exceeds 2^27 floats", a->n_fields, a->dim);
    const int64_t W = a->reduce_sum ? P : P * d;
    DCTR_REQUIRE(a->out_stride % 4 == 0, DCTR_E_ALIGN, "ffm_fwd: out_stride %lld is not a multiple of 4 floats", (long long)a->out_stride);
    DCTR_REQUIRE(a->out_stride >= a->out_offset + W + a->n_dense, DCTR_E_DIM, "ffm_fwd: out_stride %lld < out_offset + width = %lld",
                 (long long)a->out_stride, (long long)(a->out_offset + W + a->n_dense));
    DCTR_REQUIRE(a->n_dense == 0 || a->dense_stride >= a->n_dense, DCTR_E_DIM, "ffm_fwd: dense_stride %lld < n_dense %d",
                 (long long)a->dense_stride, a->n_dense);
    return DCTR_OK;
}

void ffm_plan(const dctr_ffm_args_t* a, FfmPlan* pl) {
    const int F = a->n_fields, d = a->dim;
    const size_t per_sample = (size_t)F * (F - 1) * d * 4;
    pl->direct = a->route == DCTR_FFM_ROUTE_DIRECT || ffm_layout(F, d, 1, false).total > DCTR_LDS_MAX;
    if (pl->direct) {
        int S = FFM_S_DIRECT;
        while (S > 1 && ffm_layout(F, d, S, true).total > DCTR_LDS_MAX / 4) S >>= 1;
        pl->S = S;
        pl->lds = ffm_layout(F, d, S, true).total;
        return;
    }
    int64_t S = (int64_t)(FFM_TILE_BUDGET / per_sample);
    S = S < 1 ? 1 : S > FFM_S_MAX ? FFM_S_MAX : S;
    if (a->batch > 0 && S > a->batch) S = a->batch;
    while (S > 1 && ffm_layout(F, d, (int)S, false).total > DCTR_LDS_MAX) --S;
    pl->S = (int)S;
    pl->lds = ffm_layout(F, d, (int)S, false).total;
}

}  // namespace

extern "C" size_t dctr_ffm_workspace_bytes(const dctr_ffm_args_t* args) {
    (void)args;
    return 0;       // both routes keep their state on chip
}

extern "C" int dctr_ffm_route(const dctr_ffm_args_t* args) {
    int rc = ffm_check(args);
    if (rc != DCTR_OK) return rc;
    FfmPlan pl;
    ffm_plan(args, &pl);
    DCTR_REQUIRE(pl.lds <= DCTR_LDS_MAX, DCTR_E_DIM, "ffm_fwd: %d fields: the row-address table alone exceeds the LDS", args->n_fields);
    return pl.direct ? DCTR_FFM_ROUTE_DIRECT : DCTR_FFM_ROUTE_LDS;
}

extern "C" int dctr_ffm_fwd(const dctr_ffm_args_t* a, void* stream) {
    int rc = ffm_check(a);
    if (rc != DCTR_OK) return rc;
    DCTR_REQUIRE(a->fields && a->out, DCTR_E_NULL, "ffm_fwd: null fields / out");
    DCTR_REQUIRE((a->scale != nullptr) == (a->shift != nullptr), DCTR_E_NULL, "ffm_fwd: scale and shift come together");
    DCTR_REQUIRE(a->n_dense == 0 || a->dense, DCTR_E_NULL, "ffm_fwd: n_dense = %d without a dense matrix", a->n_dense);
    DCTR_REQUIRE(!a->workspace || dctr_aligned16(a->workspace), DCTR_E_ALIGN, "ffm_fwd: workspace not 16-B aligned");
    FfmPlan pl;
    ffm_plan(a, &pl);
    DCTR_REQUIRE(pl.lds <= DCTR_LDS_MAX, DCTR_E_DIM, "ffm_fwd: %d fields: the row-address table alone exceeds the LDS", a->n_fields);
    if (a->batch == 0) return DCTR_OK;
    const int64_t F = a->n_fields, d = a->dim, P = F * (F - 1) / 2;
    FfmParams p = {};
    p.fields = a->fields;
    p.batch = a->batch;
    p.F = (int32_t)F;
    p.d = (int32_t)d;
    p.R = (int32_t)((F - 1) * d);
    p.S = pl.S;
    p.P = (int32_t)P;
    p.W = (int32_t)(a->reduce_sum ? P : P * d);
    p.reduce = a->reduce_sum ? 1 : 0;
    p.n_dense = a->n_dense;
    p.scale = a->scale;
    p.shift = a->shift;
    p.dense = a->dense;
    p.dense_stride = a->dense_stride;
    p.out = a->out + a->out_offset;
    p.out_stride = a->out_stride;
    p.status = a->status;
    p.n_tiles = dctr_ceil_div(a->batch, (int64_t)pl.S);
    const bool vec = d % 4 == 0;
    size_t per_cu = DCTR_LDS_MAX / (pl.lds > 1024 ? pl.lds : 1024);
    per_cu = per_cu < 1 ? 1 : per_cu > 8 ? 8 : per_cu;
    const int64_t cap = (int64_t)dctr_n_cus() * (int64_t)per_cu;
    const int64_t grid = p.n_tiles < cap ? p.n_tiles : cap;
    const hipStream_t st = (hipStream_t)stream;
    static thread_local size_t granted[4][DCTR_MAX_DEVICES] = {{0}};
    const int which = (pl.direct ? 2 : 0) + (vec ? 1 : 0);
    const void* fn = which == 0   ? (const void*)ffm_kernel<false, false>
                     : which == 1 ? (const void*)ffm_kernel<false, true>
                     : which == 2 ? (const void*)ffm_kernel<true, false>
                                  : (const void*)ffm_kernel<true, true>;
    hipError_t e = dctr_grant_lds(fn, pl.lds, granted[which]);
    DCTR_REQUIRE(e == hipSuccess, (int)e, "ffm_fwd: cannot raise dynamic LDS: %s", hipGetErrorString(e));
    switch (which) {
        case 0: DCTR_LAUNCH((ffm_kernel<false, false>), dim3((unsigned)grid), dim3(FFM_THREADS), pl.lds, st, p); break;
        case 1: DCTR_LAUNCH((ffm_kernel<false, true>), dim3((unsigned)grid), dim3(FFM_THREADS), pl.lds, st, p); break;
        case 2: DCTR_LAUNCH((ffm_kernel<true, false>), dim3((unsigned)grid), dim3(FFM_THREADS), pl.lds, st, p); break;
        default: DCTR_LAUNCH((ffm_kernel<true, true>), dim3((unsigned)grid), dim3(FFM_THREADS), pl.lds, st, p); break;
    }
    return dctr_launch_status("dctr_ffm_fwd");
}
