// FieldWiseBiInteraction of FLEN (reference deepctr/layers/interaction.py:1224-1348), forward and backward.
//
// Per sample, elementwise over the d embedding columns, G groups of fields (group g: n_g fields from column first_g):
//     s_g = sum_f x_f,  q_g = sum_f x_f^2
//     y   = (sum_{i<j} w[p(i,j)] s_i s_j + bias_mf) + (sum_g k[g] (s_g^2 - q_g) + bias_fm)
//     logit = y . head_w (+ add)
//
// A thread owns one sample and V adjacent columns (V = 4: 16-byte loads; V = 1 where d, an offset or a stride is no multiple of 4
// floats).  The lanes of a sample are nvp = pow2(d / V) <= 64 neighbours of one wave, so a wave instruction reads nvp * V contiguous
// floats of 64 / nvp samples; wider d is walked in chunks of nvp * V columns.  The thread walks the groups once: s and q in registers,
// the FM term at the end of a group, the MF term as s_g * (sum_{i<g} w[p(i,g)] s_i) with the earlier s_i in the thread's own LDS slots
// (route ON_CHIP) or summed again from x (route REREAD: more groups than the LDS holds) — the same additions in the same order.  The
// group table and the weights are wave-uniform reads.  The forward has no atomics and no barrier.
//
// Backward: the same walk (pass 1: s_g to LDS, the weight-gradient terms), then per group ds_g and the dx of its fields (pass 2: x is
// read a second time, from cache).  A weight-gradient term is summed over the wave in shuffles, over the workgroup in LDS accumulators
// (which persist over the tiles a workgroup walks), and leaves with one atomic per workgroup and destination.
#include <stdint.h>
#include "dctr_common.h"

namespace {

constexpr int FW_MAX_THREADS = 256;
constexpr size_t FW_LDS_SOFT = 64 * 1024;         // a block size is chosen to stay below this where one can
constexpr size_t FW_LDS_MAX = 128 * 1024;

struct FwParams {
    int64_t batch;
    const float* x;               // already advanced by x_offset
    int64_t x_stride;
    const dctr_fieldwise_group_t* groups;
    int32_t G, d, nv, nvp;        // nv: column vectors of a sample; nvp: lanes of a sample
    const float* kernel_mf;
    const float* kernel_fm;
    const float* bias_mf;
    const float* bias_fm;
    float* y;                     // already advanced by y_offset
    int64_t y_stride;
    const float* head_w;
    const float* add;
    float* logit;
    // backward
    const float* dy;
    int64_t dy_stride;
    const float* dlogit;
    float* dx;                    // already advanced by dx_offset
    int64_t dx_stride;
    int32_t accumulate;
    int64_t n_tiles;
    float* d_kernel_mf;
    float* d_kernel_fm;
    float* d_bias_mf;
    float* d_bias_fm;
    float* d_head_w;
};

template <int V>
__device__ __forceinline__ void fw_load(float (&v)[V], const float* p) {
    if constexpr (V == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        v[0] = *p;
    }
}

template <int V>
__device__ __forceinline__ void fw_store(float* p, const float (&v)[V]) {
    if constexpr (V == 4) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        *p = v[0];
    }
}

// s (and q) of one group for the thread's columns: xg = the group's first field at the thread's columns
template <int V, bool WITH_Q>
__device__ __forceinline__ void fw_group_sums(const float* xg, int n, int d, float (&s)[V], float (&q)[V]) {
#pragma unroll
    for (int k = 0; k < V; ++k) s[k] = q[k] = 0.f;
#pragma unroll 4
    for (int f = 0; f < n; ++f) {
        float v[V];
        fw_load<V>(v, xg + (int64_t)f * d);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            s[k] += v[k];
            if (WITH_Q) q[k] = fmaf(v[k], v[k], q[k]);
        }
    }
}

// index of the pair (i, j), i < j, in itertools.combinations(range(G), 2) order
__device__ __forceinline__ int64_t fw_pair(int64_t i, int64_t j, int64_t G) { return i * (2 * G - i - 1) / 2 + (j - i - 1); }

__device__ __forceinline__ float fw_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// y of the thread's columns [col, col + V) of sample row xr; S: the thread's LDS slots (pitch floats between groups), ON_CHIP only
template <int V, bool ON_CHIP>
__device__ __forceinline__ void fw_row(const FwParams& p, const float* xr, int col, float* S, int pitch, float (&y)[V]) {
    const int G = p.G, d = p.d;
    float mf[V], fm[V];
#pragma unroll
    for (int k = 0; k < V; ++k) mf[k] = fm[k] = 0.f;
    for (int g = 0; g < G; ++g) {
        const dctr_fieldwise_group_t grp = p.groups[g];
        float s[V], q[V], t[V];
        fw_group_sums<V, true>(xr + grp.first + col, grp.n_fields, d, s, q);
        const float kg = p.kernel_fm[g];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            fm[k] = fmaf(kg, fmaf(s[k], s[k], -q[k]), fm[k]);
            t[k] = 0.f;
        }
        for (int i = 0; i < g; ++i) {
            const float w = p.kernel_mf[fw_pair(i, g, G)];
            float si[V];
            if (ON_CHIP) {
                fw_load<V>(si, S + (size_t)i * pitch);
            } else {
                const dctr_fieldwise_group_t gi = p.groups[i];
                float unused[V];
                fw_group_sums<V, false>(xr + gi.first + col, gi.n_fields, d, si, unused);
            }
#pragma unroll
            for (int k = 0; k < V; ++k) t[k] = fmaf(w, si[k], t[k]);
        }
#pragma unroll
        for (int k = 0; k < V; ++k) mf[k] = fmaf(s[k], t[k], mf[k]);
        if (ON_CHIP) fw_store<V>(S + (size_t)g * pitch, s);
    }
#pragma unroll
    for (int k = 0; k < V; ++k)
        y[k] = (mf[k] + (p.bias_mf ? p.bias_mf[col + k] : 0.f)) + (fm[k] + (p.bias_fm ? p.bias_fm[col + k] : 0.f));
}

template <int V, bool ON_CHIP>
__global__ void __launch_bounds__(FW_MAX_THREADS) fieldwise_fwd_kernel(FwParams p) {
    extern __shared__ __align__(16) float fw_smem[];
    const int T = blockDim.x, tid = threadIdx.x;
    const int r = tid / p.nvp, cv = tid - r * p.nvp;
    const int64_t b = (int64_t)blockIdx.x * (T / p.nvp) + r;
    const bool row_on = b < p.batch;
    float acc = 0.f;
    if (row_on) {
        const float* xr = p.x + b * p.x_stride;
        for (int cq = cv; cq < p.nv; cq += p.nvp) {
            const int col = cq * V;
            float y[V];
            fw_row<V, ON_CHIP>(p, xr, col, fw_smem + (size_t)tid * V, T * V, y);
            if (p.y) {
#pragma unroll
                for (int k = 0; k < V; ++k) p.y[b * p.y_stride + col + k] = y[k];
            }
            if (p.logit) {
#pragma unroll
                for (int k = 0; k < V; ++k) acc = fmaf(y[k], p.head_w[col + k], acc);
            }
        }
    }
    if (p.logit) {                      // (wave-uniform: every lane takes part in the shuffles)
        for (int o = p.nvp >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        if (row_on && cv == 0) p.logit[b] = p.add ? acc + p.add[b] : acc;
    }
}

template <int V>
__global__ void __launch_bounds__(FW_MAX_THREADS) fieldwise_bwd_kernel(FwParams p) {
    extern __shared__ __align__(16) float fw_smem[];
    const int T = blockDim.x, tid = threadIdx.x, lane = tid & 63;
    const int G = p.G, d = p.d, nvp = p.nvp;
    const int64_t P = (int64_t)G * (G - 1) / 2;
    const int pitch = T * V;
    float* S = fw_smem + (size_t)tid * V;
    float* acc_mf = fw_smem + (size_t)G * pitch;
    float* acc_fm = acc_mf + P;
    float* acc_b = acc_fm + G;
    float* acc_h = acc_b + d;
    for (int64_t i = tid; i < P + G + 2 * (int64_t)d; i += T) acc_mf[i] = 0.f;
    __syncthreads();
    const int r = tid / nvp, cv = tid - r * nvp, rows = T / nvp;
    const bool want_mf = p.d_kernel_mf != nullptr, want_fm = p.d_kernel_fm != nullptr;
    const bool want_b = p.d_bias_mf != nullptr || p.d_bias_fm != nullptr, want_h = p.d_head_w != nullptr && p.dlogit != nullptr;
    for (int64_t tile = blockIdx.x; tile < p.n_tiles; tile += gridDim.x) {
        const int64_t b = tile * rows + r;
        const bool row_on = b < p.batch;
        const float* xr = p.x + (row_on ? b : 0) * p.x_stride;
        const float dl = (row_on && p.dlogit) ? p.dlogit[b] : 0.f;
        for (int cq0 = 0; cq0 < p.nv; cq0 += nvp) {         // (the same trips for every thread: the shuffles below are wave-wide)
            const int cq = cq0 + cv, col = cq * V;
            const bool on = row_on && cq < p.nv;
            float dyv[V], mf[V], fm[V];
#pragma unroll
            for (int k = 0; k < V; ++k) {
                dyv[k] = !on ? 0.f : (p.dy ? p.dy[b * p.dy_stride + col + k] : dl * p.head_w[col + k]);
                mf[k] = fm[k] = 0.f;
            }
            // ---- pass 1: the group sums, y, the gradients of kernel_mf / kernel_fm -----------------------------------------------
            for (int g = 0; g < G; ++g) {
                const dctr_fieldwise_group_t grp = p.groups[g];
                float s[V], q[V], t[V];
                if (on) {
                    fw_group_sums<V, true>(xr + grp.first + col, grp.n_fields, d, s, q);
                } else {
#pragma unroll
                    for (int k = 0; k < V; ++k) s[k] = q[k] = 0.f;
                }
                fw_store<V>(S + (size_t)g * pitch, s);
                const float kg = p.kernel_fm[g];
                float a = 0.f;
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    const float u = fmaf(s[k], s[k], -q[k]);
                    fm[k] = fmaf(kg, u, fm[k]);
                    a = fmaf(dyv[k], u, a);
                    t[k] = 0.f;
                }
                if (want_fm) {
                    a = fw_wave_sum(a);
                    if (lane == 0) atomicAdd(&acc_fm[g], a);
                }
                for (int i = 0; i < g; ++i) {
                    const int64_t pi = fw_pair(i, g, G);
                    const float w = p.kernel_mf[pi];
                    float si[V];
                    fw_load<V>(si, S + (size_t)i * pitch);
                    float c = 0.f;
#pragma unroll
                    for (int k = 0; k < V; ++k) {
                        t[k] = fmaf(w, si[k], t[k]);
                        c = fmaf(dyv[k] * si[k], s[k], c);
                    }
                    if (want_mf) {
                        c = fw_wave_sum(c);
                        if (lane == 0) atomicAdd(&acc_mf[pi], c);
                    }
                }
#pragma unroll
                for (int k = 0; k < V; ++k) mf[k] = fmaf(s[k], t[k], mf[k]);
            }
            // ---- the bias and head gradients: sums over the samples of a column, first over the wave's samples ---------------------
            if (want_b || want_h) {
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    float vb = dyv[k];
                    float vh = !on ? 0.f : dl * ((mf[k] + (p.bias_mf ? p.bias_mf[col + k] : 0.f)) + (fm[k] + (p.bias_fm ? p.bias_fm[col + k] : 0.f)));
                    for (int o = nvp; o < 64; o <<= 1) {
                        vb += __shfl_xor(vb, o, 64);
                        vh += __shfl_xor(vh, o, 64);
                    }
                    if (lane < nvp && cq < p.nv) {
                        if (want_b) atomicAdd(&acc_b[col + k], vb);
                        if (want_h) atomicAdd(&acc_h[col + k], vh);
                    }
                }
            }
            // ---- pass 2: ds_g = dy (sum_{j != g} w_gj s_j + 2 k_g s_g), dx_f = ds_g - 2 k_g dy x_f ----------------------------------
            if (on && p.dx) {
                float* dxr = p.dx + b * p.dx_stride;
                for (int g = 0; g < G; ++g) {
                    const dctr_fieldwise_group_t grp = p.groups[g];
                    const float k2 = 2.f * p.kernel_fm[g];
                    float t[V], ds[V], m2[V];
#pragma unroll
                    for (int k = 0; k < V; ++k) t[k] = 0.f;
                    for (int j = 0; j < G; ++j) {
                        const float w = j == g ? k2 : p.kernel_mf[j < g ? fw_pair(j, g, G) : fw_pair(g, j, G)];
                        float sj[V];
                        fw_load<V>(sj, S + (size_t)j * pitch);
#pragma unroll
                        for (int k = 0; k < V; ++k) t[k] = fmaf(w, sj[k], t[k]);
                    }
#pragma unroll
                    for (int k = 0; k < V; ++k) {
                        ds[k] = dyv[k] * t[k];
                        m2[k] = -k2 * dyv[k];
                    }
                    const int64_t c0 = grp.first + col;
#pragma unroll 2
                    for (int f = 0; f < grp.n_fields; ++f) {
                        float v[V], o[V];
                        fw_load<V>(v, xr + c0 + (int64_t)f * d);
                        if (p.accumulate) {
                            fw_load<V>(o, dxr + c0 + (int64_t)f * d);
#pragma unroll
                            for (int k = 0; k < V; ++k) o[k] += fmaf(m2[k], v[k], ds[k]);
                        } else {
#pragma unroll
                            for (int k = 0; k < V; ++k) o[k] = fmaf(m2[k], v[k], ds[k]);
                        }
                        fw_store<V>(dxr + c0 + (int64_t)f * d, o);
                    }
                }
            }
        }
    }
    __syncthreads();
    // one atomic per workgroup and destination
    for (int64_t i = tid; i < P; i += T)
        if (want_mf) atomicAdd(&p.d_kernel_mf[i], acc_mf[i]);
    for (int i = tid; i < G; i += T)
        if (want_fm) atomicAdd(&p.d_kernel_fm[i], acc_fm[i]);
    for (int i = tid; i < d; i += T) {
        if (p.d_bias_mf) atomicAdd(&p.d_bias_mf[i], acc_b[i]);
        if (p.d_bias_fm) atomicAdd(&p.d_bias_fm[i], acc_b[i]);
        if (want_h) atomicAdd(&p.d_head_w[i], acc_h[i]);
    }
}

struct FwPlan {
    int V;                 // columns of a thread
    int nv, nvp;
    int threads;
    bool on_chip;
    size_t lds;
};

inline bool fw_mult4(int64_t v) { return (v & 3) == 0; }

int fieldwise_check(const dctr_fieldwise_args_t* a, const char* what) {
    DCTR_REQUIRE(a, DCTR_E_NULL, "%s: null args", what);
    DCTR_REQUIRE(a->batch >= 0, DCTR_E_DIM, "%s: negative batch", what);
    DCTR_REQUIRE(a->n_groups >= 2 && a->n_groups < (1 << 20), DCTR_E_DIM, "%s: n_groups = %d: at least 2 groups (below 2^20)", what,
                 a->n_groups);
    DCTR_REQUIRE(a->dim >= 1, DCTR_E_DIM, "%s: dim = %d", what, a->dim);
    DCTR_REQUIRE(a->x_offset >= 0 && a->x_stride >= 0, DCTR_E_DIM, "%s: negative x_offset / x_stride", what);
    DCTR_REQUIRE(a->groups_host, DCTR_E_NULL, "%s: null groups_host", what);
    for (int g = 0; g < a->n_groups; ++g) {
        const dctr_fieldwise_group_t& gr = a->groups_host[g];
        DCTR_REQUIRE(gr.n_fields >= 1 && gr.first >= 0, DCTR_E_DIM, "%s: group %d: first = %lld, n_fields = %d", what, g,
                     (long long)gr.first, gr.n_fields);
        DCTR_REQUIRE(a->x_offset + gr.first + (int64_t)gr.n_fields * a->dim <= a->x_stride, DCTR_E_DIM,
                     "%s: group %d ends at column %lld of rows of %lld", what, g,
                     (long long)(a->x_offset + gr.first + (int64_t)gr.n_fields * a->dim), (long long)a->x_stride);
    }
    DCTR_REQUIRE(a->route == DCTR_FIELDWISE_ROUTE_AUTO || a->route == DCTR_FIELDWISE_ROUTE_REREAD, DCTR_E_ENUM, "%s: unknown route %d",
                 what, a->route);
    DCTR_REQUIRE(a->max_blocks >= 0, DCTR_E_DIM, "%s: max_blocks = %d", what, a->max_blocks);
    return DCTR_OK;
}

// extra: LDS floats beside the group sums (the backward's accumulators); vec_ok: the caller's further 16-byte conditions
void fieldwise_plan(const dctr_fieldwise_args_t* a, size_t extra, bool vec_ok, FwPlan* pl) {
    bool v4 = vec_ok && fw_mult4(a->dim) && fw_mult4(a->x_stride) && fw_mult4(a->x_offset) && dctr_aligned16(a->x);
    for (int g = 0; v4 && g < a->n_groups; ++g) v4 = fw_mult4(a->groups_host[g].first);
    pl->V = v4 ? 4 : 1;
    pl->nv = a->dim / pl->V;
    pl->nvp = 1;
    while (pl->nvp < pl->nv && pl->nvp < 64) pl->nvp <<= 1;
    pl->on_chip = false;
    pl->threads = FW_MAX_THREADS;
    pl->lds = extra * 4;
    if (a->route == DCTR_FIELDWISE_ROUTE_REREAD) return;
    for (int pass = 0; pass < 2 && !pl->on_chip; ++pass) {
        const size_t cap = pass == 0 ? FW_LDS_SOFT : FW_LDS_MAX;
        for (int t = pass == 0 ? FW_MAX_THREADS : 64; t >= 64; t >>= 1) {
            const size_t need = ((size_t)a->n_groups * t * pl->V + extra) * 4;
            if (need <= cap) {
                pl->on_chip = true;
                pl->threads = t;
                pl->lds = need;
                break;
            }
        }
    }
}

void fieldwise_params(const dctr_fieldwise_args_t* a, const FwPlan& pl, FwParams* p) {
    p->batch = a->batch;
    p->x = a->x + a->x_offset;
    p->x_stride = a->x_stride;
    p->groups = a->groups;
    p->G = a->n_groups;
    p->d = a->dim;
    p->nv = pl.nv;
    p->nvp = pl.nvp;
    p->kernel_mf = a->kernel_mf;
    p->kernel_fm = a->kernel_fm;
    p->bias_mf = a->bias_mf;
    p->bias_fm = a->bias_fm;
    p->head_w = a->head_w;
}

int fieldwise_bwd_check(const dctr_fieldwise_bwd_args_t* a, FwPlan* pl) {
    DCTR_REQUIRE(a, DCTR_E_NULL, "fieldwise_bwd: null args");
    int rc = fieldwise_check(&a->fwd, "fieldwise_bwd");
    if (rc != DCTR_OK) return rc;
    DCTR_REQUIRE(a->accumulate == 0 || a->accumulate == 1, DCTR_E_ENUM, "fieldwise_bwd: accumulate = %d", a->accumulate);
    DCTR_REQUIRE(a->dx_offset >= 0, DCTR_E_DIM, "fieldwise_bwd: negative dx_offset");
    const dctr_fieldwise_args_t& f = a->fwd;
    const size_t G = (size_t)f.n_groups;
    const size_t extra = G * (G - 1) / 2 + G + 2 * (size_t)f.dim;
    const bool vec_ok = !a->dx || (fw_mult4(a->dx_stride) && fw_mult4(a->dx_offset) && dctr_aligned16(a->dx));
    dctr_fieldwise_args_t auto_route = f;
    auto_route.route = DCTR_FIELDWISE_ROUTE_AUTO;
    fieldwise_plan(&auto_route, extra, vec_ok, pl);
    return DCTR_OK;
}

}  // namespace

extern "C" int dctr_fieldwise_route(const dctr_fieldwise_args_t* a) {
    int rc = fieldwise_check(a, "fieldwise_fwd");
    if (rc != DCTR_OK) return rc;
    FwPlan pl;
    fieldwise_plan(a, 0, true, &pl);
    return pl.on_chip ? DCTR_FIELDWISE_ROUTE_ON_CHIP : DCTR_FIELDWISE_ROUTE_REREAD;
}

extern "C" int dctr_fieldwise_fwd(const dctr_fieldwise_args_t* a, void* stream) {
    int rc = fieldwise_check(a, "fieldwise_fwd");
    if (rc != DCTR_OK) return rc;
    DCTR_REQUIRE(a->x && a->groups && a->kernel_mf && a->kernel_fm, DCTR_E_NULL, "fieldwise_fwd: null x / groups / kernel_mf / kernel_fm");
    DCTR_REQUIRE(a->y || a->logit, DCTR_E_NULL, "fieldwise_fwd: neither y nor logit");
    DCTR_REQUIRE(!a->logit || a->head_w, DCTR_E_NULL, "fieldwise_fwd: logit without head_w");
    DCTR_REQUIRE(!a->add || a->logit, DCTR_E_NULL, "fieldwise_fwd: add without logit");
    DCTR_REQUIRE(!a->y || (a->y_offset >= 0 && a->y_offset + a->dim <= a->y_stride), DCTR_E_DIM,
                 "fieldwise_fwd: y columns [%lld, %lld) in rows of %lld", (long long)a->y_offset, (long long)(a->y_offset + a->dim),
                 (long long)a->y_stride);
    if (a->batch == 0) return DCTR_OK;
    FwPlan pl;
    fieldwise_plan(a, 0, true, &pl);
    FwParams p = {};
    fieldwise_params(a, pl, &p);
    p.y = a->y ? a->y + a->y_offset : nullptr;
    p.y_stride = a->y_stride;
    p.add = a->add;
    p.logit = a->logit;
    const int rows = pl.threads / pl.nvp;
    const int64_t n_blocks = dctr_ceil_div(a->batch, (int64_t)rows);
    DCTR_REQUIRE(n_blocks < (1LL << 31), DCTR_E_DIM, "fieldwise_fwd: batch %lld needs %lld workgroups", (long long)a->batch,
                 (long long)n_blocks);
    const dim3 grid((unsigned)n_blocks), block(pl.threads);
    const hipStream_t st = (hipStream_t)stream;
    static thread_local size_t granted4[DCTR_MAX_DEVICES] = {0}, granted1[DCTR_MAX_DEVICES] = {0};
    if (pl.on_chip) {
        const void* fn = pl.V == 4 ? (const void*)fieldwise_fwd_kernel<4, true> : (const void*)fieldwise_fwd_kernel<1, true>;
        if (pl.lds > FW_LDS_SOFT) {
            hipError_t e = dctr_grant_lds(fn, pl.lds, pl.V == 4 ? granted4 : granted1);
            DCTR_REQUIRE(e == hipSuccess, (int)e, "fieldwise_fwd: cannot raise dynamic LDS: %s", hipGetErrorString(e));
        }
        if (pl.V == 4)
            DCTR_LAUNCH((fieldwise_fwd_kernel<4, true>), grid, block, pl.lds, st, p);
        else
            DCTR_LAUNCH((fieldwise_fwd_kernel<1, true>), grid, block, pl.lds, st, p);
    } else if (pl.V == 4) {
        DCTR_LAUNCH((fieldwise_fwd_kernel<4, false>), grid, block, 0, st, p);
    } else {
        DCTR_LAUNCH((fieldwise_fwd_kernel<1, false>), grid, block, 0, st, p);
    }
    return dctr_launch_status("dctr_fieldwise_fwd");
}

extern "C" int dctr_fieldwise_bwd_supported(const dctr_fieldwise_bwd_args_t* a) {
    FwPlan pl;
    return fieldwise_bwd_check(a, &pl) == DCTR_OK && pl.on_chip ? 1 : 0;
}

extern "C" int dctr_fieldwise_bwd(const dctr_fieldwise_bwd_args_t* a, void* stream) {
    FwPlan pl;
    int rc = fieldwise_bwd_check(a, &pl);
    if (rc != DCTR_OK) return rc;
    const dctr_fieldwise_args_t& f = a->fwd;
    DCTR_REQUIRE(f.x && f.groups && f.kernel_mf && f.kernel_fm, DCTR_E_NULL, "fieldwise_bwd: null x / groups / kernel_mf / kernel_fm");
    DCTR_REQUIRE((a->dy != nullptr) != (a->dlogit != nullptr), DCTR_E_NULL, "fieldwise_bwd: exactly one of dy / dlogit");
    DCTR_REQUIRE(!a->dlogit || f.head_w, DCTR_E_NULL, "fieldwise_bwd: dlogit without head_w");
    DCTR_REQUIRE(!a->dy || a->dy_stride >= f.dim, DCTR_E_DIM, "fieldwise_bwd: dy_stride %lld < dim = %d", (long long)a->dy_stride, f.dim);
    DCTR_REQUIRE(!a->d_head_w || a->dlogit, DCTR_E_NULL, "fieldwise_bwd: d_head_w needs the dlogit form");
    if (a->dx)
        for (int g = 0; g < f.n_groups; ++g)
            DCTR_REQUIRE(a->dx_offset + f.groups_host[g].first + (int64_t)f.groups_host[g].n_fields * f.dim <= a->dx_stride, DCTR_E_DIM,
                         "fieldwise_bwd: group %d ends past dx's rows of %lld", g, (long long)a->dx_stride);
    DCTR_REQUIRE(pl.on_chip, DCTR_E_UNSUPPORTED, "fieldwise_bwd: %d groups of dim %d: the group sums and accumulators exceed %zu bytes of LDS",
                 f.n_groups, f.dim, FW_LDS_MAX);
    if (f.batch == 0) return DCTR_OK;
    FwParams p = {};
    fieldwise_params(&f, pl, &p);
    p.dy = a->dy;
    p.dy_stride = a->dy_stride;
    p.dlogit = a->dlogit;
    p.dx = a->dx ? a->dx + a->dx_offset : nullptr;
    p.dx_stride = a->dx_stride;
    p.accumulate = a->accumulate;
    p.d_kernel_mf = a->d_kernel_mf;
    p.d_kernel_fm = a->d_kernel_fm;
    p.d_bias_mf = a->d_bias_mf;
    p.d_bias_fm = a->d_bias_fm;
    p.d_head_w = a->d_head_w;
    p.n_tiles = dctr_ceil_div(f.batch, (int64_t)(pl.threads / pl.nvp));
    const int64_t cap = f.max_blocks > 0 ? (int64_t)f.max_blocks : (int64_t)4 * dctr_n_cus();
    const dim3 grid((unsigned)(p.n_tiles < cap ? p.n_tiles : cap)), block(pl.threads);
    const hipStream_t st = (hipStream_t)stream;
    static thread_local size_t granted4[DCTR_MAX_DEVICES] = {0}, granted1[DCTR_MAX_DEVICES] = {0};
    if (pl.lds > FW_LDS_SOFT) {
        const void* fn = pl.V == 4 ? (const void*)fieldwise_bwd_kernel<4> : (const void*)fieldwise_bwd_kernel<1>;
        hipError_t e = dctr_grant_lds(fn, pl.lds, pl.V == 4 ? granted4 : granted1);
        DCTR_REQUIRE(e == hipSuccess, (int)e, "fieldwise_bwd: cannot raise dynamic LDS: %s", hipGetErrorString(e));
    }
    if (pl.V == 4)
        DCTR_LAUNCH((fieldwise_bwd_kernel<4>), grid, block, pl.lds, st, p);
    else
        DCTR_LAUNCH((fieldwise_bwd_kernel<1>), grid, block, pl.lds, st, p);
    return dctr_launch_status("dctr_fieldwise_bwd");
}
