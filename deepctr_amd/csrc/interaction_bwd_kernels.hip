// Backward of the pairwise interaction layers.
//   dctr_bi_interaction_bwd   BiInteractionPooling (NFM): y[b,e] = 0.5((sum_f x)^2 - sum_f x^2)
//   dctr_fm_bwd               FM.call (interaction.py:588-604): that pooling summed over e
//   dctr_inner_product_bwd    InnerProductLayer(reduce_sum) (PNN)
//   dctr_afm_bwd              AFMLayer (interaction.py:116-146)
// Nothing is saved by the forwards: each kernel re-reads the forward's input.
#include "dctr_common.h"

namespace {

// ---------------------------------------------------------------------------------------------------
// sibling interaction layers: backward of BiInteractionPooling (NFM) and InnerProductLayer(reduce_sum) (PNN).
// One thread per (row, e); the F embeddings of the row are re-read from the forward's input (HBM/L2, F*E*4 B per row).
// ---------------------------------------------------------------------------------------------------
// y[b,e] = 0.5((sum_f x)^2 - sum_f x^2)  =>  dx[b,f,e] = dy[b,e] * (sum_f' x[b,f',e] - x[b,f,e])
// (dy_estride 1: dy [B, E] — BiInteractionPooling; 0: dy [B] broadcast over e — FM, whose logit is that pooling summed over e)
__global__ __launch_bounds__(256) void bi_interaction_bwd_kernel(const float* __restrict__ x, int64_t x_stride, int64_t batch, int F,
                                                                 int E, const float* __restrict__ dy, int64_t dy_stride,
                                                                 float* __restrict__ dx, int64_t dx_stride, int accumulate,
                                                                 int dy_estride = 1) {
    const int64_t total = batch * E;
    for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (int64_t)gridDim.x * 256) {
        const int64_t b = o / E;
        const int e = (int)(o - b * E);
        const float* xb = x + b * x_stride + e;
        float s = 0.f;
        for (int f = 0; f < F; ++f) s += xb[(int64_t)f * E];
        const float g = dy[b * dy_stride + (int64_t)e * dy_estride];
        float* db = dx + b * dx_stride + e;
        for (int f = 0; f < F; ++f) {
            const float v = g * (s - xb[(int64_t)f * E]);
            db[(int64_t)f * E] = accumulate ? db[(int64_t)f * E] + v : v;
        }
    }
}

// y[b,p(i,j)] = <x_i, x_j> (i<j, pairs ordered by i then j)  =>  dx[b,i,e] = sum_{j != i} dy[b,p(min,max)] * x[b,j,e]
__global__ __launch_bounds__(256) void inner_product_bwd_kernel(const float* __restrict__ x, int64_t x_stride, int64_t batch, int F,
                                                                int E, const float* __restrict__ dy, int64_t dy_stride,
                                                                float* __restrict__ dx, int64_t dx_stride, int accumulate) {
    const int64_t total = batch * F * E;
    const int FE = F * E;
    for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (int64_t)gridDim.x * 256) {
        const int64_t b = o / FE;
        const int c = (int)(o - b * FE);
        const int i = c / E, e = c - i * E;
        const float* xb = x + b * x_stride + e;
        const float* gb = dy + b * dy_stride;
        float acc = 0.f;
        for (int j = 0; j < i; ++j) acc = fmaf(gb[j * (2 * F - j - 1) / 2 + (i - j - 1)], xb[(int64_t)j * E], acc);
        const int base = i * (2 * F - i - 1) / 2 - i - 1;
        for (int j = i + 1; j < F; ++j) acc = fmaf(gb[base + j], xb[(int64_t)j * E], acc);
        float* d = dx + b * dx_stride + c;
        *d = accumulate ? *d + acc : acc;
    }
}

// ---------------------------------------------------------------------------------------------------
// backward of AFMLayer (interaction.py:116-146).  Same shape as the forward kernel: one wave per sample, the sample's [F,E]
// tile and the layer's weights in LDS, lanes walk the F(F-1)/2 pairs; nothing was saved by the forward, so the attention
// logits and the softmax are recomputed.  With bi_p = x_i * x_j, pre_pa = b_a + sum_e bi_pe W_ea, s_p = sum_a relu(pre_pa) h_a,
// alpha = softmax_p(s), t_p = bi_p . proj_p, y = sum_p alpha_p t_p and g = dy:
//     ds_p = alpha_p (g t_p - g y),  d pre_pa = ds_p h_a [pre_pa > 0],  d bi_pe = g alpha_p proj_p[e] + sum_a d pre_pa W_ea,
//     d x_i += d bi_p * x_j,  d x_j += d bi_p * x_i;   weight gradients are summed in LDS per workgroup, then one atomic each.
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ void afm_pair_ij(int p, int F, int& i, int& j) {
    int ii = 0, rem = p;
    while (rem >= F - 1 - ii) {
        rem -= F - 1 - ii;
        ++ii;
    }
    i = ii;
    j = ii + 1 + rem;
}

__global__ __launch_bounds__(256) void afm_bwd_kernel(const float* __restrict__ x, int64_t x_stride, int64_t batch, int F, int E,
                                                      const float* __restrict__ att_w, const float* __restrict__ att_b,
                                                      const float* __restrict__ proj_h, const float* __restrict__ proj_p, int A,
                                                      const float* __restrict__ dy, float* __restrict__ dx, int64_t dx_stride,
                                                      int accumulate, float* __restrict__ g_w, float* __restrict__ g_b,
                                                      float* __restrict__ g_h, float* __restrict__ g_p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int P = F * (F - 1) / 2;
    const int NW = E * A + 2 * A + E;
    float* wsh = smem;                       // [E*A] attention_W, then b[A], h[A], p[E]
    float* bsh = wsh + E * A;
    float* hsh = bsh + A;
    float* psh = hsh + A;
    float* gsh = psh + E;                    // gradients in the same order: W, b, h, p
    float* per_wave = gsh + NW;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float* xs = per_wave + wave * (2 * F * E + P);   // [F*E] sample tile
    float* dxs = xs + F * E;                         // [F*E] its gradient
    float* alpha = dxs + F * E;                      // [P]
    for (int i = threadIdx.x; i < E * A; i += 256) wsh[i] = att_w[i];
    for (int i = threadIdx.x; i < A; i += 256) {
        bsh[i] = att_b[i];
        hsh[i] = proj_h[i];
    }
    for (int i = threadIdx.x; i < E; i += 256) psh[i] = proj_p[i];
    for (int i = threadIdx.x; i < NW; i += 256) gsh[i] = 0.f;
    const int64_t b = (int64_t)blockIdx.x * 4 + wave;
    const bool valid = b < batch;
    if (valid)
        for (int i = lane; i < F * E; i += 64) {
            xs[i] = x[b * x_stride + i];
            dxs[i] = 0.f;
        }
    __syncthreads();
    if (valid) {
        // forward recompute: logits, softmax, y
        float mx = -INFINITY;
        for (int p = lane; p < P; p += 64) {
            int i, j;
            afm_pair_ij(p, F, i, j);
            float lg = 0.f;
            for (int a = 0; a < A; ++a) {
                float t = bsh[a];
                for (int e = 0; e < E; ++e) t = fmaf(xs[i * E + e] * xs[j * E + e], wsh[e * A + a], t);
                lg = fmaf(fmaxf(t, 0.f), hsh[a], lg);
            }
            alpha[p] = lg;
            mx = fmaxf(mx, lg);
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) mx = fmaxf(mx, __shfl_xor(mx, m, 64));
        float den = 0.f;
        for (int p = lane; p < P; p += 64) {
            const float e_ = expf(alpha[p] - mx);
            alpha[p] = e_;
            den += e_;
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) den += __shfl_xor(den, m, 64);
        float yv = 0.f;
        for (int p = lane; p < P; p += 64) {
            int i, j;
            afm_pair_ij(p, F, i, j);
            const float sc = alpha[p] / den;
            alpha[p] = sc;
            float t = 0.f;
            for (int e = 0; e < E; ++e) t = fmaf(xs[i * E + e] * xs[j * E + e], psh[e], t);
            yv = fmaf(sc, t, yv);
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) yv += __shfl_xor(yv, m, 64);
        // backward per pair
        const float g = dy[b];
        for (int p = lane; p < P; p += 64) {
            int i, j;
            afm_pair_ij(p, F, i, j);
            const float sc = alpha[p];
            float t = 0.f;
            for (int e = 0; e < E; ++e) t = fmaf(xs[i * E + e] * xs[j * E + e], psh[e], t);
            const float ds = sc * g * (t - yv);
            const float gsc = g * sc;
            for (int e = 0; e < E; ++e) {
                const float bi = xs[i * E + e] * xs[j * E + e];
                atomicAdd(&gsh[E * A + 2 * A + e], gsc * bi);                        // d proj_p
                const float dbi = gsc * psh[e];
                atomicAdd(&dxs[i * E + e], dbi * xs[j * E + e]);
                atomicAdd(&dxs[j * E + e], dbi * xs[i * E + e]);
            }
            for (int a = 0; a < A; ++a) {
                float pre = bsh[a];
                for (int e = 0; e < E; ++e) pre = fmaf(xs[i * E + e] * xs[j * E + e], wsh[e * A + a], pre);
                if (pre > 0.f) {
                    atomicAdd(&gsh[E * A + A + a], ds * pre);                        // d proj_h
                    const float dpre = ds * hsh[a];
                    atomicAdd(&gsh[E * A + a], dpre);                                // d attention_b
                    for (int e = 0; e < E; ++e) {
                        const float xi = xs[i * E + e], xj = xs[j * E + e];
                        atomicAdd(&gsh[e * A + a], dpre * xi * xj);                  // d attention_W
                        const float dbi = dpre * wsh[e * A + a];
                        atomicAdd(&dxs[i * E + e], dbi * xj);
                        atomicAdd(&dxs[j * E + e], dbi * xi);
                    }
                }
            }
        }
    }
    __syncthreads();
    if (valid) {
        float* d = dx + b * dx_stride;
        for (int i = lane; i < F * E; i += 64) d[i] = accumulate ? d[i] + dxs[i] : dxs[i];
    }
    for (int i = threadIdx.x; i < NW; i += 256) {
        const float v = gsh[i];
        if (v != 0.f) {
            float* dst = i < E * A ? g_w + i : i < E * A + A ? g_b + (i - E * A) : i < E * A + 2 * A ? g_h + (i - E * A - A)
                                                                                                   : g_p + (i - E * A - 2 * A);
            unsafeAtomicAdd(dst, v);
        }
    }
}

// what dctr_afm_bwd and its dry check share: the sizes the op takes, and the dynamic LDS of afm_bwd_kernel for them (the weights and
// their gradients once per workgroup, a sample tile, its gradient and the pair scores per wave)
constexpr size_t AFM_BWD_LDS_MAX = 160 * 1024;
bool afm_bwd_sizes_ok(int fields, int dim, int att_factor) { return fields >= 2 && dim >= 1 && att_factor >= 1; }
size_t afm_bwd_lds_bytes(int fields, int dim, int att_factor) {
    const size_t P = (size_t)fields * (fields - 1) / 2;
    const size_t nw = (size_t)dim * att_factor + 2 * (size_t)att_factor + dim;
    return (2 * nw + 4 * (2 * (size_t)fields * dim + P)) * sizeof(float);
}

}  // namespace

extern "C" int dctr_afm_bwd_supported(int32_t fields, int32_t dim, int32_t att_factor) {
    return afm_bwd_sizes_ok(fields, dim, att_factor) && afm_bwd_lds_bytes(fields, dim, att_factor) <= AFM_BWD_LDS_MAX ? 1 : 0;
}

extern "C" int dctr_afm_bwd(const dctr_afm_bwd_args_t* a, void* stream) {
    DCTR_REQUIRE(a != nullptr, DCTR_E_NULL, "afm_bwd: null args");
    DCTR_REQUIRE(a->batch >= 0 && afm_bwd_sizes_ok(a->fields, a->dim, a->att_factor), DCTR_E_DIM, "afm_bwd: bad sizes");
    DCTR_REQUIRE(a->x_stride >= (int64_t)a->fields * a->dim && a->dx_stride >= (int64_t)a->fields * a->dim, DCTR_E_DIM,
                 "afm_bwd: stride smaller than fields*dim");
    if (a->batch == 0) return DCTR_OK;
    DCTR_REQUIRE(a->x && a->att_w && a->att_b && a->proj_h && a->proj_p && a->dy && a->dx, DCTR_E_NULL, "afm_bwd: null pointer");
    DCTR_REQUIRE(a->d_att_w && a->d_att_b && a->d_proj_h && a->d_proj_p, DCTR_E_NULL, "afm_bwd: null gradient pointer");
    const size_t lds = afm_bwd_lds_bytes(a->fields, a->dim, a->att_factor);
    DCTR_REQUIRE(lds <= AFM_BWD_LDS_MAX, DCTR_E_UNSUPPORTED, "afm_bwd: needs %zu B of LDS", lds);
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)afm_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        DCTR_REQUIRE(e == hipSuccess, (int)e, "afm_bwd: cannot raise dynamic LDS: %s", hipGetErrorString(e));
    }
    const int64_t blocks = dctr_ceil_div(a->batch, (int64_t)4);
    DCTR_REQUIRE(blocks <= 0x7fffffffLL, DCTR_E_DIM, "afm_bwd: batch too large");
    hipLaunchKernelGGL(afm_bwd_kernel, dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, a->x, a->x_stride, a->batch,
                       (int)a->fields, (int)a->dim, a->att_w, a->att_b, a->proj_h, a->proj_p, (int)a->att_factor, a->dy, a->dx,
                       a->dx_stride, (int)a->dx_accumulate, a->d_att_w, a->d_att_b, a->d_proj_h, a->d_proj_p);
    return dctr_launch_status("dctr_afm_bwd");
}

extern "C" int dctr_bi_interaction_bwd(const float* x, int64_t batch, int64_t x_stride, int32_t fields, int32_t dim, const float* dy,
                                       int64_t dy_stride, float* dx, int64_t dx_stride, int32_t accumulate, void* stream) {
    DCTR_REQUIRE(batch >= 0 && fields >= 1 && dim >= 1, DCTR_E_DIM, "bi_interaction_bwd: bad sizes");
    DCTR_REQUIRE(x_stride >= (int64_t)fields * dim && dx_stride >= (int64_t)fields * dim && dy_stride >= dim, DCTR_E_DIM,
                 "bi_interaction_bwd: stride smaller than a row");
    if (batch == 0) return DCTR_OK;
    DCTR_REQUIRE(x && dy && dx, DCTR_E_NULL, "bi_interaction_bwd: null pointer");
    int64_t blocks = dctr_ceil_div(batch * dim, (int64_t)256);
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(bi_interaction_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, x_stride, batch,
                       (int)fields, (int)dim, dy, dy_stride, dx, dx_stride, (int)accumulate);
    return dctr_launch_status("dctr_bi_interaction_bwd");
}

// FM.call backward (interaction.py:588-604) on a strided [B, >= F*E] buffer: dx[b,f,:] (+)= dlogit[b] * (sum_f' x[b,f',:] - x[b,f,:])
extern "C" int dctr_fm_bwd(const float* x, int64_t batch, int64_t x_stride, int32_t fields, int32_t dim, const float* dlogit, float* dx,
                           int64_t dx_stride, int32_t accumulate, void* stream) {
    DCTR_REQUIRE(batch >= 0 && fields >= 1 && dim >= 1, DCTR_E_DIM, "fm_bwd: bad sizes");
    DCTR_REQUIRE(x_stride >= (int64_t)fields * dim && dx_stride >= (int64_t)fields * dim, DCTR_E_DIM, "fm_bwd: stride < fields*dim");
    if (batch == 0) return DCTR_OK;
    DCTR_REQUIRE(x && dlogit && dx, DCTR_E_NULL, "fm_bwd: null pointer");
    int64_t blocks = dctr_ceil_div(batch * dim, (int64_t)256);
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(bi_interaction_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, x_stride, batch, (int)fields,
                       (int)dim, dlogit, (int64_t)1, dx, dx_stride, (int)accumulate, 0);
    return dctr_launch_status("dctr_fm_bwd");
}

extern "C" int dctr_inner_product_bwd(const float* x, int64_t batch, int64_t x_stride, int32_t fields, int32_t dim, const float* dy,
                                      int64_t dy_stride, float* dx, int64_t dx_stride, int32_t accumulate, void* stream) {
    DCTR_REQUIRE(batch >= 0 && fields >= 2 && fields <= 1024 && dim >= 1, DCTR_E_DIM, "inner_product_bwd: bad sizes");
    DCTR_REQUIRE(x_stride >= (int64_t)fields * dim && dx_stride >= (int64_t)fields * dim &&
                     dy_stride >= (int64_t)fields * (fields - 1) / 2,
                 DCTR_E_DIM, "inner_product_bwd: stride smaller than a row");
    if (batch == 0) return DCTR_OK;
    DCTR_REQUIRE(x && dy && dx, DCTR_E_NULL, "inner_product_bwd: null pointer");
    int64_t blocks = dctr_ceil_div(batch * fields * dim, (int64_t)256);
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(inner_product_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, x_stride, batch,
                       (int)fields, (int)dim, dy, dy_stride, dx, dx_stride, (int)accumulate);
    return dctr_launch_status("dctr_inner_product_bwd");
}
