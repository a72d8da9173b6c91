// The CrossNet backwards of the HIP training step.
//   dctr_crossnet_bwd (+ _workspace_bytes)   CrossNet, vector and matrix (layers/interaction.py:405-424)
//   dctr_crossnet_mix_bwd (+ _supported, _workspace_bytes)   CrossNetMix (layers/interaction.py:511-549)
// The GEMMs are dctr_gemm (gemm_kernels.hip); the row copies / sums go through the launchers of namespace dctr_train
// (train_common.h; their kernels live in dnn_train_kernels.hip).  The reference has no code of its own for any of this (Keras
// autodiff): the formulas are the derivatives of the forward expressions cited at each section.
#include "dctr_gemm.h"

#include "dctr_common.h"
#include "train_common.h"

namespace {

// ---------------------------------------------------------------------------------------------------
// CrossNet backward (interaction.py:405-424).  No activations are saved by the forward: both forms recompute x_l.
//   vector: x_{l+1} = x0 * s_l + b_l + x_l,  s_l = x_l . w_l
//     ds = g . x0;  d b_l += g;  d w_l += ds * x_l;  d x0 += g * s_l;  g += ds * w_l      (l = L-1 .. 0),  d x0 += g
//   One wave walks CROSS_SPW samples (x_l per layer in LDS), accumulating d w / d b in LDS, flushed once with atomics.
// ---------------------------------------------------------------------------------------------------
constexpr int CROSS_SPW = 4;       // (16 at first: 64 workgroups, 174 us at B = 4096; the accumulators are combined per workgroup now)

__global__ __launch_bounds__(256) void cross_vector_bwd_kernel(const float* __restrict__ x, int64_t x_stride, int64_t batch, int d,
                                                               int L, const float* __restrict__ w, const float* __restrict__ bias,
                                                               const float* __restrict__ dy, int64_t dy_stride,
                                                               float* __restrict__ dw, float* __restrict__ db,
                                                               float* __restrict__ dx, int64_t dx_stride, int accumulate) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float* xs = smem + (size_t)wave * (3 * L * d + L);      // [L][d] x_l
    float* aw = xs + (size_t)L * d;                           // [L][d] d w accumulators
    float* ab = aw + (size_t)L * d;                           // [L][d] d b accumulators
    float* sl = ab + (size_t)L * d;                           // [L] s_l
    for (int i = lane; i < 2 * L * d; i += 64) aw[i] = 0.f;
    const int64_t b_first = ((int64_t)blockIdx.x * 4 + wave) * CROSS_SPW;
    for (int it = 0; it < CROSS_SPW; ++it) {
        const int64_t b = b_first + it;
        if (b >= batch) break;
        const float* x0 = x + b * x_stride;
        // forward, keeping x_l
        for (int i = lane; i < d; i += 64) xs[i] = x0[i];
        for (int l = 0; l < L; ++l) {
            const float* xl = xs + (size_t)l * d;
            float dot = 0.f;
            for (int i = lane; i < d; i += 64) dot = fmaf(xl[i], w[(size_t)l * d + i], dot);
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) dot += __shfl_xor(dot, m, 64);
            if (lane == 0) sl[l] = dot;
            if (l + 1 < L)
                for (int i = lane; i < d; i += 64) xs[(size_t)(l + 1) * d + i] = x0[i] * dot + bias[(size_t)l * d + i] + xl[i];
        }
        // backward: g lives in dx (or a register-free walk over LDS): reuse ab? no — keep g in the output row
        float* gout = dx + b * dx_stride;
        const float* gin = dy + b * dy_stride;
        // g is held in registers in chunks of 64 columns: up to 32 chunks (d <= 2048)
        float g[32], dx0[32];
#pragma unroll
        for (int r = 0; r < 32; ++r) {
            const int i = lane + 64 * r;
            g[r] = i < d ? gin[i] : 0.f;
            dx0[r] = 0.f;
        }
        for (int l = L - 1; l >= 0; --l) {
            const float* xl = xs + (size_t)l * d;
            const float s = sl[l];
            float ds = 0.f;
#pragma unroll
            for (int r = 0; r < 32; ++r) {
                const int i = lane + 64 * r;
                if (i < d) ds = fmaf(g[r], x0[i], ds);
            }
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) ds += __shfl_xor(ds, m, 64);
#pragma unroll
            for (int r = 0; r < 32; ++r) {
                const int i = lane + 64 * r;
                if (i < d) {
                    ab[(size_t)l * d + i] += g[r];
                    aw[(size_t)l * d + i] = fmaf(ds, xl[i], aw[(size_t)l * d + i]);
                    dx0[r] = fmaf(g[r], s, dx0[r]);
                    g[r] = fmaf(ds, w[(size_t)l * d + i], g[r]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 32; ++r) {
            const int i = lane + 64 * r;
            if (i < d) gout[i] = (accumulate ? gout[i] : 0.f) + dx0[r] + g[r];
        }
    }
    // the four waves' accumulators meet here: one atomic per element and WORKGROUP (they serialise per address)
    __syncthreads();
    const size_t region = (size_t)3 * L * d + L;
    for (int i = threadIdx.x; i < L * d; i += 256) {
        const float* r0 = smem + (size_t)L * d + i;
        unsafeAtomicAdd(dw + i, (r0[0] + r0[region]) + (r0[2 * region] + r0[3 * region]));
        const float* r1 = r0 + (size_t)L * d;
        unsafeAtomicAdd(db + i, (r1[0] + r1[region]) + (r1[2 * region] + r1[3 * region]));
    }
}

// vector form, any width (the kernel above keeps a wave's x_l, d w, d b in LDS and a row's gradient in registers: <= 2048 columns and
// 48 L d bytes of LDS): the same recurrence layer by layer over the whole batch, x_l / s_l / g / d x0 in the caller's workspace —
// memory-bound passes, no limit on d.  Forward step: s_l[b] = x_l[b] . w_l;  x_{l+1}[b] = x0[b] * s_l[b] + b_l + x_l[b]  (one wave per sample)
__global__ __launch_bounds__(256) void cross_vec_fwd_step_kernel(const float* __restrict__ x0, int64_t x0_stride, const float* __restrict__ xl,
                                                                 int64_t xl_stride, const float* __restrict__ w, const float* __restrict__ bias,
                                                                 int64_t batch, int d, float* __restrict__ s, float* __restrict__ xn) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + wave;
    if (b >= batch) return;
    const float* r0 = x0 + b * x0_stride;
    const float* rl = xl + b * xl_stride;
    float dot = 0.f;
    for (int i = lane; i < d; i += 64) dot = fmaf(rl[i], w[i], dot);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) dot += __shfl_xor(dot, m, 64);
    if (lane == 0) s[b] = dot;
    if (xn != nullptr)
        for (int i = lane; i < d; i += 64) xn[b * d + i] = r0[i] * dot + bias[i] + rl[i];
}

// ds[b] = g[b] . x0[b]
__global__ __launch_bounds__(256) void cross_vec_dot_kernel(const float* __restrict__ g, const float* __restrict__ x0, int64_t x0_stride,
                                                            int64_t batch, int d, float* __restrict__ ds) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + wave;
    if (b >= batch) return;
    const float* gr = g + b * d;
    const float* r0 = x0 + b * x0_stride;
    float dot = 0.f;
    for (int i = lane; i < d; i += 64) dot = fmaf(gr[i], r0[i], dot);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) dot += __shfl_xor(dot, m, 64);
    if (lane == 0) ds[b] = dot;
}

// d b_l[i] += sum_b g[b, i];  d w_l[i] += sum_b ds[b] * x_l[b, i]: a thread owns a column over a slice of the rows (coalesced across the
// workgroup), one atomic per column and slice
__global__ __launch_bounds__(256) void cross_vec_colsum_kernel(const float* __restrict__ g, const float* __restrict__ ds,
                                                               const float* __restrict__ xl, int64_t xl_stride, int64_t batch, int d,
                                                               float* __restrict__ dw, float* __restrict__ db) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= d) return;
    const int64_t per = (batch + gridDim.y - 1) / gridDim.y;
    const int64_t b0 = (int64_t)blockIdx.y * per, b1 = b0 + per < batch ? b0 + per : batch;
    float aw = 0.f, ab = 0.f;
    for (int64_t b = b0; b < b1; ++b) {
        ab += g[b * d + i];
        aw = fmaf(ds[b], xl[b * xl_stride + i], aw);
    }
    if (b1 > b0) {
        unsafeAtomicAdd(dw + i, aw);
        unsafeAtomicAdd(db + i, ab);
    }
}

// d x0[b, i] += g[b, i] * s_l[b];  g[b, i] += ds[b] * w_l[i]
__global__ __launch_bounds__(256) void cross_vec_update_kernel(float* __restrict__ g, float* __restrict__ dx0, const float* __restrict__ ds,
                                                               const float* __restrict__ s, const float* __restrict__ w, int64_t batch, int d) {
    const int64_t total = batch * d;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t b = e / d;
        const int i = (int)(e - b * d);
        const float gv = g[e];
        dx0[e] = fmaf(gv, s[b], dx0[e]);
        g[e] = fmaf(ds[b], w[i], gv);
    }
}

// matrix form, elementwise parts (the GEMMs are dctr_gemm): forward  x_next = x0 .* (u + b) + x_l
__global__ __launch_bounds__(256) void cross_matrix_fwd_elem_kernel(const float* __restrict__ x0, int64_t x_stride,
                                                                    const float* __restrict__ xl, int64_t xl_stride,
                                                                    const float* __restrict__ u, const float* __restrict__ bias,
                                                                    int64_t batch, int d, float* __restrict__ xn) {
    const int64_t total = batch * d;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / d;
        const int c = (int)(i - b * d);
        xn[i] = x0[b * x_stride + c] * (u[i] + bias[c]) + xl[b * xl_stride + c];
    }
}

// backward: du = g .* x0;  dx0 (+)= g .* (u + b)
__global__ __launch_bounds__(256) void cross_matrix_bwd_elem_kernel(const float* __restrict__ x0, int64_t x_stride,
                                                                    const float* __restrict__ g, const float* __restrict__ u,
                                                                    const float* __restrict__ bias, int64_t batch, int d,
                                                                    float* __restrict__ du, float* __restrict__ dx0) {
    const int64_t total = batch * d;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / d;
        const int c = (int)(i - b * d);
        const float gv = g[i];
        du[i] = gv * x0[b * x_stride + c];
        dx0[i] += gv * (u[i] + bias[c]);
    }
}

}  // namespace

// vector form: does the one-kernel backward (x_l of a wave's sample + its d w / d b accumulators in LDS, the row's gradient in registers) hold it?
static bool cross_vector_bwd_on_chip(int d, int L) { return d <= 2048 && (size_t)4 * (3 * (size_t)L * d + L) * sizeof(float) <= 160 * 1024; }

extern "C" size_t dctr_crossnet_bwd_workspace_bytes(const dctr_crossnet_bwd_args_t* a) {
    if (a == nullptr || a->batch <= 0 || a->layers <= 0) return 0;
    if (a->mode == DCTR_CROSS_VECTOR) {
        // the layer-by-layer form of wide inputs: x_1 .. x_{L-1}, g, d x0 [B, d] each; s_0 .. s_{L-1}, ds [B] each
        if (a->dim < 1 || cross_vector_bwd_on_chip(a->dim, a->layers)) return 0;
        return ((size_t)(a->layers + 1) * a->batch * a->dim + (size_t)(a->layers + 1) * a->batch) * sizeof(float);
    }
    if (a->mode != DCTR_CROSS_MATRIX) return 0;
    // x_1 .. x_{L-1}, u_0 .. u_{L-1}, g, du, dx0; from 8192 rows on the partial dW of the row slices (as in dctr_mlp_bwd)
    const int parts = mlp_dw_parts(a->batch, (int64_t)a->dim * a->dim);
    return ((size_t)(2 * a->layers + 2) * a->batch * a->dim + (parts > 1 ? (size_t)parts * a->dim * a->dim : 0)) * sizeof(float);
}

extern "C" int dctr_crossnet_bwd(const dctr_crossnet_bwd_args_t* a, void* stream) {
    DCTR_REQUIRE(a != nullptr, DCTR_E_NULL, "crossnet_bwd: null args");
    DCTR_REQUIRE(a->batch >= 0 && a->dim >= 1 && a->layers >= 0, DCTR_E_DIM, "crossnet_bwd: bad sizes");
    DCTR_REQUIRE(a->mode == DCTR_CROSS_VECTOR || a->mode == DCTR_CROSS_MATRIX, DCTR_E_ENUM, "crossnet_bwd: mode %d", a->mode);
    if (a->batch == 0) return DCTR_OK;
    DCTR_REQUIRE(a->x && a->dy && a->dx && a->x_stride >= a->dim && a->dy_stride >= a->dim && a->dx_stride >= a->dim, DCTR_E_NULL,
                 "crossnet_bwd: null pointer or stride < dim");
    hipStream_t st = (hipStream_t)stream;
    const int d = a->dim, L = a->layers;
    const unsigned eb = (unsigned)(dctr_ceil_div(a->batch * d, (int64_t)256) > 4096 ? 4096 : dctr_ceil_div(a->batch * d, (int64_t)256));
    if (L == 0) {
        dctr_train::launch_add_rows(st, eb, a->dy, a->dy_stride, a->batch, d, a->dx, a->dx_stride, (int)a->dx_accumulate);
        return dctr_launch_status("dctr_crossnet_bwd");
    }
    DCTR_REQUIRE(a->kernels && a->bias && a->d_kernels && a->d_bias, DCTR_E_NULL, "crossnet_bwd: null weights / gradients");
    if (a->mode == DCTR_CROSS_VECTOR && !cross_vector_bwd_on_chip(d, L)) {
        // any width (round 6; the reference's CrossNet has none, interaction.py:405-424): layer by layer over the batch
        DCTR_REQUIRE(a->workspace != nullptr && a->workspace_bytes >= dctr_crossnet_bwd_workspace_bytes(a), DCTR_E_NULL,
                     "crossnet_bwd(vector): %d layers x dim %d need a workspace of dctr_crossnet_bwd_workspace_bytes() bytes", L, d);
        const size_t bd = (size_t)a->batch * d;
        float* ws = static_cast<float*>(a->workspace);
        float* xsave = ws;                                   // x_1 .. x_{L-1}
        float* g = ws + (size_t)(L - 1) * bd;
        float* dx0 = g + bd;
        float* sl = dx0 + bd;                                // [L][B]
        float* ds = sl + (size_t)L * a->batch;               // [B]
        const unsigned wb = (unsigned)dctr_ceil_div(a->batch, (int64_t)4);
        DCTR_REQUIRE(dctr_ceil_div(a->batch, (int64_t)4) <= 0x7fffffffLL, DCTR_E_DIM, "crossnet_bwd: batch too large");
        auto xl_of = [&](int l, const float*& p, int64_t& ld) {
            if (l == 0) { p = a->x; ld = a->x_stride; }
            else { p = xsave + (size_t)(l - 1) * bd; ld = d; }
        };
        for (int l = 0; l < L; ++l) {
            const float* xl; int64_t ldx;
            xl_of(l, xl, ldx);
            hipLaunchKernelGGL(cross_vec_fwd_step_kernel, dim3(wb), dim3(256), 0, st, a->x, a->x_stride, xl, ldx, a->kernels + (size_t)l * d,
                               a->bias + (size_t)l * d, a->batch, d, sl + (size_t)l * a->batch, l + 1 < L ? xsave + (size_t)l * bd : (float*)nullptr);
        }
        dctr_train::launch_add_rows(st, eb, a->dy, a->dy_stride, a->batch, d, g, (int64_t)d, 0);
        hipError_t me = hipMemsetAsync(dx0, 0, bd * sizeof(float), st);
        DCTR_REQUIRE(me == hipSuccess, (int)me, "crossnet_bwd: memset failed: %s", hipGetErrorString(me));
        int64_t slices = dctr_ceil_div(a->batch, (int64_t)64);
        if (slices > 64) slices = 64;
        for (int l = L - 1; l >= 0; --l) {
            const float* xl; int64_t ldx;
            xl_of(l, xl, ldx);
            hipLaunchKernelGGL(cross_vec_dot_kernel, dim3(wb), dim3(256), 0, st, (const float*)g, a->x, a->x_stride, a->batch, d, ds);
            hipLaunchKernelGGL(cross_vec_colsum_kernel, dim3((unsigned)((d + 255) / 256), (unsigned)slices), dim3(256), 0, st, (const float*)g,
                               (const float*)ds, xl, ldx, a->batch, d, a->d_kernels + (size_t)l * d, a->d_bias + (size_t)l * d);
            hipLaunchKernelGGL(cross_vec_update_kernel, dim3(eb), dim3(256), 0, st, g, dx0, (const float*)ds, (const float*)(sl + (size_t)l * a->batch),
                               a->kernels + (size_t)l * d, a->batch, d);
        }
        dctr_train::launch_add_rows(st, eb, (const float*)g, (int64_t)d, a->batch, d, dx0, (int64_t)d, 1);
        dctr_train::launch_add_rows(st, eb, (const float*)dx0, (int64_t)d, a->batch, d, a->dx, a->dx_stride, (int)a->dx_accumulate);
        return dctr_launch_status("dctr_crossnet_bwd");
    }
    if (a->mode == DCTR_CROSS_VECTOR) {
        const size_t lds = (size_t)4 * (3 * (size_t)L * d + L) * sizeof(float);
        if (lds > 64 * 1024) {
            hipError_t e = hipFuncSetAttribute((const void*)cross_vector_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            DCTR_REQUIRE(e == hipSuccess, (int)e, "crossnet_bwd: cannot raise dynamic LDS: %s", hipGetErrorString(e));
        }
        const int64_t blocks = dctr_ceil_div(a->batch, (int64_t)(4 * CROSS_SPW));
        hipLaunchKernelGGL(cross_vector_bwd_kernel, dim3((unsigned)blocks), dim3(256), lds, st, a->x, a->x_stride, a->batch, d, L,
                           a->kernels, a->bias, a->dy, a->dy_stride, a->d_kernels, a->d_bias, a->dx, a->dx_stride,
                           (int)a->dx_accumulate);
        return dctr_launch_status("dctr_crossnet_bwd");
    }
    // matrix: dctr_gemm GEMMs + elementwise kernels, intermediates in the workspace
    DCTR_REQUIRE(a->workspace != nullptr && a->workspace_bytes >= dctr_crossnet_bwd_workspace_bytes(a) && a->batch < 0x7fffffffLL,
                 DCTR_E_NULL, "crossnet_bwd(matrix): needs a workspace of dctr_crossnet_bwd_workspace_bytes() bytes");
    const int B = (int)a->batch;
    const size_t bd = (size_t)a->batch * d;
    float* ws = static_cast<float*>(a->workspace);
    float* xsave = ws;                       // x_1 .. x_{L-1}  (x_0 = a->x)
    float* us = ws + (size_t)(L - 1) * bd;   // u_0 .. u_{L-1}
    float* g = us + (size_t)L * bd;
    float* du = g + bd;
    float* dx0 = du + bd;
    float* dw_parts = dx0 + bd;
    const int n_parts = mlp_dw_parts(a->batch, (int64_t)a->dim * a->dim);
    // (saved_u / saved_x: the forward kernel's own u_l and x_l — no recompute)
    const bool saved = a->saved_u != nullptr && (L == 1 || a->saved_x != nullptr);
    const float* us_r = saved ? a->saved_u : us;
    const float* xs_r = saved ? a->saved_x : xsave;
    auto xl_of = [&](int l, const float*& p, int& ld) {
        if (l == 0) { p = a->x; ld = (int)a->x_stride; }
        else { p = xs_r + (size_t)(l - 1) * bd; ld = d; }
    };
    for (int l = 0; l < L && !saved; ++l) {  // forward recompute: u_l = x_l W_l^T;  x_{l+1} = x0 .* (u_l + b_l) + x_l
        const float* xl; int ldx;
        xl_of(l, xl, ldx);
        const float* W = a->kernels + (size_t)l * d * d;
        int rs = dctr_gemm::sgemm(st, dctr_gemm::OP_T, dctr_gemm::OP_N, d, B, d, W, d, xl, ldx, 0.f, us + (size_t)l * bd, d);
        DCTR_REQUIRE(rs == 0, DCTR_E_UNSUPPORTED, "crossnet_bwd: sgemm(u) failed (%d)", (int)rs);
        if (l + 1 < L)
            hipLaunchKernelGGL(cross_matrix_fwd_elem_kernel, dim3(eb), dim3(256), 0, st, a->x, a->x_stride, xl, (int64_t)ldx,
                               us + (size_t)l * bd, a->bias + (size_t)l * d, a->batch, d, xsave + (size_t)l * bd);
    }
    dctr_train::launch_add_rows(st, eb, a->dy, a->dy_stride, a->batch, d, g, (int64_t)d, 0);
    hipError_t me = hipMemsetAsync(dx0, 0, bd * sizeof(float), st);
    DCTR_REQUIRE(me == hipSuccess, (int)me, "crossnet_bwd: memset failed: %s", hipGetErrorString(me));
    for (int l = L - 1; l >= 0; --l) {
        const float* xl; int ldx;
        xl_of(l, xl, ldx);
        const float* W = a->kernels + (size_t)l * d * d;
        hipLaunchKernelGGL(cross_matrix_bwd_elem_kernel, dim3(eb), dim3(256), 0, st, a->x, a->x_stride, g, us_r + (size_t)l * bd,
                           a->bias + (size_t)l * d, a->batch, d, du, dx0);
        dctr_train::launch_act_bwd_colsum(st, du, (const float*)nullptr, a->batch, d, 0, a->d_bias + (size_t)l * d);
        // dW[n][k] += sum_b du[b][n] x_l[b][k]:  column-major  dW'(k x n) = X'(k x B) * du'(n x B)^T
        // g[b][k] += sum_n du[b][n] W[n][k]:  column-major  g'(k x B) += W'(k x n) * du'(n x B)
        // both read du and nothing of each other: ONE grouped launch (the dW reduction over the batch as row slices + a sum)
        int rs;
        if (n_parts > 1) {
            const int rs_ = B / n_parts;
            const int64_t dd = (int64_t)d * d;
            dctr_gemm::GroupDesc gd[2];
            gd[0] = dctr_gemm::GroupDesc{};
            gd[0].op_a = dctr_gemm::OP_N; gd[0].op_b = dctr_gemm::OP_T; gd[0].m = d; gd[0].n = d; gd[0].k = rs_;
            gd[0].A = xl; gd[0].lda = ldx; gd[0].stride_a = (int64_t)rs_ * ldx;
            gd[0].B = du; gd[0].ldb = d; gd[0].stride_b = (int64_t)rs_ * d;
            gd[0].C = dw_parts; gd[0].ldc = d; gd[0].stride_c = dd; gd[0].batch = n_parts;
            gd[1] = dctr_gemm::GroupDesc{};
            gd[1].op_a = dctr_gemm::OP_N; gd[1].op_b = dctr_gemm::OP_N; gd[1].m = d; gd[1].n = B; gd[1].k = d;
            gd[1].A = W; gd[1].lda = d; gd[1].B = du; gd[1].ldb = d; gd[1].C = g; gd[1].ldc = d; gd[1].batch = 1; gd[1].accumulate = 1;
            rs = dctr_gemm::sgemm_grouped(st, gd, 2);
            DCTR_REQUIRE(rs == 0, DCTR_E_UNSUPPORTED, "crossnet_bwd: sgemm_grouped(dW, g) failed (%d)", (int)rs);
            int64_t gp = dctr_ceil_div(dd, (int64_t)256);
            dctr_train::launch_sum_parts(st, (unsigned)(gp > 8192 ? 8192 : gp), (const float*)dw_parts, dd, n_parts,
                                         a->d_kernels + (size_t)l * d * d);
        } else {
            rs = dctr_gemm::sgemm(st, dctr_gemm::OP_N, dctr_gemm::OP_T, d, d, B, xl, ldx, du, d, 1.f, a->d_kernels + (size_t)l * d * d, d);
            DCTR_REQUIRE(rs == 0, DCTR_E_UNSUPPORTED, "crossnet_bwd: sgemm(dW) failed (%d)", (int)rs);
            rs = dctr_gemm::sgemm(st, dctr_gemm::OP_N, dctr_gemm::OP_N, d, B, d, W, d, du, d, 1.f, g, d);
            DCTR_REQUIRE(rs == 0, DCTR_E_UNSUPPORTED, "crossnet_bwd: sgemm(g) failed (%d)", (int)rs);
        }
    }
    // d x0 = dx0 + g  (x_0 is also the first x_l)
    dctr_train::launch_add_rows(st, eb, g, (int64_t)d, a->batch, d, dx0, (int64_t)d, 1);
    dctr_train::launch_add_rows(st, eb, dx0, (int64_t)d, a->batch, d, a->dx, a->dx_stride, (int)a->dx_accumulate);
    return dctr_launch_status("dctr_crossnet_bwd");
}

// ---------------------------------------------------------------------------------------------------
// CrossNetMix backward (reference forward: deepctr/layers/interaction.py:511-549, DCNMix):
//   per layer l, expert e:  v1 = tanh(x_l V_e),  v2 = tanh(v1 C_e^T),  out_e = x_0 .* (v2 U_e^T + b_l),  s_e = x_l . g_e
//   p = softmax_e(s),  x_{l+1} = sum_e p_e out_e + x_l
// Nothing is saved by the forward kernel: the intermediates (x_l, v1, v2, uv = v2 U^T, p) are recomputed here into the
// workspace — the low-rank projections as plain GEMMs (dctr_gemm), the gating / softmax / combination as one row kernel — and the
// backward walks the layers in reverse:
//   dp_e = g . out_e,  ds_e = p_e (dp_e - sum_e' p_e' dp_e'),  t_e = p_e g .* x_0   (gradient of  v2 U^T + b)
//   d b += sum_b g .* x_0 (sum_e p_e = 1),  d U_e += t_e^T v2,  d v2 = t_e U_e,  a2 = d v2 .* (1 - v2^2),  d C_e += a2^T v1,
//   d v1 = a2 C_e,  a1 = d v1 .* (1 - v1^2),  d V_e += x_l^T a1,  d g_e += x_l^T ds_e,
//   d x_l = g + sum_e (ds_e (x) g_e + a1 V_e^T),   d x_0 += sum_e p_e g .* (uv_e + b)
// ---------------------------------------------------------------------------------------------------
namespace {

__global__ __launch_bounds__(256) void mix_copy_rows_kernel(const float* __restrict__ x, int64_t x_stride, int64_t batch, int d,
                                                           float* __restrict__ y) {
    const int64_t total = batch * d;
    for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (int64_t)gridDim.x * 256) {
        const int64_t b = o / d;
        y[o] = x[b * x_stride + (o - b * d)];
    }
}

__global__ __launch_bounds__(256) void mix_tanh_kernel(float* __restrict__ v, int64_t n) {
    for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < n; o += (int64_t)gridDim.x * 256) v[o] = tanhf(v[o]);
}

// a = d .* (1 - v^2), in place over d
__global__ __launch_bounds__(256) void mix_tanh_bwd_kernel(float* __restrict__ dv, const float* __restrict__ v, int64_t n) {
    for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < n; o += (int64_t)gridDim.x * 256) dv[o] *= 1.f - v[o] * v[o];
}

__device__ __forceinline__ float mix_wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

constexpr int MIX_MAX_EXPERTS = 16;

// forward combination, one wave per row: p = softmax_e(x_l . g_e),  x_next = sum_e p_e x_0 .* (uv_e + b) + x_l
__global__ __launch_bounds__(256) void mix_combine_kernel(const float* __restrict__ x0, const float* __restrict__ xl,
                                                         const float* __restrict__ uv, int64_t uv_expert_stride,
                                                         const float* __restrict__ gating, const float* __restrict__ bias,
                                                         int64_t batch, int d, int ne, float* __restrict__ p_out,
                                                         float* __restrict__ xn) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= batch) return;
    float s[MIX_MAX_EXPERTS];
    for (int e = 0; e < ne; ++e) {
        float a = 0.f;
        for (int i = lane; i < d; i += 64) a = fmaf(xl[b * d + i], gating[(int64_t)e * d + i], a);
        s[e] = mix_wave_sum(a);
    }
    float mx = s[0];
    for (int e = 1; e < ne; ++e) mx = fmaxf(mx, s[e]);
    float den = 0.f;
    for (int e = 0; e < ne; ++e) {
        s[e] = expf(s[e] - mx);
        den += s[e];
    }
    for (int e = 0; e < ne; ++e) {
        s[e] /= den;
        if (lane == 0) p_out[b * ne + e] = s[e];
    }
    for (int i = lane; i < d; i += 64) {
        float acc = 0.f;
        for (int e = 0; e < ne; ++e) acc = fmaf(s[e], uv[e * uv_expert_stride + b * d + i], acc);
        xn[b * d + i] = fmaf(x0[b * d + i], acc + bias[i], xl[b * d + i]);        // sum_e p_e = 1: the bias comes out of the sum
    }
}

// backward gate part, one wave per row.  In: g (gradient w.r.t. x_{l+1}), x_0, uv_e, p.  Out: ds [B, ne];
// gx = g + sum_e ds_e g_e;  dx0 += sum_e p_e g .* (uv_e + b)      (d_bias[i] += sum_b g x_0: colsum_prod_kernel)
__global__ __launch_bounds__(256) void mix_bwd_gate_kernel(const float* __restrict__ g, const float* __restrict__ x0,
                                                          const float* __restrict__ uv, int64_t uv_expert_stride,
                                                          const float* __restrict__ p, const float* __restrict__ gating,
                                                          const float* __restrict__ bias, int64_t batch, int d, int ne,
                                                          float* __restrict__ ds, float* __restrict__ gx, float* __restrict__ dx0,
                                                          float* __restrict__ d_bias) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= batch) return;
    float pe[MIX_MAX_EXPERTS], dp[MIX_MAX_EXPERTS];
    float mean = 0.f;
    for (int e = 0; e < ne; ++e) {
        pe[e] = p[b * ne + e];
        float a = 0.f;
        for (int i = lane; i < d; i += 64) a = fmaf(g[b * d + i], x0[b * d + i] * (uv[e * uv_expert_stride + b * d + i] + bias[i]), a);
        dp[e] = mix_wave_sum(a);
        mean = fmaf(pe[e], dp[e], mean);
    }
    for (int e = 0; e < ne; ++e) {
        dp[e] = pe[e] * (dp[e] - mean);                                           // now ds_e
        if (lane == 0) ds[b * ne + e] = dp[e];
    }
    for (int i = lane; i < d; i += 64) {
        const float gi = g[b * d + i];
        float a = gi, u = 0.f;
        for (int e = 0; e < ne; ++e) {
            a = fmaf(dp[e], gating[(int64_t)e * d + i], a);
            u = fmaf(pe[e], uv[e * uv_expert_stride + b * d + i], u);
        }
        gx[b * d + i] = a;
        dx0[b * d + i] = fmaf(gi, u + bias[i], dx0[b * d + i]);
    }
}

// out[n] += sum_b a[b, n] * c[b, n]   (the bias gradient of a CrossNetMix layer: one atomic per row and column from the gate kernel
// put B atomics on each address — 214 us per layer at B = 4096): rows strided over few workgroups, one atomic per column each
__global__ __launch_bounds__(256) void colsum_prod_kernel(const float* __restrict__ a, const float* __restrict__ c, int64_t batch, int d,
                                                         float* __restrict__ out) {
    const int n = blockIdx.y * 256 + threadIdx.x;
    if (n >= d) return;
    float acc = 0.f;
#pragma unroll 4
    for (int64_t b = blockIdx.x; b < batch; b += gridDim.x) acc = fmaf(a[b * d + n], c[b * d + n], acc);
    unsafeAtomicAdd(out + n, acc);
}

// t[e][b, i] = p[b, e] g[b, i] x0[b, i] for every expert e
__global__ __launch_bounds__(256) void mix_t_all_kernel(const float* __restrict__ g, const float* __restrict__ x0, const float* __restrict__ p,
                                                       int ne, int64_t batch, int d, float* __restrict__ t) {
    const int64_t bd = batch * d, total = bd * ne;
    for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (int64_t)gridDim.x * 256) {
        const int e = (int)(o / bd);
        const int64_t rem = o - (int64_t)e * bd;
        t[o] = p[(rem / d) * ne + e] * g[rem] * x0[rem];
    }
}

// dx[b, :] (+)= g[b, :] + dx0[b, :];  also used as a strided copy of dy into g
__global__ __launch_bounds__(256) void mix_out_kernel(const float* __restrict__ g, const float* __restrict__ dx0, int64_t batch, int d,
                                                     float* __restrict__ dx, int64_t dx_stride, int accumulate) {
    const int64_t total = batch * d;
    for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (int64_t)gridDim.x * 256) {
        const int64_t b = o / d;
        const float v = g[o] + (dx0 != nullptr ? dx0[o] : 0.f);
        float* dst = dx + b * dx_stride + (o - b * d);
        *dst = accumulate ? *dst + v : v;
    }
}

struct MixPlan {
    size_t X, V1, V2, UV, P, G, GX, T, DX0, DV2, DV1, DS, total;
};
MixPlan mix_plan(int64_t B, int d, int L, int ne, int r) {
    MixPlan m{};
    size_t o = 0;
    auto take = [&](size_t n) { size_t at = o; o += (n + 3) & ~(size_t)3; return at; };
    m.X = take((size_t)L * B * d);
    m.V1 = take((size_t)L * ne * B * r);
    m.V2 = take((size_t)L * ne * B * r);
    m.UV = take((size_t)L * ne * B * d);
    m.P = take((size_t)L * B * ne);
    m.G = take((size_t)B * d);
    m.GX = take((size_t)B * d);
    m.T = take((size_t)ne * B * d);          // per expert: the GEMMs of a layer run as strided batches over the experts
    m.DX0 = take((size_t)B * d);
    m.DV2 = take((size_t)ne * B * r);
    m.DV1 = take((size_t)ne * B * r);
    m.DS = take((size_t)B * ne);
    m.total = o;
    return m;
}

// the sizes dctr_crossnet_mix_bwd takes (the row kernels keep a row's gate in MIX_MAX_EXPERTS registers); its dry check asks the same
bool mix_bwd_sizes_ok(int d, int L, int ne, int r) { return d >= 1 && L >= 0 && ne >= 1 && ne <= MIX_MAX_EXPERTS && r >= 1; }

}  // namespace

extern "C" int dctr_crossnet_mix_bwd_supported(int32_t dim, int32_t layers, int32_t experts, int32_t low_rank) {
    return mix_bwd_sizes_ok(dim, layers, experts, low_rank) ? 1 : 0;
}

extern "C" size_t dctr_crossnet_mix_bwd_workspace_bytes(const dctr_crossnet_mix_bwd_args_t* a) {
    if (a == nullptr || a->batch <= 0 || a->dim <= 0 || a->layers <= 0 || a->experts <= 0 || a->low_rank <= 0) return 0;
    return mix_plan(a->batch, a->dim, a->layers, a->experts, a->low_rank).total * sizeof(float);
}

extern "C" int dctr_crossnet_mix_bwd(const dctr_crossnet_mix_bwd_args_t* a, void* stream) {
    DCTR_REQUIRE(a != nullptr, DCTR_E_NULL, "crossnet_mix_bwd: null args");
    DCTR_REQUIRE(a->batch >= 0 && mix_bwd_sizes_ok(a->dim, a->layers, a->experts, a->low_rank), DCTR_E_DIM,
                 "crossnet_mix_bwd: bad sizes (batch=%lld dim=%d layers=%d experts=%d (max %d) low_rank=%d)", (long long)a->batch,
                 a->dim, a->layers, a->experts, MIX_MAX_EXPERTS, a->low_rank);
    if (a->batch == 0) return DCTR_OK;
    DCTR_REQUIRE(a->x && a->dy && a->dx && a->x_stride >= a->dim && a->dy_stride >= a->dim && a->dx_stride >= a->dim, DCTR_E_NULL,
                 "crossnet_mix_bwd: null x / dy / dx or a stride < dim");
    hipStream_t st = (hipStream_t)stream;
    const int64_t B = a->batch;
    const int d = a->dim, L = a->layers, ne = a->experts, r = a->low_rank;
    auto grid = [](int64_t n) { int64_t g = dctr_ceil_div(n, (int64_t)256); return dim3((unsigned)(g < 8192 ? g : 8192)); };
    if (L == 0) {                                                  // identity: dx (+)= dy
        DCTR_REQUIRE(a->workspace != nullptr && a->workspace_bytes >= (size_t)B * d * sizeof(float), DCTR_E_NULL,
                     "crossnet_mix_bwd: layers == 0 needs a workspace of batch * dim floats");
        hipLaunchKernelGGL(mix_copy_rows_kernel, grid(B * d), dim3(256), 0, st, a->dy, a->dy_stride, B, d, (float*)a->workspace);
        hipLaunchKernelGGL(mix_out_kernel, grid(B * d), dim3(256), 0, st, (const float*)a->workspace, (const float*)nullptr, B, d, a->dx,
                           a->dx_stride, (int)a->dx_accumulate);
        return dctr_launch_status("dctr_crossnet_mix_bwd");
    }
    DCTR_REQUIRE(a->U && a->V && a->C && a->gating && a->bias && a->dU && a->dV && a->dC && a->dgating && a->dbias, DCTR_E_NULL,
                 "crossnet_mix_bwd: null weights / gradients");
    const MixPlan m = mix_plan(B, d, L, ne, r);
    DCTR_REQUIRE(a->workspace != nullptr && a->workspace_bytes >= m.total * sizeof(float), DCTR_E_NULL,
                 "crossnet_mix_bwd: needs a workspace of dctr_crossnet_mix_bwd_workspace_bytes() bytes");
    DCTR_REQUIRE(B < 0x7fffffffLL / (d > r ? d : r), DCTR_E_DIM, "crossnet_mix_bwd: batch too large");
    float* ws = static_cast<float*>(a->workspace);
    const float one = 1.f, zero = 0.f;
    const int Bi = (int)B;
    const int64_t Br = B * r, Bd = B * d;
    const unsigned row_blocks = (unsigned)dctr_ceil_div(B, (int64_t)4);
#define MIX_GEMM(ta, tb, mm, nn, kk, A_, lda, B_, ldb, beta, C_, ldc)                                                      \
    do {                                                                                                                   \
        int rs_ = dctr_gemm::sgemm(st, ta, tb, mm, nn, kk, A_, lda, B_, ldb, *(beta), C_, ldc);                  \
        DCTR_REQUIRE(rs_ == 0, DCTR_E_UNSUPPORTED, "crossnet_mix_bwd: sgemm failed (%d)", (int)rs_); \
    } while (0)
#define MIX_BGEMM(ta, tb, mm, nn, kk, A_, lda, sa, B_, ldb, sb, beta, C_, ldc, sc)                                            \
    do {                                                                                                                   \
        int rs_ = dctr_gemm::sgemm_strided_batched(st, ta, tb, mm, nn, kk, A_, lda, (int64_t)(sa), B_, ldb, \
                                                           (int64_t)(sb), *(beta), C_, ldc, (int64_t)(sc), ne);     \
        DCTR_REQUIRE(rs_ == 0, DCTR_E_UNSUPPORTED, "crossnet_mix_bwd: sgemm_strided_batched failed (%d)", (int)rs_); \
    } while (0)
    const dctr_gemm::Op N_ = dctr_gemm::OP_N, T_ = dctr_gemm::OP_T;
    // ---- forward recompute.  X[0] = x_0 (contiguous copy), X[l+1] needed only for l + 1 < L
    hipLaunchKernelGGL(mix_copy_rows_kernel, grid(Bd), dim3(256), 0, st, a->x, a->x_stride, B, d, ws + m.X);
    const float* x0 = ws + m.X;
    for (int l = 0; l < L; ++l) {
        const float* xl = ws + m.X + (size_t)l * Bd;
        {
            // the experts of a layer as ONE strided batch per GEMM (4 experts x 3 GEMMs x 2 tanh launches per layer before: the
            // step spent 1.0 of its 1.74 ms in 106 small rocBLAS calls)
            const size_t l0 = (size_t)l * ne;
            const float* Ul = a->U + l0 * d * r;
            const float* Vl = a->V + l0 * d * r;
            const float* Cl = a->C + l0 * r * r;
            float* v1 = ws + m.V1 + l0 * Br;
            float* v2 = ws + m.V2 + l0 * Br;
            float* uv = ws + m.UV + l0 * Bd;
            MIX_BGEMM(N_, N_, r, Bi, d, Vl, r, (int64_t)d * r, xl, d, 0, &zero, v1, r, Br);      // v1'(r x B) = V'(r x d) x_l'(d x B)
            hipLaunchKernelGGL(mix_tanh_kernel, grid(ne * Br), dim3(256), 0, st, v1, ne * Br);
            MIX_BGEMM(T_, N_, r, Bi, r, Cl, r, (int64_t)r * r, (const float*)v1, r, Br, &zero, v2, r, Br);   // v2[b, j] = sum_k C[j][k] v1[b, k]
            hipLaunchKernelGGL(mix_tanh_kernel, grid(ne * Br), dim3(256), 0, st, v2, ne * Br);
            MIX_BGEMM(T_, N_, d, Bi, r, Ul, r, (int64_t)d * r, (const float*)v2, r, Br, &zero, uv, d, Bd);   // uv[b, i] = sum_j U[i][j] v2[b, j]
        }
        // the last layer's output is not needed (its gradient comes in as dy); the kernel still needs somewhere to write: GX
        float* xn = l + 1 < L ? ws + m.X + (size_t)(l + 1) * Bd : ws + m.GX;
        hipLaunchKernelGGL(mix_combine_kernel, dim3(row_blocks), dim3(256), 0, st, x0, xl, (const float*)(ws + m.UV + (size_t)l * ne * Bd),
                           Bd, a->gating, a->bias + (size_t)l * d, B, d, ne, ws + m.P + (size_t)l * B * ne, xn);
    }
    // ---- backward
    float* g = ws + m.G;
    float* gx = ws + m.GX;
    hipLaunchKernelGGL(mix_copy_rows_kernel, grid(Bd), dim3(256), 0, st, a->dy, a->dy_stride, B, d, g);
    hipError_t me = hipMemsetAsync(ws + m.DX0, 0, (size_t)Bd * sizeof(float), st);
    DCTR_REQUIRE(me == hipSuccess, (int)me, "crossnet_mix_bwd: memset failed: %s", hipGetErrorString(me));
    for (int l = L - 1; l >= 0; --l) {
        const float* xl = ws + m.X + (size_t)l * Bd;
        const float* p = ws + m.P + (size_t)l * B * ne;
        const float* uvl = ws + m.UV + (size_t)l * ne * Bd;
        hipLaunchKernelGGL(mix_bwd_gate_kernel, dim3(row_blocks), dim3(256), 0, st, (const float*)g, x0, uvl, Bd, p, a->gating,
                           a->bias + (size_t)l * d, B, d, ne, ws + m.DS, gx, ws + m.DX0, a->dbias + (size_t)l * d);
        hipLaunchKernelGGL(colsum_prod_kernel, dim3((unsigned)(B < COLSUM_MAX_WG ? B : COLSUM_MAX_WG), (unsigned)((d + 255) / 256)), dim3(256),
                           0, st, (const float*)g, x0, B, d, a->dbias + (size_t)l * d);
        {
            // Independent products share a launch (dctr_gemm::sgemm_grouped): {d gating, dU, dv2}, {dC, dv1}, {dV, gx of expert 0} —
            // 13 GEMM launches per layer were 6 + ne; the small outputs under the batch-long reduction (d gating, dU, dC, dV) add
            // their k slices with float atomics as dctr_gemm::sgemm does for such shapes
            const size_t l0 = (size_t)l * ne;
            const float* Ul = a->U + l0 * d * r;
            const float* Vl = a->V + l0 * d * r;
            const float* Cl = a->C + l0 * r * r;
            const float* v1 = ws + m.V1 + l0 * Br;
            const float* v2 = ws + m.V2 + l0 * Br;
            float* t = ws + m.T;
            float* dv2 = ws + m.DV2;
            float* dv1 = ws + m.DV1;
            const int ks = dctr_gemm::k_slices(Bi, 256) > 16 ? 16 : dctr_gemm::k_slices(Bi, 256);
            auto desc = [&](dctr_gemm::Op ta, dctr_gemm::Op tb, int mm, int nn, int kk, const float* A_, int lda, int64_t sa, const float* B_,
                            int ldb, int64_t sb, float* C_, int ldc, int64_t sc, int batch, bool acc, bool long_k) {
                dctr_gemm::GroupDesc gd_ = dctr_gemm::GroupDesc{};
                gd_.op_a = ta; gd_.op_b = tb; gd_.m = mm; gd_.n = nn; gd_.k = kk; gd_.A = A_; gd_.lda = lda; gd_.stride_a = sa;
                gd_.B = B_; gd_.ldb = ldb; gd_.stride_b = sb; gd_.C = C_; gd_.ldc = ldc; gd_.stride_c = sc; gd_.batch = batch;
                gd_.accumulate = acc ? 1 : 0;
                if (long_k && acc) gd_.k_slices = dctr_gemm::k_slices(kk, (kk + ks - 1) / ks);
                return gd_;
            };
            hipLaunchKernelGGL(mix_t_all_kernel, grid(ne * Bd), dim3(256), 0, st, (const float*)g, x0, p, ne, B, d, t);
            dctr_gemm::GroupDesc g1[3] = {
                // d gating[e][i] += sum_b ds[b, e] x_l[b, i]:  column-major dG'(d x ne) += x_l'(d x B) ds'(ne x B)^T
                desc(N_, T_, d, ne, Bi, xl, d, 0, (const float*)(ws + m.DS), ne, 0, a->dgating, d, 0, 1, true, true),
                // dU[i][j] += sum_b t[b,i] v2[b,j]
                desc(N_, T_, r, d, Bi, v2, r, Br, (const float*)t, d, Bd, a->dU + l0 * d * r, r, (int64_t)d * r, ne, true, true),
                // dv2[b,j] = sum_i t[b,i] U[i][j]
                desc(N_, N_, r, Bi, d, Ul, r, (int64_t)d * r, (const float*)t, d, Bd, dv2, r, Br, ne, false, false)};
            int rsg = dctr_gemm::sgemm_grouped(st, g1, 3);
            DCTR_REQUIRE(rsg == 0, DCTR_E_UNSUPPORTED, "crossnet_mix_bwd: sgemm_grouped(1) failed (%d)", rsg);
            hipLaunchKernelGGL(mix_tanh_bwd_kernel, grid(ne * Br), dim3(256), 0, st, dv2, v2, ne * Br);                    // a2
            dctr_gemm::GroupDesc g2[2] = {
                // dC[j][k] += sum_b a2[b,j] v1[b,k]
                desc(N_, T_, r, r, Bi, v1, r, Br, (const float*)dv2, r, Br, a->dC + l0 * r * r, r, (int64_t)r * r, ne, true, true),
                // dv1[b,k] = sum_j a2[b,j] C[j][k]
                desc(N_, N_, r, Bi, r, Cl, r, (int64_t)r * r, (const float*)dv2, r, Br, dv1, r, Br, ne, false, false)};
            rsg = dctr_gemm::sgemm_grouped(st, g2, 2);
            DCTR_REQUIRE(rsg == 0, DCTR_E_UNSUPPORTED, "crossnet_mix_bwd: sgemm_grouped(2) failed (%d)", rsg);
            hipLaunchKernelGGL(mix_tanh_bwd_kernel, grid(ne * Br), dim3(256), 0, st, dv1, v1, ne * Br);                    // a1
            dctr_gemm::GroupDesc g3[2] = {
                // dV[i][j] += sum_b x_l[b,i] a1[b,j]
                desc(N_, T_, r, d, Bi, (const float*)dv1, r, Br, xl, d, 0, a->dV + l0 * d * r, r, (int64_t)d * r, ne, true, true),
                // gx[b,i] += sum_j a1[b,j] V[i][j]: one output, expert by expert — expert 0 here, the others behind it
                desc(T_, N_, d, Bi, r, Vl, r, 0, (const float*)dv1, r, 0, gx, d, 0, 1, true, false)};
            rsg = dctr_gemm::sgemm_grouped(st, g3, 2);
            DCTR_REQUIRE(rsg == 0, DCTR_E_UNSUPPORTED, "crossnet_mix_bwd: sgemm_grouped(3) failed (%d)", rsg);
            for (int e = 1; e < ne; ++e)
                MIX_GEMM(T_, N_, d, Bi, r, Vl + (size_t)e * d * r, r, (const float*)(dv1 + (size_t)e * Br), r, &one, gx, d);
        }
        float* tmp = g;
        g = gx;
        gx = tmp;
    }
#undef MIX_GEMM
#undef MIX_BGEMM
    hipLaunchKernelGGL(mix_out_kernel, grid(Bd), dim3(256), 0, st, (const float*)g, (const float*)(ws + m.DX0), B, d, a->dx, a->dx_stride,
                       (int)a->dx_accumulate);
    return dctr_launch_status("dctr_crossnet_mix_bwd");
}
