// The DNN backward of the HIP training step.
//   dctr_mlp_bwd (+ _workspace_bytes, _join), dctr_dense1_bwd
//                             backward of DNN.call + Dense(1) head (layers/core.py:189-208) on dctr_gemm (gemm_kernels.hip) and
//                             the chain of mlp_bwd_kernels.hip
//   dctr_dice_train_fwd       Dice under training=True (layers/activation.py:51-64)
//   dctr_dnn_train_layer_fwd / _bwd   BatchNormalization and Dropout under training=True (layers/core.py:196-208)
// Also the launchers of namespace dctr_train (declared in train_common.h), next to their kernels: cin_layered_kernels.hip and
// crossnet_bwd_kernels.hip reach head_bwd / act_bwd_colsum / add_rows / sum_parts through them.  Dice and the train-layer passes
// stay in this unit because dctr_mlp_bwd launches the Dice kernels directly.  The reference has no code of its own for any of
// this (Keras autodiff): the formulas are the derivatives of the forward expressions cited at each section.
#include <stdlib.h>

#include "dctr_gemm.h"

#include "dctr_common.h"
#include "train_common.h"

namespace {

// ---------------------------------------------------------------------------------------------------
// DNN backward helpers
// ---------------------------------------------------------------------------------------------------
// dZ[b, n] = dlogit[b] * head_w[n] * act'(h[b, n]);   d_head_w[n] += sum_b dlogit[b] * h[b, n]
// (any N / strides: thread = one column (blockIdx.y * 256 + threadIdx.x), rows grid-strided over blockIdx.x; the 16-B forms below
// take over when the shapes allow)
__global__ __launch_bounds__(256) void head_bwd_kernel(const float* __restrict__ dlogit, const float* __restrict__ head_w,
                                                       const float* __restrict__ h, int64_t h_stride, int64_t batch, int N,
                                                       int act, float* __restrict__ dz, int64_t dz_stride,
                                                       float* __restrict__ d_head_w) {
    const int n = blockIdx.y * 256 + threadIdx.x;
    if (n >= N) return;
    const float hw = head_w[n];
    float acc = 0.f;
#pragma unroll 4
    for (int64_t b = blockIdx.x; b < batch; b += gridDim.x) {
        const float hv = h[b * h_stride + n], dl = dlogit[b];
        float d = dl * hw;
        if (act == DCTR_ACT_RELU) d = hv > 0.f ? d : 0.f;
        else if (act == DCTR_ACT_SIGMOID) d *= hv * (1.f - hv);
        else if (act == DCTR_ACT_TANH) d *= 1.f - hv * hv;
        else if (dctr_act::is_extended(act)) d *= dctr_act::deriv_from_output(act, hv);
        dz[b * dz_stride + n] = d;
        acc = fmaf(dl, hv, acc);
    }
    unsafeAtomicAdd(d_head_w + n, acc);
}

// in place: dh[i] *= act'(z[i] + bias[i % N]) with act' taken from the PRE-activation (swish / gelu: dctr_mlp_bwd's layer-by-layer form)
__global__ __launch_bounds__(256) void act_bwd_from_z_kernel(float* __restrict__ dh, const float* __restrict__ z,
                                                             const float* __restrict__ bias, int64_t total, int N, int act) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const float zv = z[i] + (bias != nullptr ? bias[(int)(i % N)] : 0.f);
        dh[i] *= dctr_act::deriv_from_z(act, zv);
    }
}

// in place: dh[b, n] *= act'(h[b, n]);  db[n] += sum_b dz[b, n]   (also used with h == NULL: only the column sums)
__global__ __launch_bounds__(256) void act_bwd_colsum_kernel(float* __restrict__ dh, const float* __restrict__ h, int64_t batch,
                                                             int N, int act, float* __restrict__ db) {
    const int n = blockIdx.y * 256 + threadIdx.x;
    if (n >= N) return;
    float acc = 0.f;
#pragma unroll 4
    for (int64_t b = blockIdx.x; b < batch; b += gridDim.x) {
        float d = dh[b * N + n];
        if (h != nullptr) {
            const float hv = h[b * N + n];
            if (act == DCTR_ACT_RELU) d = hv > 0.f ? d : 0.f;
            else if (act == DCTR_ACT_SIGMOID) d *= hv * (1.f - hv);
            else if (act == DCTR_ACT_TANH) d *= 1.f - hv * hv;
            else if (dctr_act::is_extended(act)) d *= dctr_act::deriv_from_output(act, hv);
            dh[b * N + n] = d;
        }
        acc += d;
    }
    if (db != nullptr) unsafeAtomicAdd(db + n, acc);
}

// The two helpers above with 16-B accesses and the rows spread over the workgroup: thread (rl, c) owns columns 4c .. 4c+3 of rows
// rl, rl + RL, ... (RL = 256 / (N/4) row lanes; a workgroup sweeps RL x N contiguous floats per iteration, grid-stride), the column
// sums meet in LDS and leave as ONE atomic per column and workgroup (N % 4 == 0, N <= 1024, strides % 4 == 0, 16-B aligned).
__global__ __launch_bounds__(256) void head_bwd4_kernel(const float* __restrict__ dlogit, const float* __restrict__ head_w,
                                                        const float* __restrict__ h, int64_t h_stride, int64_t batch, int N,
                                                        int act, float* __restrict__ dz, int64_t dz_stride,
                                                        float* __restrict__ d_head_w) {
    const int N4 = N >> 2, RL = 256 / N4;
    const int c = threadIdx.x % N4, rl = threadIdx.x / N4;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (rl < RL) {
        const float4 hw = *reinterpret_cast<const float4*>(head_w + 4 * c);
#pragma unroll 4
        for (int64_t r = (int64_t)blockIdx.x * RL + rl; r < batch; r += (int64_t)gridDim.x * RL) {
            const float4 hv = *reinterpret_cast<const float4*>(h + r * h_stride + 4 * c);
            const float dl = dlogit[r];
            const float4 d = act_grad4(make_float4(dl * hw.x, dl * hw.y, dl * hw.z, dl * hw.w), hv, act);
            *reinterpret_cast<float4*>(dz + r * dz_stride + 4 * c) = d;
            acc.x = fmaf(dl, hv.x, acc.x); acc.y = fmaf(dl, hv.y, acc.y); acc.z = fmaf(dl, hv.z, acc.z); acc.w = fmaf(dl, hv.w, acc.w);
        }
    }
    colsum4_finish(acc, N4, RL, c, d_head_w);
}

__global__ __launch_bounds__(256) void act_bwd_colsum4_kernel(float* __restrict__ dh, const float* __restrict__ h, int64_t batch,
                                                              int N, int act, float* __restrict__ db) {
    const int N4 = N >> 2, RL = 256 / N4;
    const int c = threadIdx.x % N4, rl = threadIdx.x / N4;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (rl < RL) {
#pragma unroll 4
        for (int64_t r = (int64_t)blockIdx.x * RL + rl; r < batch; r += (int64_t)gridDim.x * RL) {
            float4 d = *reinterpret_cast<const float4*>(dh + r * N + 4 * c);
            if (h != nullptr) {
                d = act_grad4(d, *reinterpret_cast<const float4*>(h + r * N + 4 * c), act);
                *reinterpret_cast<float4*>(dh + r * N + 4 * c) = d;
            }
            acc.x += d.x; acc.y += d.y; acc.z += d.z; acc.w += d.w;
        }
    }
    colsum4_finish(acc, N4, RL, c, db);
}

// out[b, c] (+)= src[b, c]   (strided rows)
__global__ __launch_bounds__(256) void add_rows_kernel(const float* __restrict__ src, int64_t src_stride, int64_t batch, int d,
                                                       float* __restrict__ out, int64_t out_stride, int accumulate) {
    const int64_t total = batch * d;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / d;
        const int c = (int)(i - b * d);
        out[b * out_stride + c] = (accumulate ? out[b * out_stride + c] : 0.f) + src[b * src_stride + c];
    }
}

// out[i] += sum_s parts[s * n + i]
__global__ __launch_bounds__(256) void sum_parts_kernel(const float* __restrict__ parts, int64_t n, int n_parts,
                                                        float* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;          // four independent chains: the loads of 4 slices in flight per step
        int s = 0;
        for (; s + 4 <= n_parts; s += 4) {
            a0 += parts[(int64_t)s * n + i];
            a1 += parts[(int64_t)(s + 1) * n + i];
            a2 += parts[(int64_t)(s + 2) * n + i];
            a3 += parts[(int64_t)(s + 3) * n + i];
        }
        for (; s < n_parts; ++s) a0 += parts[(int64_t)s * n + i];
        out[i] += (a0 + a1) + (a2 + a3);
    }
}

}  // namespace

// the launchers of the kernels above: declared in train_common.h, called from the DNN hosts below and from
// crossnet_bwd_kernels.hip and cin_layered_kernels.hip
namespace dctr_train {

// launch either form: the 16-B one when the shapes allow it
void launch_act_bwd_colsum(hipStream_t st, float* dh, const float* h, int64_t batch, int N, int act, float* db) {
    if (N % 4 == 0 && N <= 1024 && dctr_aligned16(dh) && (h == nullptr || dctr_aligned16(h))) {
        const int RL = 256 / (N / 4);
        int64_t g = dctr_ceil_div(batch, (int64_t)RL * 4);           // >= 4 rows per thread where the batch has them
        // atomics on ONE address serialise at ~100 ns each on this part (measured: 256 workgroups x 256 columns = 27 us of a
        // 4-MB pass): with column sums wanted, few workgroups with long row loops; without, as many as the rows give
        const int64_t cap = db != nullptr ? (int64_t)colsum_grid(batch, RL) : 1024;
        g = g < 1 ? 1 : (g > cap ? cap : g);
        hipLaunchKernelGGL(act_bwd_colsum4_kernel, dim3((unsigned)g), dim3(256), 0, st, dh, h, batch, N, act, db);
    } else {
        const int64_t gx = db != nullptr ? COLSUM_MAX_WG : 1024;
        hipLaunchKernelGGL(act_bwd_colsum_kernel, dim3((unsigned)(batch < gx ? batch : gx), (unsigned)((N + 255) / 256)), dim3(256), 0, st,
                           dh, h, batch, N, act, db);
    }
}

void launch_head_bwd(hipStream_t st, const float* dlogit, const float* head_w, const float* h, int64_t h_stride, int64_t batch,
                     int N, int act, float* dz, int64_t dz_stride, float* d_head_w) {
    if (N % 4 == 0 && N <= 1024 && h_stride % 4 == 0 && dz_stride % 4 == 0 && dctr_aligned16(h) && dctr_aligned16(dz) &&
        dctr_aligned16(head_w)) {
        const int RL = 256 / (N / 4);
        int64_t g = dctr_ceil_div(batch, (int64_t)RL * 4);
        g = colsum_grid(batch, RL);
        hipLaunchKernelGGL(head_bwd4_kernel, dim3((unsigned)g), dim3(256), 0, st, dlogit, head_w, h, h_stride, batch, N, act, dz,
                           dz_stride, d_head_w);
    } else {
        hipLaunchKernelGGL(head_bwd_kernel, dim3((unsigned)(batch < COLSUM_MAX_WG ? batch : COLSUM_MAX_WG), (unsigned)((N + 255) / 256)),
                           dim3(256), 0, st, dlogit, head_w, h, h_stride, batch, N, act, dz, dz_stride, d_head_w);
    }
}

void launch_add_rows(hipStream_t st, unsigned blocks, const float* src, int64_t src_stride, int64_t batch, int d, float* out,
                     int64_t out_stride, int accumulate) {
    hipLaunchKernelGGL(add_rows_kernel, dim3(blocks), dim3(256), 0, st, src, src_stride, batch, d, out, out_stride, accumulate);
}

void launch_sum_parts(hipStream_t st, unsigned blocks, const float* parts, int64_t n, int n_parts, float* out) {
    hipLaunchKernelGGL(sum_parts_kernel, dim3(blocks), dim3(256), 0, st, parts, n, n_parts, out);
}

}  // namespace dctr_train

namespace {

// ---------------------------------------------------------------------------------------------------
// Dice (layers/activation.py:59-64, inference statistics):  y = z (alpha + (1 - alpha) p),  p = sigmoid((z - mean) / sqrt(var + eps))
//   dy/dz = alpha + (1 - alpha) p + z (1 - alpha) p (1 - p) / sqrt(var + eps);   dy/dalpha = z (1 - p)
// z is not recoverable from y, so dctr_mlp_bwd recomputes Z = X W with one more GEMM and this kernel adds the bias.
// in place: dh[b,n] (gradient w.r.t. y) -> gradient w.r.t. z;  d_alpha[n] += sum_b dh[b,n] z (1 - p)
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dice_bwd_kernel(float* __restrict__ dh, const float* __restrict__ zw, const float* __restrict__ bias,
                                                       const float* __restrict__ alpha, const float* __restrict__ mean,
                                                       const float* __restrict__ var, float eps, int64_t batch, int N,
                                                       float* __restrict__ d_alpha) {
    for (int n = threadIdx.x; n < N; n += 256) {
        const float bn = bias != nullptr ? bias[n] : 0.f, al = alpha[n], mu = mean[n];
        const float rs = 1.f / sqrtf(var[n] + eps);
        float acc = 0.f;
        for (int64_t r0 = (int64_t)blockIdx.x * BWD_ROWS; r0 < batch; r0 += (int64_t)gridDim.x * BWD_ROWS)     // grid-stride: few workgroups when column sums follow
        for (int r = 0; r < BWD_ROWS; ++r) {
            const int64_t b = r0 + r;
            if (b >= batch) break;
            const float z = zw[b * N + n] + bn;
            const float p = 1.f / (1.f + expf(-(z - mu) * rs));
            const float d = dh[b * N + n];
            acc = fmaf(d, z * (1.f - p), acc);
            dh[b * N + n] = d * (al + (1.f - al) * p + z * (1.f - al) * p * (1.f - p) * rs);
        }
        if (d_alpha != nullptr) unsafeAtomicAdd(d_alpha + n, acc);
    }
}

// ---------------------------------------------------------------------------------------------------
// Dice under training=True (layers/activation.py:51-64: BatchNormalization(center=False, scale=False, epsilon=1e-9) called with
// the training flag): the statistics are those of THIS batch over every row (biased variance), gradients flow through them,
// and the stored statistics move towards them with the layer's momentum.
//   xn = (z - mu) rs,  p = sigmoid(xn),  y = z (alpha + (1 - alpha) p)
//   dy/dz (direct) = alpha + (1 - alpha) p;   dxn = dy * z (1 - alpha) * p (1 - p);   dalpha = sum dy * z (1 - p)
//   dz = dy * direct + rs * (dxn - mean_rows(dxn) - xn * mean_rows(dxn * xn))          (BatchNormalization backward)
// Column statistics: two passes over z (sum -> mean, then sum of squared deviations): E[z^2] - E[z]^2 would cancel in fp32.
// ---------------------------------------------------------------------------------------------------
// pass kind 0: acc[n] += sum_b (z + bias);  kind 1: acc[n] += sum_b (z + bias - mean)^2     (mean = acc0 / rows)
__global__ __launch_bounds__(256) void dice_colstat_kernel(const float* __restrict__ z, int64_t z_stride, const float* __restrict__ bias,
                                                          int64_t rows, int N, int kind, const float* __restrict__ sum0,
                                                          float* __restrict__ acc) {
    const float inv = 1.f / (float)rows;
    for (int n = threadIdx.x; n < N; n += 256) {
        const float bn = bias != nullptr ? bias[n] : 0.f;
        const float mu = kind ? sum0[n] * inv : 0.f;
        float a = 0.f;
        for (int64_t r0 = (int64_t)blockIdx.x * BWD_ROWS; r0 < rows; r0 += (int64_t)gridDim.x * BWD_ROWS)     // grid-stride: few workgroups when column sums follow
        for (int r = 0; r < BWD_ROWS; ++r) {
            const int64_t b = r0 + r;
            if (b >= rows) break;
            const float v = z[b * z_stride + n] + bn - mu;
            a += kind ? v * v : v;
        }
        unsafeAtomicAdd(acc + n, a);
    }
}

// sums -> batch mean / biased variance (in place), stored statistics moved towards them
__global__ void dice_stat_finish_kernel(float* __restrict__ mean_sum, float* __restrict__ var_sum, int64_t rows, int N, float momentum,
                                        float* __restrict__ moving_mean, float* __restrict__ moving_var) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const float inv = 1.f / (float)rows;
    const float m = mean_sum[n] * inv, v = var_sum[n] * inv;
    mean_sum[n] = m;
    var_sum[n] = v;
    if (moving_mean != nullptr) moving_mean[n] = moving_mean[n] * momentum + m * (1.f - momentum);
    if (moving_var != nullptr) moving_var[n] = moving_var[n] * momentum + v * (1.f - momentum);
}

__global__ __launch_bounds__(256) void dice_apply_kernel(const float* __restrict__ z, int64_t z_stride, const float* __restrict__ bias,
                                                        const float* __restrict__ alpha, const float* __restrict__ mean,
                                                        const float* __restrict__ var, float eps, int64_t rows, int N,
                                                        float* __restrict__ h, int64_t h_stride) {
    const int64_t total = rows * N;
    for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (int64_t)gridDim.x * 256) {
        const int64_t b = o / N;
        const int n = (int)(o - b * N);
        const float zz = z[b * z_stride + n] + (bias != nullptr ? bias[n] : 0.f);
        const float p = 1.f / (1.f + expf(-(zz - mean[n]) / sqrtf(var[n] + eps)));
        h[b * h_stride + n] = zz * (alpha[n] + (1.f - alpha[n]) * p);
    }
}

// backward pass 1: S1[n] += sum dxn, S2[n] += sum dxn xn, d_alpha[n] += sum dy z (1 - p)      (zw = X W without the bias)
__global__ __launch_bounds__(256) void dice_train_bwd_reduce_kernel(const float* __restrict__ dh, const float* __restrict__ zw,
                                                                   const float* __restrict__ bias, const float* __restrict__ alpha,
                                                                   const float* __restrict__ mean, const float* __restrict__ var,
                                                                   float eps, int64_t batch, int N, float* __restrict__ s12,
                                                                   float* __restrict__ d_alpha) {
    for (int n = threadIdx.x; n < N; n += 256) {
        const float bn = bias != nullptr ? bias[n] : 0.f, al = alpha[n], mu = mean[n];
        const float rs = 1.f / sqrtf(var[n] + eps);
        float a1 = 0.f, a2 = 0.f, aa = 0.f;
        for (int64_t r0 = (int64_t)blockIdx.x * BWD_ROWS; r0 < batch; r0 += (int64_t)gridDim.x * BWD_ROWS)     // grid-stride: few workgroups when column sums follow
        for (int r = 0; r < BWD_ROWS; ++r) {
            const int64_t b = r0 + r;
            if (b >= batch) break;
            const float z = zw[b * N + n] + bn;
            const float xn = (z - mu) * rs;
            const float p = 1.f / (1.f + expf(-xn));
            const float d = dh[b * N + n];
            const float dxn = d * z * (1.f - al) * p * (1.f - p);
            a1 += dxn;
            a2 = fmaf(dxn, xn, a2);
            aa = fmaf(d, z * (1.f - p), aa);
        }
        unsafeAtomicAdd(s12 + n, a1);
        unsafeAtomicAdd(s12 + N + n, a2);
        if (d_alpha != nullptr) unsafeAtomicAdd(d_alpha + n, aa);
    }
}

// backward pass 2, in place: dh (gradient w.r.t. y) -> gradient w.r.t. z
__global__ __launch_bounds__(256) void dice_train_bwd_apply_kernel(float* __restrict__ dh, const float* __restrict__ zw,
                                                                  const float* __restrict__ bias, const float* __restrict__ alpha,
                                                                  const float* __restrict__ mean, const float* __restrict__ var,
                                                                  float eps, int64_t batch, int N, const float* __restrict__ s12) {
    const float inv = 1.f / (float)batch;
    for (int n = threadIdx.x; n < N; n += 256) {
        const float bn = bias != nullptr ? bias[n] : 0.f, al = alpha[n], mu = mean[n];
        const float rs = 1.f / sqrtf(var[n] + eps);
        const float m1 = s12[n] * inv, m2 = s12[N + n] * inv;
        for (int64_t r0 = (int64_t)blockIdx.x * BWD_ROWS; r0 < batch; r0 += (int64_t)gridDim.x * BWD_ROWS)     // grid-stride: few workgroups when column sums follow
        for (int r = 0; r < BWD_ROWS; ++r) {
            const int64_t b = r0 + r;
            if (b >= batch) break;
            const float z = zw[b * N + n] + bn;
            const float xn = (z - mu) * rs;
            const float p = 1.f / (1.f + expf(-xn));
            const float d = dh[b * N + n];
            const float dxn = d * z * (1.f - al) * p * (1.f - p);
            dh[b * N + n] = d * (al + (1.f - al) * p) + rs * (dxn - m1 - xn * m2);
        }
    }
}

// The three Dice passes that end in column sums, in the 16-B / row-lane layout of act_bwd_colsum4_kernel (N % 4 == 0, N <= 1024):
// DIN runs them on B*T = 102,400 rows x 80 / 40 columns, where one workgroup per 16 rows meant 6,400 atomics per column address
// (140-190 us per pass, all of it the serialised atomics).
template <int K>
__device__ __forceinline__ void colsum4_finish_k(const float (&acc)[K][4], int N4, int RL, int c, float* const (&out)[K]) {
    __shared__ float red[K][256][4];
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) red[k][threadIdx.x][j] = acc[k][j];
    __syncthreads();
    if ((int)threadIdx.x < N4) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (out[k] == nullptr) continue;
            float t[4] = {red[k][c][0], red[k][c][1], red[k][c][2], red[k][c][3]};
            for (int r = 1; r < RL; ++r)
#pragma unroll
                for (int j = 0; j < 4; ++j) t[j] += red[k][r * N4 + c][j];
#pragma unroll
            for (int j = 0; j < 4; ++j) unsafeAtomicAdd(out[k] + 4 * c + j, t[j]);
        }
    }
}

struct DiceCols {            // per-thread constants of its four columns
    float bn[4], al[4], mu[4], rs[4];
};
__device__ __forceinline__ DiceCols dice_cols(const float* bias, const float* alpha, const float* mean, const float* var, float eps, int c) {
    DiceCols k;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = 4 * c + j;
        k.bn[j] = bias != nullptr ? bias[n] : 0.f;
        k.al[j] = alpha != nullptr ? alpha[n] : 0.f;
        k.mu[j] = mean != nullptr ? mean[n] : 0.f;
        k.rs[j] = var != nullptr ? 1.f / sqrtf(var[n] + eps) : 1.f;
    }
    return k;
}

__global__ __launch_bounds__(256) void dice_colstat4_kernel(const float* __restrict__ z, int64_t z_stride, const float* __restrict__ bias,
                                                           int64_t rows, int N, int kind, const float* __restrict__ sum0,
                                                           float* __restrict__ acc_out) {
    const int N4 = N >> 2, RL = 256 / N4;
    const int c = threadIdx.x % N4, rl = threadIdx.x / N4;
    float acc[1][4] = {{0.f, 0.f, 0.f, 0.f}};
    if (rl < RL) {
        const float inv = 1.f / (float)rows;
        float sh[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) sh[j] = (bias != nullptr ? bias[4 * c + j] : 0.f) - (kind ? sum0[4 * c + j] * inv : 0.f);
#pragma unroll 4
        for (int64_t r = (int64_t)blockIdx.x * RL + rl; r < rows; r += (int64_t)gridDim.x * RL) {
            const float4 t = *reinterpret_cast<const float4*>(z + r * z_stride + 4 * c);
            const float v[4] = {t.x + sh[0], t.y + sh[1], t.z + sh[2], t.w + sh[3]};
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[0][j] += kind ? v[j] * v[j] : v[j];
        }
    }
    float* const outs[1] = {acc_out};
    colsum4_finish_k<1>(acc, N4, RL, c, outs);
}

__global__ __launch_bounds__(256) void dice_bwd4_kernel(float* __restrict__ dh, const float* __restrict__ zw, const float* __restrict__ bias,
                                                        const float* __restrict__ alpha, const float* __restrict__ mean,
                                                        const float* __restrict__ var, float eps, int64_t batch, int N,
                                                        float* __restrict__ d_alpha) {
    const int N4 = N >> 2, RL = 256 / N4;
    const int c = threadIdx.x % N4, rl = threadIdx.x / N4;
    float acc[1][4] = {{0.f, 0.f, 0.f, 0.f}};
    if (rl < RL) {
        const DiceCols k = dice_cols(bias, alpha, mean, var, eps, c);
#pragma unroll 2
        for (int64_t r = (int64_t)blockIdx.x * RL + rl; r < batch; r += (int64_t)gridDim.x * RL) {
            const float4 zt = *reinterpret_cast<const float4*>(zw + r * N + 4 * c);
            const float4 dt = *reinterpret_cast<const float4*>(dh + r * N + 4 * c);
            const float zz[4] = {zt.x, zt.y, zt.z, zt.w}, dd[4] = {dt.x, dt.y, dt.z, dt.w};
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float z = zz[j] + k.bn[j];
                const float p = 1.f / (1.f + expf(-(z - k.mu[j]) * k.rs[j]));
                acc[0][j] = fmaf(dd[j], z * (1.f - p), acc[0][j]);
                o[j] = dd[j] * (k.al[j] + (1.f - k.al[j]) * p + z * (1.f - k.al[j]) * p * (1.f - p) * k.rs[j]);
            }
            *reinterpret_cast<float4*>(dh + r * N + 4 * c) = make_float4(o[0], o[1], o[2], o[3]);
        }
    }
    float* const outs[1] = {d_alpha};
    colsum4_finish_k<1>(acc, N4, RL, c, outs);
}

__global__ __launch_bounds__(256) void dice_train_bwd_reduce4_kernel(const float* __restrict__ dh, const float* __restrict__ zw,
                                                                    const float* __restrict__ bias, const float* __restrict__ alpha,
                                                                    const float* __restrict__ mean, const float* __restrict__ var,
                                                                    float eps, int64_t batch, int N, float* __restrict__ s12,
                                                                    float* __restrict__ d_alpha) {
    const int N4 = N >> 2, RL = 256 / N4;
    const int c = threadIdx.x % N4, rl = threadIdx.x / N4;
    float acc[3][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    if (rl < RL) {
        const DiceCols k = dice_cols(bias, alpha, mean, var, eps, c);
#pragma unroll 2
        for (int64_t r = (int64_t)blockIdx.x * RL + rl; r < batch; r += (int64_t)gridDim.x * RL) {
            const float4 zt = *reinterpret_cast<const float4*>(zw + r * N + 4 * c);
            const float4 dt = *reinterpret_cast<const float4*>(dh + r * N + 4 * c);
            const float zz[4] = {zt.x, zt.y, zt.z, zt.w}, dd[4] = {dt.x, dt.y, dt.z, dt.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float z = zz[j] + k.bn[j];
                const float xn = (z - k.mu[j]) * k.rs[j];
                const float p = 1.f / (1.f + expf(-xn));
                const float dxn = dd[j] * z * (1.f - k.al[j]) * p * (1.f - p);
                acc[0][j] += dxn;
                acc[1][j] = fmaf(dxn, xn, acc[1][j]);
                acc[2][j] = fmaf(dd[j], z * (1.f - p), acc[2][j]);
            }
        }
    }
    float* const outs[3] = {s12, s12 + N, d_alpha};
    colsum4_finish_k<3>(acc, N4, RL, c, outs);
}

extern "C" int dctr_dice_train_fwd(const float* z, int64_t z_stride, const float* bias, int64_t rows, int32_t n, const float* alpha,
                                   float eps, float momentum, float* moving_mean, float* moving_var, float* batch_mean,
                                   float* batch_var, float* h, int64_t h_stride, void* stream) {
    DCTR_REQUIRE(z && alpha && batch_mean && batch_var && h, DCTR_E_NULL, "dice_train_fwd: null pointer");
    DCTR_REQUIRE(rows >= 1 && n >= 1 && z_stride >= n && h_stride >= n, DCTR_E_DIM, "dice_train_fwd: bad sizes (rows=%lld n=%d)",
                 (long long)rows, n);
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(batch_mean, 0, (size_t)n * sizeof(float), st);
    if (e == hipSuccess) e = hipMemsetAsync(batch_var, 0, (size_t)n * sizeof(float), st);
    DCTR_REQUIRE(e == hipSuccess, (int)e, "dice_train_fwd: memset failed: %s", hipGetErrorString(e));
    if (rowlane4_ok((int)n, z, nullptr, z_stride)) {
        const unsigned g = colsum_grid(rows, 256 / ((int)n / 4));
        hipLaunchKernelGGL(dice_colstat4_kernel, dim3(g), dim3(256), 0, st, z, z_stride, bias, rows, (int)n, 0, (const float*)nullptr, batch_mean);
        hipLaunchKernelGGL(dice_colstat4_kernel, dim3(g), dim3(256), 0, st, z, z_stride, bias, rows, (int)n, 1, (const float*)batch_mean, batch_var);
    } else {
        const unsigned rb = rows_grid(rows, true);
        hipLaunchKernelGGL(dice_colstat_kernel, dim3(rb), dim3(256), 0, st, z, z_stride, bias, rows, (int)n, 0, (const float*)nullptr, batch_mean);
        hipLaunchKernelGGL(dice_colstat_kernel, dim3(rb), dim3(256), 0, st, z, z_stride, bias, rows, (int)n, 1, (const float*)batch_mean, batch_var);
    }
    hipLaunchKernelGGL(dice_stat_finish_kernel, dim3((n + 63) / 64), dim3(64), 0, st, batch_mean, batch_var, rows, (int)n, momentum,
                       moving_mean, moving_var);
    const int64_t total = rows * n;
    const unsigned blocks = (unsigned)(dctr_ceil_div(total, (int64_t)256) < 4096 ? dctr_ceil_div(total, (int64_t)256) : 4096);
    hipLaunchKernelGGL(dice_apply_kernel, dim3(blocks), dim3(256), 0, st, z, z_stride, bias, alpha, (const float*)batch_mean,
                       (const float*)batch_var, eps, rows, (int)n, h, h_stride);
    return dctr_launch_status("dctr_dice_train_fwd");
}

// ---------------------------------------------------------------------------------------------------
// DNN layer under training=True with BatchNormalization / Dropout (include/dctr.h: dctr_dnn_train_layer_t; reference
// layers/core.py:196-208).  Elementwise passes: thread = column, rows grid-strided over blockIdx.x (coalesced along n); the column
// sums of the BatchNormalization backward leave as one atomic per column and workgroup (few workgroups, long row loops).
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool dropout_keep(unsigned long long seed, unsigned long long idx, float rate) {
    unsigned long long x = idx * 0x9E3779B97F4A7C15ull + seed;                    // splitmix64 finaliser over (seed, element)
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return (float)(unsigned)(x >> 40) * (1.f / 16777216.f) >= rate;               // 24 uniform bits
}

struct TrainLayerCol {
    float mu, rs, g, bt;
};
__device__ __forceinline__ TrainLayerCol train_layer_col(const dctr_dnn_train_layer_t& a, int n) {
    TrainLayerCol c{0.f, 1.f, 1.f, 0.f};
    if (a.use_bn) {
        c.mu = a.bn_batch_mean[n];
        c.rs = 1.f / sqrtf(a.bn_batch_var[n] + a.bn_eps);
        c.g = a.bn_gamma != nullptr ? a.bn_gamma[n] : 1.f;
        c.bt = a.bn_beta != nullptr ? a.bn_beta[n] : 0.f;
    }
    return c;
}

__global__ __launch_bounds__(256) void train_layer_fwd_kernel(dctr_dnn_train_layer_t a) {
    const int n = blockIdx.y * 256 + threadIdx.x;
    if (n >= a.n) return;
    const TrainLayerCol c = train_layer_col(a, n);
    const float scale = a.dropout_rate > 0.f ? 1.f / (1.f - a.dropout_rate) : 1.f;
    for (int64_t b = blockIdx.x; b < a.rows; b += gridDim.x) {
        const float z = a.z[b * a.z_stride + n];
        const float y = a.use_bn ? c.g * ((z - c.mu) * c.rs) + c.bt : z;
        float h = act_value(y, a.activation);
        if (a.dropout_rate > 0.f) h = dropout_keep(a.dropout_seed, (unsigned long long)b * a.n + n, a.dropout_rate) ? h * scale : 0.f;
        a.h[b * a.h_stride + n] = h;
    }
}

// dy of one element (shared by the two backward passes)
__device__ __forceinline__ float train_layer_dy(const dctr_dnn_train_layer_t& a, const TrainLayerCol& c, int64_t b, int n, float scale,
                                                float& xh) {
    const float z = a.z[b * a.z_stride + n];
    xh = (z - c.mu) * c.rs;
    const float y = a.use_bn ? c.g * xh + c.bt : z;
    float d = a.dh[b * a.dh_stride + n];
    if (a.dropout_rate > 0.f) d = dropout_keep(a.dropout_seed, (unsigned long long)b * a.n + n, a.dropout_rate) ? d * scale : 0.f;
    return d * act_deriv(y, a.activation);
}

// BatchNormalization backward, pass 1: ws[n] += sum_b dy, ws[N + n] += sum_b dy xhat
__global__ __launch_bounds__(256) void train_layer_bwd_reduce_kernel(dctr_dnn_train_layer_t a) {
    const int n = blockIdx.y * 256 + threadIdx.x;
    if (n >= a.n) return;
    const TrainLayerCol c = train_layer_col(a, n);
    const float scale = a.dropout_rate > 0.f ? 1.f / (1.f - a.dropout_rate) : 1.f;
    float s1 = 0.f, s2 = 0.f;
    for (int64_t b = blockIdx.x; b < a.rows; b += gridDim.x) {
        float xh;
        const float dy = train_layer_dy(a, c, b, n, scale, xh);
        s1 += dy;
        s2 = fmaf(dy, xh, s2);
    }
    unsafeAtomicAdd(a.workspace + n, s1);
    unsafeAtomicAdd(a.workspace + a.n + n, s2);
}

// pass 2 (the only pass without BatchNormalization): dz; blockIdx.x == 0 also adds the sums to d_beta / d_gamma
__global__ __launch_bounds__(256) void train_layer_bwd_apply_kernel(dctr_dnn_train_layer_t a) {
    const int n = blockIdx.y * 256 + threadIdx.x;
    if (n >= a.n) return;
    const TrainLayerCol c = train_layer_col(a, n);
    const float scale = a.dropout_rate > 0.f ? 1.f / (1.f - a.dropout_rate) : 1.f;
    float m1 = 0.f, m2 = 0.f;
    if (a.use_bn) {
        const float s1 = a.workspace[n], s2 = a.workspace[a.n + n];
        m1 = s1 / (float)a.rows;
        m2 = s2 / (float)a.rows;
        if (blockIdx.x == 0) {
            if (a.d_beta != nullptr) a.d_beta[n] += s1;
            if (a.d_gamma != nullptr) a.d_gamma[n] += s2;
        }
    }
    for (int64_t b = blockIdx.x; b < a.rows; b += gridDim.x) {
        float xh;
        const float dy = train_layer_dy(a, c, b, n, scale, xh);
        a.dz[b * a.n + n] = a.use_bn ? c.g * c.rs * (dy - m1 - xh * m2) : dy;
    }
}

static int train_layer_check(const dctr_dnn_train_layer_t* a, const char* what) {
    DCTR_REQUIRE(a != nullptr, DCTR_E_NULL, "%s: null args", what);
    DCTR_REQUIRE(a->rows >= 0 && a->n >= 1 && a->z_stride >= a->n, DCTR_E_DIM, "%s: bad sizes (rows=%lld n=%d z_stride=%lld)", what,
                 (long long)a->rows, a->n, (long long)a->z_stride);
    DCTR_REQUIRE((a->activation >= DCTR_ACT_LINEAR && a->activation <= DCTR_ACT_TANH) || dctr_act::is_extended(a->activation), DCTR_E_ENUM,
                 "%s: activation %d", what, a->activation);
    DCTR_REQUIRE(a->dropout_rate >= 0.f && a->dropout_rate < 1.f, DCTR_E_DIM, "%s: dropout_rate %g outside [0, 1)", what, (double)a->dropout_rate);
    DCTR_REQUIRE(a->z != nullptr, DCTR_E_NULL, "%s: null z", what);
    DCTR_REQUIRE(!a->use_bn || (a->bn_batch_mean != nullptr && a->bn_batch_var != nullptr), DCTR_E_NULL,
                 "%s: use_bn needs bn_batch_mean / bn_batch_var", what);
    return DCTR_OK;
}

extern "C" int dctr_dnn_train_layer_fwd(const dctr_dnn_train_layer_t* a, void* stream) {
    const int rc = train_layer_check(a, "dnn_train_layer_fwd");
    if (rc != DCTR_OK) return rc;
    if (a->rows == 0) return DCTR_OK;
    DCTR_REQUIRE(a->h != nullptr && a->h_stride >= a->n, DCTR_E_NULL, "dnn_train_layer_fwd: h missing or h_stride < n");
    hipStream_t st = (hipStream_t)stream;
    const int n = a->n;
    if (a->use_bn) {
        // this batch's statistics: two passes (sum -> mean, then squared deviations), then the stored statistics move towards them
        hipError_t e = hipMemsetAsync(a->bn_batch_mean, 0, (size_t)n * sizeof(float), st);
        if (e == hipSuccess) e = hipMemsetAsync(a->bn_batch_var, 0, (size_t)n * sizeof(float), st);
        DCTR_REQUIRE(e == hipSuccess, (int)e, "dnn_train_layer_fwd: memset failed: %s", hipGetErrorString(e));
        if (rowlane4_ok(n, a->z, nullptr, a->z_stride)) {
            const unsigned g = colsum_grid(a->rows, 256 / (n / 4));
            hipLaunchKernelGGL(dice_colstat4_kernel, dim3(g), dim3(256), 0, st, a->z, a->z_stride, (const float*)nullptr, a->rows, n, 0, (const float*)nullptr, a->bn_batch_mean);
            hipLaunchKernelGGL(dice_colstat4_kernel, dim3(g), dim3(256), 0, st, a->z, a->z_stride, (const float*)nullptr, a->rows, n, 1, (const float*)a->bn_batch_mean, a->bn_batch_var);
        } else {
            const unsigned rb = rows_grid(a->rows, true);
            hipLaunchKernelGGL(dice_colstat_kernel, dim3(rb), dim3(256), 0, st, a->z, a->z_stride, (const float*)nullptr, a->rows, n, 0, (const float*)nullptr, a->bn_batch_mean);
            hipLaunchKernelGGL(dice_colstat_kernel, dim3(rb), dim3(256), 0, st, a->z, a->z_stride, (const float*)nullptr, a->rows, n, 1, (const float*)a->bn_batch_mean, a->bn_batch_var);
        }
        hipLaunchKernelGGL(dice_stat_finish_kernel, dim3((n + 63) / 64), dim3(64), 0, st, a->bn_batch_mean, a->bn_batch_var, a->rows, n,
                           a->bn_momentum, a->bn_moving_mean, a->bn_moving_var);
    }
    const unsigned gx = (unsigned)(a->rows < 2048 ? a->rows : 2048);
    hipLaunchKernelGGL(train_layer_fwd_kernel, dim3(gx, (unsigned)((n + 255) / 256)), dim3(256), 0, st, *a);
    return dctr_launch_status("dctr_dnn_train_layer_fwd");
}

extern "C" int dctr_dnn_train_layer_bwd(const dctr_dnn_train_layer_t* a, void* stream) {
    const int rc = train_layer_check(a, "dnn_train_layer_bwd");
    if (rc != DCTR_OK) return rc;
    if (a->rows == 0) return DCTR_OK;
    DCTR_REQUIRE(a->dh != nullptr && a->dz != nullptr && a->dh_stride >= a->n, DCTR_E_NULL, "dnn_train_layer_bwd: dh / dz missing or dh_stride < n");
    DCTR_REQUIRE(a->dz != a->dh || a->dh_stride == a->n, DCTR_E_DIM, "dnn_train_layer_bwd: in place needs dh_stride == n");
    DCTR_REQUIRE(!a->use_bn || a->workspace != nullptr, DCTR_E_NULL, "dnn_train_layer_bwd: use_bn needs a workspace of 2 n floats");
    hipStream_t st = (hipStream_t)stream;
    const int n = a->n;
    const unsigned gy = (unsigned)((n + 255) / 256);
    if (a->use_bn) {
        hipError_t e = hipMemsetAsync(a->workspace, 0, (size_t)2 * n * sizeof(float), st);
        DCTR_REQUIRE(e == hipSuccess, (int)e, "dnn_train_layer_bwd: memset failed: %s", hipGetErrorString(e));
        hipLaunchKernelGGL(train_layer_bwd_reduce_kernel, dim3((unsigned)(a->rows < COLSUM_MAX_WG ? a->rows : COLSUM_MAX_WG), gy), dim3(256), 0, st, *a);
    }
    const unsigned gx = (unsigned)(a->rows < 2048 ? a->rows : 2048);
    hipLaunchKernelGGL(train_layer_bwd_apply_kernel, dim3(gx, gy), dim3(256), 0, st, *a);
    return dctr_launch_status("dctr_dnn_train_layer_bwd");
}

}  // namespace

// ---------------------------------------------------------------------------------------------------
// dctr_mlp_bwd, chained form (relu / linear / sigmoid / tanh; elu / selu / softplus / softsign / exponential / hard_sigmoid): head -> dZ_{L-1};  W_l^T of every layer (one launch);  the backward
// chain (mlp_bwd_kernels.hip: every dZ_l and dX in ONE launch);  dW_l (+ d_bias_l as one more output row) of every layer as row
// slices in ONE grouped GEMM launch;  one launch that sums the slices into the gradient buffers.  Five launches per step where the
// layer-by-layer form below took 4 L + 1 (a 3-layer DNN at B = 4096: ~60 us against ~210).
// ---------------------------------------------------------------------------------------------------
struct TransposeGroups {
    const float* src[8];
    float* dst[8];
    int rows[8], cols[8];       // src is [rows, cols] row-major, dst [cols, rows]
};
__global__ __launch_bounds__(256) void transpose_multi_kernel(TransposeGroups tg) {
    __shared__ float tile[32][33];
    const int gi = blockIdx.y;
    const int R = tg.rows[gi], C = tg.cols[gi];
    const int tc = (C + 31) / 32, n_tiles = ((R + 31) / 32) * tc;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int r0 = (t / tc) * 32, c0 = (t % tc) * 32;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = r0 + ty + 8 * i, c = c0 + tx;
            tile[ty + 8 * i][tx] = (r < R && c < C) ? tg.src[gi][(int64_t)r * C + c] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = c0 + ty + 8 * i, r = r0 + tx;
            if (c < C && r < R) tg.dst[gi][(int64_t)c * R + r] = tile[tx][ty + 8 * i];
        }
        __syncthreads();
    }
}

// dst_w[i] += sum_s parts[s * n + i] (i < n_w);  dst_b[i - n_w] += the same for the bias row behind the kernel's rows
struct SumGroups {
    const float* parts[8];
    float* dst_w[8];
    float* dst_b[8];
    int64_t n[8], n_w[8];
    int n_parts[8];
};
__global__ __launch_bounds__(256) void sum_parts_multi_kernel(SumGroups sg) {
    const int gi = blockIdx.y;
    const float* __restrict__ parts = sg.parts[gi];
    const int64_t n = sg.n[gi], n_w = sg.n_w[gi];
    const int n_parts = sg.n_parts[gi];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        int s = 0;
        for (; s + 4 <= n_parts; s += 4) {
            a0 += parts[(int64_t)s * n + i];
            a1 += parts[(int64_t)(s + 1) * n + i];
            a2 += parts[(int64_t)(s + 2) * n + i];
            a3 += parts[(int64_t)(s + 3) * n + i];
        }
        for (; s < n_parts; ++s) a0 += parts[(int64_t)s * n + i];
        const float v = (a0 + a1) + (a2 + a3);
        if (i < n_w) sg.dst_w[gi][i] += v;
        else sg.dst_b[gi][i - n_w] += v;
    }
}

// rows per dW slice of the chained form (DCTR_DW_ROWS overrides: scripts/gemm_lab.py)
static int chain_dw_rows() {
    static const int v = [] {
        const char* e = dctr_lab_env("DCTR_DW_ROWS");
        const int x = e != nullptr ? atoi(e) : 0;
        return (x >= 32 && x <= 4096 && x % 32 == 0) ? x : 256;      // (whole 32-row tiles, bounded: the value sizes a workspace)
    }();
    return v;
}
static bool chain_disabled() {
    static const bool v = [] { const char* e = dctr_lab_env("DCTR_MLP_BWD_CHAIN"); return e != nullptr && atoi(e) == 0; }();
    return v;
}
// act' needs the pre-activation: Dice, swish, gelu — the layer-by-layer form with saved_z or the recompute GEMM
static bool mlp_bwd_from_z(int act) { return act == DCTR_ACT_DICE || dctr_act::needs_z(act); }
static bool mlp_bwd_chained(const dctr_mlp_bwd_args_t* a) {
    return !chain_disabled() && !mlp_bwd_from_z(a->activation) && a->n_layers <= 8 && dctr_mlp::bwd_chain_fits(a->in_dim, a->n_layers, a->units);
}
// workspace of the chained form, in floats: dZ_l [B, units[l]] | W_l^T | dW slices [(K_l + 1) units[l]] x slices   (each 4-float aligned)
static size_t mlp_bwd_chain_floats(const dctr_mlp_bwd_args_t* a) {
    size_t f = 0;
    const int slices = dctr_gemm::k_slices((int)a->batch, chain_dw_rows());
    for (int l = 0; l < a->n_layers; ++l) {
        const size_t K = l == 0 ? a->in_dim : a->units[l - 1], N = a->units[l];
        f += ((size_t)a->batch * N + 3) & ~(size_t)3;
        f += (K * N + 3) & ~(size_t)3;
        f += ((size_t)slices * (K + 1) * N + 3) & ~(size_t)3;
    }
    return f;
}

static size_t mlp_bwd_main_floats(const dctr_mlp_bwd_args_t* a, int w) {
    // two ping-pong buffers [B, widest layer]; Dice / swish / gelu need a third for the recomputed pre-activations
    // ... and Dice, with batch statistics, 2 x widest for the two column sums of the BatchNormalization backward
    return ((size_t)(mlp_bwd_from_z(a->activation) ? 3 : 2) * a->batch * w + (a->activation == DCTR_ACT_DICE ? 2 * (size_t)w : 0) + 3) &
           ~(size_t)3;
}

extern "C" size_t dctr_mlp_bwd_workspace_bytes(const dctr_mlp_bwd_args_t* a) {
    if (a == nullptr || a->batch <= 0 || a->n_layers < 1 || a->units == nullptr) return 0;
    int w = a->in_dim;
    size_t kn = 0;
    for (int l = 0; l < a->n_layers; ++l) {
        const size_t k = l == 0 ? a->in_dim : a->units[l - 1];
        kn = k * a->units[l] > kn ? k * a->units[l] : kn;
        w = a->units[l] > w ? a->units[l] : w;
    }
    size_t parts_floats = 0;
    for (int l = 0; l < a->n_layers; ++l) {
        const size_t k = l == 0 ? a->in_dim : a->units[l - 1], knl = k * a->units[l];
        const int parts = mlp_dw_parts(a->batch, (int64_t)knl);
        if (parts > 1 && (size_t)parts * knl > parts_floats) parts_floats = (size_t)parts * knl;
    }
    const size_t layered = mlp_bwd_main_floats(a, w) + parts_floats;
    const size_t chained = (a->n_layers <= 8 && a->in_dim >= 1 && a->batch < 0x7fffffffLL && mlp_bwd_chained(a)) ? mlp_bwd_chain_floats(a) : 0;
    return (layered > chained ? layered : chained) * sizeof(float);
}

extern "C" int dctr_mlp_bwd(const dctr_mlp_bwd_args_t* a, void* stream) {
    DCTR_REQUIRE(a != nullptr, DCTR_E_NULL, "mlp_bwd: null args");
    DCTR_REQUIRE(a->batch >= 0 && a->in_dim >= 1 && a->n_layers >= 1 && a->n_layers <= 8, DCTR_E_DIM, "mlp_bwd: bad sizes");
    if (a->batch == 0) return DCTR_OK;
    DCTR_REQUIRE(a->x && a->units && a->kernels && a->acts && a->d_kernels, DCTR_E_NULL, "mlp_bwd: null pointer");
    DCTR_REQUIRE((a->head_w != nullptr && a->dlogit != nullptr && a->d_head_w != nullptr) ||
                     (a->head_w == nullptr && a->d_out != nullptr && a->d_out_stride >= a->units[a->n_layers - 1]),
                 DCTR_E_NULL, "mlp_bwd: needs either (head_w, dlogit, d_head_w) or d_out");
    const bool dice = a->activation == DCTR_ACT_DICE;
    const bool zact = dctr_act::needs_z(a->activation);        // swish / gelu: act' from the pre-activations, as Dice
    DCTR_REQUIRE(a->activation >= DCTR_ACT_LINEAR && a->activation <= DCTR_ACT_GELU, DCTR_E_UNSUPPORTED,
                 "mlp_bwd: activation %d has no backward (DCTR_ACT_LINEAR .. DCTR_ACT_GELU)", a->activation);
    DCTR_REQUIRE(!dice || (a->dice_alpha && a->dice_mean && a->dice_var), DCTR_E_NULL, "mlp_bwd: dice needs alpha / mean / var");
    DCTR_REQUIRE(a->workspace != nullptr && a->workspace_bytes >= dctr_mlp_bwd_workspace_bytes(a), DCTR_E_NULL,
                 "mlp_bwd: needs a workspace of dctr_mlp_bwd_workspace_bytes() bytes");
    DCTR_REQUIRE(a->batch < 0x7fffffffLL, DCTR_E_DIM, "mlp_bwd: batch too large");
    hipStream_t st = (hipStream_t)stream;
    if (mlp_bwd_chained(a)) {
        const int L = a->n_layers, B = (int)a->batch;
        const int slices = dctr_gemm::k_slices(B, chain_dw_rows());
        float* dz[8];
        float* wt[8];
        float* parts[8];
        float* ws = static_cast<float*>(a->workspace);
        for (int l = 0; l < L; ++l) {
            const size_t K = l == 0 ? a->in_dim : a->units[l - 1], N = a->units[l];
            dz[l] = ws; ws += ((size_t)a->batch * N + 3) & ~(size_t)3;
            wt[l] = ws; ws += (K * N + 3) & ~(size_t)3;
            parts[l] = ws; ws += ((size_t)slices * (K + 1) * N + 3) & ~(size_t)3;
        }
        // head: dZ_last = dlogit (x) head_w .* act'(h_last);  d_head_w = h_last^T dlogit   (headless: d_out .* act'(h_last))
        const int NL = a->units[L - 1];
        if (a->head_w != nullptr) {
            dctr_train::launch_head_bwd(st, a->dlogit, a->head_w, a->acts[L - 1], (int64_t)NL, a->batch, NL, (int)a->activation, dz[L - 1], (int64_t)NL,
                                        a->d_head_w);
        } else {
            hipError_t ce = hipMemcpy2DAsync(dz[L - 1], (size_t)NL * sizeof(float), a->d_out, (size_t)a->d_out_stride * sizeof(float),
                                             (size_t)NL * sizeof(float), (size_t)a->batch, hipMemcpyDeviceToDevice, st);
            DCTR_REQUIRE(ce == hipSuccess, (int)ce, "mlp_bwd: copy of d_out failed: %s", hipGetErrorString(ce));
            if (a->activation != DCTR_ACT_LINEAR)
                dctr_train::launch_act_bwd_colsum(st, dz[L - 1], a->acts[L - 1], a->batch, NL, (int)a->activation, (float*)nullptr);
        }
        const int l_first = a->dx != nullptr ? 0 : 1;       // layers whose transposed kernel the chain multiplies by
        if (l_first < L) {
            TransposeGroups tg{};
            int ng = 0, max_tiles = 1;
            for (int l = l_first; l < L; ++l, ++ng) {
                const int K = l == 0 ? a->in_dim : a->units[l - 1], N = a->units[l];
                tg.src[ng] = a->kernels[l];
                tg.dst[ng] = wt[l];
                tg.rows[ng] = K;
                tg.cols[ng] = N;
                const int t = ((K + 31) / 32) * ((N + 31) / 32);
                max_tiles = t > max_tiles ? t : max_tiles;
            }
            hipLaunchKernelGGL(transpose_multi_kernel, dim3((unsigned)max_tiles, (unsigned)ng), dim3(256), 0, st, tg);
            const int rc = dctr_mlp::launch_bwd_chain(st, a->batch, a->in_dim, L, a->units, wt, a->acts, (int)a->activation, dz[L - 1], dz,
                                                      a->dx, a->dx_stride);
            if (rc != DCTR_OK) return rc;
        }
        // dW_l[K, N] (row-major) += X_l^T dZ_l, d_bias_l += colsum(dZ_l): column-major  dW'(N x (K + 1)) = dZ'(N x rows) * [X' ; 1](.. x rows)^T
        dctr_gemm::GroupDesc gd[8];
        SumGroups sg{};
        int64_t max_n = 0;
        for (int l = 0; l < L; ++l) {
            const int N = a->units[l], K = l == 0 ? a->in_dim : a->units[l - 1];
            const bool bias = a->d_biases != nullptr && a->d_biases[l] != nullptr;
            dctr_gemm::GroupDesc& d = gd[l];
            d = dctr_gemm::GroupDesc{};
            d.op_a = dctr_gemm::OP_N;
            d.op_b = dctr_gemm::OP_T;
            d.m = N;
            d.n = K + (bias ? 1 : 0);
            d.k = B;
            d.A = dz[l];
            d.lda = N;
            d.B = l == 0 ? a->x : a->acts[l - 1];
            d.ldb = l == 0 ? (int)a->x_stride : K;
            d.C = parts[l];
            d.ldc = N;
            d.batch = 1;
            d.ones_last = bias ? 1 : 0;
            d.k_slices = slices;
            d.slice_stride_c = (int64_t)d.n * N;            // (sum_parts_multi reads slice s at parts + s * n)
            sg.parts[l] = parts[l];
            sg.dst_w[l] = a->d_kernels[l];
            sg.dst_b[l] = bias ? a->d_biases[l] : nullptr;
            sg.n[l] = (int64_t)d.n * N;
            sg.n_w[l] = (int64_t)K * N;
            sg.n_parts[l] = slices;
            max_n = sg.n[l] > max_n ? sg.n[l] : max_n;
        }
        // the weight-gradient half: on the caller's second stream when it gave one (behind an event on `stream`; the caller joins)
        hipStream_t dws = st;
        if (a->dw_stream != nullptr && (hipStream_t)a->dw_stream != st) {
            // (one event per device and calling thread, alive as long as the process: hipEventRecord re-arms it on every call)
            static thread_local hipEvent_t ev[DCTR_MAX_DEVICES] = {};
            int dev = 0;
            hipError_t e = hipGetDevice(&dev);
            DCTR_REQUIRE(e == hipSuccess && dev >= 0 && dev < DCTR_MAX_DEVICES, DCTR_E_UNSUPPORTED, "mlp_bwd: dw_stream on device %d", dev);
            if (ev[dev] == nullptr) {
                e = hipEventCreateWithFlags(&ev[dev], hipEventDisableTiming);
                DCTR_REQUIRE(e == hipSuccess, (int)e, "mlp_bwd: hipEventCreate failed: %s", hipGetErrorString(e));
            }
            dws = (hipStream_t)a->dw_stream;
            e = hipEventRecord(ev[dev], st);
            if (e == hipSuccess) e = hipStreamWaitEvent(dws, ev[dev], 0);
            DCTR_REQUIRE(e == hipSuccess, (int)e, "mlp_bwd: cannot order dw_stream behind stream: %s", hipGetErrorString(e));
        }
        const int rg = dctr_gemm::sgemm_grouped(dws, gd, L);
        DCTR_REQUIRE(rg == 0, DCTR_E_UNSUPPORTED, "mlp_bwd: sgemm_grouped(dW) failed (%d)", rg);
        int64_t gx = dctr_ceil_div(max_n, (int64_t)256);
        hipLaunchKernelGGL(sum_parts_multi_kernel, dim3((unsigned)(gx > 512 ? 512 : gx), (unsigned)L), dim3(256), 0, dws, sg);
        return dctr_launch_status("dctr_mlp_bwd");
    }
    int w = a->in_dim;
    for (int l = 0; l < a->n_layers; ++l) w = a->units[l] > w ? a->units[l] : w;
    float* bufA = static_cast<float*>(a->workspace);
    float* bufB = bufA + (size_t)a->batch * w;
    float* bufZ = bufB + (size_t)a->batch * w;                 // dice only
    float* dw_parts = bufA + mlp_bwd_main_floats(a, w);        // partial dW of the row slices (batch >= 1024)
    const int B = (int)a->batch;
    const unsigned rb = (unsigned)dctr_ceil_div(a->batch, (int64_t)BWD_ROWS);
    const int L = a->n_layers;
    // Dice: dH of layer l (in `buf`, in place) -> dZ.  Z_l = X_l W_l is recomputed (column-major Z'(N x B) = W'(N x K) X'(K x B)).
    auto dice_bwd = [&](int l, float* buf) -> int {
        const int N = a->units[l], K = l == 0 ? a->in_dim : a->units[l - 1];
        const float* xin = l == 0 ? a->x : a->acts[l - 1];
        const int ldx = l == 0 ? (int)a->x_stride : K;
        // (saved_z: the forward's own pre-activations, bias included — no recompute, no bias in the kernels below)
        const float* zsrc = bufZ;
        const float* bl = a->biases != nullptr ? a->biases[l] : nullptr;
        if (a->saved_z != nullptr && a->saved_z[l] != nullptr) {
            zsrc = a->saved_z[l];
            bl = nullptr;
        } else {
            int rs = dctr_gemm::sgemm(st, dctr_gemm::OP_N, dctr_gemm::OP_N, N, B, K, a->kernels[l], N, xin, ldx, 0.f, bufZ, N);
            if (rs != 0) return (int)rs;
        }
        float* dal = a->d_dice_alpha != nullptr ? a->d_dice_alpha[l] : nullptr;
        if (a->dice_batch_mean != nullptr && a->dice_batch_var != nullptr && a->dice_batch_mean[l] != nullptr) {
            // training-mode Dice: this batch's statistics, gradients through them
            float* s12 = bufZ + (size_t)a->batch * w;
            if (hipMemsetAsync(s12, 0, (size_t)2 * N * sizeof(float), st) != hipSuccess) return -1;
            if (rowlane4_ok(N, buf, zsrc, N))
                hipLaunchKernelGGL(dice_train_bwd_reduce4_kernel, dim3(colsum_grid(a->batch, 256 / (N / 4))), dim3(256), 0, st,
                                   (const float*)buf, zsrc, bl, a->dice_alpha[l], a->dice_batch_mean[l],
                                   a->dice_batch_var[l], a->dice_eps, a->batch, N, s12, dal);
            else
                hipLaunchKernelGGL(dice_train_bwd_reduce_kernel, dim3(rows_grid(a->batch, true)), dim3(256), 0, st, (const float*)buf, zsrc, bl,
                                   a->dice_alpha[l], a->dice_batch_mean[l], a->dice_batch_var[l], a->dice_eps, a->batch, N, s12, dal);
            hipLaunchKernelGGL(dice_train_bwd_apply_kernel, dim3(rb), dim3(256), 0, st, buf, zsrc, bl, a->dice_alpha[l],
                               a->dice_batch_mean[l], a->dice_batch_var[l], a->dice_eps, a->batch, N, (const float*)s12);
            return 0;
        }
        if (rowlane4_ok(N, buf, zsrc, N))
            hipLaunchKernelGGL(dice_bwd4_kernel, dim3(colsum_grid(a->batch, 256 / (N / 4))), dim3(256), 0, st, buf, zsrc, bl,
                               a->dice_alpha[l], a->dice_mean[l], a->dice_var[l], a->dice_eps, a->batch, N, dal);
        else
            hipLaunchKernelGGL(dice_bwd_kernel, dim3(rows_grid(a->batch, true)), dim3(256), 0, st, buf, zsrc, bl, a->dice_alpha[l], a->dice_mean[l], a->dice_var[l],
                               a->dice_eps, a->batch, N, dal);
        return 0;
    };
    // swish / gelu: dH of layer l (in `buf`, in place) -> dZ = dH .* act'(z), z from saved_z or recomputed as for Dice
    auto zact_bwd = [&](int l, float* buf) -> int {
        const int N = a->units[l], K = l == 0 ? a->in_dim : a->units[l - 1];
        const float* zsrc = bufZ;
        const float* bl = a->biases != nullptr ? a->biases[l] : nullptr;
        if (a->saved_z != nullptr && a->saved_z[l] != nullptr) {
            zsrc = a->saved_z[l];
            bl = nullptr;
        } else {
            int rs = dctr_gemm::sgemm(st, dctr_gemm::OP_N, dctr_gemm::OP_N, N, B, K, a->kernels[l], N, l == 0 ? a->x : a->acts[l - 1],
                                      l == 0 ? (int)a->x_stride : K, 0.f, bufZ, N);
            if (rs != 0) return (int)rs;
        }
        const int64_t g = dctr_ceil_div(a->batch * N, (int64_t)256);
        hipLaunchKernelGGL(act_bwd_from_z_kernel, dim3((unsigned)(g > 16384 ? 16384 : g)), dim3(256), 0, st, buf, zsrc, bl, a->batch * N, N,
                           (int)a->activation);
        return 0;
    };
    const bool from_z = dice || zact;
    // head: dZ_last = dlogit (x) head_w .* act'(h_last);  d_head_w = h_last^T dlogit
    const int NL = a->units[L - 1];
    if (a->head_w != nullptr) {
        dctr_train::launch_head_bwd(st, a->dlogit, a->head_w, a->acts[L - 1], (int64_t)NL, a->batch, NL,
                                    from_z ? (int)DCTR_ACT_LINEAR : (int)a->activation, bufA, (int64_t)NL, a->d_head_w);
    } else {
        // headless (the DNN branch of DCN): the caller hands d(loss)/d(h_last); dZ_last = d_out .* act'(h_last)
        hipError_t ce = hipMemcpy2DAsync(bufA, (size_t)NL * sizeof(float), a->d_out, (size_t)a->d_out_stride * sizeof(float),
                                         (size_t)NL * sizeof(float), (size_t)a->batch, hipMemcpyDeviceToDevice, st);
        DCTR_REQUIRE(ce == hipSuccess, (int)ce, "mlp_bwd: copy of d_out failed: %s", hipGetErrorString(ce));
        if (a->activation != DCTR_ACT_LINEAR && !from_z)
            dctr_train::launch_act_bwd_colsum(st, bufA, a->acts[L - 1], a->batch, NL, (int)a->activation, (float*)nullptr);
    }
    if (from_z) {
        const int rc = dice ? dice_bwd(L - 1, bufA) : zact_bwd(L - 1, bufA);
        DCTR_REQUIRE(rc == 0, DCTR_E_UNSUPPORTED, "mlp_bwd: sgemm(Z) failed (%d)", rc);
    }
    float* dz = bufA;
    float* other = bufB;
    for (int l = L - 1; l >= 0; --l) {
        const int N = a->units[l], K = l == 0 ? a->in_dim : a->units[l - 1];
        const float* xin = l == 0 ? a->x : a->acts[l - 1];
        const int ldx = l == 0 ? (int)a->x_stride : K;
        // d_bias[n] += sum_b dZ[b, n]   (dZ is final here: the head / the previous iteration applied act')
        if (a->d_biases != nullptr && a->d_biases[l] != nullptr)
            dctr_train::launch_act_bwd_colsum(st, dz, (const float*)nullptr, a->batch, N, 0, a->d_biases[l]);
        // dW[K, N] (row-major) += X^T dZ:  column-major  dW'(N x K) = dZ'(N x B) * X'(K x B)^T
        int rs;
        const int n_parts = mlp_dw_parts(a->batch, (int64_t)K * N);
        const bool to_dx = l == 0;
        const bool want_dx = !(to_dx && a->dx == nullptr);
        float* dst = to_dx ? a->dx : other;
        const int ldd = to_dx ? (int)a->dx_stride : K;
        if (n_parts > 1) {
            // dW slices and dH_prev[B, K] = dZ W^T (column-major dH'(K x B) = W'(N x K)^T * dZ'(N x B)) read dZ and nothing of each
            // other: ONE grouped launch (two latency-bound problems side by side: DCN-matrix's pair went from 2 x 35 to 45 us)
            const int rs_ = B / n_parts;
            const int64_t kn = (int64_t)K * N;
            dctr_gemm::GroupDesc gd[2];
            gd[0] = dctr_gemm::GroupDesc{};
            gd[0].op_a = dctr_gemm::OP_N; gd[0].op_b = dctr_gemm::OP_T; gd[0].m = N; gd[0].n = K; gd[0].k = rs_;
            gd[0].A = dz; gd[0].lda = N; gd[0].stride_a = (int64_t)rs_ * N;
            gd[0].B = xin; gd[0].ldb = ldx; gd[0].stride_b = (int64_t)rs_ * ldx;
            gd[0].C = dw_parts; gd[0].ldc = N; gd[0].stride_c = kn; gd[0].batch = n_parts;
            gd[1] = dctr_gemm::GroupDesc{};
            gd[1].op_a = dctr_gemm::OP_T; gd[1].op_b = dctr_gemm::OP_N; gd[1].m = K; gd[1].n = B; gd[1].k = N;
            gd[1].A = a->kernels[l]; gd[1].lda = N; gd[1].B = dz; gd[1].ldb = N; gd[1].C = dst; gd[1].ldc = ldd; gd[1].batch = 1;
            rs = dctr_gemm::sgemm_grouped(st, gd, want_dx ? 2 : 1);
            DCTR_REQUIRE(rs == 0, DCTR_E_UNSUPPORTED, "mlp_bwd: sgemm_grouped(dW, dX) failed (%d)", (int)rs);
            int64_t g = dctr_ceil_div(kn, (int64_t)256);
            hipLaunchKernelGGL(sum_parts_kernel, dim3((unsigned)(g > 8192 ? 8192 : g)), dim3(256), 0, st, (const float*)dw_parts, kn, n_parts,
                               a->d_kernels[l]);
            if (!want_dx) break;
        } else {
            rs = dctr_gemm::sgemm(st, dctr_gemm::OP_N, dctr_gemm::OP_T, N, K, B, dz, N, xin, ldx, 1.f, a->d_kernels[l], N);
            DCTR_REQUIRE(rs == 0, DCTR_E_UNSUPPORTED, "mlp_bwd: sgemm(dW) failed (%d)", (int)rs);
            if (!want_dx) break;
            rs = dctr_gemm::sgemm(st, dctr_gemm::OP_T, dctr_gemm::OP_N, K, B, N, a->kernels[l], N, dz, N, 0.f, dst, ldd);
            DCTR_REQUIRE(rs == 0, DCTR_E_UNSUPPORTED, "mlp_bwd: sgemm(dX) failed (%d)", (int)rs);
        }
        if (!to_dx) {
            // dZ_prev = dH_prev .* act'(h_prev)
            if (from_z) {
                const int rc = dice ? dice_bwd(l - 1, other) : zact_bwd(l - 1, other);
                DCTR_REQUIRE(rc == 0, DCTR_E_UNSUPPORTED, "mlp_bwd: sgemm(Z) failed (%d)", rc);
            } else if (a->activation != DCTR_ACT_LINEAR) {
                dctr_train::launch_act_bwd_colsum(st, other, a->acts[l - 1], a->batch, K, (int)a->activation, (float*)nullptr);
            }
            float* t = dz;
            dz = other;
            other = t;
        }
    }
    return dctr_launch_status("dctr_mlp_bwd");
}

// Dense(1, use_bias=False) on an arbitrary [B, N] input with row stride (DCN's head over the [cross, deep] stack):
// dx[b, n] = dlogit[b] * w[n];  d_w[n] += sum_b dlogit[b] * x[b, n]
extern "C" int dctr_dense1_bwd(const float* x, int64_t x_stride, int64_t batch, int32_t n, const float* w, const float* dlogit,
                               float* dx, int64_t dx_stride, float* d_w, void* stream) {
    DCTR_REQUIRE(batch >= 0 && n >= 1 && x_stride >= n && dx_stride >= n, DCTR_E_DIM, "dense1_bwd: bad sizes");
    if (batch == 0) return DCTR_OK;
    DCTR_REQUIRE(x && w && dlogit && dx && d_w, DCTR_E_NULL, "dense1_bwd: null pointer");
    dctr_train::launch_head_bwd((hipStream_t)stream, dlogit, w, x, x_stride, batch, (int)n, (int)DCTR_ACT_LINEAR, dx, dx_stride, d_w);
    return dctr_launch_status("dctr_dense1_bwd");
}

// The join dctr_mlp_bwd_args_t.dw_stream asks of the caller, as one call: `stream` waits for everything issued to `dw_stream` so far.
extern "C" int dctr_mlp_bwd_join(void* stream, void* dw_stream) {
    if (dw_stream == nullptr || dw_stream == stream) return DCTR_OK;
    static thread_local hipEvent_t ev[DCTR_MAX_DEVICES] = {};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    DCTR_REQUIRE(e == hipSuccess && dev >= 0 && dev < DCTR_MAX_DEVICES, DCTR_E_UNSUPPORTED, "mlp_bwd_join: device %d", dev);
    if (ev[dev] == nullptr) {
        e = hipEventCreateWithFlags(&ev[dev], hipEventDisableTiming);
        DCTR_REQUIRE(e == hipSuccess, (int)e, "mlp_bwd_join: hipEventCreate failed: %s", hipGetErrorString(e));
    }
    e = hipEventRecord(ev[dev], (hipStream_t)dw_stream);
    if (e == hipSuccess) e = hipStreamWaitEvent((hipStream_t)stream, ev[dev], 0);
    DCTR_REQUIRE(e == hipSuccess, (int)e, "mlp_bwd_join: %s", hipGetErrorString(e));
    return DCTR_OK;
}
