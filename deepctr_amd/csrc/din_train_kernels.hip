// DIN's attention as a training step (LocalActivationUnit, layers/core.py:94-108; AttentionSequencePoolingLayer,
// layers/sequence.py:261-298): the attention MLP itself runs through dctr_mlp_fwd / dctr_mlp_bwd, the pieces around it are here.
//   dctr_din_att_in_fwd, dctr_din_att_in_bwd     the attention input [q, k, q - k, q * k], materialised once per batch
//   dctr_din_wsum_fwd, dctr_din_wsum_bwd         the masked weighted sum of the keys
//   dctr_din_softmax_fwd, dctr_din_softmax_bwd   att_weight_normalization=True (layers/sequence.py:283-289)
#include "train_common.h"

namespace {

// ---------------------------------------------------------------------------------------------------
// DIN's LocalActivationUnit as a training step (layers/core.py:94-108, layers/sequence.py:261-298): the attention input
// [q, k, q - k, q * k] is materialised once per batch ([B*T, 4E]) so that the attention MLP runs through dctr_mlp_fwd /
// dctr_mlp_bwd with saved activations; the masked weighted sum and the scatter of the key gradients are kernels here.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void din_att_in_kernel(const float* __restrict__ q, const float* __restrict__ k, int64_t rows, int T,
                                                         int E, float* __restrict__ a) {
    // one thread per (row = b*T + t, e)
    const int64_t total = rows * E;
    for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (int64_t)gridDim.x * 256) {
        const int64_t r = o / E;
        const int e = (int)(o - r * E);
        const float qv = q[(r / T) * E + e], kv = k[o];
        float* ar = a + r * 4 * E;
        ar[e] = qv;
        ar[E + e] = kv;
        ar[2 * E + e] = qv - kv;
        ar[3 * E + e] = qv * kv;
    }
}

// out[b, e] = sum_t (mask ? score : 0) k[b,t,e]                         (weight_normalization=False, sequence.py:286-296)
__global__ __launch_bounds__(256) void din_wsum_kernel(const float* __restrict__ score, const uint8_t* __restrict__ mask,
                                                       const float* __restrict__ k, int64_t batch, int T, int E,
                                                       float* __restrict__ out, int64_t out_stride) {
    const int64_t total = batch * E;
    for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (int64_t)gridDim.x * 256) {
        const int64_t b = o / E;
        const int e = (int)(o - b * E);
        float acc = 0.f;
        for (int t = 0; t < T; ++t) {
            const float s = mask[b * T + t] ? score[b * T + t] : 0.f;
            acc = fmaf(s, k[(b * T + t) * E + e], acc);
        }
        out[b * out_stride + e] = acc;
    }
}

// d_score[b,t] = mask ? <d_out[b,:], k[b,t,:]> : 0;  dk[b,t,:] = (mask ? score : 0) d_out[b,:] (written);
// d_bias += sum d_score (the bias of the unit's final Dense(1));  one wave per (b, t)
__global__ __launch_bounds__(256) void din_wsum_bwd_kernel(const float* __restrict__ d_out, int64_t d_stride,
                                                           const float* __restrict__ score, const uint8_t* __restrict__ mask,
                                                           const float* __restrict__ k, int64_t batch, int T, int E,
                                                           float* __restrict__ d_score, float* __restrict__ dk,
                                                           float* __restrict__ d_bias) {
    const int lane = threadIdx.x & 63;
    const int64_t rows = batch * T;
    float bsum = 0.f;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * 4) {
        const int64_t b = r / T;
        const bool m = mask[r] != 0;
        const float s = m ? score[r] : 0.f;
        float dot = 0.f;
        for (int e = lane; e < E; e += 64) {
            const float g = d_out[b * d_stride + e];
            dot = fmaf(g, k[r * E + e], dot);
            dk[r * E + e] = s * g;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) dot += __shfl_xor(dot, o, 64);
        const float ds = m ? dot : 0.f;
        if (lane == 0) d_score[r] = ds;
        bsum += ds;
    }
    // one atomic per workgroup (B*T / 4 of them on ONE address serialised to 0.5 ms at C4)
    __shared__ float wsum[4];
    if (lane == 0) wsum[threadIdx.x >> 6] = bsum;
    __syncthreads();
    if (d_bias != nullptr && threadIdx.x == 0) {
        const float t = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
        if (t != 0.f) unsafeAtomicAdd(d_bias, t);
    }
}

// out[0] += sum_i v[i]: grid-stride, wave sums, one atomic per workgroup
__global__ __launch_bounds__(256) void sum_vec_kernel(const float* __restrict__ v, int64_t n, float* __restrict__ out) {
    __shared__ float ws4[4];
    float a = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) a += v[i];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) a += __shfl_xor(a, o, 64);
    if ((threadIdx.x & 63) == 0) ws4[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float t = (ws4[0] + ws4[1]) + (ws4[2] + ws4[3]);
        if (t != 0.f) unsafeAtomicAdd(out, t);
    }
}

// da [B*T, 4E] -> dq[b,e] = sum_t (d0 + d2 + d3 k), added into dx[b, qcol[e]];  dk[b,t,e] += d1 - d2 + d3 q
__global__ __launch_bounds__(256) void din_att_in_bwd_kernel(const float* __restrict__ da, const float* __restrict__ q,
                                                             const float* __restrict__ k, int64_t batch, int T, int E,
                                                             float* __restrict__ dk, float* __restrict__ dx, int64_t dx_stride,
                                                             const int32_t* __restrict__ qcol) {
    const int64_t total = batch * E;
    for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (int64_t)gridDim.x * 256) {
        const int64_t b = o / E;
        const int e = (int)(o - b * E);
        const float qv = q[o];
        float dq = 0.f;
        for (int t = 0; t < T; ++t) {
            const int64_t r = b * T + t;
            const float* ar = da + r * 4 * E;
            const float d0 = ar[e], d1 = ar[E + e], d2 = ar[2 * E + e], d3 = ar[3 * E + e];
            const float kv = k[r * E + e];
            dq += d0 + d2 + d3 * kv;
            dk[r * E + e] += d1 - d2 + d3 * qv;
        }
        dx[b * dx_stride + qcol[e]] += dq;
    }
}

}  // namespace

extern "C" int dctr_din_att_in_fwd(const float* q, const float* k, int64_t batch, int32_t maxlen, int32_t dim, float* a, void* stream) {
    DCTR_REQUIRE(batch >= 0 && maxlen >= 1 && dim >= 1, DCTR_E_DIM, "din_att_in_fwd: bad sizes");
    if (batch == 0) return DCTR_OK;
    DCTR_REQUIRE(q && k && a, DCTR_E_NULL, "din_att_in_fwd: null pointer");
    int64_t blocks = dctr_ceil_div(batch * maxlen * dim, (int64_t)256);
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(din_att_in_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, q, k, batch * maxlen, (int)maxlen,
                       (int)dim, a);
    return dctr_launch_status("dctr_din_att_in_fwd");
}

extern "C" int dctr_din_wsum_fwd(const float* score, const uint8_t* mask, const float* k, int64_t batch, int32_t maxlen, int32_t dim,
                                 float* out, int64_t out_stride, void* stream) {
    DCTR_REQUIRE(batch >= 0 && maxlen >= 1 && dim >= 1 && out_stride >= dim, DCTR_E_DIM, "din_wsum_fwd: bad sizes");
    if (batch == 0) return DCTR_OK;
    DCTR_REQUIRE(score && mask && k && out, DCTR_E_NULL, "din_wsum_fwd: null pointer");
    int64_t blocks = dctr_ceil_div(batch * dim, (int64_t)256);
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(din_wsum_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, score, mask, k, batch, (int)maxlen,
                       (int)dim, out, out_stride);
    return dctr_launch_status("dctr_din_wsum_fwd");
}

extern "C" int dctr_din_wsum_bwd(const float* d_out, int64_t d_stride, const float* score, const uint8_t* mask, const float* k,
                                 int64_t batch, int32_t maxlen, int32_t dim, float* d_score, float* dk, float* d_bias, void* stream) {
    DCTR_REQUIRE(batch >= 0 && maxlen >= 1 && dim >= 1 && d_stride >= dim, DCTR_E_DIM, "din_wsum_bwd: bad sizes");
    if (batch == 0) return DCTR_OK;
    DCTR_REQUIRE(d_out && score && mask && k && d_score && dk, DCTR_E_NULL, "din_wsum_bwd: null pointer");
    int64_t blocks = dctr_ceil_div(batch * maxlen, (int64_t)4);
    if (blocks > 16384) blocks = 16384;
    // the bias gradient (sum of d_score) is taken by a second small kernel: as one atomic per workgroup of this one it either
    // serialised thousands of atomics on one address (0.5 ms at C4) or capped the grid at 256 workgroups (86 us)
    hipLaunchKernelGGL(din_wsum_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, d_out, d_stride, score, mask, k,
                       batch, (int)maxlen, (int)dim, d_score, dk, (float*)nullptr);
    if (d_bias != nullptr) {
        const int64_t n = batch * maxlen;
        int64_t g = dctr_ceil_div(n, (int64_t)256 * 8);
        g = g < 1 ? 1 : (g > COLSUM_MAX_WG ? COLSUM_MAX_WG : g);
        hipLaunchKernelGGL(sum_vec_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, (const float*)d_score, n, d_bias);
    }
    return dctr_launch_status("dctr_din_wsum_bwd");
}

// att_weight_normalization=True (layers/sequence.py:283-289): p = softmax over ALL T positions of where(mask, score, -2^32 + 1) — a
// row without valid positions gets the uniform 1/T, as tf.nn.softmax gives it — and the weighted sum then runs over every position.
// One wave per row.  Backward: ds = p (dp - <p, dp>), kept where the mask is set (a padded position's input is the constant).
__global__ __launch_bounds__(256) void din_softmax_kernel(const float* __restrict__ score, const uint8_t* __restrict__ mask, int64_t batch,
                                                          int T, float* __restrict__ p) {
    const int lane = threadIdx.x & 63;
    const float pad = -4294967295.f;                       // float(-2 ** 32 + 1)
    for (int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); b < batch; b += (int64_t)gridDim.x * 4) {
        float mx = -__builtin_inff();
        for (int t = lane; t < T; t += 64) mx = fmaxf(mx, mask[b * T + t] ? score[b * T + t] : pad);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        float sum = 0.f;
        for (int t = lane; t < T; t += 64) sum += expf((mask[b * T + t] ? score[b * T + t] : pad) - mx);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o, 64);
        for (int t = lane; t < T; t += 64) p[b * T + t] = expf((mask[b * T + t] ? score[b * T + t] : pad) - mx) / sum;
    }
}
__global__ __launch_bounds__(256) void din_softmax_bwd_kernel(const float* __restrict__ p, const uint8_t* __restrict__ mask,
                                                              const float* __restrict__ dp, int64_t batch, int T, float* __restrict__ ds) {
    const int lane = threadIdx.x & 63;
    for (int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); b < batch; b += (int64_t)gridDim.x * 4) {
        float dot = 0.f;
        for (int t = lane; t < T; t += 64) dot = fmaf(p[b * T + t], dp[b * T + t], dot);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) dot += __shfl_xor(dot, o, 64);
        for (int t = lane; t < T; t += 64) ds[b * T + t] = mask[b * T + t] ? p[b * T + t] * (dp[b * T + t] - dot) : 0.f;
    }
}

extern "C" int dctr_din_softmax_fwd(const float* score, const uint8_t* mask, int64_t batch, int32_t maxlen, float* p, void* stream) {
    DCTR_REQUIRE(batch >= 0 && maxlen >= 1, DCTR_E_DIM, "din_softmax_fwd: bad sizes");
    if (batch == 0) return DCTR_OK;
    DCTR_REQUIRE(score && mask && p, DCTR_E_NULL, "din_softmax_fwd: null pointer");
    int64_t blocks = dctr_ceil_div(batch, (int64_t)4);
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(din_softmax_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, score, mask, batch, (int)maxlen, p);
    return dctr_launch_status("dctr_din_softmax_fwd");
}

// d_score (may alias dp) = softmax backward masked; d_bias (NULL ok) += sum d_score
extern "C" int dctr_din_softmax_bwd(const float* p, const uint8_t* mask, const float* dp, int64_t batch, int32_t maxlen, float* d_score,
                                    float* d_bias, void* stream) {
    DCTR_REQUIRE(batch >= 0 && maxlen >= 1, DCTR_E_DIM, "din_softmax_bwd: bad sizes");
    if (batch == 0) return DCTR_OK;
    DCTR_REQUIRE(p && mask && dp && d_score, DCTR_E_NULL, "din_softmax_bwd: null pointer");
    int64_t blocks = dctr_ceil_div(batch, (int64_t)4);
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(din_softmax_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, mask, dp, batch, (int)maxlen, d_score);
    if (d_bias != nullptr) {
        const int64_t n = batch * maxlen;
        int64_t g = dctr_ceil_div(n, (int64_t)256 * 8);
        g = g < 1 ? 1 : (g > COLSUM_MAX_WG ? COLSUM_MAX_WG : g);
        hipLaunchKernelGGL(sum_vec_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, (const float*)d_score, n, d_bias);
    }
    return dctr_launch_status("dctr_din_softmax_bwd");
}

extern "C" int dctr_din_att_in_bwd(const float* da, const float* q, const float* k, int64_t batch, int32_t maxlen, int32_t dim,
                                   float* dk, float* dx, int64_t dx_stride, const int32_t* qcol, void* stream) {
    DCTR_REQUIRE(batch >= 0 && maxlen >= 1 && dim >= 1, DCTR_E_DIM, "din_att_in_bwd: bad sizes");
    if (batch == 0) return DCTR_OK;
    DCTR_REQUIRE(da && q && k && dk && dx && qcol, DCTR_E_NULL, "din_att_in_bwd: null pointer");
    int64_t blocks = dctr_ceil_div(batch * dim, (int64_t)256);
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(din_att_in_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, da, q, k, batch, (int)maxlen,
                       (int)dim, dk, dx, dx_stride, qcol);
    return dctr_launch_status("dctr_din_att_in_bwd");
}
