// What the units of the training step share (dnn_train_kernels.hip, crossnet_bwd_kernels.hip, cin_layered_kernels.hip,
// din_train_kernels.hip, mlp_bwd_kernels.hip): the grid sizing of the column-sum passes, the activation helpers of the elementwise
// kernels, and the declarations of every host launcher that one unit defines and another calls.  No kernel is defined here: the
// objects are built without relocatable device code, so a __global__ function lives in ONE unit and the other units reach it
// through the launcher next to it.
#pragma once
#include "dctr_common.h"
#include "act_device.h"

constexpr int BWD_ROWS = 16;     // batch rows per iteration of the generic Dice passes (the 16-B forms take over when N % 4 == 0)
constexpr int COLSUM_MAX_WG = 64;      // workgroups of a pass that ends in one atomic per column and workgroup

// workgroups of a column-sum pass over `rows` rows: enough of them to keep the loads in flight, few enough that the final atomics
// (one per column and workgroup, ~90 ns each on one address) stay a short tail
static inline unsigned colsum_grid(int64_t rows, int RL) {
    int64_t g = dctr_ceil_div(rows, (int64_t)RL * 4);
    const int64_t cap = rows >= 32768 ? 128 : COLSUM_MAX_WG;
    return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}

// grid of the BWD_ROWS-rows-per-iteration kernels (grid-stride over row blocks)
static inline unsigned rows_grid(int64_t rows, bool column_sums) {
    const int64_t nb = dctr_ceil_div(rows, (int64_t)BWD_ROWS), cap = column_sums ? COLSUM_MAX_WG : 16384;
    return (unsigned)(nb < 1 ? 1 : (nb > cap ? cap : nb));
}

// shapes the 16-B row-lane kernels take (thread (rl, c) owns columns 4c .. 4c+3 of rows rl, rl + RL, ...)
static inline bool rowlane4_ok(int N, const void* a, const void* b, int64_t stride) {
    return N % 4 == 0 && N >= 4 && N <= 1024 && stride % 4 == 0 && dctr_aligned16(a) && (b == nullptr || dctr_aligned16(b));
}

// dW = X^T dZ has a small output and a reduction as long as the batch: it runs as a strided batch of row slices into partial
// products + a sum (deterministic), 512 rows per slice from 1024 rows on, at most 32 slices (as ONE gemm a 429 x 256 output is 28
// workgroups walking the whole batch: 64 us per layer at B = 4096; round 2's rocBLAS call split K by itself at small batches and took
// 1.78 ms per layer at B = 65,536)
// (a SMALL output under a very long reduction — DIN's attention unit: 256 x 80 over 102,400 rows — gets up to 128 slices: as 32 slices
//  of 3,200 rows on 10 tiles it ran 268 us per layer on 320 workgroups)
static inline int mlp_dw_parts(int64_t batch, int64_t out_elems) {
    if (batch < 1024) return 1;
    const int64_t tiles = out_elems / 4096 > 1 ? out_elems / 4096 : 1;
    int64_t cap = 1024 / tiles;
    cap = cap < 32 ? 32 : (cap > 128 ? 128 : cap);
    int parts = (int)(batch / 512 > cap ? cap : batch / 512);
    while (parts > 1 && batch % parts != 0) --parts;
    return parts;
}

__device__ __forceinline__ float4 act_grad4(float4 d, float4 hv, int act) {
    if (act == DCTR_ACT_RELU) {
        d.x = hv.x > 0.f ? d.x : 0.f; d.y = hv.y > 0.f ? d.y : 0.f; d.z = hv.z > 0.f ? d.z : 0.f; d.w = hv.w > 0.f ? d.w : 0.f;
    } else if (act == DCTR_ACT_SIGMOID) {
        d.x *= hv.x * (1.f - hv.x); d.y *= hv.y * (1.f - hv.y); d.z *= hv.z * (1.f - hv.z); d.w *= hv.w * (1.f - hv.w);
    } else if (act == DCTR_ACT_TANH) {
        d.x *= 1.f - hv.x * hv.x; d.y *= 1.f - hv.y * hv.y; d.z *= 1.f - hv.z * hv.z; d.w *= 1.f - hv.w * hv.w;
    } else if (dctr_act::is_extended(act)) {      // elu, selu, softplus, softsign, exponential, hard_sigmoid: act' from the output
        d.x *= dctr_act::deriv_from_output(act, hv.x); d.y *= dctr_act::deriv_from_output(act, hv.y);
        d.z *= dctr_act::deriv_from_output(act, hv.z); d.w *= dctr_act::deriv_from_output(act, hv.w);
    }
    return d;
}

__device__ __forceinline__ void colsum4_finish(float4 acc, int N4, int RL, int c, float* __restrict__ out) {
    __shared__ float4 red[256];
    red[threadIdx.x] = acc;
    __syncthreads();
    if (out != nullptr && (int)threadIdx.x < N4) {
        float4 t = red[c];
        for (int r = 1; r < RL; ++r) {
            const float4 u = red[r * N4 + c];
            t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w;
        }
        unsafeAtomicAdd(out + 4 * c + 0, t.x);
        unsafeAtomicAdd(out + 4 * c + 1, t.y);
        unsafeAtomicAdd(out + 4 * c + 2, t.z);
        unsafeAtomicAdd(out + 4 * c + 3, t.w);
    }
}

__device__ __forceinline__ float act_value(float y, int act) {
    if (act == DCTR_ACT_RELU) return fmaxf(y, 0.f);
    if (act == DCTR_ACT_SIGMOID) return 1.f / (1.f + expf(-y));
    if (act == DCTR_ACT_TANH) return tanhf(y);
    return dctr_act::value(act, y);             // DCTR_ACT_ELU .. DCTR_ACT_GELU; anything else: y
}
__device__ __forceinline__ float act_deriv(float y, int act) {
    if (act == DCTR_ACT_RELU) return y > 0.f ? 1.f : 0.f;
    if (act == DCTR_ACT_SIGMOID) { const float s = 1.f / (1.f + expf(-y)); return s * (1.f - s); }
    if (act == DCTR_ACT_TANH) { const float t = tanhf(y); return 1.f - t * t; }
    return dctr_act::deriv_from_z(act, y);      // DCTR_ACT_ELU .. DCTR_ACT_GELU; anything else: 1
}

namespace dctr_train {   // defined in dnn_train_kernels.hip, next to their kernels
// in place: dh[b, n] *= act'(h[b, n]);  db[n] += sum_b dh[b, n]   (h == NULL: only the column sums)
void launch_act_bwd_colsum(hipStream_t st, float* dh, const float* h, int64_t batch, int N, int act, float* db);
// dz[b, n] = dlogit[b] * head_w[n] * act'(h[b, n]);  d_head_w[n] += sum_b dlogit[b] * h[b, n]
void launch_head_bwd(hipStream_t st, const float* dlogit, const float* head_w, const float* h, int64_t h_stride, int64_t batch,
                     int N, int act, float* dz, int64_t dz_stride, float* d_head_w);
// out[b, c] (+)= src[b, c] on `blocks` workgroups
void launch_add_rows(hipStream_t st, unsigned blocks, const float* src, int64_t src_stride, int64_t batch, int d, float* out,
                     int64_t out_stride, int accumulate);
// out[i] += sum_s parts[s * n + i] on `blocks` workgroups (the callers cap their grids differently)
void launch_sum_parts(hipStream_t st, unsigned blocks, const float* parts, int64_t n, int n_parts, float* out);
}  // namespace dctr_train

namespace dctr_mlp {   // mlp_bwd_kernels.hip: the backward chain of the DNN as one launch
int launch_bwd_chain(hipStream_t stream, int64_t batch, int in_dim, int n_layers, const int32_t* units_fwd, const float* const* Wt,
                     const float* const* acts, int activation, const float* dz_in, float* const* dz_out, float* dx, int64_t dx_stride);
bool bwd_chain_fits(int in_dim, int n_layers, const int32_t* units_fwd);
}  // namespace dctr_mlp
