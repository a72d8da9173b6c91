// The multi-task models' training step (DESIGN.md §4.15 "Training"): what the layered forward route (dctr_mlp_fwd per DNN, dctr_mtl_mix)
// needs beside dctr_mlp_bwd / dctr_dense1_bwd to run backwards.
//
// dctr_mtl_mix_bwd    backward of dctr_mtl_mix.  Per row b and gate g, with p = softmax(z_g Wg_g) recomputed (the forward saves nothing):
//                         a_j       = <d_out_g[b, :], h_{m_j}[b, :]>
//                         ds_g[b,j] = p_j (a_j - sum_i p_i a_i)                              (d loss / d gate logit)
//                         dh[b, e]  = sum over (g, j) with m_j = e of p_j d_out_g[b, :]      (g ascending, then j; zeros where no gate mixes e)
//                     The weight gradient dWg_g = z_g^T ds_g and dz_g = ds_g Wg_g^T are a bias-free linear layer's: dctr_mlp_bwd's GEMMs.
//                     One wave per row, as mtl_mix_kernel.  A gate of up to 8 members keeps its logits and a_j in registers (one sweep
//                     over z_g, one over d_out_g); a larger one takes them twice (first the softmax statistics and sum_i p_i a_i in
//                     one online sweep, then the outputs) and keeps nothing per member — any n_g, any width.
// dctr_mtl_loss_grad  d(sum_t w_t mean_b loss_t) / d logit_t for T tasks, the tasks' summed losses and bias gradients.  One workgroup
//                     per task walks the batch and reduces in a fixed order.
// dctr_mtl_sum_slots  dst[:, off : off + n] = (or +=) sum_k src_k[:, :n]: the gradient of a slot several DNNs read (dctr_mlp_bwd writes dx).
// No atomics anywhere: the same bits on every call.
#include <math.h>
#include "dctr_common.h"

namespace {

constexpr int XB_THREADS = 256;
constexpr int XB_MAX_GATES = 8;               // gates per dctr_mtl_mix_bwd launch (kernel-argument space)
constexpr int LG_THREADS = 512;
constexpr int LG_MAX_TASKS = 16;              // tasks per dctr_mtl_loss_grad launch
constexpr int SS_MAX_SRC = 16;

__device__ __forceinline__ float xb_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

struct XbParams {
    int64_t batch;
    const float* h;
    int64_t h_stride;
    int32_t E, H, G, dz, first;               // first: this launch clears the row of dh before it adds
    const float* z[XB_MAX_GATES];
    int64_t z_stride[XB_MAX_GATES];
    const float* gk[XB_MAX_GATES];
    int32_t gn[XB_MAX_GATES], goff[XB_MAX_GATES];   // goff: first member of the gate in `members` = its first column in ds / logits
    const int32_t* members;                    // device
    const float* d_out;                        // advanced to the first gate of this launch
    int64_t d_out_stride;
    float* dh;
    int64_t dh_stride;
    float* ds;
    int64_t ds_stride;
    float* logits;                             // may be null
    int64_t logits_stride;
};

__device__ __forceinline__ float xb_dot(const float* a, const float* b, int n, int lane) {
    float v = 0.f;
    for (int k = lane; k < n; k += 64) v = fmaf(a[k], b[k], v);
    return xb_wave_sum(v);
}

__device__ __forceinline__ float xb_logit(const float* zr, const float* W, int dz, int n, int j, int lane) {
    float l = 0.f;
    for (int k = lane; k < dz; k += 64) l = fmaf(zr[k], W[(int64_t)k * n + j], l);
    return xb_wave_sum(l);
}

constexpr int XB_SMALL = 8;                   // gates of up to this many members keep their logits and a_j in registers

// A gate of n <= XB_SMALL members: one sweep over z_g for all n logits, one over d_out_g for all n a_j, everything else in registers.
__device__ __forceinline__ void xb_gate_small(const float* zr, const float* W, int dz, int n, const int32_t* mem, const float* hr, const float* dg,
                                              int H, float* dhr, float* ds, float* logits, int lane) {
    float l[XB_SMALL], a[XB_SMALL];
    int32_t e[XB_SMALL];
#pragma unroll
    for (int j = 0; j < XB_SMALL; ++j) l[j] = 0.f, a[j] = 0.f, e[j] = j < n ? mem[j] : 0;
    for (int k = lane; k < dz; k += 64) {
        const float zk = zr[k];
        const float* wk = W + (int64_t)k * n;
#pragma unroll
        for (int j = 0; j < XB_SMALL; ++j)
            if (j < n) l[j] = fmaf(zk, wk[j], l[j]);
    }
    for (int c = lane; c < H; c += 64) {
        const float d = dg[c];
#pragma unroll
        for (int j = 0; j < XB_SMALL; ++j)
            if (j < n) a[j] = fmaf(d, hr[(int64_t)e[j] * H + c], a[j]);
    }
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < XB_SMALL; ++j)
        if (j < n) {
            l[j] = xb_wave_sum(l[j]);
            a[j] = xb_wave_sum(a[j]);
            m = fmaxf(m, l[j]);
        }
    float s = 0.f, mean = 0.f;
#pragma unroll
    for (int j = 0; j < XB_SMALL; ++j)
        if (j < n) {
            if (logits && lane == j) logits[j] = l[j];
            l[j] = expf(l[j] - m);          // from here on: the unnormalised weight
            s += l[j];
        }
#pragma unroll
    for (int j = 0; j < XB_SMALL; ++j)
        if (j < n) {
            l[j] = l[j] / s;
            mean = fmaf(l[j], a[j], mean);
        }
#pragma unroll
    for (int j = 0; j < XB_SMALL; ++j)
        if (j < n && lane == j) ds[j] = l[j] * (a[j] - mean);
    for (int c = lane; c < H; c += 64) {
        const float d = dg[c];
#pragma unroll
        for (int j = 0; j < XB_SMALL; ++j)
            if (j < n) {
                float* de = dhr + (int64_t)e[j] * H + c;          // (two members may name one expert: in order, through memory)
                *de = fmaf(l[j], d, *de);
            }
    }
}

// One wave per row.  A lane owns the columns c = lane, lane + 64, ... of every expert's slice of dh: it alone clears, reads and
// writes them, in the order (g, j) of the loops.
__global__ __launch_bounds__(XB_THREADS) void mtl_mix_bwd_kernel(XbParams p) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t)blockIdx.x * (XB_THREADS / 64) + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * (XB_THREADS / 64);
    for (int64_t r = wave0; r < p.batch; r += n_waves) {
        const float* hr = p.h + r * p.h_stride;
        float* dhr = p.dh + r * p.dh_stride;
        if (p.first)
            for (int e = 0; e < p.E; ++e)
                for (int c = lane; c < p.H; c += 64) dhr[(int64_t)e * p.H + c] = 0.f;
        for (int g = 0; g < p.G; ++g) {
            const float* zr = p.z[g] + r * p.z_stride[g];
            const float* W = p.gk[g];
            const int n = p.gn[g];
            const int32_t* mem = p.members + p.goff[g];
            const float* dg = p.d_out + r * p.d_out_stride + (int64_t)g * p.H;
            if (n <= XB_SMALL) {
                xb_gate_small(zr, W, p.dz, n, mem, hr, dg, p.H, dhr, p.ds + r * p.ds_stride + p.goff[g],
                              p.logits ? p.logits + r * p.logits_stride + p.goff[g] : nullptr, lane);
                continue;
            }
            // the softmax statistics and t = sum_j exp(l_j - m) a_j in one sweep
            float m = -INFINITY, s = 0.f, t = 0.f;
            for (int j = 0; j < n; ++j) {
                const float l = xb_logit(zr, W, p.dz, n, j, lane);
                const float a = xb_dot(dg, hr + (int64_t)mem[j] * p.H, p.H, lane);
                if (p.logits && lane == 0) p.logits[r * p.logits_stride + p.goff[g] + j] = l;
                const float m2 = fmaxf(m, l), keep = expf(m - m2), w = expf(l - m2);
                s = s * keep + w;
                t = t * keep + w * a;
                m = m2;
            }
            const float mean = t / s;
            for (int j = 0; j < n; ++j) {
                const float l = xb_logit(zr, W, p.dz, n, j, lane);
                const float a = xb_dot(dg, hr + (int64_t)mem[j] * p.H, p.H, lane);
                const float pj = expf(l - m) / s;
                if (lane == 0) p.ds[r * p.ds_stride + p.goff[g] + j] = pj * (a - mean);
                float* de = dhr + (int64_t)mem[j] * p.H;
                for (int c = lane; c < p.H; c += 64) de[c] = fmaf(pj, dg[c], de[c]);
            }
        }
    }
}

struct LgParams {
    int64_t batch;
    const float* pred;
    int64_t pred_stride;
    const float* y;
    int64_t y_stride;
    float* dlogit;
    int64_t dlogit_stride;
    float* loss_sum;
    int32_t T, esmm;
    int32_t mse[LG_MAX_TASKS];
    float weight[LG_MAX_TASKS];
    float* dbias[LG_MAX_TASKS];
};

// Keras' epsilon clip of a probability (backend.epsilon = 1e-7; in float32 the upper bound is 1 - 2^-23)
constexpr float LG_LO = 1e-7f, LG_HI = 1.f - 1e-7f;

__device__ __forceinline__ float lg_bce_value(float pc, float y) { return -(y * logf(pc) + (1.f - y) * logf(1.f - pc)); }

// sums[0 .. n) over the workgroup in a fixed order: lanes by butterfly, the waves one after the other; the result in thread 0
template <int N>
__device__ __forceinline__ void lg_block_sum(float (&v)[N], float* lds) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = xb_wave_sum(v[i]);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < N; ++i) lds[wave * N + i] = v[i];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < LG_THREADS / 64; ++w) {
#pragma unroll
            for (int i = 0; i < N; ++i) v[i] += lds[w * N + i];
        }
    }
}

// workgroup t = task t; with esmm workgroup 0 takes both tasks (task 1's gradient reaches logit 0 through ctcvr = ctr * cvr)
__global__ __launch_bounds__(LG_THREADS) void mtl_loss_grad_kernel(LgParams p) {
    __shared__ float lds[(LG_THREADS / 64) * 4];
    const int t = blockIdx.x;
    const float inv = 1.f / (float)p.batch;
    if (p.esmm) {
        if (t != 0) return;
        const float w0 = p.weight[0], w1 = p.weight[1];
        float acc[4] = {0.f, 0.f, 0.f, 0.f};            // loss 0, loss 1, d bias 0, d bias 1
        for (int64_t b = threadIdx.x; b < p.batch; b += LG_THREADS) {
            const float p0 = p.pred[b], c = p.pred[p.pred_stride + b], y0 = p.y[b], y1 = p.y[p.y_stride + b];
            const float p1 = p0 * c;
            const float pc1 = fminf(fmaxf(p1, LG_LO), LG_HI);
            // torch's clamp passes the gradient where lo <= x <= hi
            const float g = (p1 >= LG_LO && p1 <= LG_HI) ? w1 * (-y1 / pc1 + (1.f - y1) / (1.f - pc1)) * inv : 0.f;
            const float d0 = w0 * (p0 - y0) * inv + g * p1 * (1.f - p0), d1 = g * p1 * (1.f - c);
            p.dlogit[b] = d0;
            p.dlogit[p.dlogit_stride + b] = d1;
            acc[0] += lg_bce_value(fminf(fmaxf(p0, LG_LO), LG_HI), y0);
            acc[1] += lg_bce_value(pc1, y1);
            acc[2] += d0;
            acc[3] += d1;
        }
        lg_block_sum(acc, lds);
        if (threadIdx.x == 0) {
            p.loss_sum[0] += acc[0];
            p.loss_sum[1] += acc[1];
            if (p.dbias[0]) p.dbias[0][0] += acc[2];
            if (p.dbias[1]) p.dbias[1][0] += acc[3];
        }
        return;
    }
    const float* pr = p.pred + (int64_t)t * p.pred_stride;
    const float* yr = p.y + (int64_t)t * p.y_stride;
    float* dl = p.dlogit + (int64_t)t * p.dlogit_stride;
    const float w = p.weight[t];
    const bool mse = p.mse[t] != 0;
    float acc[2] = {0.f, 0.f};
    for (int64_t b = threadIdx.x; b < p.batch; b += LG_THREADS) {
        const float v = pr[b], y = yr[b];
        float d;
        if (mse) {
            d = 2.f * w * (v - y) * inv;
            acc[0] += (v - y) * (v - y);
        } else {
            d = w * (v - y) * inv;
            acc[0] += lg_bce_value(fminf(fmaxf(v, LG_LO), LG_HI), y);
        }
        dl[b] = d;
        acc[1] += d;
    }
    lg_block_sum(acc, lds);
    if (threadIdx.x == 0) {
        p.loss_sum[t] += acc[0];
        if (p.dbias[t]) p.dbias[t][0] += acc[1];
    }
}

struct SsParams {
    const float* src[SS_MAX_SRC];
    int64_t stride[SS_MAX_SRC];
};

__global__ __launch_bounds__(256) void mtl_sum_slots_kernel(SsParams p, int n_src, int64_t batch, int n, float* dst, int64_t dst_stride,
                                                            int accumulate) {
    const int64_t total = batch * n, step = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += step) {
        const int64_t r = i / n;
        const int c = (int)(i - r * n);
        float* d = dst + r * dst_stride + c;
        float v = accumulate ? *d + p.src[0][r * p.stride[0] + c] : p.src[0][r * p.stride[0] + c];
#pragma unroll 4
        for (int k = 1; k < n_src; ++k) v += p.src[k][r * p.stride[k] + c];
        *d = v;
    }
}

}  // namespace

extern "C" int dctr_mtl_mix_bwd(const dctr_mtl_mix_bwd_args_t* a, void* stream) {
    DCTR_REQUIRE(a, DCTR_E_NULL, "mtl_mix_bwd: null args");
    DCTR_REQUIRE(a->batch >= 0 && a->n_experts >= 1 && a->n_experts <= (1 << 16) && a->width >= 1 && a->width <= (1 << 24) && a->n_gates >= 1 &&
                     a->n_gates <= (1 << 16) && a->z_dim >= 1 && a->z_dim <= (1 << 24), DCTR_E_DIM,
                 "mtl_mix_bwd: batch = %lld, n_experts = %d, width = %d, n_gates = %d, z_dim = %d", (long long)a->batch, a->n_experts, a->width,
                 a->n_gates, a->z_dim);
    DCTR_REQUIRE(a->h && a->z && a->z_stride && a->gate_kernel && a->gate_n && a->members && a->members_dev && a->d_out && a->dh && a->ds, DCTR_E_NULL,
                 "mtl_mix_bwd: null h / z / z_stride / gate_kernel / gate_n / members / members_dev / d_out / dh / ds");
    const int64_t EH = (int64_t)a->n_experts * a->width, GH = (int64_t)a->n_gates * a->width;
    DCTR_REQUIRE(a->h_stride >= EH && a->dh_stride >= EH && a->d_out_offset >= 0 && a->d_out_offset + GH <= a->d_out_stride, DCTR_E_DIM,
                 "mtl_mix_bwd: h / dh rows of %lld / %lld for %lld columns, d_out columns [%lld, %lld) in rows of %lld", (long long)a->h_stride,
                 (long long)a->dh_stride, (long long)EH, (long long)a->d_out_offset, (long long)(a->d_out_offset + GH), (long long)a->d_out_stride);
    int64_t off = 0;
    for (int g = 0; g < a->n_gates; ++g) {
        DCTR_REQUIRE(a->z[g] && a->gate_kernel[g], DCTR_E_NULL, "mtl_mix_bwd: gate %d: null input / kernel", g);
        DCTR_REQUIRE(a->z_stride[g] >= a->z_dim, DCTR_E_DIM, "mtl_mix_bwd: gate %d: input rows of %lld for %d columns", g, (long long)a->z_stride[g],
                     a->z_dim);
        DCTR_REQUIRE(a->gate_n[g] >= 1 && a->gate_n[g] <= (1 << 16), DCTR_E_DIM, "mtl_mix_bwd: gate_n[%d] = %d", g, a->gate_n[g]);
        for (int j = 0; j < a->gate_n[g]; ++j)
            DCTR_REQUIRE(a->members[off + j] >= 0 && a->members[off + j] < a->n_experts, DCTR_E_DIM,
                         "mtl_mix_bwd: gate %d: member %d = %d with %d experts", g, j, a->members[off + j], a->n_experts);
        off += a->gate_n[g];
    }
    DCTR_REQUIRE(off <= 0x7fffffffLL && a->ds_stride >= off && (a->logits == nullptr || a->logits_stride >= off), DCTR_E_DIM,
                 "mtl_mix_bwd: ds / logits rows of %lld / %lld for %lld members", (long long)a->ds_stride, (long long)a->logits_stride, (long long)off);
    if (a->batch == 0) return DCTR_OK;
    const int64_t blocks = dctr_ceil_div(a->batch, (int64_t)(XB_THREADS / 64)), cap = 16 * (int64_t)dctr_n_cus();
    const dim3 grid((unsigned)(blocks < cap ? blocks : cap)), block(XB_THREADS);
    off = 0;
    for (int g0 = 0; g0 < a->n_gates; g0 += XB_MAX_GATES) {
        XbParams p = {};
        p.batch = a->batch, p.h = a->h, p.h_stride = a->h_stride, p.E = a->n_experts, p.H = a->width, p.dz = a->z_dim, p.first = g0 == 0;
        p.G = a->n_gates - g0 < XB_MAX_GATES ? a->n_gates - g0 : XB_MAX_GATES;
        p.members = a->members_dev;
        for (int g = 0; g < p.G; ++g) {
            p.z[g] = a->z[g0 + g], p.z_stride[g] = a->z_stride[g0 + g], p.gk[g] = a->gate_kernel[g0 + g];
            p.gn[g] = a->gate_n[g0 + g];
            p.goff[g] = (int32_t)off;
            off += a->gate_n[g0 + g];
        }
        p.d_out = a->d_out + a->d_out_offset + (int64_t)g0 * a->width;
        p.d_out_stride = a->d_out_stride;
        p.dh = a->dh, p.dh_stride = a->dh_stride, p.ds = a->ds, p.ds_stride = a->ds_stride;
        p.logits = a->logits, p.logits_stride = a->logits_stride;
        DCTR_LAUNCH(mtl_mix_bwd_kernel, grid, block, 0, (hipStream_t)stream, p);
        int rc = dctr_launch_status("dctr_mtl_mix_bwd");
        if (rc != DCTR_OK) return rc;
    }
    return DCTR_OK;
}

extern "C" int dctr_mtl_loss_grad(const dctr_mtl_loss_args_t* a, void* stream) {
    DCTR_REQUIRE(a, DCTR_E_NULL, "mtl_loss_grad: null args");
    DCTR_REQUIRE(a->batch >= 0 && a->n_tasks >= 1 && a->n_tasks <= (1 << 16), DCTR_E_DIM, "mtl_loss_grad: batch = %lld, n_tasks = %d",
                 (long long)a->batch, a->n_tasks);
    DCTR_REQUIRE(a->pred && a->y && a->loss_kind && a->binary && a->loss_weight && a->dlogit && a->loss_sum, DCTR_E_NULL,
                 "mtl_loss_grad: null pred / y / loss_kind / binary / loss_weight / dlogit / loss_sum");
    DCTR_REQUIRE(a->pred_stride >= a->batch && a->y_stride >= a->batch && a->dlogit_stride >= a->batch, DCTR_E_DIM,
                 "mtl_loss_grad: pred / y / dlogit rows of %lld / %lld / %lld for %lld samples", (long long)a->pred_stride, (long long)a->y_stride,
                 (long long)a->dlogit_stride, (long long)a->batch);
    DCTR_REQUIRE(a->esmm == 0 || a->esmm == 1, DCTR_E_ENUM, "mtl_loss_grad: esmm = %d", a->esmm);
    for (int t = 0; t < a->n_tasks; ++t) {
        DCTR_REQUIRE(a->loss_kind[t] == DCTR_MTL_LOSS_BCE || a->loss_kind[t] == DCTR_MTL_LOSS_MSE, DCTR_E_ENUM, "mtl_loss_grad: task %d: unknown loss kind %d", t,
                     a->loss_kind[t]);
        DCTR_REQUIRE((a->binary[t] != 0) == (a->loss_kind[t] == DCTR_MTL_LOSS_BCE), DCTR_E_UNSUPPORTED,
                     "mtl_loss_grad: task %d: binary = %d with loss kind %d (binary + BCE or regression + MSE)", t, a->binary[t], a->loss_kind[t]);
    }
    DCTR_REQUIRE(!a->esmm || (a->n_tasks == 2 && a->binary[0] && a->binary[1]), DCTR_E_ENUM, "mtl_loss_grad: esmm takes two binary tasks (%d given)",
                 a->n_tasks);
    if (a->batch == 0) return DCTR_OK;
    for (int t0 = 0; t0 < a->n_tasks; t0 += LG_MAX_TASKS) {
        LgParams p = {};
        p.T = a->n_tasks - t0 < LG_MAX_TASKS ? a->n_tasks - t0 : LG_MAX_TASKS;
        p.batch = a->batch, p.esmm = a->esmm;
        p.pred = a->pred + (int64_t)t0 * a->pred_stride, p.pred_stride = a->pred_stride;
        p.y = a->y + (int64_t)t0 * a->y_stride, p.y_stride = a->y_stride;
        p.dlogit = a->dlogit + (int64_t)t0 * a->dlogit_stride, p.dlogit_stride = a->dlogit_stride;
        p.loss_sum = a->loss_sum + t0;
        for (int t = 0; t < p.T; ++t) {
            p.mse[t] = a->loss_kind[t0 + t] == DCTR_MTL_LOSS_MSE;
            p.weight[t] = a->loss_weight[t0 + t];
            p.dbias[t] = a->dbias ? a->dbias[t0 + t] : nullptr;
        }
        DCTR_LAUNCH(mtl_loss_grad_kernel, dim3((unsigned)(a->esmm ? 1 : p.T)), dim3(LG_THREADS), 0, (hipStream_t)stream, p);
        int rc = dctr_launch_status("dctr_mtl_loss_grad");
        if (rc != DCTR_OK) return rc;
    }
    return DCTR_OK;
}

extern "C" int dctr_mtl_sum_slots(const float* const* src, const int64_t* src_stride, int32_t n_src, int64_t batch, int32_t n, float* dst,
                                  int64_t dst_stride, int64_t dst_offset, int32_t accumulate, void* stream) {
    DCTR_REQUIRE(src && src_stride && dst, DCTR_E_NULL, "mtl_sum_slots: null src / src_stride / dst");
    DCTR_REQUIRE(n_src >= 1 && n_src <= SS_MAX_SRC && batch >= 0 && n >= 1 && n <= (1 << 24), DCTR_E_DIM,
                 "mtl_sum_slots: n_src = %d (1 .. %d), batch = %lld, n = %d", n_src, SS_MAX_SRC, (long long)batch, n);
    DCTR_REQUIRE(dst_offset >= 0 && dst_offset + n <= dst_stride, DCTR_E_DIM, "mtl_sum_slots: dst columns [%lld, %lld) in rows of %lld",
                 (long long)dst_offset, (long long)(dst_offset + n), (long long)dst_stride);
    SsParams p = {};
    for (int k = 0; k < n_src; ++k) {
        DCTR_REQUIRE(src[k], DCTR_E_NULL, "mtl_sum_slots: source %d is null", k);
        DCTR_REQUIRE(src_stride[k] >= n, DCTR_E_DIM, "mtl_sum_slots: source %d: rows of %lld for %d columns", k, (long long)src_stride[k], n);
        p.src[k] = src[k], p.stride[k] = src_stride[k];
    }
    if (batch == 0) return DCTR_OK;
    const int64_t blocks = dctr_ceil_div(batch * n, (int64_t)256), cap = 16 * (int64_t)dctr_n_cus();
    DCTR_LAUNCH(mtl_sum_slots_kernel, dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(256), 0, (hipStream_t)stream, p, (int)n_src, batch, (int)n,
                dst + dst_offset, dst_stride, (int)(accumulate != 0));
    return dctr_launch_status("dctr_mtl_sum_slots");
}
