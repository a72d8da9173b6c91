// The optimizers of the HIP training step, all parameter segments of a model in ONE launch.
//   dctr_opt_multi, dctr_opt_multi_l2, dctr_adam_step, dctr_adam_multi
//                             tf.keras Adam / Adagrad / RMSprop / SGD (non-lazy: every row of a table moves every step, as TF's
//                             _resource_apply_sparse does), the reference's l2 regulariser folded in
//   dctr_opt_apply, dctr_grad_clip_scales, dctr_grad_clip_scales_workspace_bytes
//                             optimizer objects (deepctr_amd/optimizers.py): every tf.keras rule and variant, and the clipnorm /
//                             global_clipnorm pre-pass
// opt_apply_kernel's launch shape is opt_multi_kernel's (below, measured in profiles/r03c_opt_lab.log): blockIdx.y = segment, two
// 16-B groups per thread and trip with every load issued before the first use, non-temporal accesses, four groups per thread in the
// largest segment.  The rules are stated in include/dctr.h and DESIGN.md §7.  The reference has no code of its own for any of this
// (tf.keras.optimizers).
#include <stdlib.h>

#include "dctr_common.h"

namespace {

// ---------------------------------------------------------------------------------------------------
// Adam (Keras): m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;  w -= alpha * m / (sqrt(v) + eps),
// alpha = lr * sqrt(1 - b2^t) / (1 - b1^t) computed by the caller;  g includes 2*l2*w;  the gradient buffer is cleared.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ w, float* __restrict__ m, float* __restrict__ v,
                                                   float* __restrict__ g, int64_t n, float alpha, float b1, float b2, float eps,
                                                   float l2, int zero_grad) {
    const int64_t n4 = n / 4;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
        float4 wv = reinterpret_cast<float4*>(w)[i], mv = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
        const float4 gv = reinterpret_cast<float4*>(g)[i];
        float* wp = &wv.x; float* mp = &mv.x; float* vp = &vv.x; const float* gp = &gv.x;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float gg = fmaf(2.f * l2, wp[c], gp[c]);
            mp[c] = fmaf(b1, mp[c], (1.f - b1) * gg);
            vp[c] = fmaf(b2, vp[c], (1.f - b2) * gg * gg);
            wp[c] -= alpha * mp[c] / (sqrtf(vp[c]) + eps);
        }
        reinterpret_cast<float4*>(w)[i] = wv;
        reinterpret_cast<float4*>(m)[i] = mv;
        reinterpret_cast<float4*>(v)[i] = vv;
        if (zero_grad) reinterpret_cast<float4*>(g)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int64_t i = 4 * n4 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const float gg = fmaf(2.f * l2, w[i], g[i]);
        m[i] = fmaf(b1, m[i], (1.f - b1) * gg);
        v[i] = fmaf(b2, v[i], (1.f - b2) * gg * gg);
        w[i] -= alpha * m[i] / (sqrtf(v[i]) + eps);
        if (zero_grad) g[i] = 0.f;
    }
}

// one optimizer update of a single element (tf.keras formulas, optimizer_v2/{adam,adagrad,rmsprop,gradient_descent}.py)
template <int KIND>
__device__ __forceinline__ void opt_update(float& w, float& m, float& v, float g, float lr, float b1, float b2, float eps) {
    if constexpr (KIND == DCTR_OPT_ADAM) {            // lr = lr0 * sqrt(1 - b2^t) / (1 - b1^t) from the caller
        m = fmaf(b1, m, (1.f - b1) * g);
        v = fmaf(b2, v, (1.f - b2) * g * g);
        w -= lr * m / (sqrtf(v) + eps);
    } else if constexpr (KIND == DCTR_OPT_ADAGRAD) {  // v = accumulator (initial_accumulator_value set by the caller)
        v = fmaf(g, g, v);
        w -= lr * g / (sqrtf(v) + eps);
    } else if constexpr (KIND == DCTR_OPT_RMSPROP) {  // b2 = rho; no momentum, not centered
        v = fmaf(b2, v, (1.f - b2) * g * g);
        w -= lr * g / (sqrtf(v) + eps);
    } else {                                          // SGD without momentum
        w -= lr * g;
    }
}

// all parameters of a model in ONE launch: blockIdx.y = segment, blockIdx.x walks the segment (blocks past its end exit).
// sg.touched (embedding tables): one byte per 16-B group of the gradient table, set by the backward kernels where they added
// something — groups with a clear byte have a ZERO gradient, which is then neither read nor cleared (a 4096-row batch touches
// < 4 % of a 1e5-row table: 24 instead of 32 bytes of traffic per element; the update itself stays non-lazy, every element moves).
// Two 16-B groups per thread and trip, all their loads issued before the first use.
typedef float f32x4_nt __attribute__((ext_vector_type(4)));
template <bool NT>
__device__ __forceinline__ float4 ld4(const float4* p) {
    if constexpr (NT) {
        const f32x4_nt t = __builtin_nontemporal_load(reinterpret_cast<const f32x4_nt*>(p));
        return make_float4(t.x, t.y, t.z, t.w);
    } else {
        return *p;
    }
}
template <bool NT>
__device__ __forceinline__ void st4(float4* p, const float4& v) {
    if constexpr (NT) __builtin_nontemporal_store(f32x4_nt{v.x, v.y, v.z, v.w}, reinterpret_cast<f32x4_nt*>(p));
    else *p = v;
}

// PEN: also adds  pen_scale * sum_segments l2 * sum(w^2)  of the weights BEFORE the update to *pen — the l2 penalties tf.keras adds to
// that batch's loss (regularizers: inputs.py:22, layers/core.py:170, interaction.py:100,258,387); the weights pass through registers anyway
template <int KIND, int U = 2, bool NT = false, bool PEN = false>
__global__ __launch_bounds__(256) void opt_multi_kernel(const dctr_adam_seg_t* __restrict__ segs, float lr, float b1, float b2,
                                                        float eps, int zero_grad, double* __restrict__ pen, float pen_scale) {
    const dctr_adam_seg_t sg = segs[blockIdx.y];
    float4* __restrict__ w = reinterpret_cast<float4*>(sg.w);
    float4* __restrict__ m = reinterpret_cast<float4*>(sg.m);
    float4* __restrict__ v = reinterpret_cast<float4*>(sg.v);
    float4* __restrict__ g = reinterpret_cast<float4*>(sg.g);
    uint8_t* __restrict__ tch = sg.touched;
    const float l2 = sg.l2;
    const int64_t n = sg.n, n4 = n / 4;
    const int64_t stride = (int64_t)gridDim.x * 256;
    constexpr bool USE_M = KIND == DCTR_OPT_ADAM, USE_V = KIND != DCTR_OPT_SGD;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float psum = 0.f;                  // (PEN: this thread's share of sum(w^2): a few hundred terms at most)
    for (int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x; i0 < n4; i0 += U * stride) {
        bool in[U], has[U];
        float4 wv[U], mv[U], vv[U], gv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = i0 + u * stride;
            in[u] = i < n4;
            has[u] = in[u] && (tch == nullptr || tch[i] != 0);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = in[u] ? i0 + u * stride : i0;
            wv[u] = ld4<NT>(w + i);
            mv[u] = USE_M ? ld4<NT>(m + i) : z4;
            vv[u] = USE_V ? ld4<NT>(v + i) : z4;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) gv[u] = has[u] ? g[i0 + u * stride] : z4;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!in[u]) continue;
            const int64_t i = i0 + u * stride;
            float* wp = &wv[u].x; float* mp = &mv[u].x; float* vp = &vv[u].x; const float* gp = &gv[u].x;
            if constexpr (PEN) psum += (wp[0] * wp[0] + wp[1] * wp[1]) + (wp[2] * wp[2] + wp[3] * wp[3]);
#pragma unroll
            for (int c = 0; c < 4; ++c) opt_update<KIND>(wp[c], mp[c], vp[c], fmaf(2.f * l2, wp[c], gp[c]), lr, b1, b2, eps);
            st4<NT>(w + i, wv[u]);
            if (USE_M) st4<NT>(m + i, mv[u]);
            if (USE_V) st4<NT>(v + i, vv[u]);
            if (zero_grad && has[u]) {
                g[i] = z4;
                if (tch != nullptr) tch[i] = 0;
            }
        }
    }
    if (blockIdx.x == 0) {
        for (int64_t i = 4 * n4 + threadIdx.x; i < n; i += 256) {
            float mm = USE_M ? sg.m[i] : 0.f, vv = USE_V ? sg.v[i] : 0.f;
            if constexpr (PEN) psum = fmaf(sg.w[i], sg.w[i], psum);
            opt_update<KIND>(sg.w[i], mm, vv, fmaf(2.f * l2, sg.w[i], sg.g[i]), lr, b1, b2, eps);
            if (USE_M) sg.m[i] = mm;
            if (USE_V) sg.v[i] = vv;
            if (zero_grad) sg.g[i] = 0.f;
        }
    }
    if constexpr (PEN) {
        if (l2 != 0.f) {               // (uniform per workgroup: a segment's l2)
            __shared__ double pw[4];
            double d = (double)psum;
#pragma unroll
            for (int mk = 32; mk >= 1; mk >>= 1) d += __shfl_xor(d, mk, 64);
            if ((threadIdx.x & 63) == 0) pw[threadIdx.x >> 6] = d;
            __syncthreads();
            if (threadIdx.x == 0) {
                const double t = (pw[0] + pw[1]) + (pw[2] + pw[3]);
                if (t != 0.0) unsafeAtomicAdd(pen, t * (double)l2 * (double)pen_scale);
            }
        }
    }
}

// the launch scalars (dctr_opt_args_t without its pointers)
struct OptP {
    float lr, b1, b2, eps, mom, p, l1, l2f, l2s, clipvalue;
    int nesterov, centered, amsgrad, zero_grad;
};

// n^p of Ftrl's accumulator (p = -learning_rate_power; tf.keras' default 0.5 takes the square root)
__device__ __forceinline__ float ftrl_pow(float n, float p) { return p == 0.5f ? sqrtf(n) : powf(n, p); }

// one update of a single element; NS = the rule's state slots.  The four kinds dctr_opt_multi has are written exactly as its
// opt_update writes them: without flags and clipping the two entry points give the same bits.
template <int KIND, int NS>
__device__ __forceinline__ void opt_elem(float& w, float& s0, float& s1, float& s2, float g, const OptP& P) {
    const float lr = P.lr;
    if constexpr (KIND == DCTR_OPT_ADAM) {
        s0 = fmaf(P.b1, s0, (1.f - P.b1) * g);
        s1 = fmaf(P.b2, s1, (1.f - P.b2) * g * g);
        if constexpr (NS == 3) {                        // amsgrad
            s2 = fmaxf(s2, s1);
            w -= lr * s0 / (sqrtf(s2) + P.eps);
        } else {
            w -= lr * s0 / (sqrtf(s1) + P.eps);
        }
    } else if constexpr (KIND == DCTR_OPT_ADAGRAD) {
        s0 = fmaf(g, g, s0);
        w -= lr * g / (sqrtf(s0) + P.eps);
    } else if constexpr (KIND == DCTR_OPT_RMSPROP) {
        s0 = fmaf(P.b2, s0, (1.f - P.b2) * g * g);
        if constexpr (NS == 1) {
            w -= lr * g / (sqrtf(s0) + P.eps);
        } else {
            float den = s0;
            if (P.centered) {                           // s1 = mg
                s1 = fmaf(P.b2, s1, (1.f - P.b2) * g);
                den = s0 - s1 * s1;
            }
            if (P.mom > 0.f) {                          // the last slot = mom
                float& mo = NS == 3 ? s2 : s1;
                mo = fmaf(P.mom, mo, lr * g / sqrtf(den + P.eps));
                w -= mo;
            } else {
                w -= lr * g / (sqrtf(den) + P.eps);
            }
        }
    } else if constexpr (KIND == DCTR_OPT_SGD) {
        if constexpr (NS == 0) {
            w -= lr * g;
        } else {
            s0 = P.mom * s0 - lr * g;
            w += P.nesterov ? P.mom * s0 - lr * g : s0;
        }
    } else if constexpr (KIND == DCTR_OPT_ADAMAX) {
        s0 = fmaf(P.b1, s0, (1.f - P.b1) * g);
        s1 = fmaxf(P.b2 * s1, fabsf(g));
        w -= lr * s0 / (s1 + P.eps);
    } else if constexpr (KIND == DCTR_OPT_ADADELTA) {
        s0 = fmaf(P.b2, s0, (1.f - P.b2) * g * g);
        const float d = sqrtf(s1 + P.eps) / sqrtf(s0 + P.eps) * g;
        s1 = fmaf(P.b2, s1, (1.f - P.b2) * d * d);
        w -= lr * d;
    } else {                                            // FTRL: s0 = n, s1 = z
        const float gs = fmaf(2.f * P.l2s, w, g);
        const float n1 = fmaf(g, g, s0);
        const float pn1 = ftrl_pow(n1, P.p), pn0 = ftrl_pow(s0, P.p);
        s1 += gs - (pn1 - pn0) / lr * w;
        const float q = pn1 / lr + 2.f * P.l2f;
        w = fabsf(s1) > P.l1 ? (copysignf(P.l1, s1) - s1) / q : 0.f;
        s0 = n1;
    }
}

// g_raw + 2 l2 w, scaled (clipnorm / global_clipnorm) and clamped (clipvalue)
__device__ __forceinline__ float clipped(float g_raw, float w, float l2x2, float scale, bool scaled, float cv) {
    float g = fmaf(l2x2, w, g_raw);
    if (scaled) g *= scale;
    if (cv > 0.f) g = fminf(fmaxf(g, -cv), cv);
    return g;
}

template <int KIND, int NS, bool PEN>
__global__ __launch_bounds__(256) void opt_apply_kernel(const dctr_opt_seg_t* __restrict__ segs, OptP P, const float* __restrict__ clip_scale,
                                                        double* __restrict__ pen, float pen_scale) {
    const dctr_opt_seg_t sg = segs[blockIdx.y];
    if (sg.w == nullptr || sg.g == nullptr || sg.n <= 0) return;
    if ((NS >= 1 && sg.s0 == nullptr) || (NS >= 2 && sg.s1 == nullptr) || (NS >= 3 && sg.s2 == nullptr)) return;
    const bool scaled = clip_scale != nullptr;
    const float scale = scaled ? clip_scale[blockIdx.y] : 1.f;
    const float l2 = sg.l2, l2x2 = 2.f * l2, cv = P.clipvalue;
    const int zero_grad = P.zero_grad;
    // 16-byte accesses need every buffer of the segment on a 16-byte boundary; a segment that is not runs element by element
    uintptr_t bits = (uintptr_t)sg.w | (uintptr_t)sg.g;
    if (NS >= 1) bits |= (uintptr_t)sg.s0;
    if (NS >= 2) bits |= (uintptr_t)sg.s1;
    if (NS >= 3) bits |= (uintptr_t)sg.s2;
    const bool wide = (bits & 15u) == 0;
    const int64_t n = sg.n, n4 = wide ? n / 4 : 0;
    const int64_t stride = (int64_t)gridDim.x * 256;
    float4* __restrict__ w = reinterpret_cast<float4*>(sg.w);
    float4* __restrict__ g = reinterpret_cast<float4*>(sg.g);
    float4* __restrict__ a0 = reinterpret_cast<float4*>(sg.s0);
    float4* __restrict__ a1 = reinterpret_cast<float4*>(sg.s1);
    float4* __restrict__ a2 = reinterpret_cast<float4*>(sg.s2);
    uint8_t* __restrict__ tch = wide ? sg.touched : nullptr;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    constexpr int U = 2;
    float psum = 0.f;                  // (PEN: this thread's share of sum(w^2))
    for (int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x; i0 < n4; i0 += U * stride) {
        bool in[U], has[U];
        float4 wv[U], v0[U], v1[U], v2[U], gv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = i0 + u * stride;
            in[u] = i < n4;
            has[u] = in[u] && (tch == nullptr || tch[i] != 0);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = in[u] ? i0 + u * stride : i0;
            wv[u] = ld4<true>(w + i);
            v0[u] = NS >= 1 ? ld4<true>(a0 + i) : z4;
            v1[u] = NS >= 2 ? ld4<true>(a1 + i) : z4;
            v2[u] = NS >= 3 ? ld4<true>(a2 + i) : z4;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) gv[u] = has[u] ? g[i0 + u * stride] : z4;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!in[u]) continue;
            const int64_t i = i0 + u * stride;
            float* wp = &wv[u].x; float* p0 = &v0[u].x; float* p1 = &v1[u].x; float* p2 = &v2[u].x; const float* gp = &gv[u].x;
            if constexpr (PEN) psum += (wp[0] * wp[0] + wp[1] * wp[1]) + (wp[2] * wp[2] + wp[3] * wp[3]);
#pragma unroll
            for (int c = 0; c < 4; ++c) opt_elem<KIND, NS>(wp[c], p0[c], p1[c], p2[c], clipped(gp[c], wp[c], l2x2, scale, scaled, cv), P);
            st4<true>(w + i, wv[u]);
            if (NS >= 1) st4<true>(a0 + i, v0[u]);
            if (NS >= 2) st4<true>(a1 + i, v1[u]);
            if (NS >= 3) st4<true>(a2 + i, v2[u]);
            if (zero_grad && has[u]) {
                g[i] = z4;
                if (tch != nullptr) tch[i] = 0;
            }
        }
    }
    // the elements past the last whole group (block 0), or the whole of a segment that is not 16-byte aligned (every block)
    const int64_t t0 = wide ? 4 * n4 + threadIdx.x : (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t tstride = wide ? 256 : stride;
    if (!wide || blockIdx.x == 0) {
        for (int64_t i = t0; i < n; i += tstride) {
            float ww = sg.w[i], q0 = NS >= 1 ? sg.s0[i] : 0.f, q1 = NS >= 2 ? sg.s1[i] : 0.f, q2 = NS >= 3 ? sg.s2[i] : 0.f;
            if constexpr (PEN) psum = fmaf(ww, ww, psum);
            opt_elem<KIND, NS>(ww, q0, q1, q2, clipped(sg.g[i], ww, l2x2, scale, scaled, cv), P);
            sg.w[i] = ww;
            if (NS >= 1) sg.s0[i] = q0;
            if (NS >= 2) sg.s1[i] = q1;
            if (NS >= 3) sg.s2[i] = q2;
            if (zero_grad) sg.g[i] = 0.f;
        }
    }
    if constexpr (PEN) {
        if (l2 != 0.f) {               // (uniform per workgroup: a segment's l2)
            __shared__ double pw[4];
            double d = (double)psum;
#pragma unroll
            for (int mk = 32; mk >= 1; mk >>= 1) d += __shfl_xor(d, mk, 64);
            if ((threadIdx.x & 63) == 0) pw[threadIdx.x >> 6] = d;
            __syncthreads();
            if (threadIdx.x == 0) {
                const double t = (pw[0] + pw[1]) + (pw[2] + pw[3]);
                if (t != 0.0) unsafeAtomicAdd(pen, t * (double)l2 * (double)pen_scale);
            }
        }
    }
}

// ---- clipnorm / global_clipnorm pre-pass -----------------------------------------------------------------------------------------
constexpr int CLIP_BX_MAX = 512;      // workgroups per segment at most: the second launch reads n_segs * bx partial sums

__host__ __device__ inline int64_t clip_bx(int64_t max_n) {
    int64_t bx = (max_n / 4 + 1 + 256 * 4 - 1) / (256 * 4);
    return bx > CLIP_BX_MAX ? CLIP_BX_MAX : (bx < 1 ? 1 : bx);
}

// sum over a workgroup's share of the segment of (g + 2 l2 w)^2, float64, into part[segment * gridDim.x + blockIdx.x]; the order of
// the additions is a function of the launch shape alone
__global__ __launch_bounds__(256) void clip_partial_kernel(const dctr_opt_seg_t* __restrict__ segs, double* __restrict__ part) {
    const dctr_opt_seg_t sg = segs[blockIdx.y];
    double acc = 0.0;
    if (sg.w != nullptr && sg.g != nullptr && sg.n > 0) {
        const float l2x2 = 2.f * sg.l2;
        const bool wide = ((((uintptr_t)sg.w) | ((uintptr_t)sg.g)) & 15u) == 0;
        const int64_t n = sg.n, n4 = wide ? n / 4 : 0;
        const int64_t stride = (int64_t)gridDim.x * 256;
        const float4* __restrict__ w = reinterpret_cast<const float4*>(sg.w);
        const float4* __restrict__ g = reinterpret_cast<const float4*>(sg.g);
        const uint8_t* __restrict__ tch = wide ? sg.touched : nullptr;
        const bool need_w = l2x2 != 0.f;
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
            const bool has = tch == nullptr || tch[i] != 0;
            if (!has && !need_w) continue;             // a clear byte = a zero data gradient, and no penalty term: nothing to add
            const float4 gv = has ? g[i] : make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 wv = need_w ? w[i] : make_float4(0.f, 0.f, 0.f, 0.f);
            const float e0 = fmaf(l2x2, wv.x, gv.x), e1 = fmaf(l2x2, wv.y, gv.y), e2 = fmaf(l2x2, wv.z, gv.z), e3 = fmaf(l2x2, wv.w, gv.w);
            acc += ((double)e0 * e0 + (double)e1 * e1) + ((double)e2 * e2 + (double)e3 * e3);
        }
        const int64_t t0 = wide ? 4 * n4 + threadIdx.x : (int64_t)blockIdx.x * 256 + threadIdx.x;
        if (!wide || blockIdx.x == 0) {
            for (int64_t i = t0; i < n; i += wide ? 256 : stride) {
                const float e = fmaf(l2x2, need_w ? sg.w[i] : 0.f, sg.g[i]);
                acc += (double)e * e;
            }
        }
    }
    __shared__ double pw[4];
#pragma unroll
    for (int mk = 32; mk >= 1; mk >>= 1) acc += __shfl_xor(acc, mk, 64);
    if ((threadIdx.x & 63) == 0) pw[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = (pw[0] + pw[1]) + (pw[2] + pw[3]);
}

// a workgroup's fixed-order sum of `count` doubles (every thread returns it)
__device__ __forceinline__ double block_sum(const double* __restrict__ v, int64_t count, double* sh) {
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < count; i += 256) acc += v[i];
#pragma unroll
    for (int mk = 32; mk >= 1; mk >>= 1) acc += __shfl_xor(acc, mk, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// one workgroup per segment: its sum of squares -> sumsq[segment]; PER_SEGMENT: its scale as well
__global__ __launch_bounds__(256) void clip_segment_kernel(const double* __restrict__ part, int bx, double* __restrict__ sumsq, int per_segment,
                                                           float clip, float* __restrict__ clip_scale) {
    __shared__ double sh[4];
    const double s = block_sum(part + (int64_t)blockIdx.x * bx, bx, sh);
    if (threadIdx.x == 0) {
        sumsq[blockIdx.x] = s;
        if (per_segment) clip_scale[blockIdx.x] = (float)((double)clip / fmax(sqrt(s), (double)clip));
    }
}

// GLOBAL: one workgroup adds the segments' sums and writes the one scale for all of them
__global__ __launch_bounds__(256) void clip_global_kernel(const double* __restrict__ sumsq, int n_segs, float clip, float* __restrict__ clip_scale) {
    __shared__ double sh[4];
    const double s = block_sum(sumsq, n_segs, sh);
    const float scale = (float)((double)clip / fmax(sqrt(s), (double)clip));
    for (int i = threadIdx.x; i < n_segs; i += 256) clip_scale[i] = scale;
}

template <int KIND, int NS>
void launch_apply(dim3 grid, hipStream_t st, const dctr_opt_seg_t* segs, const OptP& P, const dctr_opt_args_t* a) {
    if (a->l2_penalty != nullptr)
        hipLaunchKernelGGL((opt_apply_kernel<KIND, NS, true>), grid, dim3(256), 0, st, segs, P, a->clip_scale, a->l2_penalty, a->penalty_scale);
    else
        hipLaunchKernelGGL((opt_apply_kernel<KIND, NS, false>), grid, dim3(256), 0, st, segs, P, a->clip_scale, (double*)nullptr, 0.f);
}

}  // namespace

extern "C" int dctr_opt_apply(const dctr_opt_args_t* a, const dctr_opt_seg_t* segs, int32_t n_segs, int64_t max_n, void* stream) {
    DCTR_REQUIRE(a != nullptr, DCTR_E_NULL, "opt_apply: null args");
    DCTR_REQUIRE(a->kind >= DCTR_OPT_ADAM && a->kind <= DCTR_OPT_FTRL, DCTR_E_ENUM, "opt_apply: optimizer kind %d", a->kind);
    DCTR_REQUIRE(a->kind != DCTR_OPT_FTRL || (a->lr_power <= 0.f && a->lr > 0.f), DCTR_E_ENUM,
                 "opt_apply: Ftrl needs learning_rate_power <= 0 and lr > 0");
    DCTR_REQUIRE(n_segs >= 0 && n_segs <= 65535 && max_n >= 0, DCTR_E_DIM, "opt_apply: bad n_segs / max_n");
    if (n_segs == 0 || max_n == 0) return DCTR_OK;
    DCTR_REQUIRE(segs != nullptr, DCTR_E_NULL, "opt_apply: null segment array");
    DCTR_REQUIRE((((uintptr_t)segs) & 7u) == 0 && (((uintptr_t)a->clip_scale) & 3u) == 0 && (((uintptr_t)a->l2_penalty) & 7u) == 0,
                 DCTR_E_ALIGN, "opt_apply: segs / l2_penalty need 8-byte, clip_scale 4-byte alignment");
    OptP P;
    P.lr = a->lr; P.b1 = a->beta1; P.b2 = a->beta2; P.eps = a->eps; P.mom = a->momentum; P.p = -a->lr_power; P.l1 = a->l1;
    P.l2f = a->l2_ftrl; P.l2s = a->l2_shrinkage; P.clipvalue = a->clipvalue;
    P.nesterov = a->nesterov != 0; P.centered = a->centered != 0; P.amsgrad = a->amsgrad != 0; P.zero_grad = a->zero_grad != 0;
    int64_t bx = dctr_ceil_div(max_n / 4 + 1, (int64_t)(256 * 4));
    if (bx > 4096) bx = 4096;
    const dim3 grid((unsigned)bx, (unsigned)n_segs);
    hipStream_t st = (hipStream_t)stream;
    switch (a->kind) {
        case DCTR_OPT_ADAM:
            if (P.amsgrad) launch_apply<DCTR_OPT_ADAM, 3>(grid, st, segs, P, a);
            else launch_apply<DCTR_OPT_ADAM, 2>(grid, st, segs, P, a);
            break;
        case DCTR_OPT_ADAGRAD: launch_apply<DCTR_OPT_ADAGRAD, 1>(grid, st, segs, P, a); break;
        case DCTR_OPT_RMSPROP: {
            const int ns = 1 + (P.centered ? 1 : 0) + (P.mom > 0.f ? 1 : 0);
            if (ns == 1) launch_apply<DCTR_OPT_RMSPROP, 1>(grid, st, segs, P, a);
            else if (ns == 2) launch_apply<DCTR_OPT_RMSPROP, 2>(grid, st, segs, P, a);
            else launch_apply<DCTR_OPT_RMSPROP, 3>(grid, st, segs, P, a);
            break;
        }
        case DCTR_OPT_SGD:
            if (P.mom != 0.f) launch_apply<DCTR_OPT_SGD, 1>(grid, st, segs, P, a);
            else launch_apply<DCTR_OPT_SGD, 0>(grid, st, segs, P, a);
            break;
        case DCTR_OPT_ADAMAX: launch_apply<DCTR_OPT_ADAMAX, 2>(grid, st, segs, P, a); break;
        case DCTR_OPT_ADADELTA: launch_apply<DCTR_OPT_ADADELTA, 2>(grid, st, segs, P, a); break;
        default: launch_apply<DCTR_OPT_FTRL, 2>(grid, st, segs, P, a); break;
    }
    return dctr_launch_status("dctr_opt_apply");
}

extern "C" size_t dctr_grad_clip_scales_workspace_bytes(int32_t n_segs, int64_t max_n) {
    if (n_segs <= 0 || max_n < 0) return 0;
    return (size_t)n_segs * (size_t)(clip_bx(max_n) + 1) * sizeof(double);
}

extern "C" int dctr_grad_clip_scales(const dctr_opt_seg_t* segs, int32_t n_segs, int64_t max_n, int32_t mode, float clip, void* workspace,
                                     size_t workspace_bytes, float* clip_scale, void* stream) {
    DCTR_REQUIRE(mode == DCTR_CLIP_PER_SEGMENT || mode == DCTR_CLIP_GLOBAL, DCTR_E_ENUM, "grad_clip_scales: mode %d", mode);
    DCTR_REQUIRE(n_segs >= 0 && n_segs <= 65535 && max_n >= 0 && clip > 0.f, DCTR_E_DIM, "grad_clip_scales: bad n_segs / max_n / clip");
    if (n_segs == 0) return DCTR_OK;
    DCTR_REQUIRE(segs != nullptr && clip_scale != nullptr && workspace != nullptr, DCTR_E_NULL, "grad_clip_scales: null segs / clip_scale / workspace");
    DCTR_REQUIRE(workspace_bytes >= dctr_grad_clip_scales_workspace_bytes(n_segs, max_n), DCTR_E_NULL,
                 "grad_clip_scales: workspace of %zu bytes, %zu needed", workspace_bytes, dctr_grad_clip_scales_workspace_bytes(n_segs, max_n));
    DCTR_REQUIRE((((uintptr_t)segs) & 7u) == 0 && (((uintptr_t)workspace) & 7u) == 0 && (((uintptr_t)clip_scale) & 3u) == 0, DCTR_E_ALIGN,
                 "grad_clip_scales: segs / workspace need 8-byte, clip_scale 4-byte alignment");
    const int bx = (int)clip_bx(max_n);
    double* part = static_cast<double*>(workspace);
    double* sumsq = part + (size_t)n_segs * bx;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(clip_partial_kernel, dim3((unsigned)bx, (unsigned)n_segs), dim3(256), 0, st, segs, part);
    hipLaunchKernelGGL(clip_segment_kernel, dim3((unsigned)n_segs), dim3(256), 0, st, part, bx, sumsq, (int)(mode == DCTR_CLIP_PER_SEGMENT), clip,
                       clip_scale);
    if (mode == DCTR_CLIP_GLOBAL) hipLaunchKernelGGL(clip_global_kernel, dim3(1), dim3(256), 0, st, sumsq, (int)n_segs, clip, clip_scale);
    return dctr_launch_status("dctr_grad_clip_scales");
}

extern "C" int dctr_adam_step(float* w, float* m, float* v, float* g, int64_t n, float alpha, float beta1, float beta2,
                              float eps, float l2, int32_t zero_grad, void* stream) {
    DCTR_REQUIRE(n >= 0, DCTR_E_DIM, "adam_step: n < 0");
    if (n == 0) return DCTR_OK;
    DCTR_REQUIRE(w && m && v && g, DCTR_E_NULL, "adam_step: null pointer");
    DCTR_REQUIRE(dctr_aligned16(w) && dctr_aligned16(m) && dctr_aligned16(v) && dctr_aligned16(g), DCTR_E_ALIGN,
                 "adam_step: buffers must be 16-B aligned");
    int64_t blocks = dctr_ceil_div(n / 4 + 1, (int64_t)256);
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, w, m, v, g, n, alpha, beta1, beta2,
                       eps, l2, (int)zero_grad);
    return dctr_launch_status("dctr_adam_step");
}

extern "C" int dctr_opt_multi(int32_t kind, const dctr_adam_seg_t* segs, int32_t n_segs, int64_t max_n, float lr, float beta1,
                              float beta2, float eps, int32_t zero_grad, void* stream) {
    return dctr_opt_multi_l2(kind, segs, n_segs, max_n, lr, beta1, beta2, eps, zero_grad, nullptr, 0.f, stream);
}

// ABI 13 — the same step; with l2_penalty != NULL the launch also adds penalty_scale * sum over the segments of l2 * sum(w^2), taken on the
// weights BEFORE the update, to *l2_penalty (a DEVICE double): what tf.keras adds to that batch's reported loss
extern "C" int dctr_opt_multi_l2(int32_t kind, const dctr_adam_seg_t* segs, int32_t n_segs, int64_t max_n, float lr, float beta1,
                                 float beta2, float eps, int32_t zero_grad, double* l2_penalty, float penalty_scale, void* stream) {
    DCTR_REQUIRE(kind >= DCTR_OPT_ADAM && kind <= DCTR_OPT_SGD, DCTR_E_ENUM, "opt_multi: optimizer kind %d", kind);
    DCTR_REQUIRE(n_segs >= 0 && n_segs <= 65535 && max_n >= 0, DCTR_E_DIM, "opt_multi: bad n_segs / max_n");
    if (n_segs == 0 || max_n == 0) return DCTR_OK;
    DCTR_REQUIRE(segs != nullptr, DCTR_E_NULL, "opt_multi: null segment array");
    // Two 16-B groups per trip, non-temporal loads / stores, four groups per thread in the largest segment: 175 us for the C2 DeepFM
    // parameter set with touched bytes (6.15 TB/s) against 215 us with default-policy accesses and 205 us with four groups per trip
    // (profiles/r03c_opt_lab.log).  DCTR_OPT_VARIANT / DCTR_OPT_F4 re-run that lab (scripts/opt_lab.py).
    static const int f4 = [] { const char* e = dctr_lab_env("DCTR_OPT_F4"); return e != nullptr && atoi(e) >= 1 ? atoi(e) : 4; }();
    static const int variant = [] { const char* e = dctr_lab_env("DCTR_OPT_VARIANT"); return e != nullptr ? atoi(e) : 2; }();
    int64_t bx = dctr_ceil_div(max_n / 4 + 1, (int64_t)(256 * f4));
    if (bx > 4096) bx = 4096;
    const dim3 grid((unsigned)bx, (unsigned)n_segs);
    hipStream_t st = (hipStream_t)stream;
#define DCTR_OPT_LAUNCH(K)                                                                                                                     \
    do {                                                                                                                                       \
        if (pen != nullptr) hipLaunchKernelGGL((opt_multi_kernel<K, 2, true, true>), grid, dim3(256), 0, st, segs, lr, beta1, beta2, eps, (int)zero_grad, pen, penalty_scale); \
        else if (variant == 0) hipLaunchKernelGGL((opt_multi_kernel<K, 2, false>), grid, dim3(256), 0, st, segs, lr, beta1, beta2, eps, (int)zero_grad, pen, 0.f);      \
        else if (variant == 1) hipLaunchKernelGGL((opt_multi_kernel<K, 4, false>), grid, dim3(256), 0, st, segs, lr, beta1, beta2, eps, (int)zero_grad, pen, 0.f); \
        else if (variant == 3) hipLaunchKernelGGL((opt_multi_kernel<K, 4, true>), grid, dim3(256), 0, st, segs, lr, beta1, beta2, eps, (int)zero_grad, pen, 0.f);  \
        else hipLaunchKernelGGL((opt_multi_kernel<K, 2, true>), grid, dim3(256), 0, st, segs, lr, beta1, beta2, eps, (int)zero_grad, pen, 0.f);                    \
    } while (0)
#define DCTR_OPT_LAUNCH2(K)                                                                                                                    \
    do {                                                                                                                                       \
        if (pen != nullptr) hipLaunchKernelGGL((opt_multi_kernel<K, 2, true, true>), grid, dim3(256), 0, st, segs, lr, beta1, beta2, eps, (int)zero_grad, pen, penalty_scale); \
        else hipLaunchKernelGGL((opt_multi_kernel<K, 2, true>), grid, dim3(256), 0, st, segs, lr, beta1, beta2, eps, (int)zero_grad, pen, 0.f);  \
    } while (0)
    double* pen = l2_penalty;
    switch (kind) {
        case DCTR_OPT_ADAM: DCTR_OPT_LAUNCH(DCTR_OPT_ADAM); break;
        case DCTR_OPT_ADAGRAD: DCTR_OPT_LAUNCH2(DCTR_OPT_ADAGRAD); break;
        case DCTR_OPT_RMSPROP: DCTR_OPT_LAUNCH2(DCTR_OPT_RMSPROP); break;
        default: DCTR_OPT_LAUNCH2(DCTR_OPT_SGD); break;
    }
#undef DCTR_OPT_LAUNCH
#undef DCTR_OPT_LAUNCH2
    return dctr_launch_status("dctr_opt_multi");
}

extern "C" int dctr_adam_multi(const dctr_adam_seg_t* segs, int32_t n_segs, int64_t max_n, float alpha, float beta1, float beta2,
                               float eps, int32_t zero_grad, void* stream) {
    return dctr_opt_multi(DCTR_OPT_ADAM, segs, n_segs, max_n, alpha, beta1, beta2, eps, zero_grad, stream);
}
