// The tf.keras 2.x activation functions of the DNN beyond relu / sigmoid / tanh / linear / Dice (reference layers/activation.py:75-85:
// activation_layer hands the name to tf.keras.layers.Activation; keras/activations.py for the definitions): DCTR_ACT_ELU ..
// DCTR_ACT_GELU of include/dctr.h.  Three functions, each as a runtime switch on the code and as a template on it:
//     value(act, z)              f(z)
//     deriv_from_output(act, h)  f'(z) written in h = f(z) — the six functions that are invertible enough for that (the chained form of
//                                dctr_mlp_bwd keeps the forward's outputs only)
//     deriv_from_z(act, z)       f'(z) from the pre-activation (swish and gelu have no other form; dctr_dnn_train_layer_* works from z)
// Forms are chosen to stay finite and relatively accurate for |z| up to 30 and beyond: expm1f / log1pf where a difference with 1 would
// cancel, erfcf for gelu's normal tail, the sigmoid from exp(-|z|) so that nothing overflows.
//     elu           z > 0 ? z : exp(z) - 1 (alpha = 1)                               f' = h > 0 ? 1 : h + 1
//     selu          s (z > 0 ? z : a (exp(z) - 1))                                   f' = h > 0 ? s : h + s a
//     softplus      log(1 + exp(z)) = max(z, 0) + log1p(exp(-|z|))                   f' = sigmoid(z) = 1 - exp(-h) = -expm1(-h)
//     softsign      z / (1 + |z|)                                                    f' = 1 / (1 + |z|)^2 = (1 - |h|)^2
//     exponential   exp(z)                                                           f' = h
//     hard_sigmoid  clip(0.2 z + 0.5, 0, 1) (the Keras 2 form, as dctr_bilstm_fwd)   f' = 0 < h < 1 ? 0.2 : 0
//     swish (silu)  z sigmoid(z)                                                     f' = s (1 + z (1 - s)), s = sigmoid(z)
//     gelu          0.5 z (1 + erf(z / sqrt 2)) = 0.5 z erfc(-z / sqrt 2)            f' = Phi(z) + z phi(z)    (approximate=False)
#pragma once
#include <hip/hip_runtime.h>
#include "dctr.h"

namespace dctr_act {

constexpr float SELU_SCALE = 1.0507009873554805f;
constexpr float SELU_ALPHA = 1.6732632423543772f;
constexpr float SELU_SA = (float)(1.0507009873554805 * 1.6732632423543772);
// scale * alpha in two floats: selu' from the output is h + scale alpha, a difference of nearly equal numbers where the unit is saturated
// (h -> -scale alpha): h + SELU_SA is exact there and SELU_SA_LO puts back what rounding the constant to one float took
constexpr float SELU_SA_LO = (float)(1.0507009873554805 * 1.6732632423543772 - (double)SELU_SA);
constexpr float RSQRT2 = 0.70710678118654752f;
constexpr float RSQRT2PI = 0.39894228040143268f;

// host and device: which backward form a code takes
__host__ __device__ __forceinline__ constexpr bool is_extended(int act) { return act >= DCTR_ACT_ELU && act <= DCTR_ACT_GELU; }
__host__ __device__ __forceinline__ constexpr bool needs_z(int act) { return act == DCTR_ACT_SWISH || act == DCTR_ACT_GELU; }

// sigmoid(z) and sigmoid(-z) without overflow or cancellation on either side
__device__ __forceinline__ void sigmoid_pair(float z, float& s, float& sc) {
    const float e = expf(-fabsf(z)), r = 1.f / (1.f + e);
    const float big = r, small = e * r;
    s = z >= 0.f ? big : small;
    sc = z >= 0.f ? small : big;
}

template <int ACT>
__device__ __forceinline__ float value_t(float z) {
    if constexpr (ACT == DCTR_ACT_ELU) return z > 0.f ? z : expm1f(z);
    else if constexpr (ACT == DCTR_ACT_SELU) return z > 0.f ? SELU_SCALE * z : SELU_SA * expm1f(z);
    else if constexpr (ACT == DCTR_ACT_SOFTPLUS) return fmaxf(z, 0.f) + log1pf(expf(-fabsf(z)));
    else if constexpr (ACT == DCTR_ACT_SOFTSIGN) return z / (1.f + fabsf(z));
    else if constexpr (ACT == DCTR_ACT_EXPONENTIAL) return expf(z);
    else if constexpr (ACT == DCTR_ACT_HARD_SIGMOID) return fminf(fmaxf(fmaf(0.2f, z, 0.5f), 0.f), 1.f);
    else if constexpr (ACT == DCTR_ACT_SWISH) {
        float s, sc;
        sigmoid_pair(z, s, sc);
        return z * s;
    } else if constexpr (ACT == DCTR_ACT_GELU) return 0.5f * z * erfcf(-z * RSQRT2);
    else return z;
}

template <int ACT>
__device__ __forceinline__ float deriv_from_output_t(float h) {
    if constexpr (ACT == DCTR_ACT_ELU) return h > 0.f ? 1.f : h + 1.f;
    else if constexpr (ACT == DCTR_ACT_SELU) return h > 0.f ? SELU_SCALE : (h + SELU_SA) + SELU_SA_LO;
    else if constexpr (ACT == DCTR_ACT_SOFTPLUS) return -expm1f(-h);
    else if constexpr (ACT == DCTR_ACT_SOFTSIGN) { const float t = 1.f - fabsf(h); return t * t; }
    else if constexpr (ACT == DCTR_ACT_EXPONENTIAL) return h;
    else if constexpr (ACT == DCTR_ACT_HARD_SIGMOID) return (h > 0.f && h < 1.f) ? 0.2f : 0.f;
    else return 1.f;
}

template <int ACT>
__device__ __forceinline__ float deriv_from_z_t(float z) {
    if constexpr (ACT == DCTR_ACT_ELU) return z > 0.f ? 1.f : expf(z);
    else if constexpr (ACT == DCTR_ACT_SELU) return z > 0.f ? SELU_SCALE : SELU_SA * expf(z);
    else if constexpr (ACT == DCTR_ACT_SOFTPLUS) {
        float s, sc;
        sigmoid_pair(z, s, sc);
        return s;
    } else if constexpr (ACT == DCTR_ACT_SOFTSIGN) { const float t = 1.f / (1.f + fabsf(z)); return t * t; }
    else if constexpr (ACT == DCTR_ACT_EXPONENTIAL) return expf(z);
    else if constexpr (ACT == DCTR_ACT_HARD_SIGMOID) return (z > -2.5f && z < 2.5f) ? 0.2f : 0.f;
    else if constexpr (ACT == DCTR_ACT_SWISH) {
        float s, sc;
        sigmoid_pair(z, s, sc);
        return s * fmaf(z, sc, 1.f);
    } else if constexpr (ACT == DCTR_ACT_GELU) return fmaf(z * RSQRT2PI, expf(-0.5f * z * z), 0.5f * erfcf(-z * RSQRT2));
    else return 1.f;
}

#define DCTR_ACT_SWITCH(FN, act, v, dflt)                                             \
    switch (act) {                                                                    \
        case DCTR_ACT_ELU: return FN<DCTR_ACT_ELU>(v);                                \
        case DCTR_ACT_SELU: return FN<DCTR_ACT_SELU>(v);                              \
        case DCTR_ACT_SOFTPLUS: return FN<DCTR_ACT_SOFTPLUS>(v);                      \
        case DCTR_ACT_SOFTSIGN: return FN<DCTR_ACT_SOFTSIGN>(v);                      \
        case DCTR_ACT_EXPONENTIAL: return FN<DCTR_ACT_EXPONENTIAL>(v);                \
        case DCTR_ACT_HARD_SIGMOID: return FN<DCTR_ACT_HARD_SIGMOID>(v);              \
        case DCTR_ACT_SWISH: return FN<DCTR_ACT_SWISH>(v);                            \
        case DCTR_ACT_GELU: return FN<DCTR_ACT_GELU>(v);                              \
        default: return dflt;                                                         \
    }

// the runtime forms (codes outside DCTR_ACT_ELU .. DCTR_ACT_GELU: the identity / derivative 1 — the callers handle those themselves)
__device__ __forceinline__ float value(int act, float z) { DCTR_ACT_SWITCH(value_t, act, z, z) }
__device__ __forceinline__ float deriv_from_output(int act, float h) { DCTR_ACT_SWITCH(deriv_from_output_t, act, h, 1.f) }
__device__ __forceinline__ float deriv_from_z(int act, float z) { DCTR_ACT_SWITCH(deriv_from_z_t, act, z, 1.f) }
#undef DCTR_ACT_SWITCH

}  // namespace dctr_act
