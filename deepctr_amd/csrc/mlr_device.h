// What dctr_mlr_fwd and dctr_mlr_bwd share (include/dctr.h: MLR): the host checks, the lane-group reductions and the mixture itself.
// A sample is a group of G lanes (8 / 16 / 32 / 64, the smallest holding K = 2R (+1) columns), lane c of the group owns column c.
#pragma once
#include <stdint.h>
#include "dctr_common.h"
#include "act_device.h"

namespace dctr_mlr {

constexpr int THREADS = 256;

inline int columns(const dctr_mlr_args_t* a) { return 2 * a->region_num + (a->has_bias ? 1 : 0); }

inline int group_lanes(int K) { return K <= 8 ? 8 : K <= 16 ? 16 : K <= 32 ? 32 : 64; }

// the checks that look at no pointer's target: shapes, enums, K <= 64, then the pointers the forward and the backward both need
inline int check(const dctr_mlr_args_t* a, const char* op) {
    DCTR_REQUIRE(a->region_num >= 2, DCTR_E_DIM, "%s: region_num = %d: region_num must > 1", op, a->region_num);
    DCTR_REQUIRE(a->batch >= 0 && a->n_fields >= 0 && a->n_dense >= 0 && a->z_offset >= 0, DCTR_E_DIM, "%s: negative size", op);
    DCTR_REQUIRE(a->has_bias == 0 || a->has_bias == 1, DCTR_E_ENUM, "%s: has_bias = %d", op, a->has_bias);
    DCTR_REQUIRE(a->learner_act == DCTR_MLR_LEARNER_SIGMOID || a->learner_act == DCTR_MLR_LEARNER_LINEAR, DCTR_E_ENUM,
                 "%s: unknown learner_act %d", op, a->learner_act);
    DCTR_REQUIRE(a->region_num <= (DCTR_MLR_MAX_COLUMNS - a->has_bias) / 2, DCTR_E_UNSUPPORTED,
                 "%s: region_num = %d%s: more than %d logit columns", op, a->region_num, a->has_bias ? " with a bias part" : "",
                 DCTR_MLR_MAX_COLUMNS);
    DCTR_REQUIRE(a->n_fields == 0 || a->fields, DCTR_E_NULL, "%s: null fields", op);
    DCTR_REQUIRE((((uintptr_t)a->fields) & 7u) == 0, DCTR_E_ALIGN, "%s: fields not 8-byte aligned", op);
    DCTR_REQUIRE(a->batch < ((int64_t)1 << 31), DCTR_E_DIM, "%s: batch %lld: one launch takes fewer than 2^31 samples", op, (long long)a->batch);
    return DCTR_OK;
}

template <int G>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int m = G >> 1; m > 0; m >>= 1) v += __shfl_xor(v, m, G);
    return v;
}

template <int G>
__device__ __forceinline__ float group_max(float v) {
#pragma unroll
    for (int m = G >> 1; m > 0; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, G));
    return v;
}

// The row of sample b in field fd (-1: an id out of range, flagged once per group by its lane 0).
__device__ __forceinline__ int64_t row_of(const dctr_mlr_field_t& fd, int64_t b, int c, int32_t* status) {
    int64_t r = b;
    if (!fd.identity)
        r = fd.ids_is_i64 ? ((const int64_t*)fd.ids)[b * fd.ids_stride] : (int64_t)((const int32_t*)fd.ids)[b * fd.ids_stride];
    if (r < 0 || r >= fd.vocab) {
        if (status && c == 0) atomicOr(status, DCTR_STATUS_INDEX_OOR);
        r = -1;
    }
    return r;
}

// From lane c's z[c] (any value in the lanes c >= K) to the mixture.  Every lane of the group gets u = sum_r s[r] a[r] and g (the
// bias sigmoid, 1 without a bias part) and gc = 1 - g; lane c < R gets s = s[c] and a_of = a[c] (its learner's), lane R + r gets
// s = s[r], a_of = a[r] and ac = 1 - a[r] (sigmoid learners).  LINEAR: the learners' activation is the identity.
template <int G>
__device__ __forceinline__ void mixture(float z, int c, int R, bool has_bias, bool linear, float& s, float& a_of, float& ac, float& u,
                                        float& g, float& gc) {
    const bool region = c < R, learner = c >= R && c < 2 * R;
    const float m = group_max<G>(region ? z : -INFINITY);
    const float e = region ? expf(z - m) : 0.f;
    const float inv = 1.f / group_sum<G>(e);
    const float sr = e * inv;                                   // s[c] in the region lanes
    float sg, sgc;
    dctr_act::sigmoid_pair(z, sg, sgc);                         // (lanes that do not need it compute it anyway: no divergence)
    const float a = linear ? z : sg;                            // a[c - R] in the learner lanes
    // region lane c <-> learner lane c + R exchange s and a: lane c reads from c ^ ... is not a fixed xor, so two indexed moves
    const float s_from = __shfl(sr, learner ? c - R : c, G);
    const float a_from = __shfl(a, region ? c + R : c, G);
    s = region ? sr : s_from;
    a_of = region ? a_from : a;
    ac = linear ? 1.f : sgc;
    u = group_sum<G>(learner ? s * a_of : 0.f);
    g = 1.f;
    gc = 0.f;
    if (has_bias) {
        g = __shfl(sg, 2 * R, G);
        gc = __shfl(sgc, 2 * R, G);
    }
}

}  // namespace dctr_mlr
