// What EDCN's forward (edcn_kernels.hip) and backward (edcn_bwd_kernels.hip) share: the workgroup shape, the wave reductions, the
// field softmax of a RegulationModule, the fused activations, and the host-side size checks and LDS plan of the fused route.
#pragma once
#include <math.h>
#include "dctr_common.h"
#include "tile_route.h"

namespace {

constexpr int ED_THREADS = 512;
constexpr int ED_WAVES = ED_THREADS / 64;
constexpr int ED_MAX_ROUNDS = 32;                 // rounds per launch (kernel-argument space)
constexpr size_t ED_LDS_TARGET = 80 * 1024;       // two workgroups per CU where the rows allow it

__device__ __forceinline__ float ed_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ float ed_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// softmax over the F values g * inv_tau by one wave -> G[F]
__device__ __forceinline__ void ed_gate(const float* __restrict__ g, int F, float inv_tau, float* G, int lane) {
    float m = -INFINITY;
    for (int f = lane; f < F; f += 64) m = fmaxf(m, g[f] * inv_tau);
    m = ed_wave_max(m);
    float s = 0.f;
    for (int f = lane; f < F; f += 64) {
        const float e = expf(g[f] * inv_tau - m);
        G[f] = e;
        s += e;
    }
    s = ed_wave_sum(s);
    for (int f = lane; f < F; f += 64) G[f] = G[f] / s;
}

__device__ __forceinline__ float ed_act(float v, int act) { return act == DCTR_ACT_RELU ? fmaxf(v, 0.f) : v; }

struct EdPlan {
    bool fused;
    int R, ld, tpw;
    size_t lds;
    int launches;
    size_t ws_bytes;
};

inline bool ed_fused_act(int act) { return act == DCTR_ACT_LINEAR || act == DCTR_ACT_RELU; }

inline int ed_ld(int D) { return ((D + 15) & ~15) + 4; }

inline int ed_tpw(int D) { return D % 64 == 0 ? 4 : D % 32 == 0 ? 2 : 1; }

inline int edcn_check(const dctr_edcn_args_t* a) {
    DCTR_REQUIRE(a, DCTR_E_NULL, "edcn_fwd: null args");
    DCTR_REQUIRE(a->batch >= 0 && a->fields >= 1 && a->dim >= 1 && a->cross_num >= 1, DCTR_E_DIM,
                 "edcn_fwd: batch = %lld, fields = %d, dim = %d, cross_num = %d", (long long)a->batch, a->fields, a->dim, a->cross_num);
    const int64_t D = (int64_t)a->fields * a->dim;
    DCTR_REQUIRE(D <= (1 << 24), DCTR_E_DIM, "edcn_fwd: fields * dim = %lld exceeds 2^24", (long long)D);
    DCTR_REQUIRE(a->x_offset >= 0 && a->x_stride >= 0 && a->x_offset + D <= a->x_stride, DCTR_E_DIM,
                 "edcn_fwd: columns [%lld, %lld) in rows of %lld", (long long)a->x_offset, (long long)(a->x_offset + D), (long long)a->x_stride);
    DCTR_REQUIRE(a->mode == DCTR_CROSS_VECTOR || a->mode == DCTR_CROSS_MATRIX, DCTR_E_ENUM, "edcn_fwd: unknown parameterization %d", a->mode);
    DCTR_REQUIRE(a->bridge >= DCTR_EDCN_BRIDGE_ADD && a->bridge <= DCTR_EDCN_BRIDGE_ATTENTION, DCTR_E_ENUM, "edcn_fwd: unknown bridge %d",
                 a->bridge);
    DCTR_REQUIRE(a->activation >= DCTR_ACT_LINEAR && a->activation <= DCTR_ACT_DICE && a->bridge_activation >= DCTR_ACT_LINEAR &&
                     a->bridge_activation <= DCTR_ACT_DICE, DCTR_E_ENUM, "edcn_fwd: unknown activation %d / %d", a->activation,
                 a->bridge_activation);
    DCTR_REQUIRE(a->route >= DCTR_EDCN_ROUTE_AUTO && a->route <= DCTR_EDCN_ROUTE_LAYERED, DCTR_E_ENUM, "edcn_fwd: unknown route %d", a->route);
    DCTR_REQUIRE(a->sigmoid_out == 0 || a->sigmoid_out == 1, DCTR_E_ENUM, "edcn_fwd: sigmoid_out = %d", a->sigmoid_out);
    DCTR_REQUIRE(a->inv_tau == a->inv_tau && a->inv_tau - a->inv_tau == 0.f, DCTR_E_DIM, "edcn_fwd: 1 / tau is not finite");
    return DCTR_OK;
}

inline void edcn_plan(const dctr_edcn_args_t* a, EdPlan* pl) {
    const int D = a->fields * a->dim;
    pl->ld = ed_ld(D);
    pl->tpw = ed_tpw(D);
    pl->fused = false;
    pl->R = 16;
    pl->lds = 0;
    pl->launches = (a->cross_num + ED_MAX_ROUNDS - 1) / ED_MAX_ROUNDS;
    pl->ws_bytes = 0;
    if (a->route == DCTR_EDCN_ROUTE_LAYERED || a->bridge == DCTR_EDCN_BRIDGE_ATTENTION || !ed_fused_act(a->activation) ||
        (a->bridge == DCTR_EDCN_BRIDGE_CONCAT && !ed_fused_act(a->bridge_activation)))
        return;
    const size_t gates = 2 * (size_t)a->fields;
    for (int R = 64; R >= 16; R >>= 1) {
        const size_t need = (4 * (size_t)R * pl->ld + gates) * sizeof(float);
        if (need <= (R == 16 ? DCTR_LDS_MAX : ED_LDS_TARGET)) {
            pl->fused = true;
            pl->R = R;
            pl->lds = need;
            break;
        }
    }
    if (pl->fused && pl->launches > 1) pl->ws_bytes = (size_t)(a->batch > 0 ? a->batch : 0) * D * sizeof(float);
}

}  // namespace
