// MLR's forward (include/dctr.h: dctr_mlr_fwd), one launch from the ids to the prediction: K = 2R (+1) linear logits per sample gathered
// from fused rows (a feature's K one-wide tables side by side: one 32-48-byte row per id in place of K scattered dwords), the dense
// part, softmax over the regions, the learners' sigmoids, the mixture and the bias factor.
//
// A latency-bound gather with a few flops behind it, so the shape is the lane group of mlr_device.h: lane c of a sample's G lanes owns
// column c.  A (sample, field) row is one contiguous request of <= G dwords; the groups of a wave read the ids of consecutive samples,
// one contiguous run of the [F, B] id matrix per field; the rows of FIELDS_IN_FLIGHT fields are requested before the first is added.
// Everything after the gather is cross-lane moves inside the group: no LDS, no barrier.  z is summed in field order, then the dense
// columns in column order: one fixed order, the same bits on every call.
#include "mlr_device.h"

namespace {

using namespace dctr_mlr;

constexpr int FIELDS_IN_FLIGHT = 4;

template <int G>
__global__ void __launch_bounds__(THREADS) mlr_fwd_kernel(dctr_mlr_args_t p, int K) {
    const int c = threadIdx.x & (G - 1);
    const int64_t b = (int64_t)blockIdx.x * (THREADS / G) + (threadIdx.x / G);
    if (b >= p.batch) return;           // (whole groups leave: the cross-lane moves below stay inside a group)
    const int R = p.region_num;
    float z = 0.f;
    for (int f0 = 0; f0 < p.n_fields; f0 += FIELDS_IN_FLIGHT) {
        const float* src[FIELDS_IN_FLIGHT];
#pragma unroll
        for (int u = 0; u < FIELDS_IN_FLIGHT; ++u) {
            src[u] = nullptr;
            if (f0 + u < p.n_fields) {
                const dctr_mlr_field_t fd = p.fields[f0 + u];
                const int64_t r = row_of(fd, b, c, p.status);
                const int k = c - fd.col0;
                if (r >= 0 && k >= 0 && k < fd.width) src[u] = fd.rows + r * fd.row_pitch + k;
            }
        }
        float v[FIELDS_IN_FLIGHT];
#pragma unroll
        for (int u = 0; u < FIELDS_IN_FLIGHT; ++u) v[u] = src[u] ? *src[u] : 0.f;
#pragma unroll
        for (int u = 0; u < FIELDS_IN_FLIGHT; ++u) z += v[u];
    }
    if (c < K) {
        const float* x = p.dense + b * p.dense_stride;
        for (int k = 0; k < p.n_dense; ++k) z = fmaf(x[k], p.dense_w[(int64_t)k * K + c], z);
    } else {
        z = 0.f;
    }
    if (p.z && c < K) p.z[b * p.z_stride + p.z_offset + c] = z;
    float s, a, ac, u, g, gc;
    mixture<G>(z, c, R, p.has_bias != 0, p.learner_act == DCTR_MLR_LEARNER_LINEAR, s, a, ac, u, g, gc);
    if (c == 0) p.out[b * p.out_stride] = u * g;
}

}  // namespace

extern "C" int dctr_mlr_supported(const dctr_mlr_args_t* a) {
    return a && a->region_num >= 2 && (a->has_bias == 0 || a->has_bias == 1) && a->region_num <= (DCTR_MLR_MAX_COLUMNS - a->has_bias) / 2;
}

extern "C" int dctr_mlr_fwd(const dctr_mlr_args_t* a, void* stream) {
    DCTR_REQUIRE(a, DCTR_E_NULL, "mlr_fwd: null args");
    int rc = check(a, "mlr_fwd");
    if (rc != DCTR_OK) return rc;
    const int K = columns(a);
    DCTR_REQUIRE(a->out, DCTR_E_NULL, "mlr_fwd: null out");
    DCTR_REQUIRE(a->n_dense == 0 || (a->dense && a->dense_w), DCTR_E_NULL, "mlr_fwd: n_dense = %d without dense / dense_w", a->n_dense);
    DCTR_REQUIRE(a->out_stride >= 1, DCTR_E_DIM, "mlr_fwd: out_stride %lld", (long long)a->out_stride);
    DCTR_REQUIRE(a->n_dense == 0 || a->dense_stride >= a->n_dense, DCTR_E_DIM, "mlr_fwd: dense_stride %lld < n_dense %d",
                 (long long)a->dense_stride, a->n_dense);
    DCTR_REQUIRE(!a->z || a->z_stride >= a->z_offset + K, DCTR_E_DIM, "mlr_fwd: z_stride %lld < z_offset + K = %lld",
                 (long long)a->z_stride, (long long)(a->z_offset + K));
    if (a->batch == 0) return DCTR_OK;
    const int G = group_lanes(K);
    const dim3 grid((unsigned)dctr_ceil_div(a->batch, (int64_t)(THREADS / G))), block(THREADS);
    const hipStream_t st = (hipStream_t)stream;
    switch (G) {
        case 8: DCTR_LAUNCH((mlr_fwd_kernel<8>), grid, block, 0, st, *a, K); break;
        case 16: DCTR_LAUNCH((mlr_fwd_kernel<16>), grid, block, 0, st, *a, K); break;
        case 32: DCTR_LAUNCH((mlr_fwd_kernel<32>), grid, block, 0, st, *a, K); break;
        default: DCTR_LAUNCH((mlr_fwd_kernel<64>), grid, block, 0, st, *a, K); break;
    }
    return dctr_launch_status("dctr_mlr_fwd");
}
