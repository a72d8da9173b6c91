// MLR's backward (include/dctr.h: dctr_mlr_bwd), one launch from the forward's saved z and d_out to dz [B, K] and the gradients of the
// fused rows.  The lane group of the forward (mlr_device.h): lane c of a sample's G lanes owns column c, rebuilds s, a, u and g from z
// with the forward's own arithmetic and forms dz[c]; then, per field, the lanes inside the field's column range add their dz into the
// gradient row of the sample's id — one contiguous run of `width` dwords per (sample, field), unsafeAtomicAdd — or, for a pre-pooled
// field, store it into row b of its buffer.  One route, no workspace, no LDS.  Ids that repeat are not merged before the atomics.
#include "mlr_device.h"

namespace {

using namespace dctr_mlr;

template <int G>
__global__ void __launch_bounds__(THREADS) mlr_bwd_kernel(dctr_mlr_bwd_args_t q, int K) {
    const dctr_mlr_args_t& p = q.fwd;
    const int c = threadIdx.x & (G - 1);
    const int64_t b = (int64_t)blockIdx.x * (THREADS / G) + (threadIdx.x / G);
    if (b >= p.batch) return;
    const int R = p.region_num;
    const bool linear = p.learner_act == DCTR_MLR_LEARNER_LINEAR;
    const float z = c < K ? p.z[b * p.z_stride + p.z_offset + c] : 0.f;
    const float d = q.d_out[b * q.d_out_stride];
    float s, a, ac, u, g, gc;
    mixture<G>(z, c, R, p.has_bias != 0, linear, s, a, ac, u, g, gc);
    float dz;
    if (c < R)
        dz = d * g * s * (a - u);
    else if (c < 2 * R)
        dz = linear ? d * g * s : d * g * s * a * ac;
    else
        dz = d * u * g * gc;
    if (c < K) q.dz[b * q.dz_stride + c] = dz;
    if (!q.grads) return;
    for (int f = 0; f < p.n_fields; ++f) {
        const dctr_mlr_grad_t gd = q.grads[f];
        const dctr_mlr_field_t fd = p.fields[f];
        const int64_t r = row_of(fd, b, c, p.status);       // (a frozen field's id is still checked: the status is the forward's)
        const int k = c - fd.col0;
        if (!gd.grad || r < 0 || k < 0 || k >= fd.width) continue;
        float* dst = gd.grad + r * gd.row_stride + k;
        if (fd.identity)
            *dst = dz;
        else
            unsafeAtomicAdd(dst, dz);
    }
}

}  // namespace

extern "C" int dctr_mlr_bwd(const dctr_mlr_bwd_args_t* a, void* stream) {
    DCTR_REQUIRE(a, DCTR_E_NULL, "mlr_bwd: null args");
    const dctr_mlr_args_t* w = &a->fwd;
    int rc = check(w, "mlr_bwd");
    if (rc != DCTR_OK) return rc;
    const int K = columns(w);
    DCTR_REQUIRE(w->z && a->d_out && a->dz, DCTR_E_NULL, "mlr_bwd: null z / d_out / dz");
    DCTR_REQUIRE((((uintptr_t)a->grads) & 7u) == 0, DCTR_E_ALIGN, "mlr_bwd: grads not 8-byte aligned");
    DCTR_REQUIRE(w->z_stride >= w->z_offset + K, DCTR_E_DIM, "mlr_bwd: z_stride %lld < z_offset + K = %lld", (long long)w->z_stride,
                 (long long)(w->z_offset + K));
    DCTR_REQUIRE(a->d_out_stride >= 1 && a->dz_stride >= K, DCTR_E_DIM, "mlr_bwd: d_out_stride %lld, dz_stride %lld (K = %d)",
                 (long long)a->d_out_stride, (long long)a->dz_stride, K);
    if (w->batch == 0) return DCTR_OK;
    const int G = group_lanes(K);
    const dim3 grid((unsigned)dctr_ceil_div(w->batch, (int64_t)(THREADS / G))), block(THREADS);
    const hipStream_t st = (hipStream_t)stream;
    switch (G) {
        case 8: DCTR_LAUNCH((mlr_bwd_kernel<8>), grid, block, 0, st, *a, K); break;
        case 16: DCTR_LAUNCH((mlr_bwd_kernel<16>), grid, block, 0, st, *a, K); break;
        case 32: DCTR_LAUNCH((mlr_bwd_kernel<32>), grid, block, 0, st, *a, K); break;
        default: DCTR_LAUNCH((mlr_bwd_kernel<64>), grid, block, 0, st, *a, K); break;
    }
    return dctr_launch_status("dctr_mlr_bwd");
}
