// The loss of the HIP training step.
//   dctr_bce_grad, dctr_bce_grad_w   loss + d(loss)/d(logit) of PredictionLayer('binary') + binary_crossentropy / of mse
// The reference has no code of its own for this (Keras autodiff of the compiled loss): the formulas are the derivatives of
// PredictionLayer.call (layers/core.py:250-259) under tf.keras' binary_crossentropy / mse with reduction SUM_OVER_BATCH_SIZE.
#include "dctr_common.h"

namespace {

// ---------------------------------------------------------------------------------------------------
// loss
// ---------------------------------------------------------------------------------------------------
// weight (optional): tf.keras' sample_weight — loss = sum_b w_b l_b / B (reduction SUM_OVER_BATCH_SIZE), so l_b and d l_b scale by w_b
__global__ __launch_bounds__(256) void bce_grad_kernel(const float* __restrict__ pred, const float* __restrict__ y,
                                                       const float* __restrict__ weight, int64_t batch, int task,
                                                       float* __restrict__ dlogit,
                                                       float* __restrict__ loss_sum, float* __restrict__ dlogit_sum) {
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    float l = 0.f, ds = 0.f;
    if (b < batch) {
        const float p = pred[b], t = y[b];
        if (task == 0) {
            // d/dlogit of mean BCE(sigmoid(logit), y) = (p - y) / B; value with Keras' epsilon clip (backend.epsilon = 1e-7)
            const float pc = fminf(fmaxf(p, 1e-7f), 1.f - 1e-7f);
            l = -(t * logf(pc) + (1.f - t) * logf(1.f - pc));
            ds = (p - t) / (float)batch;
        } else {
            l = (p - t) * (p - t);
            ds = 2.f * (p - t) / (float)batch;
        }
        if (weight != nullptr) {
            const float w = weight[b];
            l *= w;
            ds *= w;
        }
        dlogit[b] = ds;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        l += __shfl_xor(l, m, 64);
        ds += __shfl_xor(ds, m, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (loss_sum != nullptr) unsafeAtomicAdd(loss_sum, l);
        if (dlogit_sum != nullptr) unsafeAtomicAdd(dlogit_sum, ds);     // gradient of PredictionLayer's global_bias
    }
}

}  // namespace

extern "C" int dctr_bce_grad_w(const float* pred, const float* y, const float* weight, int64_t batch, int32_t task, float* dlogit,
                               float* loss_sum, float* dlogit_sum, void* stream) {
    DCTR_REQUIRE(batch >= 0 && (task == 0 || task == 1), DCTR_E_DIM, "bce_grad: bad batch / task");
    if (batch == 0) return DCTR_OK;
    DCTR_REQUIRE(pred && y && dlogit, DCTR_E_NULL, "bce_grad: null pointer");
    hipLaunchKernelGGL(bce_grad_kernel, dim3((unsigned)dctr_ceil_div(batch, (int64_t)256)), dim3(256), 0, (hipStream_t)stream, pred,
                       y, weight, batch, (int)task, dlogit, loss_sum, dlogit_sum);
    return dctr_launch_status("dctr_bce_grad");
}

extern "C" int dctr_bce_grad(const float* pred, const float* y, int64_t batch, int32_t task, float* dlogit, float* loss_sum,
                             float* dlogit_sum, void* stream) {
    return dctr_bce_grad_w(pred, y, nullptr, batch, task, dlogit, loss_sum, dlogit_sum, stream);
}
