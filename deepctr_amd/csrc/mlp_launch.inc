// One instantiation of dctr_mlp::mlp_kernel<DCTR_MLP_RT> and its launcher (the kernel symbol must live in the
// translation unit that launches it).  Included by mlp_kernels_rt{1,2,4}.hip.
#include "mlp_device.h"

#define DCTR_CAT_(a, b) a##b
#define DCTR_CAT(a, b) DCTR_CAT_(a, b)

namespace dctr_mlp {

int DCTR_CAT(launch_rt, DCTR_MLP_RT)(const MlpParams& p, const FusedGather& fg, unsigned blocks, size_t lds,
                                     hipStream_t stream) {
    // DCTR_ACT_ELU .. DCTR_ACT_GELU: the instantiation whose epilogue switches on the code (mlp_device.h: DCTR_BY_ACT)
    const bool ext = dctr_act::is_extended(p.activation);
    const void* fn = ext ? (const void*)mlp_kernel<DCTR_MLP_RT, true> : (const void*)mlp_kernel<DCTR_MLP_RT>;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        DCTR_REQUIRE(e == hipSuccess, (int)e, "mlp_fwd: cannot raise dynamic LDS to %zu B: %s", lds, hipGetErrorString(e));
    }
    if (ext) DCTR_LAUNCH((mlp_kernel<DCTR_MLP_RT, true>), dim3(blocks), dim3(NTHR), lds, stream, p, fg);
    else DCTR_LAUNCH(mlp_kernel<DCTR_MLP_RT>, dim3(blocks), dim3(NTHR), lds, stream, p, fg);
    return dctr_launch_status("dctr_mlp_fwd");
}

}  // namespace dctr_mlp
