// Declarations the CIN units share (cin_kernels.hip, cin_layered_kernels.hip, cin_bwd_kernels.hip); none of them is part of the ABI.
#pragma once
#include "dctr_common.h"

namespace dctr_cinbwd {      // cin_bwd_kernels.hip: the z-free backward of one CIN layer (filter gradient; input gradients)
bool fused_shape_ok(int F0, int Fk, int H);
int64_t dw_parts_floats(int F0, int Fk, int H, int64_t rows);
int launch_dw_fused(const float* dpre, const float* x0t, const float* xk, int64_t ldk, int F0, int Fk, int H, int64_t rows,
                    float* parts, int* n_parts, hipStream_t st);
int launch_dz_fused(const float* dpre, const float* W, const float* x0t, const float* xk, int64_t ldk, int F0, int Fk, int H,
                    int64_t rows, float* dx0t, float* dxk, hipStream_t st);
}  // namespace dctr_cinbwd

// cin_layered_kernels.hip: CIN layer by layer on the library's GEMM (z materialised per chunk of samples) — any layer sizes
size_t dctr_cin_layered_sample_floats(const dctr_cin_args_t* a);
int dctr_cin_fwd_layered(const dctr_cin_args_t* a, void* workspace, size_t workspace_bytes, void* stream);
