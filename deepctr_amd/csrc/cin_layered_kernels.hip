// CIN (layers/interaction.py:277-325) layer by layer on dctr_gemm (gemm_kernels.hip); each section's banner has the formulas.
//   dctr_cin_fwd_layered, dctr_cin_layered_sample_floats   a FORWARD route of dctr_cin_fwd (cin_kernels.hip); cin_internal.h
//   dctr_cin_bwd, dctr_cin_bwd_workspace_bytes             the backward, with the z-free kernels of cin_bwd_kernels.hip
#include "dctr_gemm.h"

#include "cin_internal.h"
#include "train_common.h"

namespace {

// ---------------------------------------------------------------------------------------------------
// CIN backward (interaction.py:277-325), first version: the reference's own formulation — z materialised per layer,
// 1x1 conv = GEMM — in the (b,d)-major row layout R = B*D:  X0t [R,F0],  X_k = Y_{k-1}[:, :Hn] [R,F_k],
//   z_k[r, i*F_k+j] = X0t[r,i] X_k[r,j];   Y_k = act(z_k W_k + b_k) [R,H_k];   out[b, .] = sum_d of the direct maps.
// The GEMMs (forward recompute, dW = z^T dpre, dz = dpre W^T) are dctr_gemm; the rest are the kernels below.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cin_to_rows_kernel(const float* __restrict__ x, int64_t x_stride, int64_t batch, int F0,
                                                          int D, float* __restrict__ xt) {
    const int64_t total = batch * D * F0;
    for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (int64_t)gridDim.x * 256) {
        const int i = (int)(o % F0);
        const int64_t r = o / F0;
        const int64_t b = r / D;
        const int d = (int)(r - b * D);
        xt[o] = x[b * x_stride + (int64_t)i * D + d];
    }
}

__global__ __launch_bounds__(256) void cin_from_rows_kernel(const float* __restrict__ dxt, int64_t batch, int F0, int D,
                                                            float* __restrict__ dx, int64_t dx_stride, int accumulate) {
    const int64_t total = batch * F0 * D;
    for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (int64_t)gridDim.x * 256) {
        const int d = (int)(o % D);
        const int64_t t = o / D;
        const int i = (int)(t % F0);
        const int64_t b = t / F0;
        float* dst = dx + b * dx_stride + (int64_t)i * D + d;
        *dst = (accumulate ? *dst : 0.f) + dxt[(b * D + d) * F0 + i];
    }
}

__global__ __launch_bounds__(256) void cin_outer_kernel(const float* __restrict__ x0t, int F0, const float* __restrict__ xk,
                                                        int64_t ldk, int Fk, int64_t rows, float* __restrict__ z) {
    const int K = F0 * Fk;
    const int64_t total = rows * K;
    for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (int64_t)gridDim.x * 256) {
        const int64_t r = o / K;
        const int c = (int)(o - r * K);
        const int i = c / Fk, j = c - i * Fk;
        z[o] = x0t[r * F0 + i] * xk[r * ldk + j];
    }
}

// the same with 16-B stores: thread = four consecutive j of one (row, i)   (Fk % 4 == 0, ldk % 4 == 0, 16-B aligned xk / z)
__global__ __launch_bounds__(256) void cin_outer4_kernel(const float* __restrict__ x0t, int F0, const float* __restrict__ xk,
                                                         int64_t ldk, int Fk, int64_t rows, float* __restrict__ z) {
    const int Fk4 = Fk >> 2, K4 = F0 * Fk4;
    const int64_t total = rows * K4;
    for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (int64_t)gridDim.x * 256) {
        const int64_t r = o / K4;
        const int c = (int)(o - r * K4);
        const int i = c / Fk4, j4 = c - i * Fk4;
        const float a = x0t[r * F0 + i];
        const float4 b = *reinterpret_cast<const float4*>(xk + r * ldk + 4 * j4);
        *reinterpret_cast<float4*>(z + r * (int64_t)(F0 * Fk) + i * Fk + 4 * j4) = make_float4(a * b.x, a * b.y, a * b.z, a * b.w);
    }
}

// dpre[r,h] = (hidden part: dxnext[r,h] for h < Hn) + (direct part: d_out[b, off + h - d0] for h >= d0), times act'(Y)
__global__ __launch_bounds__(256) void cin_dpre_kernel(const float* __restrict__ y, const float* __restrict__ dxnext, int64_t ldn,
                                                       int Hn, const float* __restrict__ d_out, int64_t out_dim, int off, int d0,
                                                       int64_t rows, int H, int D, int act, float* __restrict__ dpre) {
    const int64_t total = rows * H;
    for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (int64_t)gridDim.x * 256) {
        const int64_t r = o / H;
        const int h = (int)(o - r * H);
        float g = 0.f;
        if (dxnext != nullptr && h < Hn) g += dxnext[r * ldn + h];
        if (h >= d0) g += d_out[(r / D) * out_dim + off + (h - d0)];
        const float v = y[o];
        if (act == DCTR_ACT_RELU) g = v > 0.f ? g : 0.f;
        else if (act == DCTR_ACT_SIGMOID) g *= v * (1.f - v);
        else if (act == DCTR_ACT_TANH) g *= 1.f - v * v;
        dpre[o] = g;
    }
}

// from dz [R, F0*Fk]:  dX0t[r,i] += sum_j dz[r, i*Fk+j] Xk[r,j];   dXk[r,j] = sum_i dz[r, i*Fk+j] X0t[r,i]
// One wave per row: the row of dz (F0*Fk floats) is staged once in LDS (coalesced) and both sums read it from there,
// so dz crosses HBM once (two independent thread-per-output passes read it twice: 860 us per step at C3).
__global__ __launch_bounds__(256) void cin_outer_bwd_kernel(const float* __restrict__ dz, const float* __restrict__ x0t, int F0,
                                                            const float* __restrict__ xk, int64_t ldk, int Fk, int64_t rows,
                                                            float* __restrict__ dx0t, float* __restrict__ dxk) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int K = F0 * Fk;
    float* zr = smem + (size_t)wave * (K + F0 + Fk);        // [K] dz row, [F0] x0t row, [Fk] xk row
    float* x0r = zr + K;
    float* xkr = x0r + F0;
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < rows; r += (int64_t)gridDim.x * 4) {
        const float* dzr = dz + r * K;
        for (int c = lane; c < K; c += 64) zr[c] = dzr[c];
        for (int i = lane; i < F0; i += 64) x0r[i] = x0t[r * F0 + i];
        for (int j = lane; j < Fk; j += 64) xkr[j] = xk[r * ldk + j];
        // (same wave: LDS operations complete in order)
        for (int i = lane; i < F0; i += 64) {
            float acc = 0.f;
            for (int j = 0; j < Fk; ++j) acc = fmaf(zr[i * Fk + j], xkr[j], acc);
            dx0t[r * F0 + i] += acc;
        }
        if (dxk != nullptr) {
            for (int j = lane; j < Fk; j += 64) {
                float acc = 0.f;
                for (int i = 0; i < F0; ++i) acc = fmaf(zr[i * Fk + j], x0r[i], acc);
                dxk[r * Fk + j] = acc;
            }
        }
    }
}

}  // namespace

// ---------------------------------------------------------------------------------------------------
// CIN.call, layer by layer (interaction.py:277-325 as the reference writes it: z materialised per layer, 1x1 conv = GEMM) — the route of
// dctr_cin_fwd for layer sizes no LDS tile of the one-kernel form holds (a layer of more than ~480 maps: cin_kernels.hip refuses it for
// every tile height).  Rows r = (b, d); samples in chunks of what the workspace holds; per chunk and layer: z = x_0 (outer) x_k
// (cin_outer_kernel), y = z W_k on dctr_gemm, bias + activation in place, the direct maps summed over d into `out`; y goes straight to
// save_y[k] when the caller asked for the activations (the same [B * D, H_k] rows).  Not part of the ABI: called by cin_kernels.hip.
// ---------------------------------------------------------------------------------------------------
namespace {
__global__ __launch_bounds__(256) void cin_bias_act_kernel(float* __restrict__ y, int64_t rows, int H, const float* __restrict__ bias, int act) {
    const int64_t total = rows * H;
    for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (int64_t)gridDim.x * 256)
        y[o] = act_value(y[o] + bias[(int)(o % H)], act);
}
// out[b, off + j] = sum_d y[(b D + d), d0 + j]   (j < nd): deterministic serial sum over d, as the one-kernel form's LDS sum
__global__ __launch_bounds__(256) void cin_sum_d_kernel(const float* __restrict__ y, int H, int64_t batch, int D, int d0, int nd,
                                                        float* __restrict__ out, int64_t out_dim, int off) {
    const int64_t total = batch * nd;
    for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (int64_t)gridDim.x * 256) {
        const int64_t b = o / nd;
        const int j = (int)(o - b * nd);
        const float* yp = y + (b * D) * H + d0 + j;
        float acc = 0.f;
        for (int d = 0; d < D; ++d) acc += yp[(int64_t)d * H];
        out[b * out_dim + off + j] = acc;
    }
}
}  // namespace

// floats of workspace per SAMPLE of the layered route: x0t [D, F0] + z [D, max F0 F_k] + two y buffers [D, max H]
size_t dctr_cin_layered_sample_floats(const dctr_cin_args_t* a) {
    size_t kmax = 0, hmax = 0;
    int fk = a->fields;
    for (int k = 0; k < a->n_layers; ++k) {
        const int H = a->layer_size[k];
        const bool last = k == a->n_layers - 1;
        kmax = (size_t)a->fields * fk > kmax ? (size_t)a->fields * fk : kmax;
        hmax = (size_t)H > hmax ? (size_t)H : hmax;
        fk = last ? 0 : (a->split_half ? H / 2 : H);
    }
    return (size_t)a->dim * ((((size_t)a->fields + 3) & ~(size_t)3) + ((kmax + 3) & ~(size_t)3) + 2 * ((hmax + 3) & ~(size_t)3));
}

int dctr_cin_fwd_layered(const dctr_cin_args_t* a, void* workspace, size_t workspace_bytes, void* stream) {
    const int F0 = a->fields, D = a->dim, L = a->n_layers;
    const size_t per = dctr_cin_layered_sample_floats(a) * sizeof(float);
    DCTR_REQUIRE(workspace != nullptr && dctr_aligned16(workspace) && workspace_bytes >= 16 * per, DCTR_E_NULL,
                 "cin_fwd: these layer sizes run layer by layer and need a 16-B aligned workspace (dctr_cin_workspace_bytes; at least %zu B)", 16 * per);
    DCTR_REQUIRE(a->x != nullptr && a->out != nullptr && a->filters != nullptr && a->bias != nullptr, DCTR_E_NULL, "cin_fwd: null pointer");
    int64_t cap = (int64_t)(workspace_bytes / per);
    cap = cap > 65536 ? 65536 : cap & ~(int64_t)3;
    size_t kmax = 0, hmax = 0;
    int out_dim = 0;
    {
        int fk = F0;
        for (int k = 0; k < L; ++k) {
            const int H = a->layer_size[k];
            const bool last = k == L - 1;
            DCTR_REQUIRE(a->filters[k] && a->bias[k], DCTR_E_NULL, "cin_fwd: filters/bias[%d] null", k);
            kmax = (size_t)F0 * fk > kmax ? (size_t)F0 * fk : kmax;
            hmax = (size_t)H > hmax ? (size_t)H : hmax;
            out_dim += a->split_half ? (last ? H : H - H / 2) : H;
            fk = last ? 0 : (a->split_half ? H / 2 : H);
        }
    }
    // (the GEMM's sizes and element offsets are ints: a chunk's z stays below 2^31 elements)
    while (cap > 16 && (int64_t)cap * D * (int64_t)(kmax > hmax ? kmax : hmax) >= 0x7fffffffLL) cap = (cap >> 1) & ~(int64_t)3;
    DCTR_REQUIRE((int64_t)cap * D * (int64_t)(kmax > hmax ? kmax : hmax) < 0x7fffffffLL, DCTR_E_DIM, "cin_fwd: layer too large (%zu products per row)", kmax);
    float* ws = static_cast<float*>(workspace);
    const size_t f0p = ((size_t)F0 + 3) & ~(size_t)3, kp = (kmax + 3) & ~(size_t)3, hp = (hmax + 3) & ~(size_t)3;
    float* x0t = ws;
    float* z = x0t + (size_t)cap * D * f0p;
    float* ybuf[2] = {z + (size_t)cap * D * kp, z + (size_t)cap * D * kp + (size_t)cap * D * hp};
    hipStream_t st = (hipStream_t)stream;
    auto grid = [](int64_t n) { int64_t b = dctr_ceil_div(n, (int64_t)256); return dim3((unsigned)(b > 16384 ? 16384 : (b < 1 ? 1 : b))); };
    for (int64_t r0 = 0; r0 < a->batch; r0 += cap) {
        const int64_t nb = a->batch - r0 < cap ? a->batch - r0 : cap;
        const int64_t R = nb * D;
        hipLaunchKernelGGL(cin_to_rows_kernel, grid(R * F0), dim3(256), 0, st, a->x + r0 * a->x_stride, a->x_stride, nb, F0, D, x0t);
        const float* xk = x0t;
        int64_t ldk = F0;
        int fk = F0, off = 0;
        for (int k = 0; k < L; ++k) {
            const int H = a->layer_size[k];
            const bool last = k == L - 1;
            const int Hn = last ? 0 : (a->split_half ? H / 2 : H), d0 = a->split_half ? (last ? 0 : H / 2) : 0;
            const int K = F0 * fk;
            hipLaunchKernelGGL(cin_outer_kernel, grid(R * K), dim3(256), 0, st, (const float*)x0t, F0, xk, ldk, fk, R, z);
            float* y = (a->save_y != nullptr && a->save_y[k] != nullptr) ? a->save_y[k] + (size_t)r0 * D * H : ybuf[k & 1];
            // row-major y [R, H] = z [R, K] W [K, H]  <=>  column-major y' (H x R) = W' (H x K) z' (K x R)
            const int rs = dctr_gemm::sgemm(st, dctr_gemm::OP_N, dctr_gemm::OP_N, H, (int)R, K, a->filters[k], H, z, K, 0.f, y, H);
            DCTR_REQUIRE(rs == 0, DCTR_E_UNSUPPORTED, "cin_fwd: sgemm(layer %d) failed (%d)", k, rs);
            hipLaunchKernelGGL(cin_bias_act_kernel, grid(R * H), dim3(256), 0, st, y, R, H, a->bias[k], (int)a->activation);
            hipLaunchKernelGGL(cin_sum_d_kernel, grid(nb * (H - d0)), dim3(256), 0, st, (const float*)y, H, nb, D, d0, H - d0, a->out + r0 * out_dim,
                               (int64_t)out_dim, off);
            off += H - d0;
            xk = y;
            ldk = H;
            fk = Hn;
        }
    }
    return dctr_launch_status("dctr_cin_fwd");
}

namespace {
struct CinPlan {
    int L, F0, D;
    int H[8], Fk[8], Hn[8], d0[8], off[8];
    bool fused[8];         // layer runs on the z-free kernels of cin_bwd_kernels.hip: no z / dz for it
    int64_t R;
    size_t x0t, y[8], z[8], dpre, dz, dx0t, dxk[2], fwd_out, fwd_ws, fwd_ws_bytes, parts, total;
    int out_dim;
};
bool cin_plan(const dctr_cin_args_t* f, CinPlan& p) {
    p.L = f->n_layers;
    p.F0 = f->fields;
    p.D = f->dim;
    p.R = f->batch * (int64_t)f->dim;
    if (p.L < 1 || p.L > 8) return false;
    int fk = p.F0, off = 0;
    size_t cur = 0;
    auto take = [&](size_t n) { size_t o = cur; cur += (n + 3) & ~(size_t)3; return o; };
    p.x0t = take((size_t)p.R * p.F0);
    size_t zmax = 0, hmax = 0, fkmax = 0, pmax = 0;
    for (int k = 0; k < p.L; ++k) {
        const int H = f->layer_size[k];
        const bool last = k == p.L - 1;
        p.H[k] = H;
        p.Fk[k] = fk;
        p.Hn[k] = last ? 0 : (f->split_half ? H / 2 : H);
        p.d0[k] = f->split_half ? (last ? 0 : H / 2) : 0;
        p.off[k] = off;
        off += H - p.d0[k];
        p.y[k] = take((size_t)p.R * H);
        p.fused[k] = dctr_cinbwd::fused_shape_ok(p.F0, fk, H);
        p.z[k] = take(p.fused[k] ? 0 : (size_t)p.R * p.F0 * fk);
        if (!p.fused[k]) zmax = (size_t)p.R * p.F0 * fk > zmax ? (size_t)p.R * p.F0 * fk : zmax;
        else {
            const size_t pf = (size_t)dctr_cinbwd::dw_parts_floats(p.F0, fk, H, p.R);
            pmax = pf > pmax ? pf : pmax;
        }
        hmax = (size_t)H > hmax ? H : hmax;
        fkmax = (size_t)fk > fkmax ? fk : fkmax;
        fk = p.Hn[k];
    }
    p.out_dim = off;
    p.fwd_out = take((size_t)f->batch * off);          // the forward kernel's [B, featuremap_num] output when it is re-run for y_k
    p.dpre = take((size_t)p.R * hmax);
    p.dz = take(zmax);
    p.parts = take(pmax);                              // the z-free dW kernel's per-row-slice partial products
    p.dx0t = take((size_t)p.R * p.F0);
    p.dxk[0] = take((size_t)p.R * fkmax);
    p.dxk[1] = take((size_t)p.R * fkmax);
    // the re-run forward's own workspace (layer 0's fold; REQUIRED by the sliced / layer-by-layer routes of wide samples / layers)
    p.fwd_ws_bytes = dctr_cin_workspace_bytes(f);
    p.fwd_ws = take((p.fwd_ws_bytes + 3) / 4);
    p.total = cur;
    return true;
}
}  // namespace

extern "C" size_t dctr_cin_bwd_workspace_bytes(const dctr_cin_bwd_args_t* a) {
    CinPlan p;
    if (a == nullptr || a->fwd == nullptr || a->fwd->batch <= 0 || !cin_plan(a->fwd, p)) return 0;
    return p.total * sizeof(float);
}

extern "C" int dctr_cin_bwd(const dctr_cin_bwd_args_t* a, void* stream) {
    DCTR_REQUIRE(a != nullptr && a->fwd != nullptr, DCTR_E_NULL, "cin_bwd: null args");
    const dctr_cin_args_t* f = a->fwd;
    DCTR_REQUIRE(f->batch >= 0 && f->fields >= 1 && f->dim >= 1, DCTR_E_DIM, "cin_bwd: bad sizes");
    if (f->batch == 0) return DCTR_OK;
    CinPlan p;
    DCTR_REQUIRE(cin_plan(f, p), DCTR_E_DIM, "cin_bwd: 1..8 layers");
    DCTR_REQUIRE(f->x && f->layer_size && f->filters && f->bias && a->d_out && a->d_filters && a->d_bias, DCTR_E_NULL,
                 "cin_bwd: null pointer");
    DCTR_REQUIRE(f->activation >= DCTR_ACT_LINEAR && f->activation <= DCTR_ACT_TANH, DCTR_E_ENUM, "cin_bwd: activation %d",
                 f->activation);
    DCTR_REQUIRE(a->workspace != nullptr && a->workspace_bytes >= p.total * sizeof(float), DCTR_E_NULL,
                 "cin_bwd: needs a workspace of dctr_cin_bwd_workspace_bytes() bytes");
    DCTR_REQUIRE(p.R < 0x7fffffffLL, DCTR_E_DIM, "cin_bwd: batch * dim too large");
    hipStream_t st = (hipStream_t)stream;
    float* ws = static_cast<float*>(a->workspace);
    const int R = (int)p.R, F0 = p.F0, D = p.D;
    auto grid = [](int64_t n) { int64_t b = dctr_ceil_div(n, (int64_t)256); return dim3((unsigned)(b > 8192 ? 8192 : b)); };
    float* x0t = ws + p.x0t;
    hipLaunchKernelGGL(cin_to_rows_kernel, grid(p.R * F0), dim3(256), 0, st, f->x, f->x_stride, f->batch, F0, D, x0t);
    // the activations y_k: written by the forward call (saved_y), else the forward kernel is re-run here with the workspace as its
    // save_y (one launch; the first version recomputed them as z W with a GEMM per layer)
    const float* yk[8];
    bool rerun = false;
    for (int k = 0; k < p.L; ++k) {
        yk[k] = (a->saved_y != nullptr && a->saved_y[k] != nullptr) ? a->saved_y[k] : ws + p.y[k];
        rerun = rerun || yk[k] == ws + p.y[k];
    }
    if (rerun) {
        dctr_cin_args_t fa = *f;
        float* sv[8];
        for (int k = 0; k < p.L; ++k) sv[k] = yk[k] == ws + p.y[k] ? ws + p.y[k] : nullptr;
        fa.save_y = sv;
        fa.out = ws + p.fwd_out;
        if (p.fwd_ws_bytes > 0 && (fa.workspace == nullptr || fa.workspace_bytes < p.fwd_ws_bytes)) {   // (fwd->workspace is documented unused here)
            fa.workspace = ws + p.fwd_ws;
            fa.workspace_bytes = p.fwd_ws_bytes;
            fa.workspace_ready = 0;
        }
        const int rc = dctr_cin_fwd(&fa, stream);
        if (rc != 0) return rc;
    }
    // z only for layers outside the z-free kernels' shapes (the dW GEMM's operand)
    for (int k = 0; k < p.L; ++k) {
        if (p.fused[k]) continue;
        const int Fk = p.Fk[k], K = F0 * Fk;
        const float* xk = k == 0 ? x0t : yk[k - 1];
        const int64_t ldk = k == 0 ? F0 : p.H[k - 1];
        float* z = ws + p.z[k];
        if (Fk % 4 == 0 && ldk % 4 == 0 && dctr_aligned16(xk) && dctr_aligned16(z))
            hipLaunchKernelGGL(cin_outer4_kernel, grid(p.R * (K / 4)), dim3(256), 0, st, x0t, F0, xk, ldk, Fk, p.R, z);
        else
            hipLaunchKernelGGL(cin_outer_kernel, grid(p.R * K), dim3(256), 0, st, x0t, F0, xk, ldk, Fk, p.R, z);
    }
    hipError_t me = hipMemsetAsync(ws + p.dx0t, 0, (size_t)p.R * F0 * sizeof(float), st);
    DCTR_REQUIRE(me == hipSuccess, (int)me, "cin_bwd: memset failed: %s", hipGetErrorString(me));
    const float* dxnext = nullptr;
    int64_t ldn = 0;
    for (int k = p.L - 1; k >= 0; --k) {
        const int Fk = p.Fk[k], H = p.H[k], K = F0 * Fk;
        const float* xk = k == 0 ? x0t : yk[k - 1];
        const int64_t ldk = k == 0 ? F0 : p.H[k - 1];
        float* dpre = ws + p.dpre;
        float* dz = ws + p.dz;
        hipLaunchKernelGGL(cin_dpre_kernel, grid(p.R * H), dim3(256), 0, st, yk[k], dxnext, ldn, p.Hn[k], a->d_out,
                           (int64_t)a->out_dim, p.off[k], p.d0[k], p.R, H, D, (int)f->activation, dpre);
        dctr_train::launch_act_bwd_colsum(st, dpre, (const float*)nullptr, p.R, H, 0, a->d_bias[k]);
        // dW[K,H] += z^T dpre:  column-major  dW'(H x K) = dpre'(H x R) z'(K x R)^T.  The output is small (H x K) and the
        // reduction long (R = B*D): as ONE gemm it runs on ~18 workgroups (1.8 ms at C3); split the rows into `parts`
        // slices computed as a strided batch of partial products in the (now free) dz buffer, then summed.
        const int64_t hk = (int64_t)H * K;
        int parts = (int)((size_t)p.R * K / (size_t)hk);                 // partials fit the dz buffer: parts*H*K <= R*K
        if (parts > 32) parts = 32;
        while (parts > 1 && R % parts != 0) --parts;
        int rs = 0;
        if (p.fused[k]) {
            // z-free: x0[r,i] xk[r,j] formed in registers as the MFMA A operand, rows = the K dimension (cin_bwd_kernels.hip)
            DCTR_REQUIRE(dctr_aligned16(dpre) && dctr_aligned16(f->filters[k]), DCTR_E_ALIGN,
                         "cin_bwd: workspace / filters[%d] must be 16-B aligned", k);
            int n_parts = 0;
            const int rc = dctr_cinbwd::launch_dw_fused(dpre, x0t, xk, ldk, F0, Fk, H, p.R, ws + p.parts, &n_parts, st);
            DCTR_REQUIRE(rc == 0, rc, "cin_bwd: cannot launch the fused dW kernel (%d)", rc);
            dctr_train::launch_sum_parts(st, grid(hk).x, (const float*)(ws + p.parts), hk, n_parts, a->d_filters[k]);
        } else if (parts > 1) {
            const int rs_ = R / parts;
            rs = dctr_gemm::sgemm_strided_batched(st, dctr_gemm::OP_N, dctr_gemm::OP_T, H, K, rs_, dpre, H, (int64_t)rs_ * H, ws + p.z[k], K, (int64_t)rs_ * K, 0.f, dz, H, (int64_t)hk, parts);
            DCTR_REQUIRE(rs == 0, DCTR_E_UNSUPPORTED, "cin_bwd: sgemm_strided_batched(dW) failed (%d)", (int)rs);
            dctr_train::launch_sum_parts(st, grid(hk).x, dz, hk, parts, a->d_filters[k]);
        } else {
            rs = dctr_gemm::sgemm(st, dctr_gemm::OP_N, dctr_gemm::OP_T, H, K, R, dpre, H, ws + p.z[k], K, 1.f, a->d_filters[k], H);
            DCTR_REQUIRE(rs == 0, DCTR_E_UNSUPPORTED, "cin_bwd: sgemm(dW) failed (%d)", (int)rs);
        }
        float* dxk = ws + p.dxk[k & 1];          // layer 0: x_0 is also its x_k; that second-factor gradient lands in dxk[0]
        if (p.fused[k]) {
            // dz = dpre W^T is formed tile by tile on the matrix cores and contracted with x_0 / x_k at once (never stored)
            const int rc = dctr_cinbwd::launch_dz_fused(dpre, f->filters[k], x0t, xk, ldk, F0, Fk, H, p.R, ws + p.dx0t, dxk, st);
            DCTR_REQUIRE(rc == 0, rc, "cin_bwd: cannot launch the fused dz kernel (%d)", rc);
        } else {
            // dz[R,K] = dpre[R,H] W^T:  column-major  dz'(K x R) = W'(H x K)^T dpre'(H x R)
            rs = dctr_gemm::sgemm(st, dctr_gemm::OP_T, dctr_gemm::OP_N, K, R, H, f->filters[k], H, dpre, H, 0.f, dz, K);
            DCTR_REQUIRE(rs == 0, DCTR_E_UNSUPPORTED, "cin_bwd: sgemm(dz) failed (%d)", (int)rs);
            const size_t lds = (size_t)4 * (K + F0 + Fk) * sizeof(float);
            DCTR_REQUIRE(lds <= 64 * 1024, DCTR_E_UNSUPPORTED, "cin_bwd: F0*Fk = %d too large for the row-staging kernel", K);
            int64_t nb = dctr_ceil_div(p.R, (int64_t)4);
            if (nb > 256 * 16) nb = 256 * 16;
            hipLaunchKernelGGL(cin_outer_bwd_kernel, dim3((unsigned)nb), dim3(256), lds, st, dz, x0t, F0, xk, ldk, Fk, p.R,
                               ws + p.dx0t, dxk);
        }
        dxnext = dxk;
        ldn = Fk;
    }
    if (a->dx != nullptr) {
        // d x0 = dX0t (first factor, all layers) + layer 0's second factor (in dxk[0], [R, F0])
        dctr_train::launch_add_rows(st, grid(p.R * F0).x, ws + p.dxk[0], (int64_t)F0, p.R, F0, ws + p.dx0t, (int64_t)F0, 1);
        hipLaunchKernelGGL(cin_from_rows_kernel, grid(p.R * F0), dim3(256), 0, st, ws + p.dx0t, f->batch, F0, D, a->dx, a->dx_stride,
                           (int)a->dx_accumulate);
    }
    return dctr_launch_status("dctr_cin_bwd");
}
