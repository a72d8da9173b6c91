// Backward of dctr_interacting_fwd (interacting_kernels.hip): the InteractingLayer stack of AutoInt / DIFM, every layer in one launch.
//
// Nothing is saved by the forward.  A workgroup owns a tile of S samples and keeps, in LDS, the input X_l of EVERY layer (the
// forward re-run, same arithmetic as interacting_kernels.hip), Q, K, V of the layer at hand, the gradients dZ, dQ, dK, dV of that
// layer and the workgroup's share of every weight gradient.  Per layer, last to first, with Z = concat_h(P_h V_h) (+ X W_res),
// Y = relu(Z), s = 1 / sqrt(d) when scaling else 1:
//     dZ = dY [Y > 0]                          (Y of layer l is X_{l+1}: no pre-activation is kept; the last layer applies it to dy
//                                               in the forward's epilogue)
//     delta_i = sum_j P_ij dP_ij,  dP_ij = dZ_h[i] . V_h[j]
//     dS_ij = s P_ij (dP_ij - delta_i);   dQ_h[i] = sum_j dS_ij K_h[j];   dK_h[j] = sum_i dS_ij Q_h[i];   dV_h[j] = sum_i P_ij dZ_h[i]
//     dX = dQ W_q^T + dK W_k^T + dV W_v^T (+ dZ W_res^T);   dW_m += X_l^T dM
//   * projections X W (mfma_tile.h: tile_gemm_kn), the dX products dM W^T (tile_gemm_nk) and X^T dM (rows of the tile as the
//     reduction) on v_mfma_f32_16x16x4_f32: exact fp32;
//   * softmax rows recomputed from Q and K as the forward does (max pass, then __expf(s - max)); the row's max, 1 / sum and delta wait
//     in LDS, so no score matrix exists anywhere;
//   * one thread per (sample, field, head) owns dQ of that query AND dK, dV of that key and walks the other fields: no atomics inside
//     a sample, dx is bit-identical from call to call;
//   * weight gradients are summed in LDS over all tiles of the workgroup and leave with one atomicAdd per element and workgroup; the
//     grid is bounded (2 workgroups per compute unit, or max_blocks) and each workgroup walks its tiles.
// A sample whose buffers exceed the LDS runs the same code with them in a per-workgroup slice of the workspace (S = 1, <= 256 workgroups).
// Cost (F 26, E 16, d 8, H 2, 3 layers): the forward (289.5 kFLOP / sample) + about twice that for the gradients.
#include <math.h>
#include "dctr_common.h"
#include "mfma_tile.h"
#include "tile_route.h"

namespace {

constexpr int IB_MAX_LAYERS = 32;
constexpr int IB_THREADS = 256;
constexpr int IB_WAVES = IB_THREADS / 64;
constexpr int IB_DC = 16;                       // columns of one head a thread accumulates per pass over the other fields
constexpr int IB_MAX_S = 16;
constexpr size_t IB_LDS_TARGET = 80 * 1024;     // as the forward: two workgroups per CU where the samples allow it

struct IbParams {
    const float* x;
    int64_t batch;
    int64_t x_stride;
    int32_t F, E, n_layers, d, H, use_res, scaling;
    float sqrt_d;
    int32_t S;
    int32_t ldx, ldq;        // row strides (floats): X_l / dZ / dQ / dK / dV (MFMA A operands), and Q / K / V
    int64_t tile_floats;     // floats of one workgroup's buffers
    int64_t acc_floats;      // ... of which the weight-gradient sums at the end
    const float* W[IB_MAX_LAYERS][4];
    float* dW[IB_MAX_LAYERS][4];
    const float* dy;
    int64_t dy_stride;
    float* dx;
    int64_t dx_stride;
    int32_t accumulate;
    float* ws;               // workspace route only
};

__device__ __forceinline__ float ib_dot(const float* a, const float* b, int n) {
    float s = 0.f;
    for (int c = 0; c < n; ++c) s = fmaf(a[c], b[c], s);
    return s;
}

// Q, K, V (, R) = X W_m for m < n_proj: one 16 x 16 output tile per wave task.  R has the row stride of X.
__device__ __forceinline__ void ib_project(const IbParams& p, int l, const float* X, int K, int n_proj, float* Qb, float* Kb, float* Vb,
                                           float* Rb, int SF, int RT, int CT) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, dH = p.d * p.H;
    const int KQ = ((K + 15) & ~15) >> 2;
    for (int t = wave; t < RT * CT * n_proj; t += IB_WAVES) {
        const int m = t % n_proj, rest = t / n_proj, ct = rest % CT, rt = rest / CT;
        dctr::f32x4 acc[1] = {{0.f, 0.f, 0.f, 0.f}};
        dctr::tile_gemm_kn<1>(X + rt * 16 * p.ldx, p.ldx, K, KQ, p.W[l][m], dH, ct * 16, acc);
        float* dst = m == 0 ? Qb : m == 1 ? Kb : m == 2 ? Vb : Rb;
        const int ld = m == 3 ? p.ldx : p.ldq;
        const int col = ct * 16 + (lane & 15), row0 = rt * 16 + 4 * (lane >> 4);
        if (col < dH) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (row0 + r < SF) dst[(row0 + r) * ld + col] = acc[0][r];
        }
    }
}

// D: att_embedding_size when the instantiation is for one (the dot products and the per-head column loops unroll and the thread's own
// rows stay in registers), 0 for any.
template <bool GLOBAL_WS, int D>
__global__ __launch_bounds__(IB_THREADS) void interacting_bwd_kernel(IbParams p) {
    extern __shared__ __attribute__((aligned(16))) float ib_lds[];
    float* base = GLOBAL_WS ? p.ws + (int64_t)blockIdx.x * p.tile_floats : ib_lds;
    const int S = p.S, F = p.F, d = D ? D : p.d, H = p.H, L = p.n_layers, dH = d * H, SF = S * F, ldx = p.ldx, ldq = p.ldq;
    const int RP = (SF + 15) & ~15, RT = RP >> 4, CT = (dH + 15) >> 4;
    const int xbuf = RP * ldx;
    float* G = base + L * xbuf;         // dZ of the layer at hand
    float* dQb = G + xbuf;              // (the forward re-run keeps R here)
    float* dKb = dQb + xbuf;
    float* dVb = dKb + xbuf;
    float* Qb = dVb + xbuf;             // Q; between two layers the dX of the upper one = dY of the lower one
    float* Kb = Qb + SF * ldq;
    float* Vb = Kb + SF * ldq;
    float* St = Vb + SF * ldq;          // per (row, head): the softmax row's max, 1 / sum, delta
    float* AW = base + (p.tile_floats - p.acc_floats);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int nw = p.use_res ? 4 : 3;
    const int64_t n_tiles = (p.batch + S - 1) / S;

    // every buffer starts finite: padding rows and columns are MFMA operands, and the weight-gradient sums start at zero
    for (int64_t e = tid; e < p.tile_floats; e += IB_THREADS) base[e] = 0.f;
    __syncthreads();

    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t b0 = tile * S;
        const int nvalid = (int)min((int64_t)S, p.batch - b0);
        const int n_att = nvalid * F * H;
        for (int e = tid; e < xbuf; e += IB_THREADS) {
            const int r = e / ldx, c = e - r * ldx;
            const int s = r / F, f = r - s * F;
            float v = 0.f;
            if (r < SF && s < nvalid && c < p.E) v = p.x[(b0 + s) * p.x_stride + (int64_t)f * p.E + c];
            base[e] = v;
            G[e] = 0.f;
        }
        __syncthreads();
        // ---- the forward again, X_l kept for every layer; the last layer's epilogue leaves dZ = dy [Y > 0] -------------------------
        for (int l = 0; l < L; ++l) {
            const float* X = base + l * xbuf;
            const bool last = l == L - 1;
            float* Xn = last ? G : base + (l + 1) * xbuf;
            ib_project(p, l, X, l ? dH : p.E, nw, Qb, Kb, Vb, dQb, SF, RT, CT);
            __syncthreads();
            for (int it = tid; it < n_att; it += IB_THREADS) {
                const int h = it % H, row = it / H, s = row / F;
                const float* q = Qb + row * ldq + h * d;
                const float* kb = Kb + s * F * ldq + h * d;
                const float* vb = Vb + s * F * ldq + h * d;
                float mx = -INFINITY;
                for (int j = 0; j < F; ++j) {
                    float sc = ib_dot(q, kb + j * ldq, d);
                    if (p.scaling) sc = sc / p.sqrt_d;
                    mx = fmaxf(mx, sc);
                }
                for (int c0 = 0; c0 < d; c0 += IB_DC) {
                    float acc[IB_DC];
#pragma unroll
                    for (int c = 0; c < IB_DC; ++c) acc[c] = 0.f;
                    float sum = 0.f;
                    for (int j = 0; j < F; ++j) {
                        float sc = ib_dot(q, kb + j * ldq, d);
                        if (p.scaling) sc = sc / p.sqrt_d;
                        const float e = __expf(sc - mx);
                        sum += e;
                        const float* vj = vb + j * ldq + c0;
#pragma unroll
                        for (int c = 0; c < IB_DC; ++c)
                            if (c0 + c < d) acc[c] = fmaf(e, vj[c], acc[c]);
                    }
                    const float inv = 1.f / sum;
                    float* xo = Xn + row * ldx + h * d + c0;
                    const float* rr = dQb + row * ldx + h * d + c0;
                    const float* dyr = p.dy + (b0 + s) * p.dy_stride + (int64_t)(row - s * F) * dH + h * d + c0;
#pragma unroll
                    for (int c = 0; c < IB_DC; ++c) {
                        if (c0 + c < d) {
                            float o = acc[c] * inv;
                            if (p.use_res) o += rr[c];
                            xo[c] = last ? (o > 0.f ? dyr[c] : 0.f) : fmaxf(o, 0.f);
                        }
                    }
                }
            }
            __syncthreads();
        }
        // R's rows leave: dQ, dK, dV are zero wherever a layer does not write them
        for (int e = tid; e < 3 * xbuf; e += IB_THREADS) dQb[e] = 0.f;
        __syncthreads();
        // ---- the layers in reverse -------------------------------------------------------------------------------------------------
        for (int l = L - 1; l >= 0; --l) {
            const float* X = base + l * xbuf;
            const int K = l ? dH : p.E;
            if (l < L - 1) {
                const float* Y = base + (l + 1) * xbuf;     // this layer's output
                for (int e = tid; e < nvalid * F * dH; e += IB_THREADS) {
                    const int r = e / dH, c = e - r * dH;
                    G[r * ldx + c] = Y[r * ldx + c] > 0.f ? Qb[r * ldq + c] : 0.f;
                }
                __syncthreads();
                ib_project(p, l, X, K, 3, Qb, Kb, Vb, nullptr, SF, RT, CT);
                __syncthreads();
            }
            // the softmax rows' statistics
            for (int it = tid; it < n_att; it += IB_THREADS) {
                const int h = it % H, row = it / H, s = row / F;
                const float* q = Qb + row * ldq + h * d;
                const float* kb = Kb + s * F * ldq + h * d;
                const float* vb = Vb + s * F * ldq + h * d;
                const float* dz = G + row * ldx + h * d;
                float mx = -INFINITY;
                for (int j = 0; j < F; ++j) {
                    float sc = ib_dot(q, kb + j * ldq, d);
                    if (p.scaling) sc = sc / p.sqrt_d;
                    mx = fmaxf(mx, sc);
                }
                float sum = 0.f, dsum = 0.f;
                for (int j = 0; j < F; ++j) {
                    float sc = ib_dot(q, kb + j * ldq, d);
                    if (p.scaling) sc = sc / p.sqrt_d;
                    const float e = __expf(sc - mx);
                    sum += e;
                    dsum = fmaf(e, ib_dot(dz, vb + j * ldq, d), dsum);
                }
                const float inv = 1.f / sum;
                St[3 * it] = mx;
                St[3 * it + 1] = inv;
                St[3 * it + 2] = dsum * inv;
            }
            __syncthreads();
            // dQ of query `row`, dK and dV of key `row`: one walk over the sample's fields
            for (int it = tid; it < n_att; it += IB_THREADS) {
                const int h = it % H, row = it / H, s = row / F;
                const float* q = Qb + row * ldq + h * d;
                const float* k = Kb + row * ldq + h * d;
                const float* v = Vb + row * ldq + h * d;
                const float* dz = G + row * ldx + h * d;
                const float mx = St[3 * it], inv = St[3 * it + 1], del = St[3 * it + 2];
                for (int c0 = 0; c0 < d; c0 += IB_DC) {
                    float aq[IB_DC], ak[IB_DC], av[IB_DC];
#pragma unroll
                    for (int c = 0; c < IB_DC; ++c) aq[c] = ak[c] = av[c] = 0.f;
                    for (int t = 0; t < F; ++t) {
                        const int orow = s * F + t;
                        const float* qo = Qb + orow * ldq + h * d;
                        const float* ko = Kb + orow * ldq + h * d;
                        const float* vo = Vb + orow * ldq + h * d;
                        const float* dzo = G + orow * ldx + h * d;
                        const float* so = St + 3 * (orow * H + h);
                        // this row as the query, field t as the key
                        float sc = ib_dot(q, ko, d);
                        if (p.scaling) sc = sc / p.sqrt_d;
                        float ds = __expf(sc - mx) * inv * (ib_dot(dz, vo, d) - del);
                        if (p.scaling) ds = ds / p.sqrt_d;
                        // this row as the key, field t as the query
                        float sc2 = ib_dot(qo, k, d);
                        if (p.scaling) sc2 = sc2 / p.sqrt_d;
                        const float pr = __expf(sc2 - so[0]) * so[1];
                        float ds2 = pr * (ib_dot(dzo, v, d) - so[2]);
                        if (p.scaling) ds2 = ds2 / p.sqrt_d;
#pragma unroll
                        for (int c = 0; c < IB_DC; ++c) {
                            if (c0 + c < d) {
                                aq[c] = fmaf(ds, ko[c0 + c], aq[c]);
                                ak[c] = fmaf(ds2, qo[c0 + c], ak[c]);
                                av[c] = fmaf(pr, dzo[c0 + c], av[c]);
                            }
                        }
                    }
                    const int o = row * ldx + h * d + c0;
#pragma unroll
                    for (int c = 0; c < IB_DC; ++c) {
                        if (c0 + c < d) {
                            dQb[o + c] = aq[c];
                            dKb[o + c] = ak[c];
                            dVb[o + c] = av[c];
                        }
                    }
                }
            }
            __syncthreads();
            // dW_m += X^T dM (the tile's rows are the reduction) and dX = sum_m dM W_m^T: one 16 x 16 output tile per wave task
            {
                const int ET = (K + 15) >> 4, n_dw = nw * ET * CT, n_dx = (l > 0 || p.dx) ? RT * ET : 0;
                const int KQ = ((dH + 15) & ~15) >> 2;
                const int g = lane >> 4, j = lane & 15;
                const int64_t l_off = l ? (int64_t)nw * p.E * dH + (int64_t)(l - 1) * nw * dH * dH : 0;
                for (int t = wave; t < n_dw + n_dx; t += IB_WAVES) {
                    dctr::f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                    if (t < n_dw) {
                        const int m = t % nw, rest = t / nw, ct = rest % CT, et = rest / CT;
                        if (!p.dW[l][m]) continue;
                        const float* Bm = m == 0 ? dQb : m == 1 ? dKb : m == 2 ? dVb : G;
                        const float* ap = X + g * ldx + et * 16 + j;
                        const float* bp = Bm + g * ldx + ct * 16 + j;
                        for (int k0 = 0; k0 < RP; k0 += 4)
                            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[k0 * ldx], bp[k0 * ldx], acc, 0, 0, 0);
                        float* aw = AW + l_off + (int64_t)m * K * dH;
                        const int col = ct * 16 + j, e0 = et * 16 + 4 * g;
                        if (col < dH) {
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                if (e0 + r < K) aw[(int64_t)(e0 + r) * dH + col] += acc[r];
                        }
                    } else {
                        const int u = t - n_dw, et = u % ET, rt = u / ET;
                        dctr::f32x4 a1[1] = {acc};
                        dctr::tile_gemm_nk<1>(dQb + rt * 16 * ldx, ldx, dH, KQ, p.W[l][0], K, et * 16, a1);
                        dctr::tile_gemm_nk<1>(dKb + rt * 16 * ldx, ldx, dH, KQ, p.W[l][1], K, et * 16, a1);
                        dctr::tile_gemm_nk<1>(dVb + rt * 16 * ldx, ldx, dH, KQ, p.W[l][2], K, et * 16, a1);
                        if (p.use_res) dctr::tile_gemm_nk<1>(G + rt * 16 * ldx, ldx, dH, KQ, p.W[l][3], K, et * 16, a1);
                        const int col = et * 16 + j, row0 = rt * 16 + 4 * g;
                        if (col < K) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const int row = row0 + r;
                                if (row >= nvalid * F) continue;
                                if (l > 0) {
                                    Qb[row * ldq + col] = a1[0][r];
                                } else {
                                    const int s = row / F;
                                    float* o = p.dx + (b0 + s) * p.dx_stride + (int64_t)(row - s * F) * p.E + col;
                                    *o = p.accumulate ? *o + a1[0][r] : a1[0][r];
                                }
                            }
                        }
                    }
                }
            }
            __syncthreads();
        }
    }
    // one atomic per workgroup and weight-gradient element
    int64_t off = 0;
    for (int l = 0; l < L; ++l) {
        const int64_t n = (int64_t)(l ? dH : p.E) * dH;
        for (int m = 0; m < nw; ++m, off += n) {
            float* dst = p.dW[l][m];
            if (!dst) continue;
            for (int64_t i = tid; i < n; i += IB_THREADS) atomicAdd(&dst[i], AW[off + i]);
        }
    }
}

struct IbPlan {
    bool ok;                // the shape is taken (<= 32 layers, one sample's buffers below 2^31 floats)
    bool global;            // buffers in the workspace
    int S, ldx, ldq;
    int64_t tile_floats, acc_floats;
    int grid_max;
    size_t route_bytes;
};

int64_t ib_tile_floats(int S, int F, int L, int H, int ldx, int ldq, int64_t acc_floats) {
    const int64_t sf = (int64_t)S * F;
    const int64_t rp = (sf + 15) & ~(int64_t)15;
    int64_t v = (L + 4) * rp * ldx + 3 * sf * ldq + 3 * sf * H;
    v = (v + 3) & ~(int64_t)3;
    return v + ((acc_floats + 3) & ~(int64_t)3);
}

void ib_plan(const dctr_interacting_args_t* a, IbPlan* pl) {
    const int64_t dH = (int64_t)a->att_embedding_size * a->head_num;
    const int64_t wmax = a->dim > dH ? a->dim : dH;
    const int nb = a->use_res ? 4 : 3;
    pl->ok = false;
    pl->global = false;
    pl->route_bytes = 0;
    pl->grid_max = 0;
    if (a->n_layers > IB_MAX_LAYERS) return;
    pl->ldx = (int)(((wmax + 15) & ~(int64_t)15) + 4);
    pl->ldq = (int)(dH | 1);
    pl->acc_floats = ((nb * (a->dim + (a->n_layers - 1) * dH) * dH) + 3) & ~(int64_t)3;
    // 32-bit indices inside a tile: refuse what one sample already overflows
    const double one = ((double)a->n_layers + 4) * ((double)a->fields + 16) * pl->ldx + 3.0 * a->fields * (pl->ldq + a->head_num) +
                       (double)nb * ((double)a->dim + (a->n_layers - 1.0) * dH) * dH;
    if (one >= 2.0e9) return;
    pl->ok = true;
    int S = IB_MAX_S;
    while (S > 1 && (size_t)ib_tile_floats(S, a->fields, a->n_layers, a->head_num, pl->ldx, pl->ldq, pl->acc_floats) * 4 > IB_LDS_TARGET) --S;
    pl->tile_floats = ib_tile_floats(S, a->fields, a->n_layers, a->head_num, pl->ldx, pl->ldq, pl->acc_floats);
    pl->S = S;
    const dctr_tile_route r = dctr_plan_tile_route((size_t)pl->tile_floats * 4);
    pl->global = r.global;
    pl->grid_max = r.grid_max;
    pl->route_bytes = r.route_bytes;
}

// the forward's size checks (ia_check of interacting_kernels.hip; out / head_w / logit are not read) and the backward's own
int ib_check(const dctr_interacting_bwd_args_t* b) {
    DCTR_REQUIRE(b, DCTR_E_NULL, "interacting_bwd: null args");
    const dctr_interacting_args_t* a = &b->fwd;
    DCTR_REQUIRE(a->batch >= 0 && a->fields >= 1 && a->dim >= 1 && a->n_layers >= 1 && a->att_embedding_size >= 1 && a->head_num >= 1,
                 DCTR_E_DIM, "interacting_bwd: bad sizes");
    const int64_t dH = (int64_t)a->att_embedding_size * a->head_num;
    DCTR_REQUIRE(dH <= (1 << 24) && a->dim <= (1 << 24), DCTR_E_DIM, "interacting_bwd: d*H / dim above 2^24");
    DCTR_REQUIRE(a->x_stride >= (int64_t)a->fields * a->dim, DCTR_E_DIM, "interacting_bwd: x_stride < fields*dim");
    DCTR_REQUIRE(b->dy_stride >= (int64_t)a->fields * dH, DCTR_E_DIM, "interacting_bwd: dy_stride < fields*d*H");
    DCTR_REQUIRE(!b->dx || b->dx_stride >= (int64_t)a->fields * a->dim, DCTR_E_DIM, "interacting_bwd: dx_stride < fields*dim");
    DCTR_REQUIRE(b->max_blocks >= 0, DCTR_E_DIM, "interacting_bwd: max_blocks = %d", b->max_blocks);
    DCTR_REQUIRE((a->use_res == 0 || a->use_res == 1) && (a->scaling == 0 || a->scaling == 1) && (b->accumulate == 0 || b->accumulate == 1),
                 DCTR_E_ENUM, "interacting_bwd: use_res / scaling / accumulate must be 0 or 1");
    return DCTR_OK;
}

}  // namespace

extern "C" int dctr_interacting_bwd_supported(const dctr_interacting_bwd_args_t* b) {
    if (ib_check(b) != DCTR_OK) return 0;
    IbPlan pl;
    ib_plan(&b->fwd, &pl);
    return pl.ok ? 1 : 0;
}

extern "C" size_t dctr_interacting_bwd_workspace_bytes(const dctr_interacting_bwd_args_t* b) {
    if (ib_check(b) != DCTR_OK) return 0;
    IbPlan pl;
    ib_plan(&b->fwd, &pl);
    return pl.ok ? pl.route_bytes : 0;
}

extern "C" int dctr_interacting_bwd(const dctr_interacting_bwd_args_t* b, void* stream) {
    int rc = ib_check(b);
    if (rc != DCTR_OK) return rc;
    const dctr_interacting_args_t* a = &b->fwd;
    IbPlan pl;
    ib_plan(a, &pl);
    DCTR_REQUIRE(pl.ok, DCTR_E_UNSUPPORTED, "interacting_bwd: %d layers (at most %d), or one sample's buffers exceed 2^31 floats",
                 a->n_layers, IB_MAX_LAYERS);
    DCTR_REQUIRE(a->x && a->layers && b->dy, DCTR_E_NULL, "interacting_bwd: null x / layers / dy");
    for (int l = 0; l < a->n_layers; ++l)
        DCTR_REQUIRE(a->layers[4 * l] && a->layers[4 * l + 1] && a->layers[4 * l + 2] && (!a->use_res || a->layers[4 * l + 3]),
                     DCTR_E_NULL, "interacting_bwd: layer %d: null weight", l);
    if (pl.route_bytes)
        DCTR_REQUIRE_WORKSPACE("interacting_bwd", "dctr_interacting_bwd_workspace_bytes", a->workspace, a->workspace_bytes, pl.route_bytes);
    if (a->batch == 0) return DCTR_OK;
    const int nb = a->use_res ? 4 : 3;
    IbParams p = {};
    p.x = a->x;
    p.batch = a->batch;
    p.x_stride = a->x_stride;
    p.F = a->fields;
    p.E = a->dim;
    p.n_layers = a->n_layers;
    p.d = a->att_embedding_size;
    p.H = a->head_num;
    p.use_res = a->use_res;
    p.scaling = a->scaling;
    p.sqrt_d = (float)sqrt((double)a->att_embedding_size);
    p.S = pl.S;
    p.ldx = pl.ldx;
    p.ldq = pl.ldq;
    p.tile_floats = pl.tile_floats;
    p.acc_floats = pl.acc_floats;
    for (int l = 0; l < a->n_layers; ++l)
        for (int m = 0; m < 4; ++m) {
            p.W[l][m] = a->layers[4 * l + m];
            p.dW[l][m] = b->d_layers && m < nb ? b->d_layers[4 * l + m] : nullptr;
        }
    p.dy = b->dy;
    p.dy_stride = b->dy_stride;
    p.dx = b->dx;
    p.dx_stride = b->dx_stride;
    p.accumulate = b->accumulate;
    p.ws = pl.global ? (float*)a->workspace : nullptr;
    const int64_t n_tiles = dctr_ceil_div(a->batch, pl.S);
    int64_t cap = b->max_blocks > 0 ? (int64_t)b->max_blocks : (int64_t)2 * dctr_n_cus();
    if (pl.global && cap > pl.grid_max) cap = pl.grid_max;
    const dim3 grid((unsigned)(n_tiles < cap ? n_tiles : cap)), block(IB_THREADS);
    if (pl.global) {
        DCTR_LAUNCH((interacting_bwd_kernel<true, 0>), grid, block, 0, (hipStream_t)stream, p);
    } else {
        // d = 8, the default of AutoInt and DIFM, has an instantiation of its own
        const size_t lds = (size_t)pl.tile_floats * sizeof(float);
        const bool d8 = p.d == 8;
        static thread_local size_t granted[DCTR_MAX_DEVICES] = {0}, granted8[DCTR_MAX_DEVICES] = {0};
        hipError_t e = d8 ? dctr_grant_lds((const void*)interacting_bwd_kernel<false, 8>, lds, granted8)
                          : dctr_grant_lds((const void*)interacting_bwd_kernel<false, 0>, lds, granted);
        DCTR_REQUIRE(e == hipSuccess, (int)e, "interacting_bwd: cannot raise dynamic LDS: %s", hipGetErrorString(e));
        if (d8)
            DCTR_LAUNCH((interacting_bwd_kernel<false, 8>), grid, block, lds, (hipStream_t)stream, p);
        else
            DCTR_LAUNCH((interacting_bwd_kernel<false, 0>), grid, block, lds, (hipStream_t)stream, p);
    }
    return dctr_launch_status("dctr_interacting_bwd");
}
