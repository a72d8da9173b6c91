// The multi-task models' expert / gate / tower stack (reference deepctr/models/multitask/{mmoe,ple,sharedbottom,esmm}.py), forward.
//
// One LEVEL (MMOE once, PLE's CGC layer num_levels times), over S input slots X_s = in_dim columns of one [B, x_stride] buffer:
//     expert e < E :  h_e = DNN_e(X_src[e])                 L layers of the same units for every expert, own weights
//     gate   g < G :  z_g = GateDNN_g(X_gsrc[g]) (or X)     p_g = softmax(z_g Wg_g),  Wg_g [dz, n_g], no bias
//                     O_g = sum_j p_g[j] * h_{members[g][j]}  -> out[B, G, H]
// The TOWERS: tower t < T = DNN_t (possibly empty) over slot src[t], Dense(1, no bias), global_bias_t, sigmoid where binary ->
// probs[T, B]; esmm: probs[1] = sigmoid(l_0) * sigmoid(l_1).
//
// dctr_mtl_level_fwd / dctr_mtl_towers_fwd, the fused route: ONE launch per level / for all towers.  A workgroup of 8 waves takes a tile
// of R rows: the slots are staged into LDS once, every DNN layer is a set of 16 x 16*TPW output tiles on v_mfma_f32_16x16x4_f32
// (mfma_tile.h: tile_gemm_kn, exact fp32) with bias / BatchNormalization affine / activation as the tile's epilogue, the layer outputs
// ping-pong through two LDS tiles, the LAST layer of every expert (tower) stays in LDS for all E; the gate logits are one more tile
// product, the softmaxes one thread per (row, gate), and the mixtures (heads) read the experts' tiles from LDS and store only `out`.
// No atomics: the same bits on every call.
//
// dctr_mtl_mix: the layered route's one new step — gate logits, softmax over members[g] and the mixtures from expert outputs that
// already lie in HBM (the host runs experts and gate DNNs through dctr_mlp_fwd).  One wave per row; any shape.
#include <math.h>
#include "dctr_common.h"
#include "tile_route.h"
#include "mfma_tile.h"

namespace {

constexpr int MT_THREADS = 512;
constexpr int MT_WAVES = MT_THREADS / 64;
constexpr int MT_MAX_SLOTS = 8, MT_MAX_EXPERTS = 16, MT_MAX_ELAYERS = 32, MT_MAX_GATES = 8, MT_MAX_GLAYERS = 16, MT_MAX_MEMBERS = 64;
constexpr int MT_MAX_DEPTH = 4;
constexpr int MX_THREADS = 256;
constexpr int MX_MAX_GATES = 8;               // gates per dctr_mtl_mix launch (kernel-argument space)

struct MtLayer {
    const float *w, *b, *sc, *sh;
};

struct MtParams {
    int64_t batch;
    const float* x;
    int64_t x_stride;
    int64_t x_off[MT_MAX_SLOTS];
    int32_t kind, S, Din, E, L, G, Lg, act, aligned, R, ldx, ldt, ldh, ldz, ldp, nT, H, dz;
    int32_t units[MT_MAX_DEPTH], gunits[MT_MAX_DEPTH];
    uint8_t esrc[MT_MAX_EXPERTS], gsrc[MT_MAX_GATES], gn[MT_MAX_GATES], goff[MT_MAX_GATES], members[MT_MAX_MEMBERS];
    MtLayer el[MT_MAX_ELAYERS];
    MtLayer gl[MT_MAX_GLAYERS];
    const float* gk[MT_MAX_GATES];
    float* out;                    // already advanced by out_offset
    int64_t out_stride;
    const float* head_w[MT_MAX_GATES];
    const float* gbias[MT_MAX_GATES];
    uint8_t binary[MT_MAX_GATES];
    int32_t esmm;
    float* probs;
    int64_t probs_stride;
};

__device__ __forceinline__ float mt_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// O[R, N] = act(bn(A[R, K] W + b)) as 16 x 16*TPW tiles over the workgroup's waves; with zero_pad the columns [N, pad16(N)) of O are
// cleared (O is the next product's A operand: its K padding must read zero whatever the tile held before)
template <int TPW>
__device__ __forceinline__ void mt_layer_t(const float* A, int lda, int K, const MtLayer ly, int N, int act, float* O, int ldo, int RT,
                                           bool zero_pad) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int CT = (N + 16 * TPW - 1) / (16 * TPW), KQ = dctr::pad16(K) >> 2;
    for (int t = wave; t < RT * CT; t += MT_WAVES) {
        const int rt = t / CT, ct = t - rt * CT;
        dctr::f32x4 acc[TPW];
#pragma unroll
        for (int c = 0; c < TPW; ++c) acc[c] = dctr::f32x4{0.f, 0.f, 0.f, 0.f};
        dctr::tile_gemm_kn<TPW>(A + rt * 16 * lda, lda, K, KQ, ly.w, N, ct * 16 * TPW, acc);
        const int row0 = rt * 16 + 4 * (lane >> 4), col0 = ct * 16 * TPW + TPW * (lane & 15);
#pragma unroll
        for (int c = 0; c < TPW; ++c) {
            const int col = col0 + c;
            if (col < N) {
                const float b = ly.b ? ly.b[col] : 0.f;
                const float sc = ly.sc ? ly.sc[col] : 1.f, sh = ly.sc ? ly.sh[col] : 0.f;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float v = acc[c][r] + b;
                    if (ly.sc) v = v * sc + sh;
                    O[(row0 + r) * ldo + col] = dctr::apply_act(v, act);
                }
            } else if (zero_pad) {          // (TPW == 1 only: col < pad16(N) <= ldo - 4)
#pragma unroll
                for (int r = 0; r < 4; ++r) O[(row0 + r) * ldo + col] = 0.f;
            }
        }
    }
}

// the widest column mapping that still gives every wave a tile (the 8- / 16-byte weight loads need N % (16 TPW) == 0 and aligned kernels)
__device__ __forceinline__ void mt_layer(const float* A, int lda, int K, const MtLayer ly, int N, int act, float* O, int ldo, int RT,
                                         int aligned, bool zero_pad) {
    if (aligned && N % 64 == 0 && RT * (N / 64) >= MT_WAVES)
        mt_layer_t<4>(A, lda, K, ly, N, act, O, ldo, RT, zero_pad);
    else if (aligned && N % 32 == 0 && RT * (N / 32) >= MT_WAVES)
        mt_layer_t<2>(A, lda, K, ly, N, act, O, ldo, RT, zero_pad);
    else
        mt_layer_t<1>(A, lda, K, ly, N, act, O, ldo, RT, zero_pad);
}

__global__ __launch_bounds__(MT_THREADS) void mtl_kernel(MtParams p) {
    extern __shared__ __attribute__((aligned(16))) float mt_lds[];
    const int R = p.R, RT = R >> 4, ldx = p.ldx, ldt = p.ldt, ldh = p.ldh, ldz = p.ldz, ldp = p.ldp;
    float* X = mt_lds;
    float* T = X + p.S * R * ldx;
    float* Hb = T + p.nT * R * ldt;
    float* Z = Hb + (p.L ? p.E * R * ldh : 0);
    float* P = Z + (p.Lg ? p.G * R * ldz : 0);
    const int lds_floats = (int)(P - X) + R * ldp;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t n_tiles = (p.batch + R - 1) / R;

    // the K padding of every tile is read by the products; the layer epilogues keep it zero from here on
    for (int e = tid; e < lds_floats; e += MT_THREADS) mt_lds[e] = 0.f;
    __syncthreads();

    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t b0 = tile * R;
        const int nvalid = (int)min((int64_t)R, p.batch - b0);
        for (int s = 0; s < p.S; ++s) {
            const float* xs = p.x + p.x_off[s];
            float* Xs = X + s * R * ldx;
            for (int e = tid; e < R * p.Din; e += MT_THREADS) {
                const int r = e / p.Din, k = e - r * p.Din;
                Xs[r * ldx + k] = r < nvalid ? xs[(b0 + r) * p.x_stride + k] : 0.f;
            }
        }
        __syncthreads();
        // the experts' (towers') DNNs: the last layer of each waits in Hb[e]
        for (int e = 0; e < p.E; ++e) {
            const float* A = X + p.esrc[e] * R * ldx;
            int lda = ldx, K = p.Din;
            for (int l = 0; l < p.L; ++l) {
                const bool last = l + 1 == p.L;
                float* O = last ? Hb + e * R * ldh : T + (l & 1) * R * ldt;
                const int ldo = last ? ldh : ldt;
                mt_layer(A, lda, K, p.el[e * p.L + l], p.units[l], p.act, O, ldo, RT, p.aligned, true);
                __syncthreads();
                A = O;
                lda = ldo;
                K = p.units[l];
            }
        }
        if (p.kind == DCTR_MTL_LEVEL) {
            // the gates' DNNs -> Z[g]
            for (int g = 0; g < p.G && p.Lg; ++g) {
                const float* A = X + p.gsrc[g] * R * ldx;
                int lda = ldx, K = p.Din;
                for (int l = 0; l < p.Lg; ++l) {
                    const bool last = l + 1 == p.Lg;
                    float* O = last ? Z + g * R * ldz : T + (l & 1) * R * ldt;
                    const int ldo = last ? ldz : ldt;
                    mt_layer(A, lda, K, p.gl[g * p.Lg + l], p.gunits[l], p.act, O, ldo, RT, p.aligned, true);
                    __syncthreads();
                    A = O;
                    lda = ldo;
                    K = p.gunits[l];
                }
            }
            // the gate logits of all gates: z_g Wg_g -> P[r, goff[g] + j]
            {
                const int KQ = dctr::pad16(p.dz) >> 2;
                int t = 0;
                for (int g = 0; g < p.G; ++g) {
                    const float* A = p.Lg ? Z + g * R * ldz : X + p.gsrc[g] * R * ldx;
                    const int lda = p.Lg ? ldz : ldx, n = p.gn[g], CT = (n + 15) >> 4;
                    for (int q = 0; q < RT * CT; ++q, ++t) {
                        if (t % MT_WAVES != wave) continue;
                        const int rt = q / CT, ct = q - rt * CT;
                        dctr::f32x4 acc[1] = {dctr::f32x4{0.f, 0.f, 0.f, 0.f}};
                        dctr::tile_gemm_kn<1>(A + rt * 16 * lda, lda, p.dz, KQ, p.gk[g], n, ct * 16, acc);
                        const int row0 = rt * 16 + 4 * (lane >> 4), col = ct * 16 + (lane & 15);
                        if (col < n) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) P[(row0 + r) * ldp + p.goff[g] + col] = acc[0][r];
                        }
                    }
                }
            }
            __syncthreads();
            for (int e = tid; e < R * p.G; e += MT_THREADS) {
                const int r = e / p.G, g = e - r * p.G, n = p.gn[g];
                float* pr = P + r * ldp + p.goff[g];
                float m = pr[0], s = 0.f;
                for (int j = 1; j < n; ++j) m = fmaxf(m, pr[j]);
                for (int j = 0; j < n; ++j) {
                    const float ex = expf(pr[j] - m);
                    pr[j] = ex;
                    s += ex;
                }
                for (int j = 0; j < n; ++j) pr[j] = pr[j] / s;
            }
            __syncthreads();
            const int H = p.H, GH = p.G * H;
            for (int e = tid; e < nvalid * GH; e += MT_THREADS) {
                const int r = e / GH, rem = e - r * GH, g = rem / H, c = rem - g * H, n = p.gn[g], off = p.goff[g];
                const float* pr = P + r * ldp + off;
                float acc = 0.f;
                for (int j = 0; j < n; ++j) acc = fmaf(pr[j], Hb[(p.members[off + j] * R + r) * ldh + c], acc);
                p.out[(b0 + r) * p.out_stride + rem] = acc;
            }
        } else {
            // the heads: one wave per row takes the T dot products, then the PredictionLayers
            const int K = p.L ? p.units[p.L - 1] : p.Din;
            for (int r = wave; r < nvalid; r += MT_WAVES) {
                float lg[MT_MAX_GATES];
#pragma unroll
                for (int t = 0; t < MT_MAX_GATES; ++t) {
                    lg[t] = 0.f;
                    if (t < p.E) {
                        const float* hr = p.L ? Hb + (t * R + r) * ldh : X + (p.esrc[t] * R + r) * ldx;
                        float acc = 0.f;
                        for (int k = lane; k < K; k += 64) acc = fmaf(hr[k], p.head_w[t][k], acc);
                        acc = mt_wave_sum(acc);
                        if (p.gbias[t]) acc += p.gbias[t][0];
                        lg[t] = p.binary[t] ? 1.f / (1.f + expf(-acc)) : acc;
                    }
                }
                if (p.esmm) lg[1] = lg[0] * lg[1];
#pragma unroll
                for (int t = 0; t < MT_MAX_GATES; ++t)
                    if (t < p.E && lane == t) p.probs[t * p.probs_stride + b0 + r] = lg[t];
            }
        }
        __syncthreads();        // the slots are staged again for the next tile
    }
}

struct MxParams {
    int64_t batch;
    const float* h;
    int64_t h_stride;
    int32_t H, G, dz;
    const float* z[MX_MAX_GATES];
    int64_t z_stride[MX_MAX_GATES];
    const float* gk[MX_MAX_GATES];
    int32_t gn[MX_MAX_GATES], goff[MX_MAX_GATES];
    const int32_t* members;        // device
    float* out;                    // advanced to the first gate of this launch
    int64_t out_stride;
};

// one wave per row: per gate the logits twice (max and sum in one sweep, then the weights), the mixture accumulated in the row of `out`
// the wave owns — any n_g, any width, nothing kept per member
__global__ __launch_bounds__(MX_THREADS) void mtl_mix_kernel(MxParams p) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t)blockIdx.x * (MX_THREADS / 64) + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * (MX_THREADS / 64);
    for (int64_t r = wave0; r < p.batch; r += n_waves) {
        const float* hr = p.h + r * p.h_stride;
        for (int g = 0; g < p.G; ++g) {
            const float* zr = p.z[g] + r * p.z_stride[g];
            const float* W = p.gk[g];
            const int n = p.gn[g];
            const int32_t* mem = p.members + p.goff[g];
            float* o = p.out + r * p.out_stride + (int64_t)g * p.H;
            float m = -INFINITY, s = 0.f;
            for (int j = 0; j < n; ++j) {
                float l = 0.f;
                for (int k = lane; k < p.dz; k += 64) l = fmaf(zr[k], W[(int64_t)k * n + j], l);
                l = mt_wave_sum(l);
                const float m2 = fmaxf(m, l);
                s = s * expf(m - m2) + expf(l - m2);
                m = m2;
            }
            for (int j = 0; j < n; ++j) {
                float l = 0.f;
                for (int k = lane; k < p.dz; k += 64) l = fmaf(zr[k], W[(int64_t)k * n + j], l);
                l = mt_wave_sum(l);
                const float pj = expf(l - m) / s;
                const float* he = hr + (int64_t)mem[j] * p.H;
                for (int c = lane; c < p.H; c += 64) o[c] = fmaf(pj, he[c], j ? o[c] : 0.f);
            }
        }
    }
}

struct MtPlan {
    bool fused;
    int R, ldx, ldt, ldh, ldz, ldp, nT, n_members;
    size_t lds;
};

int mtl_check(const dctr_mtl_args_t* a, int kind, const char* op) {
    DCTR_REQUIRE(a, DCTR_E_NULL, "%s: null args", op);
    const bool level = kind == DCTR_MTL_LEVEL;
    DCTR_REQUIRE(a->batch >= 0 && a->n_slots >= 1 && a->n_slots <= (1 << 16) && a->in_dim >= 1 && a->in_dim <= (1 << 24) && a->n_experts >= 1 &&
                     a->n_experts <= (1 << 16) && a->n_layers >= (level ? 1 : 0) && a->n_layers <= 64, DCTR_E_DIM,
                 "%s: batch = %lld, n_slots = %d, in_dim = %d, n_experts = %d, n_layers = %d", op, (long long)a->batch, a->n_slots, a->in_dim,
                 a->n_experts, a->n_layers);
    DCTR_REQUIRE(a->x_offsets && a->expert_src && (a->n_layers == 0 || a->units), DCTR_E_NULL, "%s: null x_offsets / expert_src / units", op);
    for (int s = 0; s < a->n_slots; ++s)
        DCTR_REQUIRE(a->x_offsets[s] >= 0 && a->x_offsets[s] + a->in_dim <= a->x_stride, DCTR_E_DIM, "%s: slot %d: columns [%lld, %lld) in rows of %lld",
                     op, s, (long long)a->x_offsets[s], (long long)(a->x_offsets[s] + a->in_dim), (long long)a->x_stride);
    for (int l = 0; l < a->n_layers; ++l)
        DCTR_REQUIRE(a->units[l] >= 1 && a->units[l] <= (1 << 24), DCTR_E_DIM, "%s: units[%d] = %d", op, l, a->units[l]);
    for (int e = 0; e < a->n_experts; ++e)
        DCTR_REQUIRE(a->expert_src[e] >= 0 && a->expert_src[e] < a->n_slots, DCTR_E_DIM, "%s: expert_src[%d] = %d with %d slots", op, e,
                     a->expert_src[e], a->n_slots);
    DCTR_REQUIRE(a->activation >= DCTR_ACT_LINEAR && a->activation <= DCTR_ACT_DICE, DCTR_E_ENUM, "%s: unknown activation %d", op, a->activation);
    DCTR_REQUIRE(a->route >= DCTR_MTL_ROUTE_AUTO && a->route <= DCTR_MTL_ROUTE_LAYERED, DCTR_E_ENUM, "%s: unknown route %d", op, a->route);
    DCTR_REQUIRE(a->tile_rows == 0 || a->tile_rows == 16 || a->tile_rows == 32 || a->tile_rows == 64, DCTR_E_ENUM, "%s: tile_rows = %d", op,
                 a->tile_rows);
    if (level) {
        DCTR_REQUIRE(a->n_gates >= 1 && a->n_gates <= (1 << 16) && a->n_gate_layers >= 0 && a->n_gate_layers <= 64, DCTR_E_DIM,
                     "%s: n_gates = %d, n_gate_layers = %d", op, a->n_gates, a->n_gate_layers);
        DCTR_REQUIRE(a->gate_src && a->gate_n && a->members && (a->n_gate_layers == 0 || a->gate_units), DCTR_E_NULL,
                     "%s: null gate_src / gate_n / members / gate_units", op);
        for (int l = 0; l < a->n_gate_layers; ++l)
            DCTR_REQUIRE(a->gate_units[l] >= 1 && a->gate_units[l] <= (1 << 24), DCTR_E_DIM, "%s: gate_units[%d] = %d", op, l, a->gate_units[l]);
        int64_t off = 0;
        for (int g = 0; g < a->n_gates; ++g) {
            DCTR_REQUIRE(a->gate_src[g] >= 0 && a->gate_src[g] < a->n_slots, DCTR_E_DIM, "%s: gate_src[%d] = %d with %d slots", op, g,
                         a->gate_src[g], a->n_slots);
            DCTR_REQUIRE(a->gate_n[g] >= 1 && a->gate_n[g] <= (1 << 16), DCTR_E_DIM, "%s: gate_n[%d] = %d", op, g, a->gate_n[g]);
            for (int j = 0; j < a->gate_n[g]; ++j)
                DCTR_REQUIRE(a->members[off + j] >= 0 && a->members[off + j] < a->n_experts, DCTR_E_DIM,
                             "%s: gate %d: member %d = %d with %d experts", op, g, j, a->members[off + j], a->n_experts);
            off += a->gate_n[g];
        }
    } else {
        DCTR_REQUIRE(a->esmm == 0 || (a->esmm == 1 && a->n_experts == 2), DCTR_E_ENUM, "%s: esmm = %d with %d towers", op, a->esmm, a->n_experts);
    }
    return DCTR_OK;
}

void mtl_plan(const dctr_mtl_args_t* a, int kind, MtPlan* pl) {
    const bool level = kind == DCTR_MTL_LEVEL;
    const int S = a->n_slots, E = a->n_experts, L = a->n_layers, G = level ? a->n_gates : 0, Lg = level ? a->n_gate_layers : 0;
    *pl = MtPlan{};
    pl->R = 16;
    if (a->route == DCTR_MTL_ROUTE_LAYERED || a->activation == DCTR_ACT_DICE) return;
    if (S > MT_MAX_SLOTS || E > (level ? MT_MAX_EXPERTS : MT_MAX_GATES) || L > MT_MAX_DEPTH || E * L > MT_MAX_ELAYERS || G > MT_MAX_GATES ||
        Lg > MT_MAX_DEPTH || G * Lg > MT_MAX_GLAYERS)
        return;
    int n_members = 0;
    for (int g = 0; g < G; ++g) {
        if (a->gate_n[g] > MT_MAX_MEMBERS) return;
        n_members += a->gate_n[g];
    }
    if (n_members > MT_MAX_MEMBERS) return;
    int wt = 0;                                     // widest layer output that passes through the ping-pong tiles
    for (int l = 0; l + 1 < L; ++l) wt = a->units[l] > wt ? a->units[l] : wt;
    for (int l = 0; l + 1 < Lg; ++l) wt = a->gate_units[l] > wt ? a->gate_units[l] : wt;
    const int deepest = L > Lg ? L : Lg;
    pl->nT = deepest >= 3 ? 2 : deepest == 2 ? 1 : 0;
    const int64_t ldx = ((a->in_dim + 15) & ~15) + 4, ldt = pl->nT ? ((wt + 15) & ~15) + 4 : 0;
    const int64_t ldh = L ? ((a->units[L - 1] + 15) & ~15) + 4 : 0, ldz = Lg ? ((a->gate_units[Lg - 1] + 15) & ~15) + 4 : 0;
    const int64_t ldp = (n_members + 3) & ~3;
    const int64_t per_row = S * ldx + pl->nT * ldt + E * ldh + G * ldz + ldp;
    for (int R = 64; R >= 16; R >>= 1) {
        if (a->tile_rows && R > a->tile_rows) continue;
        const int64_t need = per_row * R * (int64_t)sizeof(float);
        if (need <= (int64_t)DCTR_LDS_MAX) {
            pl->fused = true;
            pl->R = R;
            pl->lds = (size_t)need;
            break;
        }
    }
    pl->ldx = (int)ldx, pl->ldt = (int)ldt, pl->ldh = (int)ldh, pl->ldz = (int)ldz, pl->ldp = (int)ldp, pl->n_members = n_members;
}

int mtl_fwd(const dctr_mtl_args_t* a, int kind, const char* op, void* stream) {
    int rc = mtl_check(a, kind, op);
    if (rc != DCTR_OK) return rc;
    MtPlan pl;
    mtl_plan(a, kind, &pl);
    DCTR_REQUIRE(pl.fused, DCTR_E_UNSUPPORTED, "%s: not on the fused route (dctr_mtl_route); the host runs the layered one", op);
    const bool level = kind == DCTR_MTL_LEVEL;
    const int E = a->n_experts, L = a->n_layers, G = level ? a->n_gates : 0, Lg = level ? a->n_gate_layers : 0;
    DCTR_REQUIRE(a->x && (L == 0 || (a->expert_w && a->expert_b)), DCTR_E_NULL, "%s: null x / expert_w / expert_b", op);
    DCTR_REQUIRE((a->expert_bn_scale == nullptr) == (a->expert_bn_shift == nullptr) && (a->gate_bn_scale == nullptr) == (a->gate_bn_shift == nullptr),
                 DCTR_E_NULL, "%s: bn_scale and bn_shift come together", op);
    bool aligned = true;
    for (int i = 0; i < E * L; ++i) {
        DCTR_REQUIRE(a->expert_w[i] && a->expert_b[i], DCTR_E_NULL, "%s: expert %d layer %d: null weight", op, i / L, i % L);
        DCTR_REQUIRE(!a->expert_bn_scale || ((a->expert_bn_scale[i] == nullptr) == (a->expert_bn_shift[i] == nullptr)), DCTR_E_NULL,
                     "%s: expert %d layer %d: bn_scale and bn_shift come together", op, i / L, i % L);
        aligned = aligned && dctr_aligned16(a->expert_w[i]);
    }
    if (level) {
        DCTR_REQUIRE(a->gate_kernel && (Lg == 0 || (a->gate_w && a->gate_b)) && a->out, DCTR_E_NULL, "%s: null gate_kernel / gate_w / gate_b / out", op);
        for (int g = 0; g < G; ++g) DCTR_REQUIRE(a->gate_kernel[g], DCTR_E_NULL, "%s: gate %d: null kernel", op, g);
        for (int i = 0; i < G * Lg; ++i) {
            DCTR_REQUIRE(a->gate_w[i] && a->gate_b[i], DCTR_E_NULL, "%s: gate %d layer %d: null weight", op, i / Lg, i % Lg);
            DCTR_REQUIRE(!a->gate_bn_scale || ((a->gate_bn_scale[i] == nullptr) == (a->gate_bn_shift[i] == nullptr)), DCTR_E_NULL,
                         "%s: gate %d layer %d: bn_scale and bn_shift come together", op, i / Lg, i % Lg);
            aligned = aligned && dctr_aligned16(a->gate_w[i]);
        }
        const int64_t width = (int64_t)G * a->units[L - 1];
        DCTR_REQUIRE(a->out_offset >= 0 && a->out_offset + width <= a->out_stride, DCTR_E_DIM, "%s: out columns [%lld, %lld) in rows of %lld", op,
                     (long long)a->out_offset, (long long)(a->out_offset + width), (long long)a->out_stride);
    } else {
        DCTR_REQUIRE(a->head_w && a->binary && a->probs, DCTR_E_NULL, "%s: null head_w / binary / probs", op);
        for (int t = 0; t < E; ++t) DCTR_REQUIRE(a->head_w[t], DCTR_E_NULL, "%s: tower %d: null head_w", op, t);
        DCTR_REQUIRE(a->probs_stride >= a->batch, DCTR_E_DIM, "%s: probs rows of %lld for %lld samples", op, (long long)a->probs_stride,
                     (long long)a->batch);
    }
    if (a->batch == 0) return DCTR_OK;
    // fewer tiles than compute units: smaller tiles spread the rows (the weights are re-read per tile either way)
    int R = pl.R;
    while (R > 16 && !a->tile_rows && dctr_ceil_div(a->batch, (int64_t)R) < dctr_n_cus()) R >>= 1;
    const size_t lds = pl.lds / pl.R * R;
    static thread_local size_t granted[DCTR_MAX_DEVICES] = {0};
    hipError_t e = dctr_grant_lds((const void*)mtl_kernel, lds, granted);
    DCTR_REQUIRE(e == hipSuccess, (int)e, "%s: cannot raise dynamic LDS: %s", op, hipGetErrorString(e));
    MtParams p = {};
    p.batch = a->batch;
    p.x = a->x;
    p.x_stride = a->x_stride;
    for (int s = 0; s < a->n_slots; ++s) p.x_off[s] = a->x_offsets[s];
    p.kind = kind, p.S = a->n_slots, p.Din = a->in_dim, p.E = E, p.L = L, p.G = G, p.Lg = Lg, p.act = a->activation, p.aligned = aligned;
    p.R = R, p.ldx = pl.ldx, p.ldt = pl.ldt, p.ldh = pl.ldh, p.ldz = pl.ldz, p.ldp = pl.ldp, p.nT = pl.nT;
    p.H = L ? a->units[L - 1] : a->in_dim;
    p.dz = Lg ? a->gate_units[Lg - 1] : a->in_dim;
    for (int l = 0; l < L; ++l) p.units[l] = a->units[l];
    for (int l = 0; l < Lg; ++l) p.gunits[l] = a->gate_units[l];
    for (int i = 0; i < E; ++i) p.esrc[i] = (uint8_t)a->expert_src[i];
    for (int i = 0; i < E * L; ++i)
        p.el[i] = MtLayer{a->expert_w[i], a->expert_b[i], a->expert_bn_scale ? a->expert_bn_scale[i] : nullptr,
                          a->expert_bn_scale ? a->expert_bn_shift[i] : nullptr};
    if (level) {
        int off = 0;
        for (int g = 0; g < G; ++g) {
            p.gsrc[g] = (uint8_t)a->gate_src[g];
            p.gn[g] = (uint8_t)a->gate_n[g];
            p.goff[g] = (uint8_t)off;
            p.gk[g] = a->gate_kernel[g];
            for (int j = 0; j < a->gate_n[g]; ++j) p.members[off + j] = (uint8_t)a->members[off + j];
            off += a->gate_n[g];
        }
        for (int i = 0; i < G * Lg; ++i)
            p.gl[i] = MtLayer{a->gate_w[i], a->gate_b[i], a->gate_bn_scale ? a->gate_bn_scale[i] : nullptr,
                              a->gate_bn_scale ? a->gate_bn_shift[i] : nullptr};
        p.out = a->out + a->out_offset;
        p.out_stride = a->out_stride;
    } else {
        for (int t = 0; t < E; ++t) {
            p.head_w[t] = a->head_w[t];
            p.gbias[t] = a->global_bias ? a->global_bias[t] : nullptr;
            p.binary[t] = (uint8_t)(a->binary[t] != 0);
        }
        p.esmm = a->esmm;
        p.probs = a->probs;
        p.probs_stride = a->probs_stride;
    }
    const int64_t n_tiles = dctr_ceil_div(a->batch, (int64_t)R), cap = 4 * (int64_t)dctr_n_cus();
    const dim3 grid((unsigned)(n_tiles < cap ? n_tiles : cap)), block(MT_THREADS);
    DCTR_LAUNCH(mtl_kernel, grid, block, lds, (hipStream_t)stream, p);
    return dctr_launch_status(op);
}

}  // namespace

extern "C" int dctr_mtl_route(const dctr_mtl_args_t* a, int32_t kind) {
    DCTR_REQUIRE(kind == DCTR_MTL_LEVEL || kind == DCTR_MTL_TOWERS, DCTR_E_ENUM, "mtl_route: unknown kind %d", kind);
    int rc = mtl_check(a, kind, "mtl_route");
    if (rc != DCTR_OK) return rc;
    MtPlan pl;
    mtl_plan(a, kind, &pl);
    return pl.fused ? DCTR_MTL_ROUTE_FUSED : DCTR_MTL_ROUTE_LAYERED;
}

extern "C" int dctr_mtl_level_fwd(const dctr_mtl_args_t* a, void* stream) { return mtl_fwd(a, DCTR_MTL_LEVEL, "mtl_level_fwd", stream); }

extern "C" int dctr_mtl_towers_fwd(const dctr_mtl_args_t* a, void* stream) { return mtl_fwd(a, DCTR_MTL_TOWERS, "mtl_towers_fwd", stream); }

extern "C" int dctr_mtl_mix(const dctr_mtl_mix_args_t* a, void* stream) {
    DCTR_REQUIRE(a, DCTR_E_NULL, "mtl_mix: null args");
    DCTR_REQUIRE(a->batch >= 0 && a->n_experts >= 1 && a->n_experts <= (1 << 16) && a->width >= 1 && a->width <= (1 << 24) && a->n_gates >= 1 &&
                     a->n_gates <= (1 << 16) && a->z_dim >= 1 && a->z_dim <= (1 << 24), DCTR_E_DIM,
                 "mtl_mix: batch = %lld, n_experts = %d, width = %d, n_gates = %d, z_dim = %d", (long long)a->batch, a->n_experts, a->width,
                 a->n_gates, a->z_dim);
    DCTR_REQUIRE(a->h && a->z && a->z_stride && a->gate_kernel && a->gate_n && a->members && a->members_dev && a->out, DCTR_E_NULL,
                 "mtl_mix: null h / z / z_stride / gate_kernel / gate_n / members / members_dev / out");
    const int64_t EH = (int64_t)a->n_experts * a->width, GH = (int64_t)a->n_gates * a->width;
    DCTR_REQUIRE(a->h_stride >= EH && a->out_offset >= 0 && a->out_offset + GH <= a->out_stride, DCTR_E_DIM,
                 "mtl_mix: h rows of %lld for %lld columns, out columns [%lld, %lld) in rows of %lld", (long long)a->h_stride, (long long)EH,
                 (long long)a->out_offset, (long long)(a->out_offset + GH), (long long)a->out_stride);
    int64_t off = 0;
    for (int g = 0; g < a->n_gates; ++g) {
        DCTR_REQUIRE(a->z[g] && a->gate_kernel[g], DCTR_E_NULL, "mtl_mix: gate %d: null input / kernel", g);
        DCTR_REQUIRE(a->z_stride[g] >= a->z_dim, DCTR_E_DIM, "mtl_mix: gate %d: input rows of %lld for %d columns", g, (long long)a->z_stride[g],
                     a->z_dim);
        DCTR_REQUIRE(a->gate_n[g] >= 1 && a->gate_n[g] <= (1 << 16), DCTR_E_DIM, "mtl_mix: gate_n[%d] = %d", g, a->gate_n[g]);
        for (int j = 0; j < a->gate_n[g]; ++j)
            DCTR_REQUIRE(a->members[off + j] >= 0 && a->members[off + j] < a->n_experts, DCTR_E_DIM,
                         "mtl_mix: gate %d: member %d = %d with %d experts", g, j, a->members[off + j], a->n_experts);
        off += a->gate_n[g];
    }
    if (a->batch == 0) return DCTR_OK;
    const int64_t blocks = dctr_ceil_div(a->batch, (int64_t)(MX_THREADS / 64)), cap = 16 * (int64_t)dctr_n_cus();
    const dim3 grid((unsigned)(blocks < cap ? blocks : cap)), block(MX_THREADS);
    off = 0;
    for (int g0 = 0; g0 < a->n_gates; g0 += MX_MAX_GATES) {
        MxParams p = {};
        p.batch = a->batch, p.h = a->h, p.h_stride = a->h_stride, p.H = a->width, p.dz = a->z_dim;
        p.G = a->n_gates - g0 < MX_MAX_GATES ? a->n_gates - g0 : MX_MAX_GATES;
        p.members = a->members_dev;
        for (int g = 0; g < p.G; ++g) {
            p.z[g] = a->z[g0 + g], p.z_stride[g] = a->z_stride[g0 + g], p.gk[g] = a->gate_kernel[g0 + g];
            p.gn[g] = a->gate_n[g0 + g];
            p.goff[g] = (int32_t)off;
            off += a->gate_n[g0 + g];
        }
        p.out = a->out + a->out_offset + (int64_t)g0 * a->width;
        p.out_stride = a->out_stride;
        DCTR_LAUNCH(mtl_mix_kernel, grid, block, 0, (hipStream_t)stream, p);
        int rc = dctr_launch_status("dctr_mtl_mix");
        if (rc != DCTR_OK) return rc;
    }
    return DCTR_OK;
}
