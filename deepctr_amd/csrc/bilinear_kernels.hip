// SENETLayer.call + BilinearInteraction.call (reference deepctr/layers/interaction.py:1067-1221), wired as FiBiNET wires them
// (models/fibinet.py:50-58): the whole DNN input [Flatten(concat([senet_bilinear, bilinear])), dense] in one launch.  concat_func
// joins the two [P, E] outputs on the LAST axis, so a row holds per pair p the SENET-side E floats, then the raw-side E floats.
//
// Reference per sample: Z = mean_E(x) [F]; A1 = relu(Z W_1) [r]; A2 = relu(A1 W_2) [F]; v_f = A2[f] x_f.  Then for each pair
// (i < j, itertools.combinations order) p_ij = (v_i W_ij) * v_j over the SENET output and (x_i W'_ij) * x_j over the raw
// embeddings (elementwise products), W chosen by bilinear_type (all: one W; each: W_i; interaction: W_ij).
//
// A2[f] is a scalar per field, so (v_i W) * v_j = A2[i] A2[j] ((x_i W) * x_j): the reweighted embeddings never exist and both
// layers share the A operand x_i.  A workgroup owns a tile of 16 samples, their embeddings X [F][16][ldx] in LDS:
//   * SENET: Z, A1, A2 per sample by plain FMAs (2 F r FLOP per matrix);
//   * all / each: V_b[i] = X_i W_b(i) once per field (i < F-1, both layers) on v_mfma_f32_16x16x4_f32 (rows = the 16 samples,
//     K padded to 16 with zeros, W streamed from L2 in its Keras layout) — exact fp32, k-ordered;
//   * the pairs, in chunks of NP: interaction: X_i W_ij for both layers on the same MFMA, two pairs x two layers per wave task so
//     that sixteen weight loads are in flight at once; all / each: V_b[i] read back.  The epilogue multiplies by x_j (and by
//     A2[i] A2[j] on the SENET side) into a staging buffer [16][NP 2E]; the chunk then leaves as one contiguous run of 2*NP*E
//     floats per sample — the kernel is bound by its stores;
//   * the D dense columns behind x in the DNN input are copied behind the two blocks.
// A sample too large for the LDS (large F*E) takes the same kernel with those buffers in a per-workgroup slice of the workspace
// (the general route: <= 256 persistent workgroups): nothing is refused for its size.
#include <math.h>
#include "dctr_common.h"
#include "mfma_tile.h"
#include "pair_index.h"
#include "tile_route.h"

namespace {

constexpr int BL_THREADS = 512;                // 8 waves: one pair task per wave and chunk at the Criteo shape
constexpr int BL_S = 16;                        // samples per tile = the rows of one MFMA tile
constexpr int BL_CHUNK = 256;                   // output floats per sample and layer staged per chunk of pairs

struct BlParams {
    const float* x;
    int64_t batch;
    int64_t x_stride;
    int32_t F, E, type, D;
    int32_t nblk;                // bilinear layers written: 2 (model), 1 (one layer), 0 (the SENET output only)
    int32_t senet;               // A2 scales block 0 (model) or is applied to x (SENET only)
    int32_t r;                   // columns of W_1 (0 without SENET)
    int32_t ldx, NP, ldo, nV;
    int64_t P;
    int64_t tile_floats;
    const float* w1;
    const float* w2;
    const float* const* wt[2];   // DEVICE tables of the weight matrices: block 0 (SENET side, or the one layer), block 1
    float* out;
    int64_t out_stride;
    float* ws;                   // general route only
};

// offsets (floats) of a tile's buffers behind X: V, A2, Z, A1, the staging buffer, the chunk's pair table (int pairs) and its
// weight pointers (two per pair, 8-B aligned)
struct BlLayout {
    int64_t v, a2, z, a1, st, pij, wp, total;
};

__host__ __device__ inline BlLayout bl_layout(int F, int ldx, int nV, int r, int ldo, int NP) {
    BlLayout L;
    int64_t o = (int64_t)F * BL_S * ldx;
    L.v = o;
    o += (int64_t)nV * BL_S * ldx;
    L.a2 = o;
    o += (int64_t)BL_S * F;
    L.z = o;
    o += (int64_t)BL_S * F;
    L.a1 = o;
    o += (int64_t)BL_S * r;
    L.st = o;
    o += (int64_t)BL_S * ldo;
    L.pij = o;
    o += 2 * (int64_t)NP;
    L.wp = (o + 1) & ~(int64_t)1;
    o = L.wp + 4 * (int64_t)NP;
    L.total = (o + 3) & ~(int64_t)3;
    return L;
}

// acc[q][b] += A_q [16 x E] W_qb [E x 16 columns], q, b < 2.  arow[q]: this lane's A row (sample lane & 15) at its k-slot
// (k = g*KQ + t, mfma_tile.h); wcol[q][b]: this lane's weight column.  Rows k >= E are clamped: A is zero there.
__device__ __forceinline__ void bl_tiles(const float* arow[2], const float* wcol[2][2], int E, int KQ, dctr::f32x4 (&acc)[2][2]) {
    const int g = (threadIdx.x & 63) >> 4, k_last = E - 1;
    for (int t0 = 0; t0 < KQ; t0 += 4) {
        float av[2][4], bv[2][2][4];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const float4 a4 = *reinterpret_cast<const float4*>(arow[q] + t0);
            av[q][0] = a4.x;
            av[q][1] = a4.y;
            av[q][2] = a4.z;
            av[q][3] = a4.w;
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) bv[q][b][tt] = wcol[q][b][(int64_t)min(g * KQ + t0 + tt, k_last) * E];
        }
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int tt = 0; tt < 4; ++tt)
                    acc[q][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[q][tt], bv[q][b][tt], acc[q][b], 0, 0, 0);
    }
}

template <bool GLOBAL_WS>
__global__ __launch_bounds__(BL_THREADS) void bilinear_kernel(BlParams p) {
    extern __shared__ __attribute__((aligned(16))) float bl_lds[];
    float* X = GLOBAL_WS ? p.ws + (int64_t)blockIdx.x * p.tile_floats : bl_lds;
    const int F = p.F, E = p.E, ldx = p.ldx, ldo = p.ldo, nblk = p.nblk, r = p.r;
    const BlLayout L = bl_layout(F, ldx, p.nV, r, ldo, p.NP);
    float* V = X + L.v;
    float* A2 = X + L.a2;
    float* Z = X + L.z;
    float* A1 = X + L.a1;
    float* St = X + L.st;
    int* pij = reinterpret_cast<int*>(X + L.pij);
    const float** wp = reinterpret_cast<const float**>(X + L.wp);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, jl = lane & 15;
    const int fs = BL_S * ldx;                  // floats between two fields of X / V
    const int KQ = ((E + 15) & ~15) >> 2, CT = (E + 15) >> 4;
    const int FE = F * E;
    const bool via_v = p.nV > 0;
    const int64_t n_tiles = (p.batch + BL_S - 1) / BL_S;

    // the K padding of X (columns E .. ldx-1) stays zero: the MFMA reads it against clamped weight rows
    const int padc = ldx - E;
    for (int e = tid; e < F * BL_S * padc; e += BL_THREADS) {
        const int row = e / padc;
        X[row * ldx + E + (e - row * padc)] = 0.f;
    }

    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t b0 = tile * BL_S;
        const int nvalid = (int)min((int64_t)BL_S, p.batch - b0);
        for (int s = wave; s < BL_S; s += BL_THREADS / 64) {
            if (s < nvalid) {
                const float* xr = p.x + (b0 + s) * p.x_stride;
                for (int e = lane; e < FE; e += 64) {
                    const int f = e / E;
                    X[f * fs + s * ldx + (e - f * E)] = xr[e];
                }
            } else {
                for (int e = lane; e < FE; e += 64) {
                    const int f = e / E;
                    X[f * fs + s * ldx + (e - f * E)] = 0.f;
                }
            }
        }
        __syncthreads();

        if (p.senet) {
            for (int e = tid; e < BL_S * F; e += BL_THREADS) {
                const int s = e / F, f = e - s * F;
                const float* xr = X + f * fs + s * ldx;
                float z = 0.f;
                for (int c = 0; c < E; ++c) z += xr[c];
                Z[e] = z / (float)E;
            }
            __syncthreads();
            for (int e = tid; e < BL_S * r; e += BL_THREADS) {
                const int s = e / r, k = e - s * r;
                float a = 0.f;
                for (int f = 0; f < F; ++f) a = fmaf(Z[s * F + f], p.w1[(int64_t)f * r + k], a);
                A1[e] = fmaxf(a, 0.f);
            }
            __syncthreads();
            for (int e = tid; e < BL_S * F; e += BL_THREADS) {
                const int s = e / F, f = e - s * F;
                float a = 0.f;
                for (int k = 0; k < r; ++k) a = fmaf(A1[s * r + k], p.w2[(int64_t)k * F + f], a);
                A2[e] = fmaxf(a, 0.f);
            }
            __syncthreads();
            if (nblk == 0) {                    // the SENET output only: the reweighted embeddings, F*E per sample
                for (int s = wave; s < nvalid; s += BL_THREADS / 64) {
                    float* o = p.out + (b0 + s) * p.out_stride;
                    for (int e = lane; e < FE; e += 64) {
                        const int f = e / E;
                        o[e] = X[f * fs + s * ldx + (e - f * E)] * A2[s * F + f];
                    }
                }
                __syncthreads();
                continue;
            }
        }

        if (via_v) {                            // all / each: V_b[i] = X_i W_b(i), i < F-1, two fields per wave task
            const int nf = F - 1;
            for (int t = wave; t < ((nf + 1) >> 1) * CT; t += BL_THREADS / 64) {
                const int fq = t / CT, ct = t - fq * CT;
                const int col = ct * 16 + jl, n0 = min(col, E - 1);
                int fi[2];
                const float* arow[2];
                const float* wcol[2][2];
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    fi[q] = min(2 * fq + q, nf - 1);
                    arow[q] = X + fi[q] * fs + jl * ldx + g * KQ;
                    const int wi = p.type == DCTR_BILINEAR_ALL ? 0 : fi[q];
#pragma unroll
                    for (int b = 0; b < 2; ++b) wcol[q][b] = p.wt[b < nblk ? b : 0][wi] + n0;
                }
                dctr::f32x4 acc[2][2] = {};
                bl_tiles(arow, wcol, E, KQ, acc);
                if (col < E) {
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        if (2 * fq + q >= nf) continue;
                        for (int b = 0; b < nblk; ++b) {
                            float* v = V + (b * nf + fi[q]) * fs + col;
#pragma unroll
                            for (int rr = 0; rr < 4; ++rr) v[(4 * g + rr) * ldx] = acc[q][b][rr];
                        }
                    }
                }
            }
            // (the first chunk's barrier below orders these writes before the pair phase reads them)
        }

        for (int64_t q0 = 0; q0 < p.P; q0 += p.NP) {
            const int np = (int)min((int64_t)p.NP, p.P - q0);
            const int blen = np * nblk * E;
            // the chunk's pairs and (interaction) their weight pointers: one table load per pair and chunk, not per wave task
            for (int t = tid; t < np; t += BL_THREADS) {
                dctr::pair_at(q0 + t, F, &pij[2 * t], &pij[2 * t + 1]);
                if (!via_v) {
                    wp[2 * t] = p.wt[0][q0 + t];
                    wp[2 * t + 1] = p.wt[nblk > 1 ? 1 : 0][q0 + t];
                }
            }
            __syncthreads();
            for (int t = wave; t < ((np + 1) >> 1) * CT; t += BL_THREADS / 64) {
                const int pq = t / CT, ct = t - pq * CT;
                const int col = ct * 16 + jl, n0 = min(col, E - 1);
                int pp[2], pi[2], pj[2];
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    pp[q] = min(2 * pq + q, np - 1);
                    pi[q] = pij[2 * pp[q]];
                    pj[q] = pij[2 * pp[q] + 1];
                }
                dctr::f32x4 acc[2][2] = {};
                if (!via_v) {                   // interaction: X_i W_ij, both layers
                    const float* arow[2];
                    const float* wcol[2][2];
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        arow[q] = X + pi[q] * fs + jl * ldx + g * KQ;
#pragma unroll
                        for (int b = 0; b < 2; ++b) wcol[q][b] = wp[2 * pp[q] + b] + n0;
                    }
                    bl_tiles(arow, wcol, E, KQ, acc);
                } else if (col < E) {
#pragma unroll
                    for (int q = 0; q < 2; ++q)
#pragma unroll
                        for (int b = 0; b < 2; ++b) {
                            const float* v = V + ((b < nblk ? b : 0) * (F - 1) + pi[q]) * fs + col;
#pragma unroll
                            for (int rr = 0; rr < 4; ++rr) acc[q][b][rr] = v[(4 * g + rr) * ldx];
                        }
                }
                if (col < E) {
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        if (2 * pq + q >= np) continue;
#pragma unroll
                        for (int rr = 0; rr < 4; ++rr) {
                            const int s = 4 * g + rr;
                            const float xj = X[pj[q] * fs + s * ldx + col];
                            float* st = St + s * ldo + pp[q] * nblk * E + col;
                            float v0 = acc[q][0][rr] * xj;
                            if (p.senet) v0 *= A2[s * F + pi[q]] * A2[s * F + pj[q]];
                            st[0] = v0;
                            if (nblk > 1) st[E] = acc[q][1][rr] * xj;
                        }
                    }
                }
            }
            __syncthreads();
            // the chunk leaves: one run of np*nblk*E floats per sample
            for (int s = wave; s < nvalid; s += BL_THREADS / 64) {
                float* o = p.out + (b0 + s) * p.out_stride + q0 * nblk * E;
                const float* st = St + s * ldo;
                for (int c = lane; c < blen; c += 64) o[c] = st[c];
            }
            // (the next chunk's barrier keeps its staging writes behind these reads)
        }
        if (p.D > 0) {                          // the dense tail of the DNN input
            for (int s = wave; s < nvalid; s += BL_THREADS / 64) {
                const float* xr = p.x + (b0 + s) * p.x_stride + FE;
                float* o = p.out + (b0 + s) * p.out_stride + (int64_t)nblk * p.P * E;
                for (int c = lane; c < p.D; c += 64) o[c] = xr[c];
            }
        }
        __syncthreads();    // X and the staging buffer are rewritten by the next tile
    }
}

struct BlPlan {
    bool global;            // the general route (buffers in the workspace)
    int nblk, senet, r, ldx, NP, ldo, nV;
    int64_t P, tile_floats;
    int grid_max;           // general route: workgroups the workspace has slices for
    size_t route_bytes;     // workspace of the general route (0 on the LDS route)
};

void bl_plan(const dctr_bilinear_args_t* a, BlPlan* pl) {
    const int F = a->fields, E = a->dim;
    pl->nblk = a->mode == DCTR_BILINEAR_MODE_SENET ? 0 : a->mode == DCTR_BILINEAR_MODE_LAYER ? 1 : 2;
    pl->senet = a->mode != DCTR_BILINEAR_MODE_LAYER;
    pl->r = pl->senet ? a->reduction_size : 0;
    pl->P = (int64_t)F * (F - 1) / 2;
    pl->ldx = ((E + 15) & ~15) + 4;
    int64_t np = BL_CHUNK / E > 1 ? BL_CHUNK / E : 1;
    if (np > pl->P) np = pl->P;
    pl->NP = pl->nblk ? (int)np : 0;
    pl->ldo = pl->nblk ? pl->nblk * pl->NP * E + 4 : 0;
    pl->nV = pl->nblk && a->bilinear_type != DCTR_BILINEAR_INTERACTION ? pl->nblk * (F - 1) : 0;
    pl->tile_floats = bl_layout(F, pl->ldx, pl->nV, pl->r, pl->ldo, pl->NP).total;
    const dctr_tile_route r = dctr_plan_tile_route((size_t)pl->tile_floats * sizeof(float));
    pl->global = r.global;
    pl->grid_max = r.grid_max;
    pl->route_bytes = r.route_bytes;
}

int bl_check(const dctr_bilinear_args_t* a) {
    DCTR_REQUIRE(a, DCTR_E_NULL, "bilinear_fwd: null args");
    DCTR_REQUIRE(a->fields >= 2, DCTR_E_DIM, "bilinear_fwd: fields = %d: the layers need at least 2 fields", a->fields);
    DCTR_REQUIRE(a->bilinear_type >= DCTR_BILINEAR_ALL && a->bilinear_type <= DCTR_BILINEAR_INTERACTION, DCTR_E_ENUM,
                 "bilinear_fwd: unknown bilinear_type %d", a->bilinear_type);
    DCTR_REQUIRE(a->mode >= DCTR_BILINEAR_MODE_MODEL && a->mode <= DCTR_BILINEAR_MODE_LAYER, DCTR_E_ENUM, "bilinear_fwd: unknown mode %d",
                 a->mode);
    DCTR_REQUIRE(a->dim >= 1 && a->batch >= 0 && a->dense_cols >= 0, DCTR_E_DIM, "bilinear_fwd: bad sizes");
    DCTR_REQUIRE(a->mode == DCTR_BILINEAR_MODE_LAYER || a->reduction_size >= 1, DCTR_E_DIM, "bilinear_fwd: reduction_size must be >= 1");
    DCTR_REQUIRE(a->mode == DCTR_BILINEAR_MODE_MODEL || a->dense_cols == 0, DCTR_E_DIM,
                 "bilinear_fwd: dense_cols are copied in the model mode only");
    // a tile's buffers are indexed in 32 bits, the pairs of a row in 31
    DCTR_REQUIRE(a->fields <= 65536 && a->dim <= (1 << 20) && a->reduction_size <= (1 << 20) &&
                     (int64_t)a->fields * BL_S * ((int64_t)a->dim + 20) * 3 < 0x7fffffffLL,
                 DCTR_E_DIM, "bilinear_fwd: one tile's buffers exceed 2^31 floats");
    const int64_t F = a->fields, E = a->dim, P = F * (F - 1) / 2;
    const int64_t in_w = F * E + (a->mode == DCTR_BILINEAR_MODE_MODEL ? a->dense_cols : 0);
    const int64_t out_w = a->mode == DCTR_BILINEAR_MODE_SENET ? F * E : a->mode == DCTR_BILINEAR_MODE_LAYER ? P * E : 2 * P * E + a->dense_cols;
    DCTR_REQUIRE(a->x_stride >= in_w, DCTR_E_DIM, "bilinear_fwd: x_stride %lld < %lld", (long long)a->x_stride, (long long)in_w);
    DCTR_REQUIRE(a->out_stride >= out_w, DCTR_E_DIM, "bilinear_fwd: out_stride %lld < %lld", (long long)a->out_stride,
                 (long long)out_w);
    return DCTR_OK;
}

}  // namespace

extern "C" size_t dctr_bilinear_workspace_bytes(const dctr_bilinear_args_t* args) {
    if (bl_check(args) != DCTR_OK) return 0;
    BlPlan pl;
    bl_plan(args, &pl);
    return pl.route_bytes;
}

extern "C" int dctr_bilinear_fwd(const dctr_bilinear_args_t* a, void* stream) {
    int rc = bl_check(a);
    if (rc != DCTR_OK) return rc;
    BlPlan pl;
    bl_plan(a, &pl);
    DCTR_REQUIRE(a->x && a->out, DCTR_E_NULL, "bilinear_fwd: null x / out");
    DCTR_REQUIRE(!pl.senet || (a->senet_w1 && a->senet_w2), DCTR_E_NULL, "bilinear_fwd: null senet_w1 / senet_w2");
    DCTR_REQUIRE(pl.nblk == 0 || a->bilinear_w, DCTR_E_NULL, "bilinear_fwd: null bilinear_w");
    DCTR_REQUIRE(pl.nblk < 2 || a->senet_bilinear_w, DCTR_E_NULL, "bilinear_fwd: null senet_bilinear_w");
    if (a->batch == 0) return DCTR_OK;
    if (pl.route_bytes)
        DCTR_REQUIRE_WORKSPACE("bilinear_fwd", "dctr_bilinear_workspace_bytes", a->workspace, a->workspace_bytes, pl.route_bytes);
    BlParams p = {};
    p.x = a->x;
    p.batch = a->batch;
    p.x_stride = a->x_stride;
    p.F = a->fields;
    p.E = a->dim;
    p.type = a->bilinear_type;
    p.D = a->mode == DCTR_BILINEAR_MODE_MODEL ? a->dense_cols : 0;
    p.nblk = pl.nblk;
    p.senet = pl.senet;
    p.r = pl.r;
    p.ldx = pl.ldx;
    p.NP = pl.NP;
    p.ldo = pl.ldo;
    p.nV = pl.nV;
    p.P = pl.P;
    p.tile_floats = pl.tile_floats;
    p.w1 = a->senet_w1;
    p.w2 = a->senet_w2;
    p.wt[0] = pl.nblk == 2 ? a->senet_bilinear_w : a->bilinear_w;
    p.wt[1] = a->bilinear_w;
    p.out = a->out;
    p.out_stride = a->out_stride;
    p.ws = pl.global ? (float*)a->workspace : nullptr;
    const int64_t n_tiles = dctr_ceil_div(a->batch, BL_S);
    if (pl.global) {
        const int64_t grid = n_tiles < pl.grid_max ? n_tiles : pl.grid_max;
        DCTR_LAUNCH(bilinear_kernel<true>, dim3((unsigned)grid), dim3(BL_THREADS), 0, (hipStream_t)stream, p);
    } else {
        const size_t lds = (size_t)pl.tile_floats * sizeof(float);
        static thread_local size_t granted[DCTR_MAX_DEVICES] = {0};
        hipError_t e = dctr_grant_lds((const void*)bilinear_kernel<false>, lds, granted);
        DCTR_REQUIRE(e == hipSuccess, (int)e, "bilinear_fwd: cannot raise dynamic LDS: %s", hipGetErrorString(e));
        const int64_t grid = n_tiles < (1 << 24) ? n_tiles : (1 << 24);
        DCTR_LAUNCH(bilinear_kernel<false>, dim3((unsigned)grid), dim3(BL_THREADS), lds, (hipStream_t)stream, p);
    }
    return dctr_launch_status("dctr_bilinear_fwd");
}
