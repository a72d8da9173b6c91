// FwFMLayer.call and FEFMLayer.call (reference deepctr/layers/interaction.py:1351-1499): a weight per field pair applied to the
// pair's embeddings and reduced over the embedding axis — P = F(F-1)/2 scalars per sample (FEFM) or one logit (FwFM).
//
// FEFM, per sample and pair (i < j, itertools.combinations order): s_ij = x_i^T S_ij x_j with S_ij = W_ij + W_ij^T formed here from
// the live W_ij (the per-pair tensors stay the real weights; the kernel gets a device table of their addresses).  A workgroup owns a
// tile of 16*M samples (M = 1 or 2 sub-tiles of 16), their embeddings X [F][16 M][ldx] in LDS.  S is symmetric, so the product is
// taken TRANSPOSED on v_mfma_f32_16x16x4_f32:  T^T = S X_i^T  — A operand = S (rows = the output column c, read from L2: the row part
// W[c][k..k+3] as one 16-B load, the column part W[k][c] as four 4-B loads that are contiguous across the lanes), B operand = X_i^T
// (k-major, one ds_read_b128 of the sample's row).  In the 16x16 C layout a lane then holds T[s = lane & 15][c = 4g .. 4g+3]: the
// epilogue T (.) x_j is four FMAs against one more ds_read_b128, and the sum over the E columns is a sum over g, taken as one more
// MFMA against ones (B[k = g][s] = the lane's partial sum): no 16-lane reduction, and nothing crosses lanes through the LDS.
// One set of weight registers serves the M sub-tiles, which divides the weight traffic from L2 (P E^2 floats per tile: 333 KB at the
// Criteo shape) by M; the next pair group's weights are loaded before the current group's MFMAs so that the L2 round trip is
// covered — this kernel has no store stream to hide it behind.  The scalars of a chunk of NP pairs wait in a
// staging buffer [16 M][NP] and leave as one contiguous run per sample; the row sums (the FEFM logit) are kept in registers per
// wave, joined through LDS, and leave with the optional `add` vector folded in.
// X rows are stored without padding, the 16-B chunks of a row XOR-swizzled by (s >> 1) & 3: both ds_read_b128 patterns (row s =
// lane & 15, chunk g) are then bank-conflict free in the lane groups gfx950 serves a b128 read in.
//
// FwFM: logit = sum_{i<j} r_ij <x_i, x_j> = sum_e sum_i x_i[e] (sum_{j>i} r_ij x_j[e]): 2 F^2 E / 2 FLOP per sample, plain FMAs over
// the same kind of LDS tile (a thread per (sample, e mod 16)), r read through the scalar cache.  Only r[i][j], i < j is read.
//
// A tile too large for the LDS (large F*E) takes the same kernels with the tile in a per-workgroup slice of the workspace (the general
// route: <= 256 persistent workgroups): nothing is refused for its size.
#include <math.h>
#include <stdint.h>
#include "dctr_common.h"
#include "fieldpair_device.h"
#include "mfma_tile.h"
#include "pair_index.h"
#include "tile_route.h"

namespace {

using dctr::fp_gptr;
using dctr::fp_xoff;

constexpr int FP_THREADS = 512;                // 8 waves
constexpr int FP_WAVES = FP_THREADS / 64;
constexpr int FP_Q = 2;                         // pairs per wave task: 2 x M independent accumulators, 10 weight loads in flight
constexpr int FP_NP = 128;                      // pairs per chunk (staging buffer and pair table)
constexpr int FW_THREADS = 256;                 // FwFM: 16 samples x 16 e-lanes

struct FpParams {
    const float* x;              // already advanced by x_offset
    int64_t batch;
    int64_t x_stride;
    int32_t F, E;
    int32_t ldx, NP, ldo;
    int64_t P;
    int64_t tile_floats;
    const float* const* wt;      // FEFM: DEVICE table of the P matrices
    const float* r;              // FwFM: [F, F]
    float* pairs;                // already advanced by pairs_offset (or null)
    int64_t pairs_stride;
    const float* add;
    float* logit;
    float* ws;                   // general route only
};

// offsets (floats) of a FEFM tile's buffers behind X: the staging buffer, the waves' partial row sums, the chunk's pair table (int
// pairs) and its weight pointers (8-B aligned)
struct FpLayout {
    int64_t st, lg, pij, wp, total;
};

__host__ __device__ inline FpLayout fp_layout(int F, int S, int ldx, int ldo, int NP, bool pairs) {
    FpLayout L;
    int64_t o = (int64_t)F * S * ldx;
    L.st = o;
    o += pairs ? (int64_t)S * ldo : 0;
    L.lg = o;
    o += (int64_t)FP_WAVES * S;
    L.pij = o;
    o += 2 * (int64_t)NP;
    L.wp = (o + 1) & ~(int64_t)1;
    o = L.wp + 2 * (int64_t)NP;
    L.total = (o + 3) & ~(int64_t)3;
    return L;
}

__device__ __forceinline__ float fp_dot4(const dctr::f32x4& a, const float4& b) {
    return fmaf(a[3], b.w, fmaf(a[2], b.z, fmaf(a[1], b.y, a[0] * b.x)));
}

using FpRaw = dctr::FpRaw<FP_Q>;

template <bool GLOBAL_WS, int M>
__global__ __launch_bounds__(FP_THREADS) void fefm_kernel(FpParams p) {
    extern __shared__ __attribute__((aligned(16))) float fp_lds[];
    constexpr int S = 16 * M;
    float* X = GLOBAL_WS ? p.ws + (int64_t)blockIdx.x * p.tile_floats : fp_lds;
    const int F = p.F, E = p.E, ldx = p.ldx, ldo = p.ldo;
    const bool has_pairs = p.pairs != nullptr;
    const FpLayout L = fp_layout(F, S, ldx, ldo, p.NP, has_pairs);
    float* St = X + L.st;
    float* Lg = X + L.lg;
    int* pij = reinterpret_cast<int*>(X + L.pij);
    const float** wp = reinterpret_cast<const float**>(X + L.wp);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, jl = lane & 15;
    const int fs = S * ldx;                     // floats between two fields of X
    const int KQ = ldx >> 2, CT = ldx >> 4;     // ldx = E rounded up to 16
    const int FE = F * E;
    const bool small = ldx == 16, vec = (E & 3) == 0;
    const bool one_chunk = p.P <= p.NP;
    const int64_t n_tiles = (p.batch + S - 1) / S;

    // the K padding of X (columns E .. ldx-1) stays zero: the MFMA reads it against clamped weight rows and columns
    const int padc = ldx - E;
    for (int e = tid; e < F * S * padc; e += FP_THREADS) {
        const int row = e / padc, k = E + (e - row * padc);
        const int f = row / S, s = row - f * S;
        X[f * fs + fp_xoff(s, k >> 2, ldx) + (k & 3)] = 0.f;
    }
    if (one_chunk) {                            // the pair table does not depend on the tile
        for (int t = tid; t < (int)p.P; t += FP_THREADS) {
            dctr::pair_at(t, F, &pij[2 * t], &pij[2 * t + 1]);
            wp[t] = p.wt[t];
        }
    }

    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t b0 = tile * S;
        const int nvalid = (int)min((int64_t)S, p.batch - b0);
        for (int s = wave; s < S; s += FP_WAVES) {
            const float* xr = p.x + (b0 + min(s, nvalid - 1)) * p.x_stride;
            for (int e = lane; e < FE; e += 64) {
                const int f = e / E, k = e - f * E;
                X[f * fs + fp_xoff(s, k >> 2, ldx) + (k & 3)] = s < nvalid ? xr[e] : 0.f;      // rows past the batch hold zeros
            }
        }
        float lsum[M];
#pragma unroll
        for (int m = 0; m < M; ++m) lsum[m] = 0.f;

        for (int64_t q0 = 0; q0 < p.P; q0 += p.NP) {
            const int np = (int)min((int64_t)p.NP, p.P - q0);
            if (!one_chunk) {
                for (int t = tid; t < np; t += FP_THREADS) {
                    dctr::pair_at(q0 + t, F, &pij[2 * t], &pij[2 * t + 1]);
                    wp[t] = p.wt[q0 + t];
                }
            }
            __syncthreads();                    // X (first chunk), the table; the previous chunk's staging reads are done
            const int ng = (np + FP_Q - 1) / FP_Q;
            if (small) {
                FpRaw cur = {}, nxt = {};
                if (wave < ng) dctr::fp_load_small(wp, wave * FP_Q, np, E, vec, cur);
                for (int t = wave; t < ng; t += FP_WAVES) {
                    if (t + FP_WAVES < ng) dctr::fp_load_small(wp, (t + FP_WAVES) * FP_Q, np, E, vec, nxt);
                    int pp[FP_Q], pi[FP_Q], pj[FP_Q];
                    dctr::f32x4 acc[FP_Q][M];
#pragma unroll
                    for (int q = 0; q < FP_Q; ++q) {
                        pp[q] = min(t * FP_Q + q, np - 1);
                        pi[q] = pij[2 * pp[q]];
                        pj[q] = pij[2 * pp[q] + 1];
#pragma unroll
                        for (int m = 0; m < M; ++m) acc[q][m] = dctr::f32x4{0.f, 0.f, 0.f, 0.f};
                    }
                    float4 xi[FP_Q][M];
                    float a[FP_Q][4];
#pragma unroll
                    for (int q = 0; q < FP_Q; ++q) {
#pragma unroll
                        for (int tt = 0; tt < 4; ++tt) a[q][tt] = cur.row[q][tt] + cur.col[q][tt];
#pragma unroll
                        for (int m = 0; m < M; ++m)
                            xi[q][m] = *reinterpret_cast<const float4*>(X + pi[q] * fs + fp_xoff(m * 16 + jl, g, 16));
                    }
                    // k-step outermost: FP_Q * M independent accumulators between two MFMAs that depend on each other
#pragma unroll
                    for (int tt = 0; tt < 4; ++tt)
#pragma unroll
                        for (int q = 0; q < FP_Q; ++q)
#pragma unroll
                            for (int m = 0; m < M; ++m) {
                                const float b = tt == 0 ? xi[q][m].x : tt == 1 ? xi[q][m].y : tt == 2 ? xi[q][m].z : xi[q][m].w;
                                acc[q][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q][tt], b, acc[q][m], 0, 0, 0);
                            }
                    // T (.) x_j over this lane's four columns, then the sum over g as one more MFMA against ones (B[k = g][s] = the
                    // lane's partial sum): every lane of column s receives the pair's scalar, and no value crosses lanes through LDS
                    dctr::f32x4 red[FP_Q][M];
#pragma unroll
                    for (int q = 0; q < FP_Q; ++q)
#pragma unroll
                        for (int m = 0; m < M; ++m) {
                            const float4 xj = *reinterpret_cast<const float4*>(X + pj[q] * fs + fp_xoff(m * 16 + jl, g, 16));
                            red[q][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(1.f, fp_dot4(acc[q][m], xj), dctr::f32x4{0.f, 0.f, 0.f, 0.f}, 0,
                                                                             0, 0);
                        }
#pragma unroll
                    for (int q = 0; q < FP_Q; ++q) {
                        if (t * FP_Q + q >= np) continue;
#pragma unroll
                        for (int m = 0; m < M; ++m) {
                            const float v = red[q][m][0];
                            lsum[m] += v;
                            if (has_pairs && g == (m & 3)) St[(m * 16 + jl) * ldo + pp[q]] = v;
                        }
                    }
                    cur = nxt;
                }
            } else {                            // E > 16: CT column tiles, K in KQ steps; one pair per wave task
                for (int t = wave; t < np; t += FP_WAVES) {
                    const int pi = pij[2 * t], pj = pij[2 * t + 1];
                    const fp_gptr w = (fp_gptr)wp[t];
                    float part[M];
#pragma unroll
                    for (int m = 0; m < M; ++m) part[m] = 0.f;
                    for (int ct = 0; ct < CT; ++ct) {
                        const int64_t c = min(ct * 16 + jl, E - 1);
                        dctr::f32x4 acc[M];
#pragma unroll
                        for (int m = 0; m < M; ++m) acc[m] = dctr::f32x4{0.f, 0.f, 0.f, 0.f};
                        for (int t0 = 0; t0 < KQ; t0 += 4) {
                            float a[4];
#pragma unroll
                            for (int tt = 0; tt < 4; ++tt) {
                                const int64_t k = min(g * KQ + t0 + tt, E - 1);
                                a[tt] = w[c * E + k] + w[k * E + c];
                            }
#pragma unroll
                            for (int m = 0; m < M; ++m) {
                                const float4 xi =
                                    *reinterpret_cast<const float4*>(X + pi * fs + fp_xoff(m * 16 + jl, (g * KQ + t0) >> 2, ldx));
                                acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], xi.x, acc[m], 0, 0, 0);
                                acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], xi.y, acc[m], 0, 0, 0);
                                acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2], xi.z, acc[m], 0, 0, 0);
                                acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3], xi.w, acc[m], 0, 0, 0);
                            }
                        }
#pragma unroll
                        for (int m = 0; m < M; ++m) {
                            const float4 xj = *reinterpret_cast<const float4*>(X + pj * fs + fp_xoff(m * 16 + jl, ct * 4 + g, ldx));
                            part[m] += fp_dot4(acc[m], xj);
                        }
                    }
#pragma unroll
                    for (int m = 0; m < M; ++m) {
                        const float v = __builtin_amdgcn_mfma_f32_16x16x4f32(1.f, part[m], dctr::f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0)[0];
                        lsum[m] += v;
                        if (has_pairs && g == (m & 3)) St[(m * 16 + jl) * ldo + t] = v;
                    }
                }
            }
            if (has_pairs || !one_chunk) __syncthreads();      // the staging buffer is complete; the pair table may be rewritten
            if (has_pairs) {
                // the chunk leaves: one run of np floats per sample
                for (int s = wave; s < nvalid; s += FP_WAVES) {
                    float* o = p.pairs + (b0 + s) * p.pairs_stride + q0;
                    const float* st = St + s * ldo;
                    for (int c = lane; c < np; c += 64) o[c] = st[c];
                }
            }
        }
        if (p.logit) {
#pragma unroll
            for (int m = 0; m < M; ++m)
                if (g == (m & 3)) Lg[wave * S + m * 16 + jl] = lsum[m];
            __syncthreads();
            if (tid < nvalid) {
                float v = 0.f;
#pragma unroll
                for (int w = 0; w < FP_WAVES; ++w) v += Lg[w * S + tid];
                if (p.add) v += p.add[b0 + tid];
                p.logit[b0 + tid] = v;
            }
        }
        __syncthreads();    // X, the staging buffer and the partial sums are rewritten by the next tile
    }
}

// FwFM: 16 samples per tile, X [F][16][E] in LDS (or the workspace); thread (s = tid >> 4, e = tid & 15 (+16, ...))
template <bool GLOBAL_WS>
__global__ __launch_bounds__(FW_THREADS) void fwfm_kernel(FpParams p) {
    extern __shared__ __attribute__((aligned(16))) float fp_lds[];
    float* X = GLOBAL_WS ? p.ws + (int64_t)blockIdx.x * p.tile_floats : fp_lds;
    const int F = p.F, E = p.E, fs = 16 * E, FE = F * E;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, s = tid >> 4, e0 = tid & 15;
    const int64_t n_tiles = (p.batch + 15) / 16;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t b0 = tile * 16;
        const int nvalid = (int)min((int64_t)16, p.batch - b0);
        for (int r = wave; r < nvalid; r += FW_THREADS / 64) {
            const float* xr = p.x + (b0 + r) * p.x_stride;
            for (int e = lane; e < FE; e += 64) {
                const int f = e / E;
                X[f * fs + r * E + (e - f * E)] = xr[e];
            }
        }
        __syncthreads();
        float acc = 0.f;
        if (s < nvalid) {
            for (int e = e0; e < E; e += 16) {
                const float* xs = X + s * E + e;
                for (int i = 0; i < F - 1; ++i) {
                    const float* ri = p.r + (int64_t)i * F;
                    float inner = 0.f;
                    for (int j = i + 1; j < F; ++j) inner = fmaf(ri[j], xs[j * fs], inner);
                    acc = fmaf(xs[i * fs], inner, acc);
                }
            }
        }
        acc += __shfl_xor(acc, 8);
        acc += __shfl_xor(acc, 4);
        acc += __shfl_xor(acc, 2);
        acc += __shfl_xor(acc, 1);
        if (e0 == 0 && s < nvalid) p.logit[b0 + s] = acc + (p.add ? p.add[b0 + s] : 0.f);
        __syncthreads();    // X is rewritten by the next tile
    }
}

struct FpPlan {
    bool global;            // the general route (the tile in the workspace)
    int M;                  // FEFM: sub-tiles of 16 samples per workgroup
    int ldx, NP, ldo;
    int64_t P, tile_floats;
    int grid_max;           // general route: workgroups the workspace has slices for
    size_t route_bytes;     // workspace of the general route (0 on the LDS route)
};

int64_t fp_tile_floats(const dctr_fieldpair_args_t* a, const FpPlan* pl, int M) {
    if (a->kind == DCTR_FIELDPAIR_FWFM) return ((int64_t)a->fields * 16 * a->dim + 3) & ~(int64_t)3;
    return fp_layout(a->fields, 16 * M, pl->ldx, pl->ldo, pl->NP, a->pairs_out != nullptr).total;
}

void fp_plan(const dctr_fieldpair_args_t* a, FpPlan* pl) {
    const int F = a->fields, E = a->dim;
    pl->P = (int64_t)F * (F - 1) / 2;
    pl->ldx = (E + 15) & ~15;
    pl->NP = (int)(pl->P < FP_NP ? pl->P : FP_NP);
    pl->ldo = pl->NP | 1;                       // odd: the 16 samples of a sub-tile write one pair's scalars to 16 banks
    // more samples per workgroup = fewer weight reads from L2, as long as the grid still fills the chip.  Measured at the Criteo shape,
    // 65,536 rows: M = 2 (two workgroups per CU) 0.24 ms, M = 4 (one per CU: its phases overlap with nothing) 0.29, M = 1 0.30
    int M = a->kind == DCTR_FIELDPAIR_FWFM ? 1 : a->batch >= 32 * 256 ? 2 : 1;
    while (M > 1 && (size_t)fp_tile_floats(a, pl, M) * sizeof(float) > DCTR_LDS_MAX) M >>= 1;
    pl->M = M;
    pl->tile_floats = fp_tile_floats(a, pl, M);
    const dctr_tile_route r = dctr_plan_tile_route((size_t)pl->tile_floats * sizeof(float));
    pl->global = r.global;
    pl->grid_max = r.grid_max;
    pl->route_bytes = r.route_bytes;
}

int fp_check(const dctr_fieldpair_args_t* a) {
    DCTR_REQUIRE(a, DCTR_E_NULL, "fieldpair_fwd: null args");
    DCTR_REQUIRE(a->kind == DCTR_FIELDPAIR_FEFM || a->kind == DCTR_FIELDPAIR_FWFM, DCTR_E_ENUM, "fieldpair_fwd: unknown kind %d", a->kind);
    DCTR_REQUIRE(a->fields >= 2, DCTR_E_DIM, "fieldpair_fwd: fields = %d: a field pair needs at least 2 fields", a->fields);
    DCTR_REQUIRE(a->dim >= 1 && a->batch >= 0 && a->x_offset >= 0 && a->pairs_offset >= 0, DCTR_E_DIM, "fieldpair_fwd: bad sizes");
    // a tile's buffers are indexed in 32 bits
    DCTR_REQUIRE(a->fields <= 65536 && a->dim <= (1 << 20) && (int64_t)a->fields * 64 * ((int64_t)a->dim + 16) < 0x3fffffffLL, DCTR_E_DIM,
                 "fieldpair_fwd: one tile's buffers exceed 2^30 floats");
    const int64_t F = a->fields, E = a->dim, P = F * (F - 1) / 2;
    DCTR_REQUIRE(a->x_stride >= a->x_offset + F * E, DCTR_E_DIM, "fieldpair_fwd: x_stride %lld < x_offset + fields*dim = %lld",
                 (long long)a->x_stride, (long long)(a->x_offset + F * E));
    DCTR_REQUIRE(a->kind == DCTR_FIELDPAIR_FEFM || !a->pairs_out, DCTR_E_DIM, "fieldpair_fwd: the FwFM kind has no pairs_out");
    DCTR_REQUIRE(!a->pairs_out || a->pairs_stride >= a->pairs_offset + P, DCTR_E_DIM,
                 "fieldpair_fwd: pairs_stride %lld < pairs_offset + P = %lld", (long long)a->pairs_stride,
                 (long long)(a->pairs_offset + P));
    return DCTR_OK;
}

}  // namespace

extern "C" size_t dctr_fieldpair_workspace_bytes(const dctr_fieldpair_args_t* args) {
    if (fp_check(args) != DCTR_OK) return 0;
    FpPlan pl;
    fp_plan(args, &pl);
    return pl.route_bytes;
}

extern "C" int dctr_fieldpair_fwd(const dctr_fieldpair_args_t* a, void* stream) {
    int rc = fp_check(a);
    if (rc != DCTR_OK) return rc;
    FpPlan pl;
    fp_plan(a, &pl);
    DCTR_REQUIRE(a->x && a->weights, DCTR_E_NULL, "fieldpair_fwd: null x / weights");
    DCTR_REQUIRE(a->kind == DCTR_FIELDPAIR_FEFM ? (a->pairs_out || a->logit_out) : a->logit_out != nullptr, DCTR_E_NULL,
                 "fieldpair_fwd: no output (pairs_out / logit_out)");
    if (pl.route_bytes)
        DCTR_REQUIRE_WORKSPACE("fieldpair_fwd", "dctr_fieldpair_workspace_bytes", a->workspace, a->workspace_bytes, pl.route_bytes);
    if (a->batch == 0) return DCTR_OK;
    FpParams p = {};
    p.x = a->x + a->x_offset;
    p.batch = a->batch;
    p.x_stride = a->x_stride;
    p.F = a->fields;
    p.E = a->dim;
    p.ldx = pl.ldx;
    p.NP = pl.NP;
    p.ldo = pl.ldo;
    p.P = pl.P;
    p.tile_floats = pl.tile_floats;
    p.pairs = a->pairs_out ? a->pairs_out + a->pairs_offset : nullptr;
    p.pairs_stride = a->pairs_stride;
    p.add = a->add;
    p.logit = a->logit_out;
    p.ws = pl.global ? (float*)a->workspace : nullptr;
    const bool fwfm = a->kind == DCTR_FIELDPAIR_FWFM;
    if (fwfm)
        p.r = (const float*)a->weights;
    else
        p.wt = (const float* const*)a->weights;
    const int64_t n_tiles = dctr_ceil_div(a->batch, (int64_t)16 * pl.M);
    const hipStream_t st = (hipStream_t)stream;
    if (pl.global) {
        const int64_t grid = n_tiles < pl.grid_max ? n_tiles : pl.grid_max;
        if (fwfm)
            DCTR_LAUNCH(fwfm_kernel<true>, dim3((unsigned)grid), dim3(FW_THREADS), 0, st, p);
        else
            DCTR_LAUNCH((fefm_kernel<true, 1>), dim3((unsigned)grid), dim3(FP_THREADS), 0, st, p);
    } else {
        const size_t lds = (size_t)pl.tile_floats * sizeof(float);
        const int64_t grid = n_tiles < (1 << 24) ? n_tiles : (1 << 24);
        static thread_local size_t granted[3][DCTR_MAX_DEVICES] = {{0}};
        const void* fn = fwfm      ? (const void*)fwfm_kernel<false>
                         : pl.M == 2 ? (const void*)fefm_kernel<false, 2>
                                     : (const void*)fefm_kernel<false, 1>;
        hipError_t e = dctr_grant_lds(fn, lds, granted[fwfm ? 2 : pl.M >> 1]);
        DCTR_REQUIRE(e == hipSuccess, (int)e, "fieldpair_fwd: cannot raise dynamic LDS: %s", hipGetErrorString(e));
        if (fwfm)
            DCTR_LAUNCH(fwfm_kernel<false>, dim3((unsigned)grid), dim3(FW_THREADS), lds, st, p);
        else if (pl.M == 2)
            DCTR_LAUNCH((fefm_kernel<false, 2>), dim3((unsigned)grid), dim3(FP_THREADS), lds, st, p);
        else
            DCTR_LAUNCH((fefm_kernel<false, 1>), dim3((unsigned)grid), dim3(FP_THREADS), lds, st, p);
    }
    return dctr_launch_status("dctr_fieldpair_fwd");
}
