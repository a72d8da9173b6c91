// The backward of FEFMLayer.call / FwFMLayer.call (dctr_fieldpair_fwd, fieldpair_kernels.hip), one launch.  The forward saves
// nothing: a workgroup loads the same X tile [F][16 M][ldx] with the forward's LDS layout and swizzle (fieldpair_device.h), and the
// gradients of its samples.
//
// FEFM, with g_b,ij = d_pairs[b, ij] + d_logit[b] and S_ij = W_ij + W_ij^T (the matrix of the pair (min, max)):
//   dx_i = sum_{j != i} g_ij S_ij x_j.  A wave task owns field i of the tile and chains every j != i into ONE accumulator per 16-sample
//        sub-tile: dx_i^T = sum_j S_ij (g_ij (.) X_j)^T on v_mfma_f32_16x16x4_f32, A = S formed in registers from the live W exactly as
//        the forward forms it (next j's weights are loaded before this j's MFMAs), B = the X_j rows scaled by g.  One owner per (sample,
//        field, column): no atomics, dx is bit-identical from call to call.
//   dW_ij = A + A^T with A = sum_b g_b,ij x_i x_j^T: per pair (g (.) X_i)^T X_j, an E x E result with K = the samples.  A wave owns
//        FB_NPW pairs of a chunk of FB_NP = 8 FB_NPW pairs and keeps their 16 x 16 sums in registers across ALL tiles the workgroup
//        walks; then each sum is symmetrised once through a per-wave LDS patch and leaves with one float atomic per element and
//        workgroup (so weight gradients may differ in the last bits from call to call).  More than FB_NP pairs: the workgroup walks its
//        tiles once per chunk (X is loaded again; dx is taken in the first walk): FB_NP = 168, two walks for the 325 pairs of 26
//        fields.  Up to 26 fields the tile's g [16 M][P] stays whole in LDS, so that the dx product reads it on chip; past that (1,770
//        pairs of 60 fields) the tile holds one chunk's g and the dx product reads d_pairs / d_logit from HBM.
//   E > 16 takes column tiles as the forward does; its E x E sums are too many for registers, so that path adds each tile's A to dW and
//   to dW^T directly (two atomics per element and TILE).  E no multiple of 4, or matrices off 16 B, take 4-B weight loads.
// FwFM: a vector kernel, 16 samples x 16 e-lanes per tile as in the forward.  dx_i = d_logit sum_{j != i} r'_ij x_j (r' = the strict
//   upper triangle mirrored); dr_ij = sum_b d_logit_b <x_i, x_j> for i < j is summed per workgroup in an [F, F] patch behind the tile,
//   a thread per cell, and leaves with one atomic per cell and workgroup.  The diagonal and the lower triangle are not touched.
// A tile too large for the LDS runs in a per-workgroup slice of the workspace (the forward's general route).
#include <math.h>
#include <stdint.h>
#include "dctr_common.h"
#include "fieldpair_device.h"
#include "mfma_tile.h"
#include "pair_index.h"
#include "tile_route.h"

namespace {

using dctr::fp_gptr;
using dctr::fp_xel;
using dctr::fp_xoff;
using dctr::pair_row_start;

constexpr int FB_THREADS = 512;                 // 8 waves
constexpr int FB_WAVES = FB_THREADS / 64;
constexpr int FB_NPW = 21;                      // pairs per wave and chunk: 21 x 4 accumulator registers (more spill: the kernel
                                                // already sits at the 256 registers two waves per SIMD leave a wave)
constexpr int FB_NP = FB_WAVES * FB_NPW;        // pairs per chunk
// row pitch of a tile's g: one chunk, or all pairs of up to 26 fields.  Compile-time constants: the dW loop's LDS addresses are then a
// per-lane base plus an immediate and nothing per pair is kept in registers (odd: 16 samples read 16 banks)
constexpr int FB_LDG = FB_NP | 1;
constexpr int FB_LDG_FULL = 329;
constexpr int FB_TLD = 17;                      // row pitch of a wave's 16 x 16 transpose patch
constexpr int FWB_THREADS = 256;                // FwFM: 16 samples x 16 e-lanes

struct FbParams {
    const float* x;              // already advanced by x_offset
    int64_t batch;
    int64_t x_stride;
    int32_t F, E;
    int32_t ldx, NP, ldg;
    int64_t P;
    int64_t tile_floats;
    const float* const* wt;      // FEFM: DEVICE table of the P matrices
    const float* r;              // FwFM: [F, F]
    const float* dp;             // already advanced by d_pairs_offset (or null)
    int64_t dp_stride;
    const float* dl;             // [batch] (or null)
    float* dx;                   // already advanced by dx_offset (or null)
    int64_t dx_stride;
    int32_t accumulate;
    float* dw;                   // FEFM [P, E, E]; FwFM [F, F] (or null)
    float* ws;                   // general route only
};

// offsets (floats) of a FEFM tile's buffers behind X: the chunk's g [S][ldg], the waves' transpose patches, the chunk's pair table
// (int pairs) and its weight pointers (8-B aligned)
struct FbLayout {
    int64_t g, t, pij, wp, total;
};

__host__ __device__ inline FbLayout fb_layout(int F, int S, int ldx, int ldg, int NP) {
    FbLayout L;
    int64_t o = (int64_t)F * S * ldx;
    L.g = o;
    o += (int64_t)S * ldg + FB_WAVES;              // (+ a tail: the dW loop reads g of up to 7 pairs past the chunk's last)
    L.t = o;
    o += (int64_t)FB_WAVES * 16 * FB_TLD;
    const int64_t NPa = ((int64_t)NP + FB_WAVES - 1) & ~(int64_t)(FB_WAVES - 1);
    L.pij = o;
    o += 2 * NPa;
    L.wp = (o + 1) & ~(int64_t)1;
    o = L.wp + 2 * NPa;
    L.total = (o + 3) & ~(int64_t)3;
    return L;
}

using FbRaw = dctr::FpRaw<1>;

// the forward's weight fetch for one pair
__device__ __forceinline__ void fb_load_small(const float* w, int E, bool vec, FbRaw& raw) { dctr::fp_load_small(&w, 0, 1, E, vec, raw); }

// GFULL: the tile's g holds all P pairs (pitch FB_LDG_FULL), not one chunk (pitch FB_LDG)
template <bool GLOBAL_WS, int M, bool GFULL>
__global__ __launch_bounds__(FB_THREADS) void fefm_bwd_kernel(FbParams p) {
    extern __shared__ __attribute__((aligned(16))) float fb_lds[];
    constexpr int S = 16 * M;
    float* X = GLOBAL_WS ? p.ws + (int64_t)blockIdx.x * p.tile_floats : fb_lds;
    const int F = p.F, E = p.E, ldx = p.ldx;
    constexpr int ldg = GFULL ? FB_LDG_FULL : FB_LDG;
    const FbLayout L = fb_layout(F, S, ldx, ldg, p.NP);
    float* G = X + L.g;
    float* Tw = X + L.t + (threadIdx.x >> 6) * 16 * FB_TLD;
    int* pij = reinterpret_cast<int*>(X + L.pij);
    const float** wp = reinterpret_cast<const float**>(X + L.wp);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, jl = lane & 15;
    const int fs = S * ldx;                     // floats between two fields of X
    const int KQ = ldx >> 2, CT = ldx >> 4;     // ldx = E rounded up to 16
    const int FE = F * E;
    const bool small = ldx == 16, vec = (E & 3) == 0;
    const bool one_chunk = p.P <= p.NP;
    const bool gfull = GFULL, gall = gfull || one_chunk;      // gall: the dx product finds every pair's g in the tile
    const int64_t n_tiles = (p.batch + S - 1) / S;
    const bool dx_vec = vec && (((uintptr_t)p.dx | (uintptr_t)(p.dx_stride * 4)) & 15) == 0;

    // the K padding of X (columns E .. ldx-1) stays zero: the MFMAs read it against clamped weight rows and columns
    const int padc = ldx - E;
    for (int e = tid; e < F * S * padc; e += FB_THREADS) {
        const int row = e / padc, k = E + (e - row * padc);
        const int f = row / S, s = row - f * S;
        X[f * fs + fp_xel(s, k, ldx)] = 0.f;
    }

    for (int64_t q0 = 0; q0 < p.P; q0 += p.NP) {
        if (q0 > 0 && !p.dw) break;             // dx is complete after the first walk
        const int np = (int)min((int64_t)p.NP, p.P - q0);
        __syncthreads();                        // the previous chunk's table is no longer read
        // (the table runs to a multiple of 8 pairs, the tail repeating the last pair: every wave of the dW loop finds fields there)
        for (int t = tid; t < ((np + FB_WAVES - 1) & ~(FB_WAVES - 1)); t += FB_THREADS) {
            const int64_t pt = min(q0 + t, p.P - 1);
            dctr::pair_at(pt, F, &pij[2 * t], &pij[2 * t + 1]);
            wp[t] = p.wt[pt];
        }
        dctr::f32x4 acc[FB_NPW];
#pragma unroll
        for (int q = 0; q < FB_NPW; ++q) acc[q] = dctr::f32x4{0.f, 0.f, 0.f, 0.f};

        for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
            const int64_t b0 = tile * S;
            const int nvalid = (int)min((int64_t)S, p.batch - b0);
            __syncthreads();                    // the previous tile is no longer read
            for (int s = wave; s < S; s += FB_WAVES) {
                const bool on = s < nvalid;     // rows past the batch hold zeros, and so do their g
                const int64_t b = b0 + min(s, nvalid - 1);
                const float* xr = p.x + b * p.x_stride;
                for (int e = lane; e < FE; e += 64) {
                    const int f = e / E, k = e - f * E;
                    X[f * fs + fp_xel(s, k, ldx)] = on ? xr[e] : 0.f;
                }
                const float gl = on && p.dl ? p.dl[b] : 0.f;
                const float* dr = p.dp ? p.dp + b * p.dp_stride + (gfull ? 0 : q0) : nullptr;
                const int gn = gfull ? (int)p.P : np;
                for (int c = lane; c < gn; c += 64) G[s * ldg + c] = on ? (dr ? dr[c] : 0.f) + gl : 0.f;
            }
            __syncthreads();

            // ---- dx: a wave task = field i, all j != i chained into one accumulator per sub-tile and column tile
            if (q0 == 0 && p.dx) {
                for (int i = wave; i < F; i += FB_WAVES) {
                    for (int ct = 0; ct < CT; ++ct) {
                        dctr::f32x4 dacc[M];
#pragma unroll
                        for (int m = 0; m < M; ++m) dacc[m] = dctr::f32x4{0.f, 0.f, 0.f, 0.f};
                        FbRaw cur = {}, nxt = {};
                        const int jfirst = i == 0 ? 1 : 0;
                        if (small) {
                            const int64_t pf = i == 0 ? 0 : pair_row_start(0, F) + i - 1;
                            fb_load_small(one_chunk ? wp[pf] : p.wt[pf], E, vec, cur);
                        }
                        for (int j = jfirst; j < F; ++j) {
                            if (j == i) continue;
                            const int lo = min(i, j), hi = max(i, j);
                            const int64_t pidx = pair_row_start(lo, F) + hi - lo - 1;
                            float gv[M];
#pragma unroll
                            for (int m = 0; m < M; ++m) {
                                const int s = m * 16 + jl;
                                if (gall)
                                    gv[m] = G[s * ldg + (int)pidx];
                                else if (s < nvalid)
                                    gv[m] = (p.dp ? p.dp[(b0 + s) * p.dp_stride + pidx] : 0.f) + (p.dl ? p.dl[b0 + s] : 0.f);
                                else
                                    gv[m] = 0.f;
                            }
                            if (small) {
                                int jn = j + 1;
                                if (jn == i) ++jn;
                                if (jn < F) {
                                    const int ln = min(i, jn), hn = max(i, jn);
                                    const int64_t pn = pair_row_start(ln, F) + hn - ln - 1;
                                    fb_load_small(one_chunk ? wp[pn] : p.wt[pn], E, vec, nxt);
                                }
                                float a[4];
#pragma unroll
                                for (int tt = 0; tt < 4; ++tt) a[tt] = cur.row[0][tt] + cur.col[0][tt];
                                float4 xj[M];
#pragma unroll
                                for (int m = 0; m < M; ++m) xj[m] = *reinterpret_cast<const float4*>(X + j * fs + fp_xoff(m * 16 + jl, g, 16));
#pragma unroll
                                for (int tt = 0; tt < 4; ++tt)
#pragma unroll
                                    for (int m = 0; m < M; ++m) {
                                        const float b = (tt == 0 ? xj[m].x : tt == 1 ? xj[m].y : tt == 2 ? xj[m].z : xj[m].w) * gv[m];
                                        dacc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[tt], b, dacc[m], 0, 0, 0);
                                    }
                                cur = nxt;
                            } else {
                                const fp_gptr w = (fp_gptr)(one_chunk ? wp[pidx] : p.wt[pidx]);
                                const int64_t c = min(ct * 16 + jl, E - 1);
                                for (int t0 = 0; t0 < KQ; t0 += 4) {
                                    float a[4];
#pragma unroll
                                    for (int tt = 0; tt < 4; ++tt) {
                                        const int64_t k = min(g * KQ + t0 + tt, E - 1);
                                        a[tt] = w[c * E + k] + w[k * E + c];
                                    }
#pragma unroll
                                    for (int m = 0; m < M; ++m) {
                                        const float4 xj =
                                            *reinterpret_cast<const float4*>(X + j * fs + fp_xoff(m * 16 + jl, (g * KQ + t0) >> 2, ldx));
                                        dacc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], xj.x * gv[m], dacc[m], 0, 0, 0);
                                        dacc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], xj.y * gv[m], dacc[m], 0, 0, 0);
                                        dacc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2], xj.z * gv[m], dacc[m], 0, 0, 0);
                                        dacc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3], xj.w * gv[m], dacc[m], 0, 0, 0);
                                    }
                                }
                            }
                        }
                        // the lane holds dx_i[s = jl][c = ct*16 + 4g .. + 3] of each sub-tile
#pragma unroll
                        for (int m = 0; m < M; ++m) {
                            const int s = m * 16 + jl, c0 = ct * 16 + 4 * g;
                            if (s >= nvalid || c0 >= E) continue;
                            float* o = p.dx + (b0 + s) * p.dx_stride + (int64_t)i * E + c0;
                            if (dx_vec) {
                                float4 v = make_float4(dacc[m][0], dacc[m][1], dacc[m][2], dacc[m][3]);
                                if (p.accumulate) {
                                    const float4 old = *reinterpret_cast<const float4*>(o);
                                    v.x += old.x; v.y += old.y; v.z += old.z; v.w += old.w;
                                }
                                *reinterpret_cast<float4*>(o) = v;
                            } else {
#pragma unroll
                                for (int r = 0; r < 4; ++r)
                                    if (c0 + r < E) o[r] = p.accumulate ? o[r] + dacc[m][r] : dacc[m][r];
                            }
                        }
                    }
                }
            }

            // ---- dW: (g (.) X_i)^T X_j per pair, K = the tile's samples (k-slot g of MFMA kk = sample 4 kk + g)
            if (p.dw) {
                const int gq = gfull ? (int)q0 : 0;     // the chunk's first column in G
                if (small) {
                    // (every address is a per-lane base plus a compile-time offset in q: nothing per pair stays in registers)
                    const int* pw = pij + 2 * wave;
                    const float* gw = G + g * ldg + wave + gq;
#pragma unroll
                    for (int q = 0; q < FB_NPW; ++q) {
                        if (q * FB_WAVES >= np) break;      // (a pair past np sums into registers that never leave)
                        const float* xi = X + pw[2 * FB_WAVES * q] * fs;
                        const float* xj = X + pw[2 * FB_WAVES * q + 1] * fs;
#pragma unroll
                        for (int kk = 0; kk < 4 * M; ++kk) {
                            const int o = fp_xel(4 * kk + g, jl, 16);
                            acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32((gw + 4 * kk * ldg)[FB_WAVES * q] * xi[o], xj[o], acc[q], 0, 0, 0);
                        }
                    }
                } else {
                    for (int pl = wave; pl < np; pl += FB_WAVES) {
                        const float* xi = X + pij[2 * pl] * fs;
                        const float* xj = X + pij[2 * pl + 1] * fs;
                        float* dst = p.dw + (q0 + pl) * (int64_t)E * E;
                        for (int et = 0; et < CT; ++et)
                            for (int ct = 0; ct < CT; ++ct) {
                                dctr::f32x4 a = dctr::f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                                for (int kk = 0; kk < 4 * M; ++kk) {
                                    const int s = 4 * kk + g;
                                    a = __builtin_amdgcn_mfma_f32_16x16x4f32(G[s * ldg + gq + pl] * xi[fp_xel(s, et * 16 + jl, ldx)],
                                                                             xj[fp_xel(s, ct * 16 + jl, ldx)], a, 0, 0, 0);
                                }
                                const int c = ct * 16 + jl;
#pragma unroll
                                for (int r = 0; r < 4; ++r) {
                                    const int e = et * 16 + 4 * g + r;
                                    if (e < E && c < E) {
                                        atomicAdd(dst + (int64_t)e * E + c, a[r]);
                                        atomicAdd(dst + (int64_t)c * E + e, a[r]);
                                    }
                                }
                            }
                    }
                }
            }
        }

        // the chunk's sums leave: A + A^T through the wave's patch, one atomic per element
        if (p.dw && small) {
#pragma unroll
            for (int q = 0; q < FB_NPW; ++q) {
                const int pl = q * FB_WAVES + wave;
                if (q * FB_WAVES >= np) break;  // (the same for every wave: the barriers below stay uniform)
                if (pl < np) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) Tw[(4 * g + r) * FB_TLD + jl] = acc[q][r];
                }
                __syncthreads();
                if (pl < np) {
                    float* dst = p.dw + (q0 + pl) * (int64_t)E * E;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int e = 4 * g + r;
                        if (e < E && jl < E) atomicAdd(dst + e * E + jl, Tw[e * FB_TLD + jl] + Tw[jl * FB_TLD + e]);
                    }
                }
                __syncthreads();
            }
        }
    }
}

// FwFM: 16 samples per tile, X [F][16][E] in LDS (or the workspace), behind it the workgroup's [F, F] sums and the tile's d_logit.
// Fields sit 16 E + 1 floats apart: the threads of the dr sum read the same (sample, e) of different fields j, which 16 E apart
// (a multiple of the banks at E = 16) would all meet in one bank.
template <bool GLOBAL_WS>
__global__ __launch_bounds__(FWB_THREADS) void fwfm_bwd_kernel(FbParams p) {
    extern __shared__ __attribute__((aligned(16))) float fb_lds[];
    float* X = GLOBAL_WS ? p.ws + (int64_t)blockIdx.x * p.tile_floats : fb_lds;
    const int F = p.F, E = p.E, fs = 16 * E + 1, FE = F * E, FF = F * F;
    float* R = X + (((int64_t)F * fs + 3) & ~(int64_t)3);
    float* DL = R + (((int64_t)FF + 3) & ~(int64_t)3);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, s = tid >> 4, e0 = tid & 15;
    const int64_t n_tiles = (p.batch + 15) / 16;
    if (p.dw)
        for (int t = tid; t < FF; t += FWB_THREADS) R[t] = 0.f;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t b0 = tile * 16;
        const int nvalid = (int)min((int64_t)16, p.batch - b0);
        __syncthreads();                        // the previous tile is no longer read
        for (int r = wave; r < 16; r += FWB_THREADS / 64) {
            const float* xr = p.x + (b0 + min(r, nvalid - 1)) * p.x_stride;
            for (int e = lane; e < FE; e += 64) {
                const int f = e / E;
                X[f * fs + r * E + (e - f * E)] = r < nvalid ? xr[e] : 0.f;
            }
        }
        if (tid < 16) DL[tid] = tid < nvalid ? p.dl[b0 + tid] : 0.f;
        __syncthreads();
        if (p.dx && s < nvalid) {
            const float dl = DL[s];
            float* o = p.dx + (b0 + s) * p.dx_stride;
            for (int e = e0; e < E; e += 16) {
                const float* xs = X + s * E + e;
                for (int i = 0; i < F; ++i) {
                    float sum = 0.f;
                    for (int j = 0; j < i; ++j) sum = fmaf(p.r[(int64_t)j * F + i], xs[j * fs], sum);
                    for (int j = i + 1; j < F; ++j) sum = fmaf(p.r[(int64_t)i * F + j], xs[j * fs], sum);
                    const float v = dl * sum;
                    o[i * E + e] = p.accumulate ? o[i * E + e] + v : v;
                }
            }
        }
        if (p.dw) {
            for (int t = tid; t < FF; t += FWB_THREADS) {
                const int i = t / F, j = t - i * F;
                if (i >= j) continue;
                const float* xi = X + i * fs;
                const float* xj = X + j * fs;
                float sum = 0.f;
                for (int r = 0; r < 16; ++r) {
                    float d = 0.f;
                    for (int e = 0; e < E; ++e) d = fmaf(xi[r * E + e], xj[r * E + e], d);
                    sum = fmaf(DL[r], d, sum);
                }
                R[t] += sum;                    // one owner per cell
            }
        }
    }
    if (p.dw) {
        // (each thread reads back the cells it wrote itself)
        for (int t = tid; t < FF; t += FWB_THREADS) {
            const int i = t / F, j = t - i * F;
            if (i < j) atomicAdd(p.dw + t, R[t]);
        }
    }
}

struct FbPlan {
    bool ok;                // false: DCTR_E_UNSUPPORTED
    bool global;            // the general route (the tile in the workspace)
    int M;                  // FEFM: sub-tiles of 16 samples per workgroup
    int ldx, NP, ldg;
    bool gfull;             // FEFM: the tile's g holds all P pairs
    int64_t P, tile_floats;
    int grid_max;           // general route: workgroups the workspace has slices for
    size_t route_bytes;     // workspace of the general route (0 on the LDS route)
};

int64_t fb_tile_floats(const dctr_fieldpair_args_t* a, const FbPlan* pl, int M) {
    if (a->kind == DCTR_FIELDPAIR_FWFM)
        return (((int64_t)a->fields * (16 * a->dim + 1) + 3) & ~(int64_t)3) + (((int64_t)a->fields * a->fields + 3) & ~(int64_t)3) + 16;
    return fb_layout(a->fields, 16 * M, pl->ldx, pl->ldg, pl->NP).total;
}

void fb_plan(const dctr_fieldpair_args_t* a, FbPlan* pl) {
    const int F = a->fields, E = a->dim;
    pl->P = (int64_t)F * (F - 1) / 2;
    pl->ldx = (E + 15) & ~15;
    pl->NP = (int)(pl->P < FB_NP ? pl->P : FB_NP);
    // two sub-tiles share one set of weight registers, as in the forward, as long as the grid still fills the chip.  The tile's g holds
    // all P pairs where the LDS has the room (the dx product then reads every g on chip), else one chunk of them
    int M = a->kind == DCTR_FIELDPAIR_FWFM ? 1 : a->batch >= 32 * 256 ? 2 : 1;
    for (;; M >>= 1) {
        pl->gfull = pl->P > pl->NP && pl->P < FB_LDG_FULL;
        pl->ldg = pl->gfull ? FB_LDG_FULL : FB_LDG;
        if ((size_t)fb_tile_floats(a, pl, M) * sizeof(float) <= DCTR_LDS_MAX) break;
        pl->gfull = false;
        pl->ldg = FB_LDG;
        if ((size_t)fb_tile_floats(a, pl, M) * sizeof(float) <= DCTR_LDS_MAX || M == 1) break;
    }
    pl->M = M;
    pl->tile_floats = fb_tile_floats(a, pl, M);
    pl->ok = pl->tile_floats < 0x3fffffffLL;    // a tile's buffers are indexed in 32 bits
    const dctr_tile_route r = pl->ok ? dctr_plan_tile_route((size_t)pl->tile_floats * sizeof(float)) : dctr_tile_route{false, 0, 0};
    pl->global = r.global;
    pl->grid_max = r.grid_max;
    pl->route_bytes = r.route_bytes;
}

// the forward's size checks (fp_check of fieldpair_kernels.hip; its outputs are not read) and the backward's own
int fb_check(const dctr_fieldpair_bwd_args_t* b) {
    DCTR_REQUIRE(b, DCTR_E_NULL, "fieldpair_bwd: null args");
    const dctr_fieldpair_args_t* a = &b->fwd;
    DCTR_REQUIRE(a->kind == DCTR_FIELDPAIR_FEFM || a->kind == DCTR_FIELDPAIR_FWFM, DCTR_E_ENUM, "fieldpair_bwd: unknown kind %d", a->kind);
    DCTR_REQUIRE(a->fields >= 2, DCTR_E_DIM, "fieldpair_bwd: fields = %d: a field pair needs at least 2 fields", a->fields);
    DCTR_REQUIRE(a->dim >= 1 && a->batch >= 0 && a->x_offset >= 0 && b->d_pairs_offset >= 0 && b->dx_offset >= 0, DCTR_E_DIM,
                 "fieldpair_bwd: bad sizes");
    DCTR_REQUIRE(a->fields <= 65536 && a->dim <= (1 << 20) && (int64_t)a->fields * 64 * ((int64_t)a->dim + 16) < 0x3fffffffLL, DCTR_E_DIM,
                 "fieldpair_bwd: one tile's buffers exceed 2^30 floats");
    const int64_t F = a->fields, E = a->dim, P = F * (F - 1) / 2;
    DCTR_REQUIRE(a->x_stride >= a->x_offset + F * E, DCTR_E_DIM, "fieldpair_bwd: x_stride %lld < x_offset + fields*dim = %lld",
                 (long long)a->x_stride, (long long)(a->x_offset + F * E));
    DCTR_REQUIRE(a->kind == DCTR_FIELDPAIR_FEFM || !b->d_pairs, DCTR_E_DIM, "fieldpair_bwd: the FwFM kind has no d_pairs");
    DCTR_REQUIRE(!b->d_pairs || b->d_pairs_stride >= b->d_pairs_offset + P, DCTR_E_DIM,
                 "fieldpair_bwd: d_pairs_stride %lld < d_pairs_offset + P = %lld", (long long)b->d_pairs_stride,
                 (long long)(b->d_pairs_offset + P));
    DCTR_REQUIRE(!b->dx || b->dx_stride >= b->dx_offset + F * E, DCTR_E_DIM, "fieldpair_bwd: dx_stride %lld < dx_offset + fields*dim = %lld",
                 (long long)b->dx_stride, (long long)(b->dx_offset + F * E));
    DCTR_REQUIRE(b->max_blocks >= 0, DCTR_E_DIM, "fieldpair_bwd: max_blocks = %d", b->max_blocks);
    DCTR_REQUIRE(b->accumulate == 0 || b->accumulate == 1, DCTR_E_ENUM, "fieldpair_bwd: accumulate must be 0 or 1");
    return DCTR_OK;
}

}  // namespace

extern "C" int dctr_fieldpair_bwd_supported(const dctr_fieldpair_bwd_args_t* b) {
    if (fb_check(b) != DCTR_OK) return 0;
    FbPlan pl;
    fb_plan(&b->fwd, &pl);
    return pl.ok ? 1 : 0;
}

extern "C" size_t dctr_fieldpair_bwd_workspace_bytes(const dctr_fieldpair_bwd_args_t* b) {
    if (fb_check(b) != DCTR_OK) return 0;
    FbPlan pl;
    fb_plan(&b->fwd, &pl);
    return pl.ok ? pl.route_bytes : 0;
}

extern "C" int dctr_fieldpair_bwd(const dctr_fieldpair_bwd_args_t* b, void* stream) {
    int rc = fb_check(b);
    if (rc != DCTR_OK) return rc;
    const dctr_fieldpair_args_t* a = &b->fwd;
    FbPlan pl;
    fb_plan(a, &pl);
    DCTR_REQUIRE(pl.ok, DCTR_E_UNSUPPORTED, "fieldpair_bwd: one tile's buffers exceed 2^30 floats");
    const bool fwfm = a->kind == DCTR_FIELDPAIR_FWFM;
    DCTR_REQUIRE(a->x && a->weights, DCTR_E_NULL, "fieldpair_bwd: null x / weights");
    DCTR_REQUIRE(fwfm ? b->d_logit != nullptr : (b->d_pairs || b->d_logit), DCTR_E_NULL, "fieldpair_bwd: no gradient (d_pairs / d_logit)");
    if (pl.route_bytes)
        DCTR_REQUIRE_WORKSPACE("fieldpair_bwd", "dctr_fieldpair_bwd_workspace_bytes", a->workspace, a->workspace_bytes, pl.route_bytes);
    if (a->batch == 0 || (!b->dx && !b->d_weights)) return DCTR_OK;
    FbParams p = {};
    p.x = a->x + a->x_offset;
    p.batch = a->batch;
    p.x_stride = a->x_stride;
    p.F = a->fields;
    p.E = a->dim;
    p.ldx = pl.ldx;
    p.NP = pl.NP;
    p.ldg = pl.ldg;
    p.P = pl.P;
    p.tile_floats = pl.tile_floats;
    p.dp = b->d_pairs ? b->d_pairs + b->d_pairs_offset : nullptr;
    p.dp_stride = b->d_pairs_stride;
    p.dl = b->d_logit;
    p.dx = b->dx ? b->dx + b->dx_offset : nullptr;
    p.dx_stride = b->dx_stride;
    p.accumulate = b->accumulate;
    p.dw = b->d_weights;
    p.ws = pl.global ? (float*)a->workspace : nullptr;
    if (fwfm)
        p.r = (const float*)a->weights;
    else
        p.wt = (const float* const*)a->weights;
    const int64_t n_tiles = dctr_ceil_div(a->batch, (int64_t)16 * pl.M);
    // FEFM: one workgroup per compute unit (the kernel takes the 256 registers two waves per SIMD leave a wave), each walking its
    // tiles: the grid bounds the atomics, workgroups x P x E^2
    int64_t cap = b->max_blocks > 0 ? (int64_t)b->max_blocks : (int64_t)(fwfm ? 4 : 1) * dctr_n_cus();
    if (pl.global && cap > pl.grid_max) cap = pl.grid_max;
    const dim3 grid((unsigned)(n_tiles < cap ? n_tiles : cap));
    const hipStream_t st = (hipStream_t)stream;
    if (pl.global) {
        if (fwfm)
            DCTR_LAUNCH(fwfm_bwd_kernel<true>, grid, dim3(FWB_THREADS), 0, st, p);
        else
            DCTR_LAUNCH((fefm_bwd_kernel<true, 1, false>), grid, dim3(FB_THREADS), 0, st, p);
    } else {
        const size_t lds = (size_t)pl.tile_floats * sizeof(float);
        static thread_local size_t granted[5][DCTR_MAX_DEVICES] = {{0}};
        const int which = fwfm ? 4 : (pl.M >> 1) * 2 + (pl.gfull ? 1 : 0);
        const void* fns[5] = {(const void*)fefm_bwd_kernel<false, 1, false>, (const void*)fefm_bwd_kernel<false, 1, true>,
                              (const void*)fefm_bwd_kernel<false, 2, false>, (const void*)fefm_bwd_kernel<false, 2, true>,
                              (const void*)fwfm_bwd_kernel<false>};
        hipError_t e = dctr_grant_lds(fns[which], lds, granted[which]);
        DCTR_REQUIRE(e == hipSuccess, (int)e, "fieldpair_bwd: cannot raise dynamic LDS: %s", hipGetErrorString(e));
        if (fwfm)
            DCTR_LAUNCH(fwfm_bwd_kernel<false>, grid, dim3(FWB_THREADS), lds, st, p);
        else if (which == 3)
            DCTR_LAUNCH((fefm_bwd_kernel<false, 2, true>), grid, dim3(FB_THREADS), lds, st, p);
        else if (which == 2)
            DCTR_LAUNCH((fefm_bwd_kernel<false, 2, false>), grid, dim3(FB_THREADS), lds, st, p);
        else if (which == 1)
            DCTR_LAUNCH((fefm_bwd_kernel<false, 1, true>), grid, dim3(FB_THREADS), lds, st, p);
        else
            DCTR_LAUNCH((fefm_bwd_kernel<false, 1, false>), grid, dim3(FB_THREADS), lds, st, p);
    }
    return dctr_launch_status("dctr_fieldpair_bwd");
}
