// The backward of dctr_bilinear_fwd (bilinear_kernels.hip: SENETLayer.call + BilinearInteraction.call as FiBiNET wires them), one
// launch, all three modes and bilinear types.  The forward saves nothing: a workgroup loads the same X tile [F][16][ldx] into LDS and
// recomputes Z, A1, A2 as the forward does.
//
// Per pair (i < j) and layer, with g [16, E] the tile's rows of d_out for that pair (SENET side: c = A2[i] A2[j]):
//   U  = X_i W                    -> dx_j += g (.) U            (SENET side: Y_j += A2[i] g (.) U)
//   T  = (g (.) X_j) W^T          -> dx_i += T                  (SENET side: Y_i += (A2[j] g (.) X_j) W^T)
//   dW += X_i^T (c g (.) X_j), K = the 16 samples of the tile
// all three on v_mfma_f32_16x16x4_f32, fp32 throughout.  Y_f is the SENET side's dx_f short of its own factor A2[f]: dx_f gets
// A2[f] Y_f and dA2[f] = <Y_f, x_f> (= sum_partner A2[partner] <g, s>, the forward's factorisation, without a division by A2).
// The SENET chain behind it (gates, dW_2, dA1, dW_1, the mean's gradient) is plain FMAs; it is linear in dA2.
//
// dx has one owner per element.  The pairs of a tile are walked in chunks that never cross a row i of the pair triangle: a chunk's
// d_out columns are one contiguous run per sample, staged once in LDS (16 B per lane where E allows); inside a chunk every pair has
// its own j, so the wave that owns a pair adds g (.) U into the tile's dx accumulator DX_j [F][16][ldx] in LDS without a race, and
// sums its T in a patch of its own; behind a barrier the patches are added to DX_i in wave order.  No atomics: dx is bit-identical
// from call to call.  The row leaves coalesced after the SENET chain, with the dense tail of d_out behind it (mode MODEL).
//
// Weight gradients stay in registers across all tiles a workgroup walks.  Four waves, one per SIMD, so that a wave may take the 512
// registers of a lane: BB_NACC = 64 sums of 16 x 16 per wave, each a fixed register group, because the pairs of a walk are laid out at
// compile time: a walk is BB_CPW chunks of up to BB_RPC rounds of one pair per wave and two layers.  INTERACTION has a sum per pair
// and layer, more than the registers hold: the workgroup walks its tiles once per walk (X is loaded again, dx is added to by its
// owner; the SENET chain is linear in dA2 and runs per walk), and each sum leaves with one float atomic per element and workgroup.
// EACH / ALL sum a chunk's / a walk's pairs in registers and the waves' sums through the patches before the atomic.  E > 16 (more
// than one 16 x 16 tile per matrix) adds each tile's product directly, as the field-pair backward does.  The SENET matrices'
// gradients are summed in LDS, a thread per cell.
// A tile too large for the LDS runs with its buffers in a per-workgroup slice of the workspace (the forward's general route).
#include <math.h>
#include <stdint.h>
#include "dctr_common.h"
#include "mfma_tile.h"
#include "pair_index.h"
#include "tile_route.h"

namespace {

constexpr int BB_THREADS = 256;                // 4 waves, one per SIMD: a wave may take all 512 registers of a lane
constexpr int BB_WAVES = BB_THREADS / 64;
constexpr int BB_S = 16;                        // samples per tile = the rows of one MFMA tile
constexpr int BB_CPW = 8;                       // chunks per walk
constexpr int BB_RPC = 4;                       // rounds per chunk: a chunk holds up to BB_RPC * BB_WAVES pairs
constexpr int BB_NACC = BB_CPW * BB_RPC * 2;    // 16x16 weight-gradient sums a wave keeps in registers (4 registers each)

struct BbParams {
    const float* x;
    int64_t batch;
    int64_t x_stride;
    int32_t F, E, type, D;
    int32_t nblk;                // bilinear layers: 2 (model), 1 (one layer), 0 (the SENET output only)
    int32_t senet;
    int32_t r;
    int32_t ldx, NP, ldo, ldt;
    int64_t P;
    int64_t tile_floats;
    const float* w1;
    const float* w2;
    const float* const* wt[2];   // DEVICE tables of the matrices: layer 0 (SENET side, or the one layer), layer 1
    const float* dout;           // already advanced by d_out_offset
    int64_t dout_stride;
    float* dx;                   // already advanced by dx_offset (or null)
    int64_t dx_stride;
    int32_t accumulate;
    float* dw1;
    float* dw2;
    float* dw[2];                // [nW, E, E] of layer 0 / 1 (or null)
    float* ws;                   // general route only
};

// offsets (floats) of a tile's buffers behind X: the dx accumulators of the SENET side (Y) and the raw side, the chunk's g, the waves'
// patches, the SENET vectors and the sums of the SENET matrices' gradients
struct BbLayout {
    int64_t dxs, dxr, g, tp, a2, z, a1, da2, da1, dz, pw1, pw2, total;
};

__host__ __device__ inline BbLayout bb_layout(int F, int ldx, int senet, int nblk, int r, int ldo, int ldt) {
    BbLayout L;
    const int64_t xs = (int64_t)F * BB_S * ldx;
    int64_t o = xs;
    L.dxs = o;
    if (senet) o += xs;
    L.dxr = o;
    if (nblk) o += xs;
    L.g = o;
    o += (int64_t)BB_S * ldo;
    L.tp = o;
    o += (int64_t)BB_WAVES * nblk * BB_S * ldt;
    const int64_t sf = senet ? (int64_t)BB_S * F : 0, sr = senet ? (int64_t)BB_S * r : 0;
    const int64_t fr = senet ? (((int64_t)F * r + 3) & ~(int64_t)3) : 0;
    L.a2 = o;
    o += sf;
    L.z = o;
    o += sf;
    L.da2 = o;
    o += sf;
    L.dz = o;
    o += sf;
    L.a1 = o;
    o += sr;
    L.da1 = o;
    o += sr;
    L.pw1 = o;
    o += fr;
    L.pw2 = o;
    o += fr;
    L.total = (o + 3) & ~(int64_t)3;
    return L;
}

// The chunks in pair order, the same sequence for every tile and for the flush: (row i, first partner j0, n pairs); no chunk
// crosses a row.
struct BbWalk {
    int i, j;
};
struct BbChunk {
    int i, j0, n;
};

// false: the pairs are done
__device__ __forceinline__ bool bb_next(const BbParams& p, BbWalk& st, BbChunk& c) {
    if (st.i >= p.F - 1) return false;
    c.i = st.i;
    c.j0 = st.j;
    c.n = min(p.NP, p.F - st.j);
    st.j += c.n;
    if (st.j >= p.F) {
        ++st.i;
        st.j = st.i + 1;
    }
    return true;
}

template <bool GLOBAL_WS>
__global__ __launch_bounds__(BB_THREADS) void bilinear_bwd_kernel(BbParams p) {
    extern __shared__ __attribute__((aligned(16))) float bb_lds[];
    float* X = GLOBAL_WS ? p.ws + (int64_t)blockIdx.x * p.tile_floats : bb_lds;
    const int F = p.F, E = p.E, ldx = p.ldx, ldo = p.ldo, ldt = p.ldt, nblk = p.nblk, r = p.r;
    const BbLayout L = bb_layout(F, ldx, p.senet, nblk, r, ldo, ldt);
    float* DXs = X + L.dxs;
    float* DXr = X + L.dxr;
    float* Gs = X + L.g;
    float* TP = X + L.tp;
    float* A2 = X + L.a2;
    float* Z = X + L.z;
    float* DA2 = X + L.da2;
    float* DZ = X + L.dz;
    float* A1 = X + L.a1;
    float* DA1 = X + L.da1;
    float* PW1 = X + L.pw1;
    float* PW2 = X + L.pw2;
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, g = lane >> 4, jl = lane & 15;
    const int fs = BB_S * ldx;                  // floats between two fields of X / DX
    const int EP = (E + 15) & ~15, KQ = EP >> 2, CT = EP >> 4;
    const int FE = F * E;
    const int tpw = nblk * BB_S * ldt;          // floats of one wave's patches
    const bool senet = p.senet != 0;
    const bool model = senet && nblk == 2;      // layer 0 is the SENET side
    const bool want_dw = p.dw[0] || p.dw[1];
    const bool slots = want_dw && CT == 1;      // the sums live in registers; else (E > 16) every tile's product is added directly
    const bool need_y = senet && (p.dx || p.dw1 || p.dw2);
    const bool vec4 = (E & 3) == 0;
    const bool g_vec = vec4 && (((uintptr_t)p.dout | (uintptr_t)(p.dout_stride * 4)) & 15) == 0;
    const int64_t n_tiles = (p.batch + BB_S - 1) / BB_S;

    // the K padding of X (columns E .. ldx-1) stays zero: the MFMAs read it against clamped weight rows.  The patches start at zero
    // and whoever reads one puts the zero back; the SENET matrices' sums start at zero.
    const int padc = ldx - E;
    for (int e = tid; e < F * BB_S * padc; e += BB_THREADS) {
        const int row = e / padc;
        X[row * ldx + E + (e - row * padc)] = 0.f;
    }
    for (int e = tid; e < BB_WAVES * tpw; e += BB_THREADS) TP[e] = 0.f;
    if (senet)
        for (int e = tid; e < F * r; e += BB_THREADS) {
            PW1[e] = 0.f;
            PW2[e] = 0.f;
        }

    BbWalk walk0 = {nblk ? 0 : F - 1, 1};
    for (bool first = true; first || walk0.i < F - 1; first = false) {
        dctr::f32x4 acc[BB_NACC];
#pragma unroll
        for (int q = 0; q < BB_NACC; ++q) acc[q] = dctr::f32x4{0.f, 0.f, 0.f, 0.f};
        BbWalk walk_end = walk0;

        for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
            const int64_t b0 = tile * BB_S;
            const int nvalid = (int)min((int64_t)BB_S, p.batch - b0);
            __syncthreads();                    // the previous tile is no longer read
            for (int s = wave; s < BB_S; s += BB_WAVES) {
                const bool on = s < nvalid;     // rows past the batch hold zeros, and so do their g
                const float* xr = p.x + (b0 + min(s, nvalid - 1)) * p.x_stride;
                for (int e = lane; e < FE; e += 64) {
                    const int f = e / E;
                    X[f * fs + s * ldx + (e - f * E)] = on ? xr[e] : 0.f;
                }
            }
            // the tile's dx accumulators start at zero (mode SENET: Y = d_out itself)
            if (senet)
                for (int e = tid; e < F * fs; e += BB_THREADS) DXs[e] = 0.f;
            if (nblk)
                for (int e = tid; e < F * fs; e += BB_THREADS) DXr[e] = 0.f;
            __syncthreads();
            if (nblk == 0) {
                for (int s = wave; s < nvalid; s += BB_WAVES) {
                    const float* gr = p.dout + (b0 + s) * p.dout_stride;
                    for (int e = lane; e < FE; e += 64) {
                        const int f = e / E;
                        DXs[f * fs + s * ldx + (e - f * E)] = gr[e];
                    }
                }
            }
            if (senet) {                        // Z, A1, A2 as the forward computes them
                for (int e = tid; e < BB_S * F; e += BB_THREADS) {
                    const int s = e / F, f = e - s * F;
                    const float* xr = X + f * fs + s * ldx;
                    float z = 0.f;
                    for (int c = 0; c < E; ++c) z += xr[c];
                    Z[e] = z / (float)E;
                }
                __syncthreads();
                for (int e = tid; e < BB_S * r; e += BB_THREADS) {
                    const int s = e / r, k = e - s * r;
                    float a = 0.f;
                    for (int f = 0; f < F; ++f) a = fmaf(Z[s * F + f], p.w1[(int64_t)f * r + k], a);
                    A1[e] = fmaxf(a, 0.f);
                }
                __syncthreads();
                for (int e = tid; e < BB_S * F; e += BB_THREADS) {
                    const int s = e / F, f = e - s * F;
                    float a = 0.f;
                    for (int k = 0; k < r; ++k) a = fmaf(A1[s * r + k], p.w2[(int64_t)k * F + f], a);
                    A2[e] = fmaxf(a, 0.f);
                }
            }

            // ---- the walk's chunks of pairs: BB_CPW of them when the sums live in registers (chunk cc, round rr, layer b -> a fixed
            // register group), else all of them
            BbWalk st = walk0;
            bool more = true;
            do {
#pragma unroll
                for (int cc = 0; cc < BB_CPW; ++cc) {
                    BbChunk c;
                    if (!bb_next(p, st, c)) {
                        more = false;
                        break;
                    }
                    const int i = c.i, n = c.n;
                    const int64_t p0 = dctr::pair_row_start(i, F) + c.j0 - i - 1;
                    const int blen = n * nblk * E;
                    const float* xi = X + i * fs;
                    // the chunk's g: one contiguous run of d_out per sample (the barrier behind the previous chunk's pair phase, or
                    // the one above, keeps these writes behind its reads)
                    for (int s = wave; s < BB_S; s += BB_WAVES) {
                        const bool on = s < nvalid;
                        const float* gr = p.dout + (b0 + min(s, nvalid - 1)) * p.dout_stride + p0 * nblk * E;
                        float* gd = Gs + s * ldo;
                        if (g_vec) {
                            for (int e = lane * 4; e < blen; e += 256) {
                                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                                if (on) v = *reinterpret_cast<const float4*>(gr + e);
                                *reinterpret_cast<float4*>(gd + e) = v;
                            }
                        } else {
                            for (int e = lane; e < blen; e += 64) gd[e] = on ? gr[e] : 0.f;
                        }
                    }
                    __syncthreads();
#pragma unroll 1
                    for (int pl = wave; pl < n; pl += BB_WAVES) {
                        const int j = c.j0 + pl;
                        const int64_t widx = p.type == DCTR_BILINEAR_ALL ? 0 : p.type == DCTR_BILINEAR_EACH ? i : p0 + pl;
                        const float* xj = X + j * fs;
#pragma unroll 1
                        for (int b = 0; b < nblk; ++b) {
                            const bool sside = model && b == 0;
                            const float* __restrict__ W = p.wt[b][widx];
                            const float* gp = Gs + (pl * nblk + b) * E;
                            float* DX = sside ? DXs : DXr;
                            if (sside ? need_y : p.dx != nullptr) {
                                float* tp = TP + wave * tpw + b * BB_S * ldt;
                                const float cj = sside ? A2[jl * F + j] : 1.f;       // T's A operand row is sample jl
                                for (int ct = 0; ct < CT; ++ct) {
                                    const int col = ct * 16 + jl, n0 = min(col, E - 1);
                                    dctr::f32x4 u = {0.f, 0.f, 0.f, 0.f}, t = {0.f, 0.f, 0.f, 0.f};
                                    for (int t0 = 0; t0 < KQ; t0 += 4) {
                                        const int k0 = g * KQ + t0;
                                        const float4 a4 = *reinterpret_cast<const float4*>(xi + jl * ldx + k0);
                                        const float4 x4 = *reinterpret_cast<const float4*>(xj + jl * ldx + k0);
                                        const float av[4] = {a4.x, a4.y, a4.z, a4.w}, xv[4] = {x4.x, x4.y, x4.z, x4.w};
                                        float gv[4];
                                        if (vec4) {
                                            float4 g4 = make_float4(0.f, 0.f, 0.f, 0.f);
                                            if (k0 < E) g4 = *reinterpret_cast<const float4*>(gp + jl * ldo + k0);
                                            gv[0] = g4.x;
                                            gv[1] = g4.y;
                                            gv[2] = g4.z;
                                            gv[3] = g4.w;
                                        } else {
#pragma unroll
                                            for (int tt = 0; tt < 4; ++tt) gv[tt] = k0 + tt < E ? gp[jl * ldo + k0 + tt] : 0.f;
                                        }
                                        float bu[4], bt[4];
#pragma unroll
                                        for (int tt = 0; tt < 4; ++tt) {
                                            const int k = min(k0 + tt, E - 1);
                                            bu[tt] = W[(int64_t)k * E + n0];        // U = X_i W:          B[k][n] = W[k][n]
                                            bt[tt] = W[(int64_t)n0 * E + k];        // T = (g (.) X_j) W^T: B[k][n] = W[n][k]
                                        }
#pragma unroll
                                        for (int tt = 0; tt < 4; ++tt) {
                                            u = __builtin_amdgcn_mfma_f32_16x16x4f32(av[tt], bu[tt], u, 0, 0, 0);
                                            t = __builtin_amdgcn_mfma_f32_16x16x4f32(cj * gv[tt] * xv[tt], bt[tt], t, 0, 0, 0);
                                        }
                                    }
                                    if (col < E) {
#pragma unroll
                                        for (int rr = 0; rr < 4; ++rr) {
                                            const int s = 4 * g + rr;
                                            const float ci = sside ? A2[s * F + i] : 1.f;
                                            DX[j * fs + s * ldx + col] += ci * gp[s * ldo + col] * u[rr];
                                            tp[s * ldt + col] += t[rr];
                                        }
                                    }
                                }
                            }
                            if (p.dw[b] && !slots) {
                                // E > 16: dW += X_i^T (c g (.) X_j) tile by tile, added directly
                                float* dst = p.dw[b] + widx * (int64_t)E * E;
                                for (int ct = 0; ct < CT; ++ct) {
                                    const int dcol = ct * 16 + jl;
                                    float bv[4];
#pragma unroll
                                    for (int tt = 0; tt < 4; ++tt) {
                                        const int s = 4 * g + tt;
                                        const float cc2 = sside ? A2[s * F + i] * A2[s * F + j] : 1.f;
                                        bv[tt] = dcol < E ? cc2 * gp[s * ldo + dcol] * xj[s * ldx + dcol] : 0.f;
                                    }
                                    for (int et = 0; et < CT; ++et) {
                                        dctr::f32x4 d = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                                        for (int tt = 0; tt < 4; ++tt)
                                            d = __builtin_amdgcn_mfma_f32_16x16x4f32(xi[(4 * g + tt) * ldx + et * 16 + jl], bv[tt], d, 0, 0, 0);
#pragma unroll
                                        for (int rr = 0; rr < 4; ++rr) {
                                            const int e = et * 16 + 4 * g + rr;
                                            if (e < E && dcol < E) atomicAdd(dst + (int64_t)e * E + dcol, d[rr]);
                                        }
                                    }
                                }
                            }
                        }
                    }
                    if (slots) {
                        // dW += X_i^T (c g (.) X_j) at E <= 16: rows = W's rows e (lane jl), columns = W's columns d, k-slot g of step
                        // tt = sample 4g + tt.  Round rr and layer b name the registers at compile time.
                        float av[4];
#pragma unroll
                        for (int tt = 0; tt < 4; ++tt) av[tt] = xi[(4 * g + tt) * ldx + jl];
#pragma unroll
                        for (int rr = 0; rr < BB_RPC; ++rr) {
                            const int pl = rr * BB_WAVES + wave;
                            if (pl < n) {
                                const float* xj = X + (c.j0 + pl) * fs;
                                float xg[4], ca[4];
#pragma unroll
                                for (int tt = 0; tt < 4; ++tt) {
                                    const int s = 4 * g + tt;
                                    xg[tt] = jl < E ? xj[s * ldx + jl] : 0.f;
                                    ca[tt] = model ? A2[s * F + i] * A2[s * F + c.j0 + pl] : 1.f;
                                }
#pragma unroll
                                for (int b = 0; b < 2; ++b) {
                                    if (b < nblk && p.dw[b]) {
                                        const float* gp = Gs + (pl * nblk + b) * E;
                                        float bv[4];
#pragma unroll
                                        for (int tt = 0; tt < 4; ++tt) {
                                            const float gg = jl < E ? gp[(4 * g + tt) * ldo + jl] : 0.f;
                                            bv[tt] = (b == 0 ? ca[tt] : 1.f) * gg * xg[tt];
                                        }
                                        dctr::f32x4& a = acc[(cc * BB_RPC + rr) * 2 + b];
#pragma unroll
                                        for (int tt = 0; tt < 4; ++tt) a = __builtin_amdgcn_mfma_f32_16x16x4f32(av[tt], bv[tt], a, 0, 0, 0);
                                    }
                                }
                            }
                        }
                    }
                    __syncthreads();
                    // the waves' T sums join DX_i in wave order; the reader leaves the patch at zero for the next chunk
                    for (int e = tid; e < nblk * BB_S * E; e += BB_THREADS) {
                        const int b = e / (BB_S * E), rem = e - b * BB_S * E, s = rem / E, col = rem - s * E;
                        float* tp = TP + b * BB_S * ldt + s * ldt + col;
                        float sum = 0.f;
                        for (int w = 0; w < min(n, BB_WAVES); ++w) {
                            sum += tp[w * tpw];
                            tp[w * tpw] = 0.f;
                        }
                        float* DX = model && b == 0 ? DXs : DXr;
                        DX[i * fs + s * ldx + col] += sum;
                    }
                    // (the next chunk's barrier, or the one below, orders these writes before anything reads DX or the patches)
                }
            } while (more && !slots);
            walk_end = st;
            __syncthreads();

            // ---- the SENET chain: dA2 = <Y_f, x_f> under its gate, dW_2, dA1 under its gate, dW_1, the mean's gradient
            if (need_y) {
                for (int e = tid; e < BB_S * F; e += BB_THREADS) {
                    const int s = e & (BB_S - 1), f = e >> 4;
                    const float* y = DXs + f * fs + s * ldx;
                    const float* xr = X + f * fs + s * ldx;
                    float d = 0.f;
                    for (int cc = 0; cc < E; ++cc) d = fmaf(y[cc], xr[cc], d);
                    DA2[s * F + f] = A2[s * F + f] > 0.f ? d : 0.f;
                }
                __syncthreads();
                if (p.dw2)
                    for (int e = tid; e < r * F; e += BB_THREADS) {
                        const int k = e / F, f = e - k * F;
                        float a = 0.f;
                        for (int s = 0; s < BB_S; ++s) a = fmaf(A1[s * r + k], DA2[s * F + f], a);
                        PW2[e] += a;            // one owner per cell
                    }
                for (int e = tid; e < BB_S * r; e += BB_THREADS) {
                    const int s = e / r, k = e - s * r;
                    float a = 0.f;
                    for (int f = 0; f < F; ++f) a = fmaf(DA2[s * F + f], p.w2[(int64_t)k * F + f], a);
                    DA1[e] = A1[e] > 0.f ? a : 0.f;
                }
                __syncthreads();
                if (p.dw1)
                    for (int e = tid; e < F * r; e += BB_THREADS) {
                        const int f = e / r, k = e - f * r;
                        float a = 0.f;
                        for (int s = 0; s < BB_S; ++s) a = fmaf(Z[s * F + f], DA1[s * r + k], a);
                        PW1[e] += a;
                    }
                for (int e = tid; e < BB_S * F; e += BB_THREADS) {
                    const int s = e / F, f = e - s * F;
                    float a = 0.f;
                    for (int k = 0; k < r; ++k) a = fmaf(DA1[s * r + k], p.w1[(int64_t)f * r + k], a);
                    DZ[e] = a / (float)E;
                }
                __syncthreads();
            }

            // ---- the rows of dx leave: written (or added to) in the first walk, added to by the same owner in the later ones
            if (p.dx) {
                const bool add = p.accumulate || !first;
                for (int s = wave; s < nvalid; s += BB_WAVES) {
                    float* o = p.dx + (b0 + s) * p.dx_stride;
                    for (int e = lane; e < FE; e += 64) {
                        const int f = e / E, at = f * fs + s * ldx + (e - f * E);
                        float v = nblk ? DXr[at] : 0.f;
                        if (senet) v += fmaf(A2[s * F + f], DXs[at], DZ[s * F + f]);
                        o[e] = add ? o[e] + v : v;
                    }
                    if (first && p.D > 0) {     // the transpose of the forward's copy of the dense columns
                        const float* gr = p.dout + (b0 + s) * p.dout_stride + (int64_t)nblk * p.P * E;
                        for (int cc = lane; cc < p.D; cc += 64) o[FE + cc] = p.accumulate ? o[FE + cc] + gr[cc] : gr[cc];
                    }
                }
            }
        }

        // ---- the walk's weight-gradient sums leave: one float atomic per element and workgroup
        if (slots) {
            __syncthreads();
            // ALL / EACH: every wave holds sums for the same matrix; they are added through the patches
            auto leave = [&](dctr::f32x4 v, float* dst) {
                float* tp = TP + wave * tpw;
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) tp[(4 * g + rr) * ldt + jl] = v[rr];
                __syncthreads();
                const int er = tid >> 4, dc = tid & 15;
                float sum = 0.f;
                for (int w = 0; w < BB_WAVES; ++w) {
                    sum += TP[w * tpw + er * ldt + dc];
                    TP[w * tpw + er * ldt + dc] = 0.f;
                }
                if (er < E && dc < E) atomicAdd(dst + er * E + dc, sum);
                __syncthreads();
            };
            BbWalk st = walk0;
            dctr::f32x4 tot[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
            for (int cc = 0; cc < BB_CPW; ++cc) {
                BbChunk c;
                if (!bb_next(p, st, c)) break;
                const int64_t p0 = dctr::pair_row_start(c.i, F) + c.j0 - c.i - 1;
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    if (!(b < nblk && p.dw[b])) continue;
                    if (p.type == DCTR_BILINEAR_INTERACTION) {
#pragma unroll
                        for (int rr = 0; rr < BB_RPC; ++rr) {
                            const int pl = rr * BB_WAVES + wave;
                            if (pl >= c.n) continue;
                            const dctr::f32x4 v = acc[(cc * BB_RPC + rr) * 2 + b];
                            float* dst = p.dw[b] + (p0 + pl) * (int64_t)E * E;
#pragma unroll
                            for (int q = 0; q < 4; ++q)
                                if (4 * g + q < E && jl < E) atomicAdd(dst + (4 * g + q) * E + jl, v[q]);
                        }
                    } else {
                        dctr::f32x4 v = acc[cc * BB_RPC * 2 + b];
#pragma unroll
                        for (int rr = 1; rr < BB_RPC; ++rr) v += acc[(cc * BB_RPC + rr) * 2 + b];
                        if (p.type == DCTR_BILINEAR_ALL)
                            tot[b] += v;
                        else
                            leave(v, p.dw[b] + c.i * (int64_t)E * E);
                    }
                }
            }
            if (p.type == DCTR_BILINEAR_ALL)
                for (int b = 0; b < nblk; ++b)
                    if (p.dw[b]) leave(tot[b], p.dw[b]);
        }
        walk0 = walk_end;
    }

    if (senet && (p.dw1 || p.dw2)) {
        // (each thread reads back the cells it summed itself)
        for (int e = tid; e < F * r; e += BB_THREADS) {
            if (p.dw1) atomicAdd(p.dw1 + e, PW1[e]);
            if (p.dw2) atomicAdd(p.dw2 + e, PW2[e]);
        }
    }
}

struct BbPlan {
    bool ok;                // false: DCTR_E_UNSUPPORTED
    bool global;            // the general route (buffers in the workspace)
    int nblk, senet, r, ldx, NP, ldo, ldt;
    int64_t P, tile_floats;
    int grid_max;           // general route: workgroups the workspace has slices for
    size_t route_bytes;     // workspace of the general route (0 on the LDS route)
};

void bb_plan(const dctr_bilinear_args_t* a, BbPlan* pl) {
    const int F = a->fields, E = a->dim, EP = (E + 15) & ~15;
    pl->nblk = a->mode == DCTR_BILINEAR_MODE_SENET ? 0 : a->mode == DCTR_BILINEAR_MODE_LAYER ? 1 : 2;
    pl->senet = a->mode != DCTR_BILINEAR_MODE_LAYER;
    pl->r = pl->senet ? a->reduction_size : 0;
    pl->P = (int64_t)F * (F - 1) / 2;
    pl->ldx = EP + 4;
    pl->ldt = EP + 1;
    // pairs per chunk: BB_RPC rounds of one pair per wave up to E = 16, two past it (the chunk's g must fit beside the tile)
    int np = E <= 16 ? BB_RPC * BB_WAVES : 2 * BB_WAVES;
    if (np > F - 1) np = F - 1;
    pl->NP = pl->nblk ? np : 0;
    pl->ldo = pl->nblk ? pl->nblk * pl->NP * E + 4 : 0;
    pl->tile_floats = bb_layout(F, pl->ldx, pl->senet, pl->nblk, pl->r, pl->ldo, pl->ldt).total;
    pl->ok = pl->tile_floats < 0x3fffffffLL;    // a tile's buffers are indexed in 32 bits
    const dctr_tile_route r = pl->ok ? dctr_plan_tile_route((size_t)pl->tile_floats * sizeof(float)) : dctr_tile_route{false, 0, 0};
    pl->global = r.global;
    pl->grid_max = r.grid_max;
    pl->route_bytes = r.route_bytes;
}

// the forward's size checks (bl_check of bilinear_kernels.hip; its output is not read) and the backward's own
int bb_check(const dctr_bilinear_bwd_args_t* b) {
    DCTR_REQUIRE(b, DCTR_E_NULL, "bilinear_bwd: null args");
    const dctr_bilinear_args_t* a = &b->fwd;
    DCTR_REQUIRE(a->fields >= 2, DCTR_E_DIM, "bilinear_bwd: fields = %d: the layers need at least 2 fields", a->fields);
    DCTR_REQUIRE(a->bilinear_type >= DCTR_BILINEAR_ALL && a->bilinear_type <= DCTR_BILINEAR_INTERACTION, DCTR_E_ENUM,
                 "bilinear_bwd: unknown bilinear_type %d", a->bilinear_type);
    DCTR_REQUIRE(a->mode >= DCTR_BILINEAR_MODE_MODEL && a->mode <= DCTR_BILINEAR_MODE_LAYER, DCTR_E_ENUM, "bilinear_bwd: unknown mode %d",
                 a->mode);
    DCTR_REQUIRE(a->dim >= 1 && a->batch >= 0 && a->dense_cols >= 0 && b->d_out_offset >= 0 && b->dx_offset >= 0, DCTR_E_DIM,
                 "bilinear_bwd: bad sizes");
    DCTR_REQUIRE(a->mode == DCTR_BILINEAR_MODE_LAYER || a->reduction_size >= 1, DCTR_E_DIM, "bilinear_bwd: reduction_size must be >= 1");
    DCTR_REQUIRE(a->mode == DCTR_BILINEAR_MODE_MODEL || a->dense_cols == 0, DCTR_E_DIM,
                 "bilinear_bwd: dense_cols exist in the model mode only");
    DCTR_REQUIRE(a->fields <= 65536 && a->dim <= (1 << 20) && a->reduction_size <= (1 << 20) &&
                     (int64_t)a->fields * BB_S * ((int64_t)a->dim + 20) * 3 < 0x7fffffffLL,
                 DCTR_E_DIM, "bilinear_bwd: one tile's buffers exceed 2^31 floats");
    const int64_t F = a->fields, E = a->dim, P = F * (F - 1) / 2;
    const int64_t in_w = F * E + (a->mode == DCTR_BILINEAR_MODE_MODEL ? a->dense_cols : 0);
    const int64_t out_w = a->mode == DCTR_BILINEAR_MODE_SENET ? F * E : a->mode == DCTR_BILINEAR_MODE_LAYER ? P * E : 2 * P * E + a->dense_cols;
    DCTR_REQUIRE(a->x_stride >= in_w, DCTR_E_DIM, "bilinear_bwd: x_stride %lld < %lld", (long long)a->x_stride, (long long)in_w);
    DCTR_REQUIRE(b->d_out_stride >= b->d_out_offset + out_w, DCTR_E_DIM, "bilinear_bwd: d_out_stride %lld < d_out_offset + %lld",
                 (long long)b->d_out_stride, (long long)out_w);
    DCTR_REQUIRE(!b->dx || b->dx_stride >= b->dx_offset + in_w, DCTR_E_DIM, "bilinear_bwd: dx_stride %lld < dx_offset + %lld",
                 (long long)b->dx_stride, (long long)in_w);
    DCTR_REQUIRE(b->max_blocks >= 0, DCTR_E_DIM, "bilinear_bwd: max_blocks = %d", b->max_blocks);
    DCTR_REQUIRE(b->accumulate == 0 || b->accumulate == 1, DCTR_E_ENUM, "bilinear_bwd: accumulate must be 0 or 1");
    return DCTR_OK;
}

}  // namespace

extern "C" int dctr_bilinear_bwd_supported(const dctr_bilinear_bwd_args_t* b) {
    if (bb_check(b) != DCTR_OK) return 0;
    BbPlan pl;
    bb_plan(&b->fwd, &pl);
    return pl.ok ? 1 : 0;
}

extern "C" size_t dctr_bilinear_bwd_workspace_bytes(const dctr_bilinear_bwd_args_t* b) {
    if (bb_check(b) != DCTR_OK) return 0;
    BbPlan pl;
    bb_plan(&b->fwd, &pl);
    return pl.ok ? pl.route_bytes : 0;
}

extern "C" int dctr_bilinear_bwd(const dctr_bilinear_bwd_args_t* b, void* stream) {
    int rc = bb_check(b);
    if (rc != DCTR_OK) return rc;
    const dctr_bilinear_args_t* a = &b->fwd;
    BbPlan pl;
    bb_plan(a, &pl);
    DCTR_REQUIRE(pl.ok, DCTR_E_UNSUPPORTED, "bilinear_bwd: one tile's buffers exceed 2^30 floats");
    DCTR_REQUIRE(a->x && b->d_out, DCTR_E_NULL, "bilinear_bwd: null x / d_out");
    DCTR_REQUIRE(!pl.senet || (a->senet_w1 && a->senet_w2), DCTR_E_NULL, "bilinear_bwd: null senet_w1 / senet_w2");
    DCTR_REQUIRE(pl.nblk == 0 || a->bilinear_w, DCTR_E_NULL, "bilinear_bwd: null bilinear_w");
    DCTR_REQUIRE(pl.nblk < 2 || a->senet_bilinear_w, DCTR_E_NULL, "bilinear_bwd: null senet_bilinear_w");
    // the outputs this mode has
    float* dw1 = pl.senet ? b->d_senet_w1 : nullptr;
    float* dw2 = pl.senet ? b->d_senet_w2 : nullptr;
    float* dws = pl.nblk == 2 ? b->d_senet_bilinear_w : nullptr;
    float* dwr = pl.nblk >= 1 ? b->d_bilinear_w : nullptr;
    DCTR_REQUIRE(b->dx || dw1 || dw2 || dws || dwr, DCTR_E_NULL, "bilinear_bwd: no gradient asked for (dx and every d_* are null)");
    if (pl.route_bytes)
        DCTR_REQUIRE_WORKSPACE("bilinear_bwd", "dctr_bilinear_bwd_workspace_bytes", b->workspace, b->workspace_bytes, pl.route_bytes);
    if (a->batch == 0) return DCTR_OK;
    BbParams p = {};
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
    p.ldt = pl.ldt;
    p.P = pl.P;
    p.tile_floats = pl.tile_floats;
    p.w1 = a->senet_w1;
    p.w2 = a->senet_w2;
    p.wt[0] = pl.nblk == 2 ? a->senet_bilinear_w : a->bilinear_w;
    p.wt[1] = a->bilinear_w;
    p.dout = b->d_out + b->d_out_offset;
    p.dout_stride = b->d_out_stride;
    p.dx = b->dx ? b->dx + b->dx_offset : nullptr;
    p.dx_stride = b->dx_stride;
    p.accumulate = b->accumulate;
    p.dw1 = dw1;
    p.dw2 = dw2;
    p.dw[0] = pl.nblk == 2 ? dws : dwr;
    p.dw[1] = pl.nblk == 2 ? dwr : nullptr;
    p.ws = pl.global ? (float*)b->workspace : nullptr;
    const int64_t n_tiles = dctr_ceil_div(a->batch, BB_S);
    // a persistent grid, one workgroup per compute unit (the tile takes most of the LDS), each walking its tiles: the grid bounds the
    // atomics, workgroups x the matrices' elements
    int64_t cap = b->max_blocks > 0 ? (int64_t)b->max_blocks : (int64_t)dctr_n_cus();
    if (pl.global && cap > pl.grid_max) cap = pl.grid_max;
    const dim3 grid((unsigned)(n_tiles < cap ? n_tiles : cap));
    if (pl.global) {
        DCTR_LAUNCH(bilinear_bwd_kernel<true>, grid, dim3(BB_THREADS), 0, (hipStream_t)stream, p);
    } else {
        const size_t lds = (size_t)pl.tile_floats * sizeof(float);
        static thread_local size_t granted[DCTR_MAX_DEVICES] = {0};
        hipError_t e = dctr_grant_lds((const void*)bilinear_bwd_kernel<false>, lds, granted);
        DCTR_REQUIRE(e == hipSuccess, (int)e, "bilinear_bwd: cannot raise dynamic LDS: %s", hipGetErrorString(e));
        DCTR_LAUNCH(bilinear_bwd_kernel<false>, grid, dim3(BB_THREADS), lds, (hipStream_t)stream, p);
    }
    return dctr_launch_status("dctr_bilinear_bwd");
}
