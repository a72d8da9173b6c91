// The embedding backward of the HIP training step: row gradients scatter-added into dense gradient tables.
//   dctr_embed_gather_fm_bwd   backward of embedding_lookup + concat (inputs.py:101-117, layers/utils.py:336-346), get_linear_logit
//                              (feature_column.py:171-210) and FM (layers/interaction.py:588-604)
//   dctr_embed_pool_bwd        backward of the sequence pooling (inputs.py:120-158, layers/sequence.py:76-106, :155-183)
//   dctr_embed_lookup_bwd      backward of a plain lookup (dctr_embed_lookup), with a sorted-tile form for skewed ids
// The reference has no code of its own for any of this (Keras autodiff): the formulas are the derivatives of the forward
// expressions cited at each section.
#include "dctr_common.h"
#include "embed_device.h"

namespace {

// ---------------------------------------------------------------------------------------------------
// embedding / linear / FM backward.  Lane (s, q) = 16-B chunk q of sample s, as in the forward gather.
//   d e_f = d dnn_in[b, off_f ..] + d_fm[b] * (S - e_f)     (S = sum over the FM fields of e: FM = 0.5 (S^2 - sum e^2))
//   d lin_f[row] += d_lin[b]
// ---------------------------------------------------------------------------------------------------
// One wave = 64 / LPR samples x LPR 16-B chunks; the workgroup's four waves split the FIELDS (wave w owns fields w, w + 4, ...):
// B = 4096, E = 16 -> 256 workgroups with 7 independent row reads per lane in flight (the first version walked all fields
// serially in 64 workgroups: 112 us).  S is summed per wave over its fields and combined through LDS.
// Measured and dropped (second half of round 2): 16 waves per workgroup (same 76 us: the 1.7 M float atomics run at the part's
// ~23 G distinct-address atomics/s) and a row census per table that lets rows hit once take a plain 16-B read-modify-write
// (62 us + two 6.6-us census launches = the same: then the ~640 k random sector accesses of the kernel are the limit, at the
// rate the forward gather reaches at this launch size).
// Any embedding width (round 6; the reference's embedding_dim is free, feature_column.py:44-45 gives e.g. 102 for "auto"): a lane owns
// the VEC-float chunks q, q + LPR, q + 2 LPR, ... of its sample's rows — ONE chunk when the widths fit 4 LPR <= 64 floats (the loop
// below then runs once: the kernel of rounds 2-5), several for wider rows; VEC = 1 (element per lane, scalar loads) when some width is
// not a multiple of 4 (rows are then not 16-B aligned).  The sum S is per chunk, so a chunk's share closes before the next starts.
template <int LPR, bool HASH, int VEC = 4>
__global__ __launch_bounds__(256) void gather_fm_bwd_kernel(dctr_gather_fm_args_t p, const dctr_field_grad_t* __restrict__ gr,
                                                            const float* __restrict__ d_in, int64_t d_stride,
                                                            const float* __restrict__ d_fm, const float* __restrict__ d_lin,
                                                            float* __restrict__ g_dense_lin_w,
                                                            const int32_t* __restrict__ dense_lin_rows) {
    constexpr int SPW = 64 / LPR, NWV = 4;
    __shared__ float s_part[NWV][64][VEC];
    // low-cardinality fields (DIN's `gender`: 2 rows for 2,048 samples = 1,024 atomics per address, ~90 ns each): their gradient
    // rows (and linear rows) accumulate in LDS and leave as one atomic per element and workgroup
    constexpr int SMALL_FLOATS = 2048, SMALL_FIELDS = 128, SMALL_VOCAB = 64;
    __shared__ float s_small[SMALL_FLOATS];
    __shared__ int s_soff[SMALL_FIELDS];
    __shared__ int s_total;
    if (threadIdx.x == 0) {
        int off = 0;
        for (int j = 0; j < p.n_fields && j < SMALL_FIELDS; ++j) {
            const int64_t vocab = ((cfield_ptr)p.fields)[j].vocab;
            const int64_t need = vocab * (((cfield_ptr)p.fields)[j].dim + 1);
            const bool small = gr[j].g_table != nullptr && vocab <= SMALL_VOCAB && off + need <= SMALL_FLOATS;
            s_soff[j] = small ? off : -1;
            if (small) off += (int)need;
        }
        s_total = off;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < s_total; i += 256) s_small[i] = 0.f;
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int s = lane / LPR, q0 = lane % LPR;
    const int64_t b = (int64_t)blockIdx.x * SPW + s;
    const bool valid = b < p.batch;
    cfield_ptr F = (cfield_ptr)p.fields;
    const float dfm = (valid && d_fm != nullptr) ? d_fm[b] : 0.f;
    const float dlin = (valid && d_lin != nullptr) ? d_lin[b] : 0.f;
    // the forward's dnn_in still holds every field's row of this sample (dctr_gather_fm_bwd_args_t.fwd->dnn_in; VEC = 4: 16-B aligned rows)
    const bool from_x = p.dnn_in != nullptr && (VEC == 1 || (p.out_stride % 4 == 0 && ((uintptr_t)p.dnn_in & 15) == 0));
    auto row_of = [&](const FieldRegs& f, int j) -> int64_t {
        int64_t r = f.identity ? b : read_id(p.ids, (int64_t)j * p.ids_stride_f + (valid ? b : 0) * p.ids_stride_b, p.ids_is_i64);
        if constexpr (HASH) {
            if (f.hash_mode != 0) r = resolve_row(r, f.hash_mode, p.ids_is_i64, f.vocab);
        }
        return r;
    };
    for (int q = q0; (q - q0) * VEC < p.max_dim; q += LPR) {      // (workgroup-uniform trip count: the barrier below is safe)
    // pass 1: S = sum over the FM fields of e_f (this wave's fields, then the four partial sums)
    float S[VEC];
#pragma unroll
    for (int c = 0; c < VEC; ++c) S[c] = 0.f;
    if (d_fm != nullptr) {
        if (q != q0) __syncthreads();                              // (the previous chunk's partial sums have been read)
        for (int j = wave; j < p.n_fields; j += NWV) {
            const FieldRegs f = load_field(F, j);
            if (!f.in_fm) continue;
            const int64_t r = row_of(f, j);
            const bool ok = valid && (uint64_t)r < (uint64_t)f.vocab && q * VEC < f.dim;
            float v[VEC];
            // (the forward left this row in the sample's dnn_in row: a coalesced read instead of a second random one — same bits)
            if (from_x && f.out_offset >= 0) load_vec<VEC>(p.dnn_in + (valid ? b : 0) * p.out_stride + f.out_offset + (ok ? q * VEC : 0), v);
            else load_vec<VEC>(f.table + (ok ? r : 0) * f.dim + (ok ? q * VEC : 0), v);
#pragma unroll
            for (int c = 0; c < VEC; ++c) S[c] += ok ? v[c] : 0.f;
        }
#pragma unroll
        for (int c = 0; c < VEC; ++c) s_part[wave][lane][c] = S[c];
        __syncthreads();
#pragma unroll
        for (int c = 0; c < VEC; ++c) S[c] = (s_part[0][lane][c] + s_part[1][lane][c]) + (s_part[2][lane][c] + s_part[3][lane][c]);
    }
    // pass 2: row gradients of this wave's fields
    for (int j = wave; j < p.n_fields; j += NWV) {
        const FieldRegs f = load_field(F, j);
        const int64_t r = row_of(f, j);
        const bool rok = valid && (uint64_t)r < (uint64_t)f.vocab;
        const bool ok = rok && q * VEC < f.dim;
        float* gt = gr[j].g_table;
        float* gl = gr[j].g_lin_table;
        const int so = j < SMALL_FIELDS ? s_soff[j] : -1;
        if (ok && gt != nullptr) {
            float g[VEC];
#pragma unroll
            for (int c = 0; c < VEC; ++c) g[c] = 0.f;
            if (f.out_offset >= 0 && d_in != nullptr) load_vec<VEC>(d_in + b * d_stride + f.out_offset + q * VEC, g);
            if (f.in_fm && d_fm != nullptr) {
                float v[VEC];
                if (from_x && f.out_offset >= 0) load_vec<VEC>(p.dnn_in + b * p.out_stride + f.out_offset + q * VEC, v);
                else load_vec<VEC>(f.table + r * f.dim + q * VEC, v);
#pragma unroll
                for (int c = 0; c < VEC; ++c) g[c] = fmaf(dfm, S[c] - v[c], g[c]);
            }
            if (gr[j].touched != nullptr) gr[j].touched[(r * f.dim + q * VEC) >> 2] = 1;  // (one byte per 16-B group: tables with dim % 4 == 0 only)
            if (so >= 0) {
#pragma unroll
                for (int c = 0; c < VEC; ++c) atomicAdd(&s_small[so + (int)r * f.dim + q * VEC + c], g[c]);
            } else {
                float* dst = gt + r * f.dim + q * VEC;
#pragma unroll
                for (int c = 0; c < VEC; ++c) unsafeAtomicAdd(dst + c, g[c]);
            }
        }
        if (rok && q == 0 && gl != nullptr && f.lin_table != nullptr) {
            if (so >= 0) atomicAdd(&s_small[so + (int)f.vocab * f.dim + (int)r], dlin);
            else unsafeAtomicAdd(gl + r, dlin);
        }
    }
    }   // chunks
    const int q = q0;
    // dense . Linear.kernel: d w[k] += sum_b d_lin[b] * dense[b, k]  — dense column k by wave k % 4, the wave's samples summed
    // before the one atomic (4096 atomics on one address serialise)
    if (g_dense_lin_w != nullptr && p.n_dense > 0) {
        for (int k = wave; k < p.n_dense; k += NWV) {
            const int row = dense_lin_rows != nullptr ? dense_lin_rows[k] : k;     // dense column k -> row of Linear.kernel
            if (row < 0) continue;
            float t = (valid && q == 0) ? dlin * p.dense[b * p.dense_stride + k] : 0.f;
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) t += __shfl_xor(t, m, 64);
            if (lane == 0) unsafeAtomicAdd(g_dense_lin_w + row, t);
        }
    }
    // the low-cardinality fields' LDS accumulators
    if (s_total > 0) {
        __syncthreads();
        for (int j = 0; j < p.n_fields && j < SMALL_FIELDS; ++j) {
            const int so = s_soff[j];
            if (so < 0) continue;
            const FieldRegs f = load_field(F, j);
            const int nt = (int)f.vocab * f.dim;
            for (int i = threadIdx.x; i < nt; i += 256) {
                const float v = s_small[so + i];
                if (v != 0.f) unsafeAtomicAdd(gr[j].g_table + i, v);
            }
            if (gr[j].g_lin_table != nullptr && f.lin_table != nullptr) {
                for (int i = threadIdx.x; i < (int)f.vocab; i += 256) {
                    const float v = s_small[so + nt + i];
                    if (v != 0.f) unsafeAtomicAdd(gr[j].g_lin_table + i, v);
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// backward of dctr_embed_pool (inputs.py:120-158, layers/sequence.py:76-106, :155-183): position t of sample b
// contributed  e_t * wt_t * mk_t  (sum), the same / denom (mean), or was the per-dimension maximum (max); the
// gradient of the pooled vector is scattered back to the rows with those factors.  Per-position weights are inputs.
// ---------------------------------------------------------------------------------------------------
// (any embedding width, as gather_fm_bwd_kernel: a lane walks the VEC-float chunks q0, q0 + LPR, ... of the row; VEC = 1 when dim % 4 != 0)
template <int LPR, int VEC = 4>
__global__ __launch_bounds__(256) void pool_bwd_kernel(dctr_pool_args_t a, const float* __restrict__ d_out, int64_t d_stride,
                                                       const float* __restrict__ d_lin_out, float* __restrict__ g_table,
                                                       float* __restrict__ g_lin_table) {
    constexpr int SPB = 256 / LPR;
    const int s = threadIdx.x / LPR, q0 = threadIdx.x % LPR;
    const int64_t b = (int64_t)blockIdx.x * SPB + s;
    if (b >= a.batch) return;
    for (int q = q0; q * VEC < a.dim || q == q0; q += LPR) {
    const int T = a.maxlen;
    const bool by_len = a.length != nullptr;
    const int len = by_len ? a.length[b] : 0;
    const float PAD = -4294967296.f;
    const bool has_w = a.weight != nullptr, wnorm = has_w && a.weight_norm;
    const bool colok = q * VEC < a.dim;
    auto row_of = [&](int t) { return resolve_row(read_id(a.idx, b * a.idx_stride + t, a.idx_is_i64), a.hash_mode, a.idx_is_i64, a.vocab); };
    auto mask_of = [&](int t, int64_t r) { return by_len ? (t < len) : (r != 0); };
    float wmax = -INFINITY, wden = 1.f;
    if (wnorm) {
        for (int t = 0; t < T; ++t) wmax = fmaxf(wmax, mask_of(t, row_of(t)) ? a.weight[b * (int64_t)T + t] : PAD);
        wden = 0.f;
        for (int t = 0; t < T; ++t) wden += expf((mask_of(t, row_of(t)) ? a.weight[b * (int64_t)T + t] : PAD) - wmax);
    }
    auto weight_of = [&](int t, bool m) {
        if (!has_w) return 1.f;
        const float w = a.weight[b * (int64_t)T + t];
        return wnorm ? expf((m ? w : PAD) - wmax) / wden : (m ? w : 0.f);
    };
    float dv[VEC];
#pragma unroll
    for (int c = 0; c < VEC; ++c) dv[c] = 0.f;
    if (colok && d_out != nullptr) load_vec<VEC>(d_out + b * d_stride + q * VEC, dv);
    const float dl = (d_lin_out != nullptr && q == 0) ? d_lin_out[b] : 0.f;
    const bool is_max = a.combiner == DCTR_POOL_MAX;
    float denom = 1.f;
    if (a.combiner == DCTR_POOL_MEAN) {
        float cnt = 0.f;
        if (!by_len)
            for (int t = 0; t < T; ++t) cnt += mask_of(t, row_of(t)) ? 1.f : 0.f;
        denom = (by_len ? (float)len : cnt) + 1e-8f;
    }
    // max: forward maxima per dimension (and of the 1-wide linear term), then the first position that attains each
    float mx[VEC], lmx = -INFINITY;
#pragma unroll
    for (int c = 0; c < VEC; ++c) mx[c] = -INFINITY;
    if (is_max) {
        for (int t = 0; t < T; ++t) {
            const int64_t r = row_of(t);
            const bool ok = (uint64_t)r < (uint64_t)a.vocab, m = mask_of(t, r);
            const float wt = weight_of(t, m), pen = m ? 0.f : 1e9f;
            float v[VEC];
#pragma unroll
            for (int c = 0; c < VEC; ++c) v[c] = 0.f;
            if (ok && colok) load_vec<VEC>(a.table + r * a.dim + q * VEC, v);
#pragma unroll
            for (int c = 0; c < VEC; ++c) mx[c] = fmaxf(mx[c], v[c] * wt - pen);
            if (q == 0 && a.lin_table != nullptr) lmx = fmaxf(lmx, (ok ? a.lin_table[r] : 0.f) * wt - pen);
        }
    }
    bool taken[VEC];
#pragma unroll
    for (int c = 0; c < VEC; ++c) taken[c] = false;
    bool ltaken = false;
    for (int t = 0; t < T; ++t) {
        const int64_t r = row_of(t);
        const bool ok = (uint64_t)r < (uint64_t)a.vocab;
        if (!ok && !is_max) continue;
        const bool m = mask_of(t, r);
        const float wt = weight_of(t, m);
        if (is_max) {
            // (an out-of-range id entered the forward maximum as a zero row: where it is the first position that attains the
            // maximum it takes the gradient with it — there is no row to add to — instead of passing it on to a later tie)
            const float pen = m ? 0.f : 1e9f;
            float v[VEC];
#pragma unroll
            for (int c = 0; c < VEC; ++c) v[c] = 0.f;
            if (ok && colok) load_vec<VEC>(a.table + r * a.dim + q * VEC, v);
            if (colok && g_table != nullptr) {
#pragma unroll
                for (int c = 0; c < VEC; ++c)
                    if (!taken[c] && v[c] * wt - pen == mx[c]) {
                        taken[c] = true;
                        if (ok) unsafeAtomicAdd(g_table + r * a.dim + q * VEC + c, dv[c] * wt);
                    }
            }
            if (q == 0 && g_lin_table != nullptr && a.lin_table != nullptr && !ltaken && (ok ? a.lin_table[r] : 0.f) * wt - pen == lmx) {
                ltaken = true;
                if (ok) unsafeAtomicAdd(g_lin_table + r, dl * wt);
            }
        } else {
            const float f = wt * (m ? 1.f : 0.f) / denom;
            if (f != 0.f) {
                if (colok && g_table != nullptr) {
#pragma unroll
                    for (int c = 0; c < VEC; ++c) unsafeAtomicAdd(g_table + r * a.dim + q * VEC + c, dv[c] * f);
                }
                if (q == 0 && g_lin_table != nullptr && a.lin_table != nullptr) unsafeAtomicAdd(g_lin_table + r, dl * f);
            }
        }
    }
    }   // chunks
}

// touched bytes of the rows a scatter kernel adds to (dctr_embed_lookup_bwd / dctr_embed_pool_bwd): every valid row an id
// resolves to — a superset of the rows that receive a non-zero gradient, which only costs the optimizer a read
__global__ __launch_bounds__(256) void mark_rows_kernel(const void* __restrict__ ids, int64_t n_rows, int n_cols, int64_t row_stride,
                                                        int is_i64, int hash_mode, int64_t vocab, int dim4, uint8_t* __restrict__ touched) {
    const int64_t total = n_rows * n_cols * dim4;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
        const int64_t e = t / dim4;
        const int q = (int)(t - e * dim4);
        const int64_t rr = e / n_cols;
        const int cc = (int)(e - rr * n_cols);
        const int64_t r = resolve_row(read_id(ids, rr * row_stride + cc, is_i64), hash_mode, is_i64, vocab);
        if ((uint64_t)r < (uint64_t)vocab) touched[r * dim4 + q] = 1;
    }
}
static void launch_mark_rows(hipStream_t st, const void* ids, int64_t n_rows, int n_cols, int64_t row_stride, int is_i64, int hash_mode,
                             int64_t vocab, int dim, uint8_t* touched) {
    const int dim4 = dim / 4;
    int64_t blocks = dctr_ceil_div(n_rows * n_cols * dim4, (int64_t)256);
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(mark_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, st, ids, n_rows, n_cols, row_stride, is_i64, hash_mode, vocab,
                       dim4, touched);
}

// backward of dctr_embed_lookup: g_table[row(idx[i]), :] += d_out[i, :dim]   (rows out of range are skipped, as the forward
// zero-fills them and raises the status flag)
__global__ __launch_bounds__(256) void lookup_bwd_kernel(dctr_lookup_args_t a, const float* __restrict__ d_out, int64_t d_stride,
                                                         float* __restrict__ g_table) {
    const int64_t total = a.n * a.dim;
    for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (int64_t)gridDim.x * 256) {
        const int64_t i = o / a.dim;
        const int c = (int)(o - i * a.dim);
        const float g = d_out[i * d_stride + c];
        if (g == 0.f) continue;
        const int64_t row = resolve_row(read_id(a.idx, i, a.idx_is_i64), a.hash_mode, a.idx_is_i64, a.vocab);
        if ((uint64_t)row < (uint64_t)a.vocab) unsafeAtomicAdd(g_table + row * a.dim + c, g);
    }
}

// The same scatter for skewed ids (DIN's behaviour sequences: half of the B*T positions are padding id 0, and under training-mode
// Dice the padded keys DO receive gradient through the batch statistics — 51,000 x 32 atomics on ONE row took 1.6 ms per table):
// a workgroup sorts a tile of LB_TILE positions by row in LDS (bitonic), then 64 / dimP walkers per wave run over contiguous
// stretches of the sorted tile, summing runs of equal rows in registers: one atomic per (run, column) instead of one per position.
constexpr int LB_TILE = 1024;
__global__ __launch_bounds__(256) void lookup_bwd_tile_kernel(dctr_lookup_args_t a, const float* __restrict__ d_out, int64_t d_stride,
                                                              float* __restrict__ g_table, int dimP) {
    __shared__ uint32_t key[LB_TILE];
    __shared__ uint16_t pos[LB_TILE];
    constexpr uint32_t NONE = 0xffffffffu;
    const int64_t base = (int64_t)blockIdx.x * LB_TILE;
    for (int j = threadIdx.x; j < LB_TILE; j += 256) {
        const int64_t i = base + j;
        uint32_t k = NONE;
        if (i < a.n) {
            const int64_t row = resolve_row(read_id(a.idx, i, a.idx_is_i64), a.hash_mode, a.idx_is_i64, a.vocab);
            if ((uint64_t)row < (uint64_t)a.vocab) k = (uint32_t)row;
        }
        key[j] = k;
        pos[j] = (uint16_t)j;
    }
    __syncthreads();
    for (int size = 2; size <= LB_TILE; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < LB_TILE / 2; t += 256) {
                const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                const bool up = (lo & size) == 0;
                const uint32_t k0 = key[lo], k1 = key[hi];
                if ((k0 > k1) == up) {
                    key[lo] = k1; key[hi] = k0;
                    const uint16_t p0 = pos[lo]; pos[lo] = pos[hi]; pos[hi] = p0;
                }
            }
            __syncthreads();
        }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int sub_n = 64 / dimP, sub = lane / dimP, c = lane % dimP;
    const int per = LB_TILE / (4 * sub_n);
    const int j0 = (wave * sub_n + sub) * per;
    const bool col = c < a.dim;
    uint32_t cur = NONE;
    float acc = 0.f;
    constexpr int U = 8;
    for (int j = j0; j < j0 + per; j += U) {
        uint32_t kk[U];
        float gg[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            kk[u] = key[j + u];
            const int64_t i = base + pos[j + u];
            gg[u] = (kk[u] != NONE && col) ? d_out[i * d_stride + c] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (kk[u] != cur) {
                if (cur != NONE && col && acc != 0.f) unsafeAtomicAdd(g_table + (int64_t)cur * a.dim + c, acc);
                cur = kk[u];
                acc = gg[u];
            } else {
                acc += gg[u];
            }
        }
    }
    if (cur != NONE && col && acc != 0.f) unsafeAtomicAdd(g_table + (int64_t)cur * a.dim + c, acc);
}

}  // namespace

extern "C" int dctr_embed_lookup_bwd(const dctr_lookup_args_t* fwd, const float* d_out, int64_t d_stride, float* g_table, uint8_t* touched,
                                     void* stream) {
    DCTR_REQUIRE(fwd != nullptr, DCTR_E_NULL, "embed_lookup_bwd: null args");
    DCTR_REQUIRE(fwd->n >= 0 && fwd->dim >= 1 && d_stride >= fwd->dim && fwd->vocab >= 1, DCTR_E_DIM, "embed_lookup_bwd: bad sizes");
    if (fwd->n == 0) return DCTR_OK;
    DCTR_REQUIRE(fwd->idx && d_out && g_table, DCTR_E_NULL, "embed_lookup_bwd: null pointer");
    if (touched != nullptr) {
        DCTR_REQUIRE(fwd->dim % 4 == 0, DCTR_E_DIM, "embed_lookup_bwd: touched bytes need dim %% 4 == 0 (dim %d)", fwd->dim);
        launch_mark_rows((hipStream_t)stream, fwd->idx, fwd->n, 1, 1, fwd->idx_is_i64, fwd->hash_mode, fwd->vocab, fwd->dim, touched);
    }
    // (dim >= 3: a walker's stretch of LB_TILE / (4 * 64 / dimP) sorted entries must cover its 8-entry load batches)
    if (fwd->dim >= 3 && fwd->dim <= 64 && fwd->vocab < 0xffffffffLL && fwd->n >= LB_TILE) {
        int dimP = 1;
        while (dimP < fwd->dim) dimP <<= 1;
        const int64_t tiles = dctr_ceil_div(fwd->n, (int64_t)LB_TILE);
        DCTR_REQUIRE(tiles <= 0x7fffffffLL, DCTR_E_DIM, "embed_lookup_bwd: n too large");
        hipLaunchKernelGGL(lookup_bwd_tile_kernel, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, *fwd, d_out, d_stride,
                           g_table, dimP);
        return dctr_launch_status("dctr_embed_lookup_bwd");
    }
    int64_t blocks = dctr_ceil_div(fwd->n * fwd->dim, (int64_t)256);
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(lookup_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, *fwd, d_out, d_stride, g_table);
    return dctr_launch_status("dctr_embed_lookup_bwd");
}

extern "C" int dctr_embed_gather_fm_bwd(const dctr_gather_fm_bwd_args_t* a, void* stream) {
    DCTR_REQUIRE(a != nullptr && a->fwd != nullptr, DCTR_E_NULL, "embed_gather_fm_bwd: null args");
    const dctr_gather_fm_args_t* f = a->fwd;
    DCTR_REQUIRE(f->batch >= 0 && f->n_fields >= 0, DCTR_E_DIM, "embed_gather_fm_bwd: bad sizes");
    if (f->batch == 0 || f->n_fields == 0) return DCTR_OK;
    DCTR_REQUIRE(f->fields && f->ids && a->grads, DCTR_E_NULL, "embed_gather_fm_bwd: null fields / ids / grads");
    DCTR_REQUIRE(!f->any_pitch && f->max_dim >= 1, DCTR_E_UNSUPPORTED, "embed_gather_fm_bwd: plain (not record-form) tables, max_dim >= 1");
    DCTR_REQUIRE(a->d_dnn_in == nullptr || !f->all_dim4 || (a->d_stride % 4 == 0 && dctr_aligned16(a->d_dnn_in)), DCTR_E_ALIGN,
                 "embed_gather_fm_bwd: d_dnn_in must be 16-B aligned with a stride %% 4 == 0");
    hipStream_t st = (hipStream_t)stream;
    if (!f->all_dim4) {
        // some width is not a multiple of 4 (rows / DNN-input columns not 16-B aligned): element per lane, 16 lanes per sample
        const int64_t blocks1 = dctr_ceil_div(f->batch, (int64_t)4);
        DCTR_REQUIRE(blocks1 <= 0x7fffffffLL, DCTR_E_DIM, "embed_gather_fm_bwd: batch too large");
        if (f->any_hash)
            hipLaunchKernelGGL((gather_fm_bwd_kernel<16, true, 1>), dim3((unsigned)blocks1), dim3(256), 0, st, *f, a->grads, a->d_dnn_in,
                               a->d_stride, a->d_fm, a->d_lin, a->g_dense_lin_w, a->dense_lin_rows);
        else
            hipLaunchKernelGGL((gather_fm_bwd_kernel<16, false, 1>), dim3((unsigned)blocks1), dim3(256), 0, st, *f, a->grads, a->d_dnn_in,
                               a->d_stride, a->d_fm, a->d_lin, a->g_dense_lin_w, a->dense_lin_rows);
        return dctr_launch_status("dctr_embed_gather_fm_bwd");
    }
    int lpr = 1;
    while (lpr * 4 < f->max_dim && lpr < 16) lpr <<= 1;                          // (rows wider than 64 floats: several chunks per lane)
    const int64_t blocks = dctr_ceil_div(f->batch, (int64_t)(64 / lpr));        // one wave's worth of samples per workgroup
    DCTR_REQUIRE(blocks <= 0x7fffffffLL, DCTR_E_DIM, "embed_gather_fm_bwd: batch too large");
#define CALL_BWD(L)                                                                                                       \
    do {                                                                                                                  \
        if (f->any_hash)                                                                                                  \
            hipLaunchKernelGGL((gather_fm_bwd_kernel<L, true>), dim3((unsigned)blocks), dim3(256), 0, st, *f, a->grads,   \
                               a->d_dnn_in, a->d_stride, a->d_fm, a->d_lin, a->g_dense_lin_w, a->dense_lin_rows);        \
        else                                                                                                              \
            hipLaunchKernelGGL((gather_fm_bwd_kernel<L, false>), dim3((unsigned)blocks), dim3(256), 0, st, *f, a->grads,  \
                               a->d_dnn_in, a->d_stride, a->d_fm, a->d_lin, a->g_dense_lin_w, a->dense_lin_rows);        \
    } while (0)
    switch (lpr) {
        case 1: CALL_BWD(1); break;
        case 2: CALL_BWD(2); break;
        case 4: CALL_BWD(4); break;
        case 8: CALL_BWD(8); break;
        default: CALL_BWD(16); break;
    }
#undef CALL_BWD
    return dctr_launch_status("dctr_embed_gather_fm_bwd");
}

extern "C" int dctr_embed_pool_bwd(const dctr_pool_bwd_args_t* a, void* stream) {
    DCTR_REQUIRE(a != nullptr && a->fwd != nullptr, DCTR_E_NULL, "embed_pool_bwd: null args");
    const dctr_pool_args_t* f = a->fwd;
    DCTR_REQUIRE(f->batch >= 0 && f->maxlen >= 1 && f->dim >= 1, DCTR_E_DIM, "embed_pool_bwd: bad sizes");
    if (f->batch == 0) return DCTR_OK;
    DCTR_REQUIRE(f->idx && f->table, DCTR_E_NULL, "embed_pool_bwd: null idx / table");
    const bool vec4 = f->dim % 4 == 0;
    DCTR_REQUIRE(a->d_out == nullptr || !vec4 || (a->d_stride % 4 == 0 && dctr_aligned16(a->d_out)), DCTR_E_ALIGN,
                 "embed_pool_bwd: d_out must be 16-B aligned with a stride %% 4 == 0");
    DCTR_REQUIRE(a->touched == nullptr || vec4, DCTR_E_DIM, "embed_pool_bwd: touched bytes need dim %% 4 == 0 (dim %d)", f->dim);
    int lpr = 1;
    while (lpr * 4 < f->dim && lpr < 16) lpr <<= 1;          // (rows wider than 64 floats: several chunks per lane)
    if (!vec4) lpr = 16;                                     // element per lane
    const int64_t blocks = dctr_ceil_div(f->batch, (int64_t)(256 / lpr));
    DCTR_REQUIRE(blocks <= 0x7fffffffLL, DCTR_E_DIM, "embed_pool_bwd: batch too large");
    hipStream_t st = (hipStream_t)stream;
    if (a->touched != nullptr && a->g_table != nullptr)
        launch_mark_rows(st, f->idx, f->batch, f->maxlen, f->idx_stride, f->idx_is_i64, f->hash_mode, f->vocab, f->dim, a->touched);
    if (!vec4) {
        hipLaunchKernelGGL((pool_bwd_kernel<16, 1>), dim3((unsigned)blocks), dim3(256), 0, st, *f, a->d_out, a->d_stride, a->d_lin_out,
                           a->g_table, a->g_lin_table);
        return dctr_launch_status("dctr_embed_pool_bwd");
    }
#define CALL_PB(L) \
    hipLaunchKernelGGL((pool_bwd_kernel<L>), dim3((unsigned)blocks), dim3(256), 0, st, *f, a->d_out, a->d_stride, a->d_lin_out, \
                       a->g_table, a->g_lin_table)
    switch (lpr) {
        case 1: CALL_PB(1); break;
        case 2: CALL_PB(2); break;
        case 4: CALL_PB(4); break;
        case 8: CALL_PB(8); break;
        default: CALL_PB(16); break;
    }
#undef CALL_PB
    return dctr_launch_status("dctr_embed_pool_bwd");
}
