/*
 * dctr.h — C ABI of libdctr_hip.so: the MI355X (gfx950) kernels behind DeepCTR's
 * embedding-lookup + feature-interaction forward path.
 *
 * The reference (shenweichen/DeepCTR, /root/reference) has NO native / FFI layer: every op on this
 * path is a TensorFlow op sequence issued from a Keras `Layer.call`.  Each entry point below therefore
 * replaces one such `call` (or a fused run of them); the reference symbol it stands in for is cited
 * as deepctr/<file>:<lines>.  INTEGRATION.md shows the ctypes stub a DeepCTR maintainer would add.
 *
 * Conventions (all entry points):
 *   - extern "C", plain pointers and sizes, no C++ types, no exceptions across the boundary.
 *   - every pointer inside an argument struct is a DEVICE pointer on the current HIP device unless
 *     the field comment says "host"; the struct itself is host memory, read during the call only.
 *   - the caller owns every buffer (inputs, outputs, workspace); the library never allocates,
 *     frees or synchronises; work is enqueued on `stream` (a hipStream_t; NULL = default stream).
 *   - return value: 0 = enqueued; <0 = DCTR_E_* argument error (nothing enqueued);
 *     >0 = hipError_t reported by the launch.  dctr_last_error() gives a thread-local message.
 *   - functions are re-entrant and stateless; ordering is by `stream` only.
 *   - fp32 tensors are row-major and contiguous unless a stride field says otherwise.
 */
#ifndef DCTR_H_
#define DCTR_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DCTR_ABI_VERSION 13

enum {
    DCTR_OK = 0,
    DCTR_E_NULL = -1,        /* required pointer is NULL                    */
    DCTR_E_DIM = -2,         /* size / dimension out of the supported range */
    DCTR_E_ALIGN = -3,       /* pointer or stride not aligned as documented */
    DCTR_E_ENUM = -4,        /* unknown enum value                          */
    DCTR_E_UNSUPPORTED = -5  /* valid request this build does not implement */
};

/* bits OR-ed into the optional device status word by the gather kernels */
enum {
    DCTR_STATUS_INDEX_OOR = 1,   /* an id outside [0, vocabulary): the outputs of that ROW are unspecified (the stand-alone
                                    gather substitutes zeros, the fused dctr_embed_mlp_fwd kernels read table row 0); every
                                    other row is unaffected, no memory outside the tables is touched                  */
    DCTR_STATUS_TIMEOUT = 2      /* a bounded in-kernel wait of the streaming dctr_embed_mlp_fwd kernel expired: the
                                    outputs of that launch are invalid (a defect, reported instead of a hung GPU)     */
};

int dctr_abi_version(void);
const char* dctr_last_error(void);
/* name of the gfx target the kernels were compiled for ("gfx950") */
const char* dctr_target_arch(void);
/* Measurement aid (bench.py): arm a probe for the NEXT kernel launched by this host thread; the launch then
 * carries a start/stop event pair (hipExtLaunchKernelGGL), so dctr_profile_last_ms() returns the duration of
 * that one dispatch as the GPU timestamps it (same quantity as rocprofv3 --kernel-trace), or -1 if none. */
int dctr_profile_next_launch(void);
float dctr_profile_last_ms(void);
/* The same for the next n (<= 256) launches of this host thread — launches that are in flight together on several
 * streams take longer than an isolated one, and that is what rocprofv3 reports for the timed region.
 * dctr_profile_collect waits for them, writes their durations [ms] and returns how many were timed. */
int dctr_wall_clock_khz(void);   /* rate of the device wall clock used by dctr_mlp_args_t.probe */
int dctr_profile_arm(int32_t n);
int dctr_profile_collect(float* ms, int32_t n);

/* ------------------------------------------------------------------------------------------------
 * host input pipeline — what Keras does with the dict of ndarrays handed to predict()/fit()
 * (examples/run_classification_criteo.py:40-50).  HOST pointers, no device work: rows [row_lo, row_lo + n_rows) of every
 * column are converted to dst_kind and written feature-major into dst (column c at dst + c * dst_col_stride elements,
 * normally page-locked memory), by up to n_threads host threads.  Float -> integer conversion truncates (numpy astype).
 * ------------------------------------------------------------------------------------------------ */
enum { DCTR_HOST_I32 = 0, DCTR_HOST_I64 = 1, DCTR_HOST_F32 = 2, DCTR_HOST_F64 = 3 };
typedef struct {
    const void* src;              /* first element of the column (row 0)                                 */
    int64_t stride_bytes;         /* distance between consecutive rows (a column of an [N, k] array: k * itemsize) */
    int32_t kind;                 /* DCTR_HOST_*                                                         */
    int32_t reserved_;
} dctr_host_col_t;
int dctr_host_pack_columns(const dctr_host_col_t* cols, int32_t n_cols, int64_t row_lo, int64_t n_rows, void* dst,
                           int64_t dst_col_stride, int32_t dst_kind, int32_t n_threads);

/* ------------------------------------------------------------------------------------------------
 * a2  Hash.call — deepctr/layers/utils.py:89-112
 *     out = Fingerprint64(decimal_ascii(x)) mod nb  (uint64 modulo, stored as int64),
 *     nb = num_buckets - (mask_zero ? 1 : 0);  mask_zero: out = (out + 1) * (x != 0).
 *     Bit-exact with tf.strings.to_hash_bucket_fast(tf.as_string(x), nb).
 * ------------------------------------------------------------------------------------------------ */
int dctr_hash_bucket_i32(const int32_t* x, int64_t n, int64_t num_buckets, int mask_zero, int64_t* out,
                         void* stream);
int dctr_hash_bucket_i64(const int64_t* x, int64_t n, int64_t num_buckets, int mask_zero, int64_t* out,
                         void* stream);
/* string-dtype features: `bytes` = concatenated UTF-8, offsets[n+1] (int64) delimit element i;
 * mask_zero masks the literal string "0" (utils.py:95,108-110). */
int dctr_hash_bucket_bytes(const uint8_t* bytes, const int64_t* offsets, int64_t n, int64_t num_buckets,
                           int mask_zero, int64_t* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a2 over the id matrix of a gather (declared after dctr_field_t below): dctr_hash_fields.
 * ------------------------------------------------------------------------------------------------ */

/* ------------------------------------------------------------------------------------------------
 * a3/a4/a6/a7/a8 fused:  embedding_lookup (deepctr/inputs.py:101-117, keras Embedding gather) for
 * every SparseFeat + concat into the DNN-input layout (layers/utils.py:336-346) + Linear.call
 * (layers/utils.py:160-175, the 1-wide `linear0sparse_emb_*` tables of feature_column.py:171-210)
 * + FM.call (layers/interaction.py:588-604), optional in-kernel Hash (a2).
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    const float* table;      /* [vocab, dim] fp32; 16-B aligned when dim % 4 == 0                      */
    const float* lin_table;  /* [vocab] fp32 (1-wide linear table) or NULL = no first-order term        */
    int64_t vocab;
    int32_t dim;             /* embedding_dim of this field                                             */
    int32_t out_offset;      /* column of this field inside a dnn_in row; <0: not copied                */
    int32_t in_fm;           /* 1: participates in the FM term                                          */
    int32_t hash_mode;       /* 0: id is the row; 1: Hash(vocab); 2: Hash(vocab, mask_zero=True)        */
    int32_t identity;        /* 1: row = sample index b (field pre-pooled by dctr_embed_pool); id unused */
    int32_t row_pitch;       /* 0: rows are `dim` floats apart and the linear table is a separate [vocab] vector.
                                != 0 (ABI 10, the RECORD form; a multiple of 4, >= dim + 1): row r lies at table + r * row_pitch
                                and its linear entry at lin_table[r * row_pitch] — the caller keeps the first-order weight behind
                                the embedding row (lin_table = table + dim), so that one 128-B line serves both reads of a
                                dim-16 field: 2 x row_pitch = 32 floats.  Honoured by dctr_embed_gather_fm and dctr_embed_mlp_fwd
                                (tile and row-chained kernels; there dim 16 and row_pitch 32 only); every other entry point that
                                takes descriptors rejects args->any_pitch (DCTR_E_UNSUPPORTED)                           */
} dctr_field_t;

enum { DCTR_POOL_SUM = 0, DCTR_POOL_MEAN = 1, DCTR_POOL_MAX = 2 };   /* combiner of a5 (dctr_embed_pool below, dctr_pool_seq_t) */

/* a sequence feature pooled inside dctr_embed_mlp_fwd (dctr_gather_fm_args_t.pools; 32 bytes).  Contract (the descriptors live in
 * device memory, the library cannot check them): int32 ids, idx 8-B aligned, idx_stride even, maxlen even and >= 2, the id matrix and
 * the embedding table below 4 GiB each (32-bit lane offsets from scalar bases). */
typedef struct {
    const void* idx;         /* [rows, idx_stride] int32 ids of the staged data (row 0)                 */
    const int32_t* length;   /* [rows] valid lengths (length_name given) or NULL = mask_zero on id != 0 */
    int64_t idx_stride;      /* elements                                                                */
    int32_t maxlen;          /* T                                                                       */
    int32_t combiner;        /* DCTR_POOL_SUM or DCTR_POOL_MEAN                                         */
} dctr_pool_seq_t;

typedef struct {
    const dctr_field_t* fields;   /* DEVICE array [n_fields]                                            */
    const void* ids;              /* DEVICE id matrix: field j, sample b at ids[j*ids_stride_f + b*ids_stride_b]
                                     (DeepCTR feeds one id column per feature -> natural layout [F, B]);
                                     one row per field, in field order (rows of identity fields unused)   */
    int64_t ids_stride_f;         /* in elements                                                        */
    int64_t ids_stride_b;
    int32_t ids_is_i64;           /* 0: int32 ids, 1: int64 ids                                         */
    int32_t n_fields;
    int32_t max_dim;              /* max over fields of dim (host copy, selects the lane layout)        */
    int32_t all_dim4;             /* 1: every dim % 4 == 0, tables 16-B aligned, out offsets % 4 == 0    */
    int32_t any_hash;             /* 1: some field has hash_mode != 0 (host copy; selects the hashing build)*/
    int32_t n_dense;              /* width of the dense matrix (sum of DenseFeat dimensions), 0 = none   */
    const float* dense;           /* DEVICE [B, dense_stride] dense feature values or NULL              */
    int64_t dense_stride;
    const float* dense_lin_w;     /* DEVICE [n_dense] = Linear.kernel (layers/utils.py:150-158) or NULL */
    int32_t dense_out_offset;     /* first dense column inside a dnn_in row; <0: not copied             */
    int32_t dense_copy_cols;      /* leading dense columns copied into dnn_in (the rest only feed the linear
                                     term: DenseFeat present in linear_feature_columns only); <= n_dense   */
    int64_t batch;
    float* dnn_in;                /* [B, out_stride] or NULL                                            */
    int64_t out_stride;           /* elements; % 4 == 0 when all_dim4                                   */
    float* fm_logit;              /* [B] or NULL:  0.5 * sum_d((sum_f e)^2 - sum_f e^2) over in_fm fields */
    float* lin_logit;             /* [B] or NULL:  sum_f lin_table_f[row] + dense . dense_lin_w         */
    int32_t* status;              /* optional device word, DCTR_STATUS_* bits are OR-ed in              */
    int32_t split_col;            /* dctr_embed_mlp_fwd only; 0 = none.  A dnn_in column (multiple of 64) with:
                                     fields[0 .. split_field) write only columns < split_col, fields[split_field ..)
                                     and the dense passthrough only columns >= split_col.  Lets the fused kernel
                                     build the DNN-input tile in two K-halves (half the LDS, two workgroups per CU). */
    int32_t split_field;
    int32_t uniform_dim;          /* dctr_embed_mlp_fwd only; E > 0 promises: every field has dim == E and out_offset ==
                                     field index * E (the reference's plain DNN input, inputs.py:101-117 + layers/utils.py:
                                     336-346; fields pre-pooled by dctr_embed_pool — identity == 1 — included, see any_identity).
                                     Launches of >= 64 rows per CU then take a persistent kernel: with E in {16, 32} and a DNN
                                     of two or three layers with units[0] in {128, 256}, units[1] in {64, 128}, units[2] in
                                     {64, 128} (ReLU / linear, optional BatchNormalization) the row-chained kernel
                                     (csrc/chain_device.h); else with E in {16, 32, 64} and no identity field the streaming
                                     kernel (LDS-DMA gather ring, 64-row tiles).  0 = unknown / not uniform              */
    int32_t any_identity;         /* 1: some field has identity != 0 (host copy of the descriptors' flags)               */
    int32_t any_pitch;            /* 1: some field has row_pitch != 0 (host copy; ABI 10)                                 */
    int32_t n_pools;              /* dctr_embed_mlp_fwd only (ABI 12); 0 = none.  The LAST n_pools fields are VarLenSparseFeat whose sequences
                                     are pooled INSIDE the launch (inputs.py:120-158, layers/sequence.py:76-106; combiner sum / mean): their
                                     descriptors carry table / lin_table / vocab / dim / out_offset / in_fm as a SparseFeat's would
                                     (identity = 0, hash_mode = 0; their rows of the id matrix are unused), pools[i] the ids of the i-th.
                                     Taken by the row-chained kernel only (launches of >= 64 rows per CU, uniform_dim 16, ReLU / linear DNN
                                     of the 256-128-x family, no identity / hashed / record-form fields, n_pools <= 4 and
                                     pool_pieces + 2 <= n_fields - n_pools: the sequences' rows are requested two positions per
                                     layer-0 step of the SparseFeat k-blocks); everything else answers DCTR_E_UNSUPPORTED — pre-pool with
                                     dctr_embed_pool and hand the fields over as identity fields (ask dctr_mlp_fwd_supported first).
                                     The pooled vectors are bit-identical to dctr_embed_pool's (same order over t, same arithmetic).  */
    const dctr_pool_seq_t* pools; /* DEVICE array [n_pools] (the caller's, like `fields`)                                   */
    int64_t pool_row0;            /* the launch's row 0 is row pool_row0 of the pools' id matrices / length vectors        */
    int32_t pool_pieces;          /* host copy: sum over the pools of maxlen / 2                                          */
    int32_t pool_flags;           /* host copy: bit i = pools[i].combiner == DCTR_POOL_MEAN, bit 4 + i = pools[i].length != NULL */
} dctr_gather_fm_args_t;

int dctr_embed_gather_fm(const dctr_gather_fm_args_t* args, void* stream);

/* a2 Hash.call (deepctr/layers/utils.py:89-112, applied per SparseFeat at inputs.py:108-110) over a whole id matrix in one launch:
 * out[j, b] = Hash(ids[j, b]; vocab_j, mask_zero = (hash_mode_j == 2)) for fields with hash_mode != 0, = ids[j, b] for the others
 * (and identity fields).  `fields` = the gather's DEVICE descriptors; ids / out: [n_fields, batch] with the given strides (elements),
 * int32 or int64 each (a 32-bit `out` needs every hashed vocab < 2^31 and unhashed ids that fit).  The persistent kernels of
 * dctr_embed_mlp_fwd take plain rows: run this first, then the call with descriptors whose hash_mode is 0 and any_hash = 0. */
int dctr_hash_fields(const dctr_field_t* fields, int32_t n_fields, const void* ids, int64_t ids_stride_f, int64_t ids_stride_b,
                     int32_t ids_is_i64, int64_t batch, void* out, int64_t out_stride_f, int32_t out_is_i64, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a5  varlen_embedding_lookup + WeightedSequenceLayer + SequencePoolingLayer
 *     deepctr/inputs.py:120-158, layers/sequence.py:76-106 and :155-183.
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    const void* idx;         /* [B, T] ids, row stride idx_stride (elements)                            */
    const float* table;      /* [vocab, dim]                                                            */
    const float* lin_table;  /* [vocab] or NULL: also pool the 1-wide linear table into lin_out         */
    const int32_t* length;   /* [B] valid lengths (length_name given) or NULL = mask_zero on idx != 0   */
    const float* weight;     /* [B, T] per-position weights (weight_name) or NULL                       */
    int64_t vocab;
    int64_t idx_stride;
    int64_t batch;
    int32_t idx_is_i64;
    int32_t maxlen;          /* T                                                                       */
    int32_t dim;
    int32_t combiner;        /* DCTR_POOL_*                                                             */
    int32_t weight_norm;     /* softmax-normalise the weights over valid positions (sequence.py:170-177)*/
    int32_t hash_mode;       /* 0 none, 2 = Hash(vocab, mask_zero=True) (inputs.py:125-126)             */
    float* out;              /* [B, out_stride] pooled vectors                                          */
    int64_t out_stride;
    float* lin_out;          /* [B] pooled 1-wide term or NULL                                          */
    int32_t* status;
} dctr_pool_args_t;

int dctr_embed_pool(const dctr_pool_args_t* args, void* stream);

/* stand-alone WeightedSequenceLayer.call (layers/sequence.py:155-183) on a materialised seq [B,T,dim]:
 * out = seq * w, w = weight masked by `mask` [B,T] bytes or `length` [B] (0 outside; softmax over T of the
 * -2^32+1 padded weights when weight_norm). */
int dctr_seq_weight_fwd(const float* seq, const float* weight, const uint8_t* mask, const int32_t* length,
                        int64_t batch, int32_t maxlen, int32_t dim, int32_t weight_norm, float* out, void* stream);

/* plain per-position lookup [B,T] -> [B,T,dim] (+ mask byte per position), used for DIN keys
 * (deepctr/models/sequence/din.py:68-69) and by the eager `embedding_lookup` API. */
typedef struct {
    const void* idx;
    const float* table;
    int64_t vocab;
    int64_t n;               /* number of ids (B*T)                                                     */
    int32_t idx_is_i64;
    int32_t dim;
    int32_t hash_mode;
    int32_t pad_;
    float* out;              /* [n, out_stride] (out_stride >= dim): lets callers write into a concat   */
    int64_t out_stride;
    uint8_t* mask;           /* [n] (post-hash idx != 0) or NULL                                        */
    int32_t* status;
} dctr_lookup_args_t;

int dctr_embed_lookup(const dctr_lookup_args_t* args, void* stream);
/* up to 8 lookups in ONE launch (DIN's query features + behaviour sequences, din.py:62-76).  A lookup with mask != NULL
 * additionally ANDs (id != 0) of n_extra (<= 4) further id arrays of the same length into its mask (HOST arrays of
 * DEVICE pointers / int64 flags): the conjunction of the mask_zero sequences' masks. */
int dctr_embed_lookup_multi(const dctr_lookup_args_t* args, int32_t n_lookups, const void* const* extra_mask_idx,
                            const int32_t* extra_is_i64, int32_t n_extra, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a8  FM.call stand-alone — deepctr/layers/interaction.py:588-604.   x [B,F,E] (sample stride x_stride) -> y [B]
 * ------------------------------------------------------------------------------------------------ */
int dctr_fm_fwd(const float* x, int64_t batch, int64_t x_stride, int32_t fields, int32_t dim, float* y, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a9  CrossNet.call — deepctr/layers/interaction.py:405-424
 *     vector: x_{l+1} = x0 * (x_l . w_l) + b_l + x_l ;  matrix: x_{l+1} = x0 .* (W_l x_l + b_l) + x_l
 *     kernels: [layers, d] (vector) or [layers, d, d] (matrix, W[i][j] row-major); bias [layers, d].
 * ------------------------------------------------------------------------------------------------ */
enum { DCTR_CROSS_VECTOR = 0, DCTR_CROSS_MATRIX = 1 };
/* Device scratch the matrix form needs when dim % 4 != 0 or `kernels` is not 16-B aligned (the W rows are re-packed to
 * a 16-B aligned stride for the dwordx4 weight loads); 0 otherwise. */
size_t dctr_crossnet_workspace_bytes(int32_t dim, int32_t layers, int32_t mode, const float* kernels);
int dctr_crossnet_fwd(const float* x, int64_t batch, int32_t dim, int64_t x_stride, const float* kernels,
                      const float* bias, int32_t layers, int32_t mode, float* y, int64_t y_stride, void* workspace,
                      size_t workspace_bytes, void* stream);
/* The same with the branch's share of the model's head fused in (ABI 6; models/dcn.py:61-64: Dense(1, use_bias=False) over
 * Concatenate([cross_out, deep_out]) = cross_out . kernel[:d] + deep_out . kernel[d:]):  logit[b] = x_L[b, :] . head_w  is written
 * beside the layer output (y != NULL) or instead of it (y == NULL: the [B, d] output never goes to HBM); the caller hands `logit` to
 * the DNN's fused head as one of dctr_mlp_args_t.add.  workspace_ready: the workspace already holds the re-packed rows of THESE
 * kernels (the re-pack launch is skipped; inference with fixed weights). */
typedef struct {
    const float* x;               /* [B, x_stride]                                                        */
    int64_t batch;
    int64_t x_stride;
    int32_t dim;
    int32_t layers;
    int32_t mode;                 /* DCTR_CROSS_VECTOR | DCTR_CROSS_MATRIX                                */
    int32_t workspace_ready;
    const float* kernels;
    const float* bias;
    float* y;                     /* [B, y_stride] or NULL (then head_w / logit are required)             */
    int64_t y_stride;
    void* workspace;              /* dctr_crossnet_workspace_bytes() bytes, 16-B aligned (or NULL when 0) */
    size_t workspace_bytes;
    const float* head_w;          /* [dim] or NULL                                                        */
    float* logit;                 /* [B] written, or NULL                                                 */
    float* save_u;                /* training, matrix form: NULL, or [layers, B, dim] — u_l = W_l x_l (bias excluded) written for
                                     dctr_crossnet_bwd_args_t.saved_u                                                       */
    float* save_x;                /* ... and [layers - 1, B, dim] — x_1 .. x_{L-1} for saved_x (NULL with one layer)        */
} dctr_crossnet_args_t;
int dctr_crossnet_head_fwd(const dctr_crossnet_args_t* args, void* stream);
/* ABI 8 — the same over the embeddings of a gather (models/dcn.py:48-66: dnn_input = combined_dnn_input(sparse embeddings, dense values)
 * -> CrossNet -> its share of Dense(1)): matrix parameterization; the workgroup's [64, dim] tile of the DNN input is read from the
 * embedding tables and the dense matrix inside the kernel (gather: the dctr_embed_gather_fm arguments of the same batch — fields / ids /
 * strides / dense / status are used; every field a plain lookup of width uniform_dim % 4 == 0 at column field * uniform_dim, the dense
 * columns behind them; args->x / x_stride are ignored), so the DNN input never has to exist in HBM.  Launches of >= 64 rows per CU with
 * dim <= 512 (the 64-row kernel whose layer outputs wait in registers); anything else returns DCTR_E_UNSUPPORTED — use
 * dctr_embed_gather_fm + dctr_crossnet_head_fwd.  Inference only (save_u / save_x must be NULL). */
int dctr_crossnet_gather_head_fwd(const dctr_crossnet_args_t* args, const dctr_gather_fm_args_t* gather, void* stream);
/* ABI 13 — would dctr_crossnet_head_fwd / dctr_crossnet_fwd (gather == NULL) or dctr_crossnet_gather_head_fwd (gather != NULL) take these
 * arguments?  Runs every shape check and kernel-shape decision of the call (rows per workgroup by batch and dim, LDS) without launching;
 * device pointers are not looked at (save_u non-NULL = "the training forward"; of `gather` the summary fields n_fields / batch /
 * uniform_dim / all_dim4 / any_hash / any_identity / any_pitch / ids_stride_b / dense_copy_cols / dense_out_offset).  1 = yes, 0 = no
 * (dctr_last_error() carries the reason).  A matrix form wider than the kernels hold runs as dctr_sgemm + dctr_crossnet_matrix_step. */
int dctr_crossnet_fwd_supported(const dctr_crossnet_args_t* args, const dctr_gather_fm_args_t* gather);
/* ABI 11 — the elementwise half of ONE matrix-form layer (interaction.py:416-420) for inputs wider than the kernels above hold on chip
 * (their [16, dim] tiles of x_0 / x_l / x_{l+1} live in LDS: dim <= ~800; wider calls return DCTR_E_UNSUPPORTED):
 *     x_next[b, c] = x0[b, c] * (u[b, c] + bias[c]) + xl[b, c],     u = x_l W_l^T from dctr_sgemm ([B, dim], contiguous).
 * x_next may alias xl (not x0 unless xl == x0 is no longer needed). */
int dctr_crossnet_matrix_step(const float* x0, int64_t x0_stride, const float* xl, int64_t xl_stride, const float* u, const float* bias,
                              int64_t batch, int32_t dim, float* x_next, int64_t x_next_stride, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a10 CIN.call — deepctr/layers/interaction.py:277-325   (outer product + 1x1 conv on f32 MFMA)
 *     x [B,F0,D];  filters[k]: [F0*F_k, H_k] row-major (the reference's [1,F0*F_k,H_k] squeezed,
 *     row index i*F_k + j);  bias[k]: [H_k];  out [B, featuremap_num] (already summed over D).
 * ------------------------------------------------------------------------------------------------ */
enum { DCTR_ACT_LINEAR = 0, DCTR_ACT_RELU = 1, DCTR_ACT_SIGMOID = 2, DCTR_ACT_TANH = 3, DCTR_ACT_DICE = 4,
       /* tf.keras 2.x activation names of the DNN (reference layers/activation.py:75-85 hands the name to tf.keras.layers.Activation).
        * Taken by dctr_mlp_fwd / dctr_embed_mlp_fwd (+ _supported, _workspace_bytes), dctr_mlp_bwd (+ _workspace_bytes) and
        * dctr_dnn_train_layer_fwd / _bwd ONLY; every other entry point that reads a DCTR_ACT_* answers them as it answers an
        * unknown code.  elu: alpha = 1; hard_sigmoid: clip(0.2 z + 0.5, 0, 1) (the Keras 2 form); swish = silu = z sigmoid(z);
        * gelu: the exact form 0.5 z (1 + erf(z / sqrt 2)) (approximate=False). */
       DCTR_ACT_ELU = 5, DCTR_ACT_SELU = 6, DCTR_ACT_SOFTPLUS = 7, DCTR_ACT_SOFTSIGN = 8, DCTR_ACT_EXPONENTIAL = 9,
       DCTR_ACT_HARD_SIGMOID = 10, DCTR_ACT_SWISH = 11, DCTR_ACT_GELU = 12 };
typedef struct {
    const float* x;               /* sample b at x + b * x_stride, then [F0, D] row-major */
    int64_t batch;
    int64_t x_stride;             /* elements between samples (>= F0*D): lets CIN read the dnn_in concat in place */
    int32_t fields;               /* F0 */
    int32_t dim;                  /* D  */
    int32_t n_layers;
    int32_t split_half;
    int32_t activation;           /* DCTR_ACT_LINEAR | RELU | SIGMOID | TANH */
    int32_t workspace_ready;      /* 0: the call (re)writes `workspace` from filters[0] (one small launch in front of the kernel).
                                     1: the caller vouches `workspace` still holds what an earlier call with the same filters[0]
                                     VALUES, fields and layer_size[0] wrote: the fold launch is skipped (predict() over many batches) */
    const int32_t* layer_size;    /* HOST array [n_layers] */
    const float* const* filters;  /* HOST array of n_layers DEVICE pointers */
    const float* const* bias;     /* HOST array of n_layers DEVICE pointers */
    float* out;                   /* [B, featuremap_num] */
    void* workspace;              /* NULL, or device scratch of dctr_cin_workspace_bytes() bytes, 16-B aligned: layer 0 multiplies x_0
                                     with itself (z[i,j] = z[j,i]), so with a workspace the kernel walks the F0 (F0 + 1) / 2 pairs
                                     i <= j against W[ij] + W[ji] folded there (same result up to the rounding of that sum; 1.3x
                                     faster at C3).  Without it layer 0 walks all F0 x F0 products. */
    size_t workspace_bytes;
    float* const* save_y;         /* NULL, or HOST array of n_layers DEVICE pointers (entries may be NULL): layer k's
                                   * activations y_k [B*D, H_k] row-major (row b*D + d, ALL H_k maps) are also written there
                                   * — what dctr_cin_bwd otherwise recomputes with one GEMM per layer (ABI 4) */
} dctr_cin_args_t;
/* Bytes of `workspace` for these arguments (fields, dim, n_layers, layer_size, split_half are read; batch is not): the fold of layer 0,
 * plus — ABI 13 — for samples the kernel does not take whole, room for 1,024 samples of the sliced route.  CIN never mixes embedding
 * dimensions before its final reduce_sum over d (interaction.py:288-295, :322-323), and the reference puts no limit on embedding_dim:
 * a sample wider than one workgroup's MFMA tiles (embedding_dim > 128; > 64 when the maps of a 128-row tile would not fit the LDS) is
 * walked as dim / dd pseudo-samples of dd dimensions (dd = the largest divisor of dim the kernel takes) laid out in the workspace by a
 * pre-pass, their partial map sums added in the order of d by a post-pass; rows in chunks of what the workspace holds.  A network with
 * a layer of more maps than ANY tile height leaves LDS for (~480; the reference takes any layer_size) runs layer by layer as the
 * reference writes it (interaction.py:288-300): z = x_0 (outer) x_k materialised per chunk of samples, the 1 x 1 convolution on the
 * library's GEMM, bias + activation, the direct maps summed over d (room for up to 256 samples, at most 256 MiB unless 16 samples need
 * more).  For such arguments the workspace is REQUIRED (DCTR_E_NULL without, before anything is launched; any workspace with room for
 * >= 64 / >= 16 samples works); save_y is written as for whole samples (row b * dim + d). */
size_t dctr_cin_workspace_bytes(const dctr_cin_args_t* args);
int dctr_cin_fwd(const dctr_cin_args_t* args, void* stream);
/* ABI 13 — would dctr_cin_fwd (gather == NULL) / dctr_cin_gather_fwd (gather != NULL; fused_head != 0: with head_w / logit) take these
 * arguments?  Runs every shape check and kernel-shape decision of the call without launching; device pointers are not looked at
 * (args->layer_size, a HOST array, is; of `gather` the summary fields n_fields / batch / uniform_dim / all_dim4 / any_hash / any_identity /
 * any_pitch).  1 = yes, 0 = no (dctr_last_error() carries the reason).  Hosts ask this instead of re-deriving the kernels' limits. */
int dctr_cin_fwd_supported(const dctr_cin_args_t* args, const dctr_gather_fm_args_t* gather, int32_t fused_head);

/* ABI 8 — CIN.call over the embeddings of a gather, as deepctr/models/xdeepfm.py:52-66 wires it: exFM_in = concat_func(sparse_embedding_list,
 * axis=1) -> CIN -> Dense(1, use_bias=False).  The workgroup's [samples, F0, D] tile is read from the embedding tables inside the kernel
 * (gather: the dctr_embed_gather_fm arguments of the same batch — fields / ids / strides / status are used; every field a plain lookup
 * of width args->dim, dim % 4 == 0, no hashed and no pre-pooled field, else DCTR_E_UNSUPPORTED), args->x / x_stride are ignored and the
 * DNN input never has to exist in HBM.  head_w [featuremap_num] + logit [B] (both or neither): the Dense(1) over the summed maps is taken
 * on chip and only logit[b] leaves (args->out may then be NULL); without them args->out receives the maps as in dctr_cin_fwd.
 * An id outside its vocabulary reads row 0 and raises DCTR_STATUS_INDEX_OOR in *gather->status.  Inference only (save_y must be NULL). */
int dctr_cin_gather_fwd(const dctr_cin_args_t* args, const dctr_gather_fm_args_t* gather, const float* head_w, float* logit, void* stream);

/* ------------------------------------------------------------------------------------------------
 * InteractingLayer.call x n_layers — deepctr/layers/interaction.py:749-779, stacked as deepctr/models/autoint.py:61-64
 *     per layer l, X_l [F, E_l] (E_0 = dim, E_l = d*H after): Q, K, V, R = X_l W; per head h: P = softmax_keys(Q_h K_h^T
 *     (/ sqrt(d) when scaling)), O_h = P V_h; heads concatenated on the last axis (column h*d + j); + R when use_res; ReLU.
 *     Output flattened f-major (index f*d*H + h*d + j), as Flatten() of the last layer.
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    const float* x;               /* sample b at x + b * x_stride, then [F, dim] row-major */
    int64_t batch;
    int64_t x_stride;             /* elements between samples (>= fields*dim): reads the dnn_in concat in place */
    int32_t fields;               /* F */
    int32_t dim;                  /* E_0 */
    int32_t n_layers;             /* >= 1 */
    int32_t att_embedding_size;   /* d */
    int32_t head_num;             /* H */
    int32_t use_res;              /* 0 | 1 */
    int32_t scaling;              /* 0 | 1 */
    const float* const* layers;   /* HOST array [n_layers * 4] of DEVICE pointers: layer l's query, key, value, res at 4l .. 4l+3,
                                     each [E_l, d*H] row-major (Keras layout); res may be NULL when use_res == 0 */
    float* out;                   /* NULL, or [B, F*d*H] at out_stride: the flattened output of the last layer */
    int64_t out_stride;
    const float* head_w;          /* NULL, or [F*d*H]: the Dense(1) over the flattened output taken on chip ... */
    float* logit;                 /* ... into logit [B] (head_w and logit both or neither; out and / or the head) */
    void* workspace;              /* NULL, or device scratch of dctr_interacting_workspace_bytes() bytes, 16-B aligned */
    size_t workspace_bytes;
} dctr_interacting_args_t;
/* Bytes of `workspace` these arguments need (0: none).  A workgroup keeps its samples' X, Q, K, V, R in LDS across every layer when
 * one sample fits; a sample too large for the LDS (large F, wide d*H) runs the same layers with those buffers in the workspace
 * (room for <= 256 workgroups, at most 256 MiB unless one sample needs more), and the workspace is then REQUIRED (DCTR_E_NULL
 * without, before anything is launched).  More than 32 layers run as launches of <= 32 layers chained through `out` (or, with the
 * head only, through batch * F * d*H floats of the workspace: batch is read for that case alone). */
size_t dctr_interacting_workspace_bytes(const dctr_interacting_args_t* args);
int dctr_interacting_fwd(const dctr_interacting_args_t* args, void* stream);

/* Backward of dctr_interacting_fwd over the whole stack, one launch; nothing is saved by the forward (every layer's input is
 * recomputed per tile of samples and kept on chip).  fwd: x, batch, x_stride, fields, dim, n_layers, att_embedding_size, head_num,
 * use_res, scaling, layers and workspace (+ bytes) are read; out / out_stride / head_w / logit are ignored.  The upstream gradient is
 * dy [B, dy_stride] w.r.t. the flattened last layer (index f*d*H + h*d + j).  Per layer, last to first, with s = 1/sqrt(d) when
 * scaling else 1, Z = concat_h(P_h V_h) (+ X W_res), Y = relu(Z):
 *     dZ = dY [Z > 0];   dV_h = P_h^T dZ_h;   dP = dZ_h V_h^T;   delta_i = sum_j P_ij dP_ij;   dS = s P (dP - delta);
 *     dQ_h = dS K_h;   dK_h = dS^T Q_h;   dX = dQ W_q^T + dK W_k^T + dV W_v^T (+ dZ W_res^T);   dX of layer l is dY of layer l-1.
 * dx [B, dx_stride]: columns [0, F*dim) are written (accumulate = 0) or added to (1), the others untouched; no atomics inside a
 * sample, so dx is bit-identical from call to call.  ACCUMULATED (d_layers itself or any entry may be NULL):
 * d_layers[4l + m] += X_l^T dM for M = Q, K, V (, Z for res) — summed per workgroup over all its tiles, one atomic per workgroup and
 * element.  Arithmetic is fp32 on the f32 matrix cores for the projections and the dX / dW products, as the forward.
 * A sample whose buffers exceed the LDS (large F, wide d*H, many layers) runs with them in fwd.workspace
 * (dctr_interacting_bwd_workspace_bytes; REQUIRED then: DCTR_E_NULL without, DCTR_E_ALIGN when not 16-B aligned).  More than 32
 * layers, or one sample's buffers past 2^31 floats, answer DCTR_E_UNSUPPORTED before anything is launched
 * (dctr_interacting_bwd_supported: 1 / 0).  Argument errors (DCTR_E_NULL / _DIM / _ENUM / _ALIGN) launch and write nothing. */
typedef struct {
    dctr_interacting_args_t fwd;
    const float* dy;              /* [B, dy_stride], dy_stride >= fields*d*H */
    int64_t dy_stride;
    float* dx;                    /* NULL, or [B, dx_stride], dx_stride >= fields*dim */
    int64_t dx_stride;
    float* const* d_layers;       /* NULL, or HOST array [n_layers * 4] of DEVICE pointers, shapes of fwd.layers; each may be NULL */
    int32_t accumulate;           /* 0 | 1: dx written | added to */
    int32_t max_blocks;           /* 0 = 2 per compute unit, else the most workgroups to launch (each walks its tiles) */
} dctr_interacting_bwd_args_t;
int dctr_interacting_bwd_supported(const dctr_interacting_bwd_args_t* args);          /* host only */
size_t dctr_interacting_bwd_workspace_bytes(const dctr_interacting_bwd_args_t* args); /* host only; 0: none (or an argument error) */
int dctr_interacting_bwd(const dctr_interacting_bwd_args_t* args, void* stream);

/* ------------------------------------------------------------------------------------------------
 * SENETLayer.call + BilinearInteraction.call — deepctr/layers/interaction.py:1067-1221, wired as deepctr/models/fibinet.py:50-58
 *     x_f [dim] for f < F (F >= 2, one dim).  SENET: Z = mean(x_f) [F]; A1 = relu(Z W_1) [r]; A2 = relu(A1 W_2) [F];
 *     v_f = A2[f] x_f.  Bilinear over inputs u: for each pair (i, j), i < j in itertools.combinations order (P = F(F-1)/2 pairs),
 *     p_ij = (u_i W) (.) u_j with W = W_0 (ALL), W_i (EACH, i < F-1) or W_ij (INTERACTION, pair index) — output [P, dim] pair-major.
 *   mode MODEL: out row = per pair p [p over v (senet_bilinear_w), dim floats | p over x (bilinear_w), dim floats], then the
 *               dense_cols columns of x behind its F*dim embedding columns: FiBiNET's whole DNN input (Flatten of the two outputs
 *               concatenated on their last axis, then the dense values), 2*P*dim + dense_cols floats;
 *   mode SENET: out row = [v_0 .. v_{F-1}] (F*dim floats);
 *   mode LAYER: out row = the bilinear over x with bilinear_w (P*dim floats), no SENET.
 *   The (v_i W) (.) v_j of MODEL is computed as A2[i] A2[j] ((x_i W) (.) x_j): equal within fp32 rounding, not bit for bit.
 * ------------------------------------------------------------------------------------------------ */
enum { DCTR_BILINEAR_ALL = 0, DCTR_BILINEAR_EACH = 1, DCTR_BILINEAR_INTERACTION = 2 };
enum { DCTR_BILINEAR_MODE_MODEL = 0, DCTR_BILINEAR_MODE_SENET = 1, DCTR_BILINEAR_MODE_LAYER = 2 };
typedef struct {
    const float* x;               /* sample b at x + b * x_stride, then [F, dim] row-major (+ the dense columns in mode MODEL) */
    int64_t batch;
    int64_t x_stride;             /* elements between samples (>= fields*dim (+ dense_cols)): reads the dnn_in concat in place */
    int32_t fields;               /* F >= 2 */
    int32_t dim;                  /* >= 1 */
    int32_t bilinear_type;        /* DCTR_BILINEAR_ALL | EACH | INTERACTION */
    int32_t mode;                 /* DCTR_BILINEAR_MODE_MODEL | SENET | LAYER */
    int32_t reduction_size;       /* r = columns of senet_w1 (>= 1; unused in mode LAYER) */
    int32_t dense_cols;           /* mode MODEL: columns copied behind the two blocks (else 0) */
    const float* senet_w1;        /* [F, r] row-major (modes MODEL, SENET) */
    const float* senet_w2;        /* [r, F] */
    const float* const* senet_bilinear_w;   /* DEVICE array of nW DEVICE pointers to [dim, dim] (Keras layout) matrices: the layer over
                                               the SENET output (mode MODEL); nW = 1 (ALL), F-1 (EACH), P (INTERACTION) */
    const float* const* bilinear_w;         /* DEVICE array [nW]: the layer over x (modes MODEL, LAYER) */
    float* out;                   /* [B, width] at out_stride */
    int64_t out_stride;
    void* workspace;              /* NULL, or device scratch of dctr_bilinear_workspace_bytes() bytes, 16-B aligned */
    size_t workspace_bytes;
} dctr_bilinear_args_t;
/* Bytes of `workspace` these arguments need (0: none).  A workgroup keeps 16 samples' embeddings (and, for ALL / EACH, x_i W per
 * field) in LDS; a shape too large for the LDS (large fields*dim) runs the same kernel with those buffers in the workspace (room
 * for <= 256 workgroups, at most 256 MiB unless one tile needs more), and the workspace is then REQUIRED (DCTR_E_NULL without,
 * before anything is launched).  Argument errors (null pointers, F < 2, unknown type or mode, dim < 1, short strides) are
 * reported before any launch. */
size_t dctr_bilinear_workspace_bytes(const dctr_bilinear_args_t* args);
int dctr_bilinear_fwd(const dctr_bilinear_args_t* args, void* stream);

/* Backward of dctr_bilinear_fwd, one launch, every mode and bilinear_type; nothing is saved by the forward (the kernel loads the same
 * X tile again and recomputes Z, A1, A2).  fwd: batch, x, x_stride, fields, dim, bilinear_type, mode, reduction_size, dense_cols and
 * the weights are read as the forward reads them; out / out_stride / workspace are ignored.  d_out is the gradient of the forward's
 * output row, read in place from a wider row.  Per pair (i, j), i < j, with g^s / g^r [dim] the gradients of its SENET-side / raw-side
 * output, W^s / W^r the two layers' matrices of the pair and c = A2[i] A2[j]:
 *   raw side:   dx_i += (g^r (.) x_j) W^T;  dx_j += g^r (.) (x_i W);  dW += x_i^T (g^r (.) x_j), summed over the samples;
 *   SENET side: the same three with c g^s and W^s;  dA2[i] += A2[j] <g^s, s_ij>, dA2[j] += A2[i] <g^s, s_ij>, s_ij = (x_i W^s) (.) x_j;
 *   SENET chain per sample: dA2 gated by A2 > 0 (relu'(0) = 0);  dW_2 += A1^T dA2;  dA1 = dA2 W_2^T gated by A1 > 0;  dW_1 += Z^T dA1;
 *               dx_f[e] += (dA1 W_1^T)[f] / dim for every e.
 *   mode SENET: dx_f = A2[f] g_f plus the chain with dA2[f] = <g_f, x_f>.  mode LAYER: the raw side alone, with bilinear_w.
 * dx: the F*dim columns from dx_offset of a row of dx_stride floats are written (accumulate = 0) or added to (1); in mode MODEL with
 * dense_cols > 0 the dense_cols columns behind them receive (or are added) d_out's tail: the exact transpose of the forward's in-place
 * read of x.  The other columns stay untouched.  One owner per element and no atomics: dx is bit-identical from call to call.
 * The four weight gradients are ACCUMULATED into (zero them first): summed per workgroup over all the tiles it walks, one float atomic
 * per element and workgroup (dim > 16: per element and tile; EACH / ALL: per element, workgroup and chunk / walk of the pairs), so they may differ in the last bits from call to call.  dx and each
 * d_* may be NULL (not wanted); all of the mode's outputs NULL is DCTR_E_NULL.  Arithmetic is fp32, the products on the f32 matrix
 * cores as the forward.
 * A tile too large for the LDS runs in `workspace` (dctr_bilinear_bwd_workspace_bytes; REQUIRED then: DCTR_E_NULL without, DCTR_E_ALIGN
 * when not 16-B aligned, before anything is launched).  No shape the forward takes is refused, unless one tile's buffers pass 2^30
 * floats: DCTR_E_UNSUPPORTED before anything is launched (dctr_bilinear_bwd_supported: 1 / 0).  Argument errors (DCTR_E_NULL / _DIM /
 * _ENUM / _ALIGN: null pointers, F < 2, unknown type or mode, short strides) launch and write nothing. */
typedef struct {
    dctr_bilinear_args_t fwd;
    const float* d_out;           /* row b at d_out + b * d_out_stride + d_out_offset, the forward's output width */
    int64_t d_out_stride;         /* >= d_out_offset + width */
    int64_t d_out_offset;         /* >= 0 */
    float* dx;                    /* may be NULL: row b at dx + b * dx_stride + dx_offset, fields*dim (+ dense_cols) floats */
    int64_t dx_stride;            /* >= dx_offset + fields*dim (+ dense_cols) */
    int64_t dx_offset;            /* >= 0 */
    int32_t accumulate;           /* 0 | 1: dx written | added to */
    int32_t max_blocks;           /* 0: the library's grid (one workgroup per compute unit); > 0 caps it (each workgroup walks its tiles) */
    float* d_senet_w1;            /* may be NULL; [F, r], ACCUMULATED into (modes MODEL, SENET) */
    float* d_senet_w2;            /* may be NULL; [r, F] */
    float* d_senet_bilinear_w;    /* may be NULL; ONE contiguous [nW, dim, dim] (mode MODEL) */
    float* d_bilinear_w;          /* may be NULL; ONE contiguous [nW, dim, dim] (modes MODEL, LAYER) */
    void* workspace;              /* NULL, or device scratch of dctr_bilinear_bwd_workspace_bytes() bytes, 16-B aligned */
    size_t workspace_bytes;
} dctr_bilinear_bwd_args_t;
size_t dctr_bilinear_bwd_workspace_bytes(const dctr_bilinear_bwd_args_t* args); /* host only; 0: none (or an argument error) */
int dctr_bilinear_bwd_supported(const dctr_bilinear_bwd_args_t* args);          /* host only, reads shapes only */
int dctr_bilinear_bwd(const dctr_bilinear_bwd_args_t* args, void* stream);

/* ------------------------------------------------------------------------------------------------
 * FwFMLayer.call / FEFMLayer.call — deepctr/layers/interaction.py:1351-1499, wired as deepctr/models/fwfm.py and deepfefm.py
 *     x_f [dim] for f < F (F >= 2, one dim): the embeddings of ONE feature group.  Pairs (i, j), i < j, in itertools.combinations
 *     order, P = F(F-1)/2 of them.
 *   kind FEFM: s_p = x_i^T (W_p + W_p^T) x_j with one [dim, dim] matrix per pair; the kernel forms W + W^T from the live W.
 *              pairs_out row b = [s_0 .. s_{P-1}] at pairs_out + b * pairs_stride + pairs_offset (optional);
 *              logit_out[b] = sum_p s_p (+ add[b]) (optional).  At least one of the two outputs.
 *   kind FWFM: logit_out[b] = sum_{i<j} r[i][j] <x_i, x_j> (+ add[b]) with r the [F, F] field_pair_strengths, of which only the
 *              strict upper triangle is read.  pairs_out must be NULL.
 *   The sums run in the kernel's own order: equal to the reference's within fp32 rounding, not bit for bit.
 * ------------------------------------------------------------------------------------------------ */
enum { DCTR_FIELDPAIR_FEFM = 0, DCTR_FIELDPAIR_FWFM = 1 };
typedef struct {
    const float* x;               /* sample b's [F, dim] row-major block at x + b * x_stride + x_offset */
    int64_t batch;
    int64_t x_stride;             /* elements between samples (>= x_offset + fields*dim): reads a group's slice of dnn_in in place */
    int64_t x_offset;             /* first column of the group (>= 0) */
    int32_t fields;               /* F >= 2 */
    int32_t dim;                  /* >= 1 */
    int32_t kind;                 /* DCTR_FIELDPAIR_FEFM | DCTR_FIELDPAIR_FWFM */
    int32_t reserved;             /* 0 */
    const void* weights;          /* FEFM: DEVICE array of P DEVICE pointers to [dim, dim] row-major matrices, combinations order;
                                     FWFM: const float* [F, F] row-major */
    float* pairs_out;             /* FEFM: NULL, or [B, P] at pairs_stride / pairs_offset; FWFM: NULL */
    int64_t pairs_stride;         /* elements between rows of pairs_out (>= pairs_offset + P) */
    int64_t pairs_offset;         /* first column written (>= 0): lets the scalars land behind the dense columns of a DNN-input row */
    const float* add;             /* NULL, or [B] added to logit_out (e.g. the linear logit) */
    float* logit_out;             /* [B]; FEFM: optional, FWFM: required */
    void* workspace;              /* NULL, or device scratch of dctr_fieldpair_workspace_bytes() bytes, 16-B aligned */
    size_t workspace_bytes;
} dctr_fieldpair_args_t;
/* Bytes of `workspace` these arguments need (0: none, also for invalid arguments).  A workgroup keeps its samples' embeddings in
 * LDS; a shape too large for the LDS (large fields*dim) runs the same kernel with that tile in the workspace (room for <= 256
 * workgroups), and the workspace is then REQUIRED (DCTR_E_NULL without, before anything is launched).  No shape is refused for its
 * size.  Argument errors (null pointers, F < 2, dim < 1, unknown kind, short strides, misaligned workspace) are reported before
 * any launch. */
size_t dctr_fieldpair_workspace_bytes(const dctr_fieldpair_args_t* args);
int dctr_fieldpair_fwd(const dctr_fieldpair_args_t* args, void* stream);

/* Backward of dctr_fieldpair_fwd, one launch; nothing is saved by the forward (the kernel loads the same X tile again).  fwd: batch, x,
 * x_stride, x_offset, fields, dim, kind, weights and workspace (+ bytes) are read as the forward reads them; pairs_out / pairs_stride /
 * pairs_offset / add / logit_out are ignored.  With g_b,ij = d_pairs[b, ij] + d_logit[b] (a NULL term is 0) and S = W + W^T:
 *   FEFM: dx_i = sum_{j != i} g_ij S_ij x_j, the pair (i, j) with j < i being the matrix of (j, i);
 *         d_weights[ij] += A + A^T with A = sum_b g_b,ij x_i x_j^T.  At least one of d_pairs / d_logit.
 *   FWFM: dx_i = d_logit sum_{j != i} r'_ij x_j with r' the strict upper triangle mirrored; d_weights[i][j] += sum_b d_logit_b <x_i, x_j>
 *         for i < j: the diagonal and the lower triangle of d_weights are not touched.  d_logit is required, d_pairs must be NULL.
 * dx: the F*dim columns from dx_offset of a row of dx_stride floats are written (accumulate = 0) or added to (1), the others
 * untouched; one owner per (sample, field, column) and no atomics, so dx is bit-identical from call to call.  d_weights is ACCUMULATED
 * into (zero it first): summed per workgroup over all the tiles it walks, one float atomic per element and workgroup (dim > 16: two per
 * element and tile), so weight gradients may differ in the last bits from call to call.  Arithmetic is fp32, FEFM's products on the
 * f32 matrix cores as the forward.  With neither dx nor d_weights nothing is launched.
 * A tile too large for the LDS runs in fwd.workspace (dctr_fieldpair_bwd_workspace_bytes; REQUIRED then: DCTR_E_NULL without,
 * DCTR_E_ALIGN when not 16-B aligned).  No shape the forward takes is refused, unless one tile's buffers pass 2^30 floats (FwFM over
 * more than ~32,000 fields): DCTR_E_UNSUPPORTED before anything is launched, every output untouched (dctr_fieldpair_bwd_supported:
 * 1 / 0).  Argument errors (DCTR_E_NULL / _DIM / _ENUM / _ALIGN) launch and write nothing. */
typedef struct {
    dctr_fieldpair_args_t fwd;
    const float* d_pairs;         /* FEFM only, may be NULL: row b at d_pairs + b * d_pairs_stride + d_pairs_offset, P floats */
    int64_t d_pairs_stride;       /* >= d_pairs_offset + P */
    int64_t d_pairs_offset;       /* >= 0 */
    const float* d_logit;         /* may be NULL (FEFM): [batch], the gradient w.r.t. logit_out */
    float* dx;                    /* may be NULL: row b at dx + b * dx_stride + dx_offset, fields*dim floats */
    int64_t dx_stride;            /* >= dx_offset + fields*dim */
    int64_t dx_offset;            /* >= 0 */
    int32_t accumulate;           /* 0 | 1: dx written | added to */
    int32_t reserved;             /* 0 */
    float* d_weights;             /* may be NULL; ACCUMULATED into.  FEFM: one contiguous [P, dim, dim]; FWFM: [F, F] */
    int32_t max_blocks;           /* 0: the library's choice (FEFM: one workgroup per compute unit); > 0 caps the grid */
    int32_t reserved2;            /* 0 */
} dctr_fieldpair_bwd_args_t;
size_t dctr_fieldpair_bwd_workspace_bytes(const dctr_fieldpair_bwd_args_t* args); /* host only; 0: none (or an argument error) */
int dctr_fieldpair_bwd_supported(const dctr_fieldpair_bwd_args_t* args);          /* host only, reads shapes only */
int dctr_fieldpair_bwd(const dctr_fieldpair_bwd_args_t* args, void* stream);

/* ------------------------------------------------------------------------------------------------
 * ONN's field-aware embedding lookup + pair products — deepctr/models/onn.py:59-99 (no layer class in the reference)
 *     F >= 2 fields of one embedding_dim d.  Field j owns ONE fused table [vocab_j, F-1, d] (rows row_pitch floats apart): row r holds
 *     the embeddings of id r towards every partner field, slot k = partner i in field order with j itself skipped — the reference's
 *     sparse_emb_<j>_<i>/embeddings is the strided view [:, k, :].  Per sample and pair (i, j), i < j, in itertools.combinations order
 *     (P = F(F-1)/2 pairs):  out[p*d + e] = row_i[slot of j][e] * row_j[slot of i][e]   (reduce_sum: out[p] = the sum over e),
 *     then optionally out = out * scale + shift (the inference form of the BatchNormalization over the P*d, or P, columns), then the
 *     n_dense dense values — combined_dnn_input([ffm_out], dense): the model's whole DNN-input row, in one launch from the ids.
 *     A field with identity != 0 is pre-pooled (a VarLenSparseFeat pooled over the whole fused row by dctr_embed_pool with
 *     dim = (F-1)*d): its row is the sample index, vocab = the rows of that buffer.  An id outside [0, vocab) raises
 *     DCTR_STATUS_INDEX_OOR and enters the products as a row of zeros; nothing outside the tables is read.
 *     Without scale / shift an output is one fp32 product, with them one product and one fma, on both routes: the same bits.
 *     Routes: tiles of samples gathered whole into LDS (every table byte read once, coalesced), or — rows beyond the LDS, or
 *     route = DCTR_FFM_ROUTE_DIRECT — both operands read from global memory.  No shape is refused for its size up to 2^27 floats per
 *     output row; neither route needs a workspace (dctr_ffm_workspace_bytes() = 0; the two members are reserved).
 * ------------------------------------------------------------------------------------------------ */
enum { DCTR_FFM_ROUTE_AUTO = 0, DCTR_FFM_ROUTE_DIRECT = 1, DCTR_FFM_ROUTE_LDS = 2 };
typedef struct {
    const float* rows;            /* [vocab, row_pitch] fp32: the fused table (or the pre-pooled buffer); 16-B aligned rows are read 16 B at a time */
    const void* ids;              /* sample b's id at ids[b * ids_stride]; unused when identity */
    int64_t vocab;
    int64_t row_pitch;            /* floats between rows, >= (F-1)*d */
    int64_t ids_stride;           /* elements */
    int32_t ids_is_i64;           /* 0: int32 ids, 1: int64 ids */
    int32_t identity;             /* 1: row = sample index b */
} dctr_ffm_field_t;
typedef struct {
    const dctr_ffm_field_t* fields;   /* DEVICE array [n_fields], in field order */
    int64_t batch;
    int32_t n_fields;             /* F >= 2 */
    int32_t dim;                  /* d >= 1 */
    int32_t reduce_sum;           /* 0 | 1 */
    int32_t n_dense;              /* dense columns copied behind the pair block (0 = none) */
    const float* scale;           /* NULL, or [P*d] ([P] with reduce_sum); scale and shift both or neither */
    const float* shift;
    const float* dense;           /* [B, dense_stride] or NULL */
    int64_t dense_stride;
    float* out;                   /* row b at out + b * out_stride + out_offset: P*d (or P) + n_dense floats */
    int64_t out_stride;           /* elements, a multiple of 4 (DCTR_E_ALIGN), >= out_offset + width */
    int64_t out_offset;           /* first column written (>= 0); columns outside [out_offset, out_offset + width) are not touched */
    int32_t* status;              /* optional device word, DCTR_STATUS_* bits are OR-ed in */
    int32_t route;                /* DCTR_FFM_ROUTE_AUTO | DCTR_FFM_ROUTE_DIRECT (force the direct route) */
    int32_t reserved;             /* 0 */
    void* workspace;              /* reserved: NULL, or 16-B aligned */
    size_t workspace_bytes;
} dctr_ffm_args_t;
size_t dctr_ffm_workspace_bytes(const dctr_ffm_args_t* args);
/* The route dctr_ffm_fwd takes for these arguments (DCTR_FFM_ROUTE_LDS / DCTR_FFM_ROUTE_DIRECT), or the DCTR_E_* its size checks
 * answer.  Pointers are not looked at. */
int dctr_ffm_route(const dctr_ffm_args_t* args);
int dctr_ffm_fwd(const dctr_ffm_args_t* args, void* stream);

/* Backward of dctr_ffm_fwd's pair products, one launch; the forward saves nothing (the kernel loads the ids and the rows again: they
 * are unchanged until the optimizer runs).  fwd: fields, batch, n_fields, dim, reduce_sum, status and route are read as the forward
 * reads them; scale / shift must be NULL and n_dense 0 (in training BatchNormalization uses batch statistics: it and the dense concat
 * stay with the caller), out / out_stride / out_offset / dense are ignored.  With g = d_out row b (P*d floats, P with reduce_sum,
 * from column d_out_offset of a row of d_out_stride floats), for every pair p = (i, j), i < j:
 *     d row_i[slot of j][e] += g[p*d + e] * row_j[slot of i][e]        d row_j[slot of i][e] += g[p*d + e] * row_i[slot of j][e]
 *     (reduce_sum: g[p] in place of g[p*d + e])
 * Where the gradient of field f goes is grads[f]:
 *   a table field: ACCUMULATED into the dense gradient table [vocab_f, row_stride] (zero it first) at the row of the sample's id, with
 *     float atomics — one (sample, field) row is one contiguous run of (F-1)*d floats, one dword per lane — so it may differ in the last
 *     bits from call to call;
 *   a pre-pooled (identity) field: plain stores into the first (F-1)*d floats of row b of a [batch, row_stride] buffer, one owner per
 *     element: bit-identical from call to call, columns behind (F-1)*d untouched;
 *   grad = NULL (a frozen field): skipped, nothing of it is touched.
 * An id outside [0, vocab) raises DCTR_STATUS_INDEX_OOR, receives no gradient and enters its partners' gradients as a row of zeros,
 * exactly as the forward treats it; nothing outside the tables is read or written.
 * Routes as the forward: tiles of samples gathered whole into LDS, or — rows beyond the LDS, or fwd.route = DCTR_FFM_ROUTE_DIRECT —
 * the partner rows read from global memory.  Same arithmetic on both.  No shape the forward takes is refused and neither route needs a
 * workspace (dctr_ffm_bwd_workspace_bytes() = 0; the two members are reserved).  Argument errors launch and write nothing. */
typedef struct {
    float* grad;                  /* table field: [vocab, row_stride], ACCUMULATED into; identity field: [batch, row_stride], written; NULL: skipped */
    int64_t row_stride;           /* floats between rows, >= (F-1)*d */
} dctr_ffm_grad_t;
typedef struct {
    dctr_ffm_args_t fwd;
    const float* d_out;           /* row b at d_out + b * d_out_stride + d_out_offset: P*d (or P) floats */
    int64_t d_out_stride;         /* >= d_out_offset + width */
    int64_t d_out_offset;         /* >= 0 */
    const dctr_ffm_grad_t* grads; /* DEVICE array [n_fields], in field order */
    int32_t max_blocks;           /* 0: the library's choice; > 0 caps the grid (one workgroup then walks every tile) */
    int32_t reserved;             /* 0 */
    void* workspace;              /* reserved: NULL, or 16-B aligned */
    size_t workspace_bytes;
} dctr_ffm_bwd_args_t;
size_t dctr_ffm_bwd_workspace_bytes(const dctr_ffm_bwd_args_t* args);   /* host only: 0 */
/* The route dctr_ffm_bwd takes (DCTR_FFM_ROUTE_LDS / DCTR_FFM_ROUTE_DIRECT), or the DCTR_E_* of its size checks; no pointer is read. */
int dctr_ffm_bwd_route(const dctr_ffm_bwd_args_t* args);
int dctr_ffm_bwd(const dctr_ffm_bwd_args_t* args, void* stream);

/* ------------------------------------------------------------------------------------------------
 * MLR (mixed logistic regression, piece-wise linear model) — deepctr/models/mlr.py:17-74 (no layer class in the reference)
 *     R = region_num >= 2 pieces.  K = 2R (+ 1 with has_bias) linear logits per sample, in the column order region 0..R-1,
 *     learner R..2R-1, bias 2R.  A feature's K one-wide tables are stored as ONE row [vocab, row_pitch]: the reference's
 *     region_<r>0sparse_emb_<name>/embeddings is the strided view [:, c:c+1].  A field adds the first `width` floats of its row (the row
 *     of the sample's id; the sample index for identity != 0: a VarLenSparseFeat pre-pooled by dctr_embed_pool) to the columns
 *     col0 .. col0 + width - 1.  Per sample:
 *         z[c]   = sum over the fields covering c of row[c - col0], in field order, + sum_k dense[k] * dense_w[k * K + c]
 *         s      = softmax(z[0 .. R-1])            (the row maximum subtracted)
 *         a[r]   = sigmoid(z[R + r])               (learner_act = DCTR_MLR_LEARNER_SIGMOID: task 'binary'; _LINEAR: a[r] = z[R + r])
 *         out    = sum_r s[r] * a[r]               (* sigmoid(z[2R]) with has_bias)
 *     out is the model's PREDICTION: nothing follows it.  z (optional) is what dctr_mlr_bwd reads.
 *     One lane per column, a group of 8 / 16 / 32 / 64 lanes per sample: a (sample, field) row is one contiguous request, softmax and
 *     the sums run on cross-lane moves inside the group; no LDS, no barrier, no workspace.  fp32 throughout.
 *     An id outside [0, vocab) raises DCTR_STATUS_INDEX_OOR and counts as a row of zeros; nothing outside the tables is read.
 *     K <= 64 (region_num <= 31 with a bias part, 32 without); beyond that dctr_mlr_fwd / dctr_mlr_bwd answer DCTR_E_UNSUPPORTED before
 *     anything is launched (dctr_mlr_supported: 1 / 0, host only, reads region_num and has_bias only).
 *     Argument errors (nothing launched or written): NULL args / out / fields with n_fields > 0 / dense or dense_w with n_dense > 0
 *     (DCTR_E_NULL); region_num < 2, negative batch / n_fields / n_dense / z_offset, out_stride < 1, dense_stride < n_dense,
 *     z_stride < z_offset + K (DCTR_E_DIM); has_bias not 0 / 1, unknown learner_act (DCTR_E_ENUM); a fields array that is not 8-byte
 *     aligned (DCTR_E_ALIGN).  Field contents (col0 / width inside [0, K]) live on the device and are the caller's contract.
 * ------------------------------------------------------------------------------------------------ */
enum { DCTR_MLR_LEARNER_SIGMOID = 0, DCTR_MLR_LEARNER_LINEAR = 1 };
#define DCTR_MLR_MAX_COLUMNS 64
typedef struct {
    const float* rows;            /* [vocab, row_pitch] fp32: the fused rows (or the pre-pooled buffer), already advanced to the field's first column */
    const void* ids;              /* sample b's id at ids[b * ids_stride]; unused when identity */
    int64_t vocab;
    int64_t row_pitch;            /* floats between rows, >= width */
    int64_t ids_stride;           /* elements */
    int32_t ids_is_i64;           /* 0: int32 ids, 1: int64 ids */
    int32_t identity;             /* 1: row = sample index b */
    int32_t col0;                 /* first logit column the field adds to, 0 <= col0 */
    int32_t width;                /* columns it adds to, col0 + width <= K */
} dctr_mlr_field_t;
typedef struct {
    const dctr_mlr_field_t* fields;   /* DEVICE array [n_fields]; may be NULL when n_fields = 0 */
    int64_t batch;
    int32_t n_fields;             /* >= 0 */
    int32_t region_num;           /* R >= 2 */
    int32_t has_bias;             /* 0 | 1 */
    int32_t learner_act;          /* DCTR_MLR_LEARNER_* */
    int32_t n_dense;              /* columns of the dense matrix (0 = none) */
    int32_t reserved;             /* 0 */
    const float* dense;           /* [B, dense_stride] or NULL */
    int64_t dense_stride;
    const float* dense_w;         /* [n_dense, K] row-major: zeros where a logit does not use a dense column */
    float* out;                   /* sample b's prediction at out[b * out_stride] */
    int64_t out_stride;           /* >= 1 */
    float* z;                     /* NULL, or row b at z + b * z_stride + z_offset: K floats; other columns are not touched */
    int64_t z_stride;
    int64_t z_offset;             /* >= 0 */
    int32_t* status;              /* optional device word, DCTR_STATUS_* bits are OR-ed in */
} dctr_mlr_args_t;
int dctr_mlr_supported(const dctr_mlr_args_t* args);      /* host only: 1 when K <= DCTR_MLR_MAX_COLUMNS, else 0 */
int dctr_mlr_fwd(const dctr_mlr_args_t* args, void* stream);

/* Backward of dctr_mlr_fwd, one launch, ONE route, no workspace (nothing to query: every intermediate lives in a lane group's
 * registers).  fwd: fields, batch, n_fields, region_num, has_bias, learner_act, status are read as the forward reads them; fwd.z /
 * z_stride / z_offset is the z the forward SAVED (read, REQUIRED); out, dense and dense_w are ignored (the dense weights' gradient is
 * dense^T dz: the caller's matmul).  With d = d_out[b * d_out_stride], s / a as the forward, u = sum_r s[r] a[r], g = sigmoid(z[2R])
 * (1 without a bias part):
 *     dz[r]      = d g s[r] (a[r] - u)                                 r < R
 *     dz[R + r]  = d g s[r] a[r] (1 - a[r])        (_LINEAR: d g s[r])
 *     dz[2R]     = d u g (1 - g)
 * dz row b is written to dz + b * dz_stride (K floats; REQUIRED).  Then, per field, the slice dz[col0 .. col0 + width) goes where
 * grads[f] says (grads may be NULL: no field gradient at all):
 *   a table field: ACCUMULATED with float atomics into [vocab, row_stride] at the row of the sample's id (zero it first; last bits may
 *     differ from call to call) — one row per (sample, field), one dword per lane; columns behind `width` are never touched;
 *   an identity (pre-pooled) field: plain stores into the first `width` floats of row b of a [batch, row_stride] buffer;
 *   grad = NULL (a frozen field): skipped.
 * An id outside [0, vocab) receives no gradient and raises DCTR_STATUS_INDEX_OOR.  Argument errors as the forward (plus DCTR_E_NULL
 * for a missing z / d_out / dz, DCTR_E_DIM for d_out_stride < 1 or dz_stride < K); nothing is launched or written then. */
typedef struct {
    float* grad;                  /* table field: [vocab, row_stride], ACCUMULATED into, already advanced to the field's first column;
                                     identity field: [batch, row_stride], written; NULL: skipped */
    int64_t row_stride;           /* floats between rows, >= width */
} dctr_mlr_grad_t;
typedef struct {
    dctr_mlr_args_t fwd;
    const float* d_out;           /* sample b's gradient at d_out[b * d_out_stride] */
    int64_t d_out_stride;         /* >= 1 */
    float* dz;                    /* [B, dz_stride], K floats written per row */
    int64_t dz_stride;            /* >= K */
    const dctr_mlr_grad_t* grads; /* DEVICE array [n_fields], in field order; NULL: no field gradients */
} dctr_mlr_bwd_args_t;
int dctr_mlr_bwd(const dctr_mlr_bwd_args_t* args, void* stream);

/* ------------------------------------------------------------------------------------------------
 * IFM / DIFM: the input-aware factor, the refined FM and linear terms, the prediction — deepctr/models/ifm.py:55-72, difm.py:59-80
 *     F >= 1 fields of one embedding_dim d, read in place from the leading F*d columns of x (e.g. dnn_in) at x_stride.  Per sample b:
 *       m'[f] = mprime[b, f] (0 when NULL) + sum over the n_src sources of act[b, 0..K) . kernel[0..K, f]   (Keras layout [K, F], no bias)
 *       m[f]  = softmax ? F * softmax_f(m')[f], the row maximum subtracted (IFM) : m'[f] (DIFM)
 *       fm    = 0.5 * sum_c ((sum_f m[f] e[f, c])^2 - sum_f (m[f] e[f, c])^2)
 *       lin   = sum_k m[k] * lin_k         n_lin = 0 or F first-order terms, paired with m BY POSITION as the reference pairs them
 *       out[b] = act(fm + lin + add[0][b] + .. + *global_bias),  act = sigmoid when sigmoid_out
 *     lin_k is gathered from a 1-wide table by id (int32 / int64), or read from a [B] vector already pooled (dctr_embed_pool's lin_out).
 *     An id outside [0, vocab) raises DCTR_STATUS_INDEX_OOR and contributes zero; nothing outside the tables is read.  The add vectors
 *     enter unrefined (the dense linear term is one of them).  m reaches memory only through the optional factor_out [B, F].
 *     The products run on v_mfma_f32_16x16x4_f32 (exact fp32).  Routes: the [16, F] tile of m' of a wave's samples waits in LDS, or —
 *     more than 560 fields, or route = DCTR_IFM_ROUTE_WORKSPACE — goes through a [B, F] workspace between two launches.  Both routes
 *     give the same bits; K and d never decide the route (K is walked in chunks of 64, d by the lanes).  No shape is refused for its
 *     size up to F*d < 2^27.  Without sources (mprime alone) there is nothing to project: one launch, no LDS, no workspace.
 * ------------------------------------------------------------------------------------------------ */
enum { DCTR_IFM_ROUTE_AUTO = 0, DCTR_IFM_ROUTE_WORKSPACE = 1, DCTR_IFM_ROUTE_LDS = 2 };
typedef struct {
    const float* act;             /* [B, act_stride] fp32: the DNN's last hidden layer, the flattened attention output, ... */
    const float* kernel;          /* [K, F] fp32, contiguous */
    int64_t act_stride;           /* floats between rows, >= K */
    int32_t K;                    /* >= 1 */
    int32_t reserved;             /* 0 */
} dctr_ifm_src_t;
typedef struct {
    const float* table;           /* [vocab] fp32 (a 1-wide linear embedding table); unused when vec */
    const void* ids;              /* sample b's id at ids[b * ids_stride] */
    const float* vec;             /* NULL, or the term itself: sample b's at vec[b * vec_stride] */
    int64_t vocab;
    int64_t ids_stride;           /* elements */
    int64_t vec_stride;           /* floats */
    int32_t ids_is_i64;           /* 0: int32 ids, 1: int64 ids */
    int32_t reserved;             /* 0 */
} dctr_ifm_lin_t;
typedef struct {
    int64_t batch;
    int32_t n_fields;             /* F >= 1 */
    int32_t dim;                  /* d >= 1 */
    const float* x;               /* [B, x_stride]: field f's embedding at columns [f*d, (f+1)*d) */
    int64_t x_stride;             /* floats, >= F*d */
    int32_t n_src;                /* 0, 1 or 2 */
    int32_t softmax;              /* 0 | 1 */
    dctr_ifm_src_t src[2];
    const float* mprime;          /* NULL, or [B, mprime_stride]: added to the sources' products; REQUIRED when n_src = 0 */
    int64_t mprime_stride;        /* floats, >= F */
    const dctr_ifm_lin_t* lin;    /* DEVICE array [n_lin], position order */
    int32_t n_lin;                /* 0 or F */
    int32_t n_add;                /* 0 .. 4 */
    const float* add[4];          /* [B] each */
    const float* global_bias;     /* NULL or a device scalar */
    int32_t sigmoid_out;          /* 0 | 1 */
    int32_t route;                /* DCTR_IFM_ROUTE_AUTO | DCTR_IFM_ROUTE_WORKSPACE (force the workspace route) */
    float* out;                   /* [B] */
    float* factor_out;            /* NULL, or [B, factor_stride]: m */
    int64_t factor_stride;        /* floats, >= F */
    int32_t* status;              /* optional device word, DCTR_STATUS_* bits are OR-ed in */
    void* workspace;              /* NULL, or device scratch of dctr_ifm_workspace_bytes() bytes, 16-B aligned */
    size_t workspace_bytes;
} dctr_ifm_args_t;
/* Bytes dctr_ifm_fwd needs for these arguments (batch, n_fields, n_src, route are read): 0 on the LDS route and without sources;
 * on the workspace route it is REQUIRED (DCTR_E_NULL without, before anything is launched). */
size_t dctr_ifm_workspace_bytes(const dctr_ifm_args_t* args);
/* The route dctr_ifm_fwd takes (DCTR_IFM_ROUTE_LDS / DCTR_IFM_ROUTE_WORKSPACE), or the DCTR_E_* its size checks answer.  Pointers are
 * not looked at. */
int dctr_ifm_route(const dctr_ifm_args_t* args);
int dctr_ifm_fwd(const dctr_ifm_args_t* args, void* stream);

/* Backward of the differentiable part of dctr_ifm_fwd: the logit without the unrefined tail (no add vectors, no bias, no sigmoid),
 *     y[b] = 0.5 * sum_c ((sum_f m[f] e[f,c])^2 - sum_f (m[f] e[f,c])^2) + sum_f m[f] t[f]
 * with t = terms [B, F], the first-order terms already gathered / pooled (NULL: none).  factor is the m the forward SAVED (its
 * factor_out): nothing is projected again and no exponential is taken again.  With g = d_out[b]:
 *     S[c]    = sum_f m[f] e[f,c]              u[f,c] = S[c] - m[f] e[f,c]
 *     dm[f]   = sum_c e[f,c] u[f,c] + t[f]
 *     dx[f,c] = g m[f] u[f,c]                  dterms[f] = g m[f]
 *     dm'[f]  = softmax ? g m[f] (dm[f] - (1/F) sum_h m[h] dm[h]) : g dm[f]
 *     dmprime = dm'          dact_s = dm' kernel_s^T  [B, K_s]          dkernel_s = act_s^T dm'  [K_s, F]  (a sum over the batch)
 * Outputs: a NULL pointer means the gradient is not wanted and its work is skipped; every wanted output is OVERWRITTEN (never
 * accumulated into) and nothing is written behind the width of a row (F*d of dx, F of dterms / dmprime / dkernel_s, K_s of dact_s).
 * Launches, all on the caller's stream: the row pass (a wave per sample: dx, dterms, dm'), per wanted dact one MFMA pass (a wave per
 * 16 samples), and for the wanted dkernel one MFMA pass over `S` batch slices into partials[S] in the workspace followed by a small
 * launch that adds the S partials of every element in the order 0 .. S-1.  v_mfma_f32_16x16x4_f32 throughout (exact fp32), no float
 * atomics: every output is bit-identical from call to call.  slices = 0: S is a function of the shapes alone; 1 .. 256 forces it.
 * dx, dterms, dmprime and dact do not depend on S.
 * Workspace (dctr_ifm_bwd_workspace_bytes: shapes, n_src, slices and which of dmprime / dact / dkernel are NULL are read): [B, F] floats
 * of dm' when a dact or dkernel is wanted and dmprime is not, plus the partials when a dkernel is wanted; REQUIRED then (DCTR_E_NULL).
 * dctr_ifm_bwd_supported: 1, or 0 where one row of pad16(F) floats exceeds the LDS (F > 40,960; n_fields and dim are read);
 * dctr_ifm_bwd answers DCTR_E_UNSUPPORTED there.  Argument errors launch and write nothing: NULL args / x / factor / d_out, a wanted
 * dact without the source's kernel or a wanted dkernel without its act (DCTR_E_NULL); n_fields or dim < 1, negative batch, F*d >= 2^27, a stride below its width, n_src outside
 * 0 .. 2, K < 1, slices outside 0 .. 256 (DCTR_E_DIM); a workspace that is not 16-B aligned (DCTR_E_ALIGN). */
typedef struct {
    int64_t batch;
    int32_t n_fields;             /* F >= 1 */
    int32_t dim;                  /* d >= 1 */
    const float* x;               /* [B, x_stride]: the forward's x */
    int64_t x_stride;             /* floats, >= F*d */
    const float* factor;          /* [B, factor_stride]: m, the forward's factor_out */
    int64_t factor_stride;        /* floats, >= F */
    const float* terms;           /* NULL, or [B, terms_stride]: the first-order terms by position */
    int64_t terms_stride;         /* floats, >= F */
    const float* d_out;           /* [B] */
    int32_t n_src;                /* 0, 1 or 2 */
    int32_t softmax;              /* 0 | 1: as the forward */
    dctr_ifm_src_t src[2];        /* as the forward (act is read for dkernel, kernel for dact) */
    float* dx;                    /* NULL, or [B, dx_stride]: F*d floats of a row written */
    int64_t dx_stride;
    float* dterms;                /* NULL, or [B, dterms_stride]: F floats of a row written */
    int64_t dterms_stride;
    float* dmprime;               /* NULL, or [B, dmprime_stride]: dm', F floats of a row written */
    int64_t dmprime_stride;
    float* dact[2];               /* NULL, or [B, dact_stride[s]]: K_s floats of a row written */
    int64_t dact_stride[2];
    float* dkernel[2];            /* NULL, or [K_s, dkernel_stride[s]]: F floats of a row written */
    int64_t dkernel_stride[2];
    int32_t slices;               /* 0: the library's choice (a function of the shapes); 1 .. 256: that many batch slices for dkernel */
    int32_t reserved;             /* 0 */
    void* workspace;              /* NULL, or device scratch of dctr_ifm_bwd_workspace_bytes() bytes, 16-B aligned */
    size_t workspace_bytes;
} dctr_ifm_bwd_args_t;
int dctr_ifm_bwd_supported(const dctr_ifm_bwd_args_t* args);            /* host only: 1 / 0 */
size_t dctr_ifm_bwd_workspace_bytes(const dctr_ifm_bwd_args_t* args);   /* host only; 0 for arguments dctr_ifm_bwd refuses */
int dctr_ifm_bwd(const dctr_ifm_bwd_args_t* args, void* stream);

/* ------------------------------------------------------------------------------------------------
 * FieldWiseBiInteraction.call (FLEN) — deepctr/layers/interaction.py:1224-1348, one launch
 *     x [B, x_stride] read in place from column x_offset; G >= 2 embedding groups, group g = n_fields fields of width dim from column
 *     first (relative to x_offset; groups need not be adjacent, ordered or equal in size).  Per sample, elementwise over the dim columns:
 *       s_g = sum_f x_f,  q_g = sum_f x_f^2
 *       y   = (sum_{i<j} kernel_mf[p(i,j)] s_i s_j + bias_mf) + (sum_g kernel_fm[g] (s_g^2 - q_g) + bias_fm)   (no factor 1/2)
 *     p(i,j): itertools.combinations order.  Outputs, either or both: y [B, dim] at y_stride / y_offset; logit[b] = y[b,:] . head_w
 *     (+ add[b]).  The weights are read from the given pointers on every call.  A thread owns one sample and 4 (16-B loads: dim % 4 == 0
 *     and every column offset / stride / pointer a multiple of 16 B) or 1 adjacent columns, walks the groups once and keeps the s_g
 *     in LDS; the lanes of a sample meet in shuffles for the logit.  No atomics: the same bits on every call.  Routes: ON_CHIP, or —
 *     more groups than the LDS holds (G * 256 B per thread column over 128 KiB), or route = DCTR_FIELDWISE_ROUTE_REREAD — the s_i of
 *     the earlier groups are summed again from x where the MF part needs them: the same additions in the same order, the same bits,
 *     no workspace.  No shape is refused for its size (any dim, any number of fields) up to G < 2^20.
 * ------------------------------------------------------------------------------------------------ */
enum { DCTR_FIELDWISE_ROUTE_AUTO = 0, DCTR_FIELDWISE_ROUTE_ON_CHIP = 1, DCTR_FIELDWISE_ROUTE_REREAD = 2 };
typedef struct {
    int64_t first;                /* first column of the group, relative to x_offset */
    int32_t n_fields;             /* >= 1 */
    int32_t reserved;             /* 0 */
} dctr_fieldwise_group_t;
typedef struct {
    int64_t batch;
    const float* x;               /* [B, x_stride] fp32 */
    int64_t x_stride;             /* floats between rows */
    int64_t x_offset;             /* first column the groups count from */
    const dctr_fieldwise_group_t* groups;        /* DEVICE array [n_groups] */
    const dctr_fieldwise_group_t* groups_host;   /* the same table in host memory (checked against x_stride before the launch) */
    int32_t n_groups;             /* G >= 2 */
    int32_t dim;                  /* d >= 1 */
    const float* kernel_mf;       /* [G(G-1)/2] */
    const float* kernel_fm;       /* [G] */
    const float* bias_mf;         /* NULL or [d] */
    const float* bias_fm;         /* NULL or [d] */
    float* y;                     /* NULL, or [B, y_stride]: columns [y_offset, y_offset + d) written */
    int64_t y_stride;
    int64_t y_offset;
    const float* head_w;          /* [d]; REQUIRED with logit */
    const float* add;             /* NULL or [B] */
    float* logit;                 /* NULL or [B] */
    int32_t route;                /* DCTR_FIELDWISE_ROUTE_AUTO | DCTR_FIELDWISE_ROUTE_REREAD (force) */
    int32_t max_blocks;           /* backward only: 0 = 4 per compute unit, else the most workgroups to launch (each walks its tiles) */
} dctr_fieldwise_args_t;
/* The route dctr_fieldwise_fwd takes (DCTR_FIELDWISE_ROUTE_ON_CHIP / _REREAD), or the DCTR_E_* its size checks answer. */
int dctr_fieldwise_route(const dctr_fieldwise_args_t* args);
int dctr_fieldwise_fwd(const dctr_fieldwise_args_t* args, void* stream);

/* Backward of dctr_fieldwise_fwd; nothing is saved by the forward.  The upstream gradient is dy [B, dy_stride] (the layer), or
 * dlogit [B] with fwd.head_w (the model: dy[b,e] = dlogit[b] * head_w[e]).  dx [B, dx_stride]: the groups' columns from dx_offset
 * are written (accumulate = 0) or added to (1);
 *     ds_g = dy (sum_{j != g} w_gj s_j + 2 k_g s_g),   dx_f = ds_g - 2 k_g dy x_f   for f in g.
 * ACCUMULATED (each may be NULL): d_kernel_mf[p] += sum_{b,e} dy s_i s_j, d_kernel_fm[g] += sum_{b,e} dy (s_g^2 - q_g),
 * d_bias_mf[e] and d_bias_fm[e] += sum_b dy[b,e], and with dlogit d_head_w[e] += sum_b dlogit[b] y[b,e] (y recomputed).  Partial sums
 * meet per wave in shuffles and per workgroup in LDS: one atomic per workgroup and destination.  fwd.y / logit / add are ignored.
 * Shapes whose s_g and accumulators do not fit 128 KiB of LDS answer DCTR_E_UNSUPPORTED (dctr_fieldwise_bwd_supported: 1 / 0). */
typedef struct {
    dctr_fieldwise_args_t fwd;
    const float* dy;              /* NULL or [B, dy_stride] */
    int64_t dy_stride;
    const float* dlogit;          /* NULL or [B]; exactly one of dy / dlogit */
    float* dx;                    /* NULL or [B, dx_stride] */
    int64_t dx_stride;
    int64_t dx_offset;
    int32_t accumulate;           /* 0 | 1 */
    int32_t reserved;             /* 0 */
    float* d_kernel_mf;
    float* d_kernel_fm;
    float* d_bias_mf;
    float* d_bias_fm;
    float* d_head_w;              /* dlogit form only */
} dctr_fieldwise_bwd_args_t;
int dctr_fieldwise_bwd_supported(const dctr_fieldwise_bwd_args_t* args);
int dctr_fieldwise_bwd(const dctr_fieldwise_bwd_args_t* args, void* stream);

/* ------------------------------------------------------------------------------------------------
 * EDCN's tower — deepctr/models/edcn.py:66-87 with RegulationModule (layers/core.py:270-321) and BridgeModule
 * (layers/interaction.py:1502-1565), one launch
 *     x [B, x_stride] read in place from column x_offset: F fields of width dim, D = F * dim.  deep = cross = x, then per round
 *     i < cross_num:
 *       deep  *= softmax_f(gates[2i] * inv_tau)[field of the column];  cross *= softmax_f(gates[2i+1] * inv_tau)[field of the column]
 *       c  = cross * (cross . w_i) + b_i + cross  (DCTR_CROSS_VECTOR)  |  cross * (W_i cross + b_i) + cross  (DCTR_CROSS_MATRIX, W [out, in])
 *       h  = act((deep Wd_i + bd_i) [* bn_scale_i + bn_shift_i])        (Wd: Keras layout [in, out])
 *       br = c + h | c * h | bridge_act([c, h] Wb_i + bb_i)             (Wb [2D, D], Keras layout)
 *       deep = cross = br
 *     Outputs, either or both: logit[b] = [c, h, br] . head_w + sum(add) + global_bias (sigmoid with sigmoid_out); out [B, out_stride]:
 *     c, h, br of the LAST round in columns [out_offset, out_offset + 3D).
 *     The gates are computed inside the launch from the F weights the pointers show on every call; c / h / br live in LDS; the
 *     products are exact fp32 on v_mfma_f32_16x16x4_f32.  No atomics: the same bits on every call.  More than 32 rounds are chained
 *     launches through a workspace of dctr_edcn_workspace_bytes() that carries br (0 bytes up to 32 rounds).
 *     The FUSED route takes the bridges ADD / HADAMARD / CONCAT with activation and bridge_activation in {LINEAR, RELU} while four
 *     [16, pad16(D) + 4] tiles and the gates fit 160 KiB of LDS (D <= 624 at dim 16).  Everything else — wider rows, attention pooling,
 *     other activations, route = DCTR_EDCN_ROUTE_LAYERED — answers DCTR_E_UNSUPPORTED here and DCTR_EDCN_ROUTE_LAYERED from
 *     dctr_edcn_route: the host then runs the tower layer by layer (dctr_mlp_fwd, dctr_crossnet_head_fwd or dctr_sgemm +
 *     dctr_crossnet_matrix_step, dctr_edcn_regulate, dctr_edcn_bridge).
 * ------------------------------------------------------------------------------------------------ */
enum { DCTR_EDCN_BRIDGE_ADD = 0, DCTR_EDCN_BRIDGE_HADAMARD = 1, DCTR_EDCN_BRIDGE_CONCAT = 2, DCTR_EDCN_BRIDGE_ATTENTION = 3 };
enum { DCTR_EDCN_ROUTE_AUTO = 0, DCTR_EDCN_ROUTE_FUSED = 1, DCTR_EDCN_ROUTE_LAYERED = 2 };
typedef struct {
    int64_t batch;
    const float* x;               /* [B, x_stride] fp32 */
    int64_t x_stride;             /* floats between rows */
    int64_t x_offset;             /* first column of the F * dim the tower reads */
    int32_t fields;               /* F >= 1 */
    int32_t dim;                  /* d >= 1 */
    int32_t cross_num;            /* rounds >= 1 */
    int32_t mode;                 /* DCTR_CROSS_VECTOR | DCTR_CROSS_MATRIX */
    int32_t bridge;               /* DCTR_EDCN_BRIDGE_* */
    int32_t activation;           /* the DNNs': DCTR_ACT_* (fused: LINEAR | RELU) */
    int32_t bridge_activation;    /* the concatenation bridge's Dense: DCTR_ACT_* (fused: LINEAR | RELU) */
    float inv_tau;                /* 1 / tau, finite */
    const float* const* gates;    /* HOST array [2 * cross_num] of DEVICE pointers to F floats: the deep and the cross gate of round i */
    const float* const* cross_w;  /* HOST array [cross_num] of DEVICE pointers: [D] (vector) or [D, D] (matrix) */
    const float* const* cross_b;  /* [cross_num] -> [D] */
    const float* const* dnn_w;    /* [cross_num] -> [D, D] */
    const float* const* dnn_b;    /* [cross_num] -> [D] */
    const float* const* bn_scale; /* NULL, or [cross_num] -> [D] (entries may be NULL): inference BatchNormalization as an affine */
    const float* const* bn_shift;
    const float* const* bridge_w; /* DCTR_EDCN_BRIDGE_CONCAT: [cross_num] -> [2D, D] */
    const float* const* bridge_b; /* DCTR_EDCN_BRIDGE_CONCAT: [cross_num] -> [D] */
    const float* head_w;          /* [3D]; REQUIRED with logit */
    const float* add[4];          /* NULL or [B] each */
    const float* global_bias;     /* NULL or a device scalar */
    int32_t sigmoid_out;          /* 0 | 1 */
    int32_t route;                /* DCTR_EDCN_ROUTE_AUTO | DCTR_EDCN_ROUTE_LAYERED (the query answers LAYERED, dctr_edcn_fwd declines) */
    float* logit;                 /* NULL or [B] */
    float* out;                   /* NULL, or [B, out_stride]: columns [out_offset, out_offset + 3D) written */
    int64_t out_stride;
    int64_t out_offset;
    void* workspace;              /* NULL, or device scratch of dctr_edcn_workspace_bytes() bytes, 16-B aligned */
    size_t workspace_bytes;
} dctr_edcn_args_t;
/* Bytes dctr_edcn_fwd needs (batch, fields, dim, cross_num and what decides the route are read): 0 up to 32 rounds. */
size_t dctr_edcn_workspace_bytes(const dctr_edcn_args_t* args);
/* The route these arguments take (DCTR_EDCN_ROUTE_FUSED / _LAYERED), or the DCTR_E_* the size checks answer.  Pointers are not
 * looked at. */
int dctr_edcn_route(const dctr_edcn_args_t* args);
int dctr_edcn_fwd(const dctr_edcn_args_t* args, void* stream);
/* EDCN's tower for training: a forward that keeps a tape, and its backward.
 *   dctr_edcn_train_fwd: dctr_edcn_fwd on `fwd` (the same kernel under one more flag: logit and out have dctr_edcn_fwd's bits) that also
 *     writes tape [cross_num, B, 3D] = c, h, br of every round (out is the last round's slice of the same data).
 *   dctr_edcn_bwd: from x (read in place at fwd.x_offset), the live weights of `fwd` and the tape, the gradient of
 *     sum_b d_logit[b] * ([c, h, br]_last[b] . head_w) + sum d_out * [c, h, br]_last: the seed of the last round is
 *     d_out + d_logit * head_w.  fwd.add / global_bias / sigmoid_out / logit / out are not read: the op is the tower with its head.
 *     A workgroup owns 16 rows and walks the rounds in reverse with four [16, pad16(D) + 4] tiles in LDS; the input-gradient products
 *     run on v_mfma_f32_16x16x4_f32.  The row pass leaves the pre-activation gradients in the workspace; a second pass forms the
 *     [D, D] / [2D, D] weight gradients over `slices` batch slices, and a last step adds the partials in a fixed order; the F-, D- and
 *     3D-sized gradients are summed per workgroup and added the same way.  No atomics: two calls give the same bits; another slice
 *     count changes the [D, D] / [2D, D] gradients only (by rounding).
 *   Both take what dctr_edcn_bwd_supported accepts: the fused route's bridges (ADD / HADAMARD / CONCAT), both parameterizations,
 *   activation / bridge_activation in {LINEAR, RELU}, no bn_scale, at most 32 rounds, while the backward's LDS plan fits 160 KiB
 *   (D <= 624 at dim 16).  Everything else answers DCTR_E_UNSUPPORTED: the host keeps its torch ops.
 *   Every gradient is OVERWRITTEN (dx: added to with `accumulate`); a NULL pointer (array or entry) skips that output. */
typedef struct {
    dctr_edcn_args_t fwd;         /* shapes, options, x and the live weights as dctr_edcn_fwd reads them; fwd.workspace is not used */
    float* tape;                  /* [cross_num, B, 3D] contiguous, 16-B aligned: train_fwd writes it, bwd reads it */
    const float* d_logit;         /* bwd: NULL or [B]; needs fwd.head_w */
    const float* d_out;           /* bwd: NULL or [B, d_out_stride]: the gradient of c, h, br of the last round in its first 3D columns */
    int64_t d_out_stride;         /* floats between rows, >= 3D */
    float* dx;                    /* NULL or [B, dx_stride]: columns [dx_offset, dx_offset + D) written */
    int64_t dx_stride;
    int64_t dx_offset;
    int32_t accumulate;           /* 0: dx is overwritten | 1: added to */
    int32_t slices;               /* batch slices of the weight-gradient pass: 0 (the library's choice) or 1 .. 256 */
    float* const* d_gates;        /* NULL, or HOST array [2 * cross_num] of DEVICE pointers (entries may be NULL) -> [F] */
    float* const* d_cross_w;      /* NULL, or [cross_num] -> [D] (vector) or [D, D] (matrix) */
    float* const* d_cross_b;      /* NULL, or [cross_num] -> [D] */
    float* const* d_dnn_w;        /* NULL, or [cross_num] -> [D, D] */
    float* const* d_dnn_b;        /* NULL, or [cross_num] -> [D] */
    float* const* d_bridge_w;     /* DCTR_EDCN_BRIDGE_CONCAT: NULL, or [cross_num] -> [2D, D] */
    float* const* d_bridge_b;     /* DCTR_EDCN_BRIDGE_CONCAT: NULL, or [cross_num] -> [D] */
    float* d_head_w;              /* NULL or [3D]: sum_b d_logit[b] * [c, h, br]_last[b]; needs d_logit */
    void* workspace;              /* bwd: device scratch of dctr_edcn_bwd_workspace_bytes() bytes, 16-B aligned */
    size_t workspace_bytes;
} dctr_edcn_train_args_t;
/* 1 when dctr_edcn_train_fwd / dctr_edcn_bwd take these shapes and options, else 0.  Host only: no pointer is followed (fwd.bn_scale is
 * compared with NULL). */
int dctr_edcn_bwd_supported(const dctr_edcn_train_args_t* args);
/* Bytes of the tape (batch, fields, dim, cross_num are read). */
size_t dctr_edcn_tape_bytes(const dctr_edcn_train_args_t* args);
/* Bytes dctr_edcn_bwd needs (shapes, options, slices and which weight gradients are wanted are read); 0 for what it refuses. */
size_t dctr_edcn_bwd_workspace_bytes(const dctr_edcn_train_args_t* args);
int dctr_edcn_train_fwd(const dctr_edcn_train_args_t* args, void* stream);
int dctr_edcn_bwd(const dctr_edcn_train_args_t* args, void* stream);
/* RegulationModule over one read of x [B, x_stride] (F fields of width dim): deep = x * softmax_f(g_deep * inv_tau)[field],
 * cross = x * softmax_f(g_cross * inv_tau)[field].  Either output (with its weights) may be NULL. */
int dctr_edcn_regulate(const float* x, int64_t x_stride, int64_t batch, int32_t fields, int32_t dim, const float* g_deep,
                       const float* g_cross, float inv_tau, float* deep, int64_t deep_stride, float* cross, int64_t cross_stride,
                       void* stream);
/* BridgeModule's elementwise forms over rows of dim columns: DCTR_EDCN_BRIDGE_ADD c + h, _HADAMARD c * h, _ATTENTION
 * softmax(ax) * c + softmax(ah) * h with the softmaxes over the dim columns of a row (ax / ah: the scores BEFORE the softmax). */
int dctr_edcn_bridge(int32_t kind, const float* c, int64_t c_stride, const float* h, int64_t h_stride, const float* ax, int64_t ax_stride,
                     const float* ah, int64_t ah_stride, int64_t batch, int32_t dim, float* out, int64_t out_stride, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The multi-task models' expert / gate / tower stack — deepctr/models/multitask/{mmoe,ple,sharedbottom,esmm}.py
 *   One LEVEL (DCTR_MTL_LEVEL: MMOE once, PLE's cgc_net num_levels times) over n_slots input slots, slot s = the in_dim columns from
 *   x_offsets[s] of x [B, x_stride], read in place:
 *       expert e : h_e = DNN_e(X_expert_src[e])           n_layers layers of units[l] for every expert, weights expert_w[e * n_layers + l]
 *                                                         (Keras layout [in, out]), bias, optional BatchNormalization affine, activation
 *       gate g   : z_g = GateDNN_g(X_gate_src[g])         (n_gate_layers may be 0: z_g = the slot);  p_g = softmax(z_g gate_kernel[g]),
 *                                                         gate_kernel[g] [dz, gate_n[g]], no bias
 *                  O_g = sum_j p_g[j] * h_{members[g][j]}  -> out columns [out_offset + g * H, + H),  H = units[n_layers - 1]
 *       members: the gates' index lists into the experts, concatenated (gate g's start = sum of gate_n before it).
 *   The TOWERS (DCTR_MTL_TOWERS): tower t < n_experts = DNN_t (n_layers may be 0) over slot expert_src[t], then . head_w[t],
 *       + global_bias[t][0], sigmoid where binary[t] -> probs[t * probs_stride + b];  esmm = 1 (two towers, both binary):
 *       probs[1] = sigmoid(l_0) * sigmoid(l_1) (esmm.py:60-63).
 *   dctr_mtl_level_fwd / dctr_mtl_towers_fwd are the FUSED route: one launch, slots, layer outputs, every expert's output and the gate
 *   weights in LDS, exact fp32 on v_mfma_f32_16x16x4_f32, no atomics (the same bits on every call).  It takes activations LINEAR | RELU |
 *   SIGMOID | TANH, <= 8 slots, <= 16 experts (8 towers) of <= 4 layers and <= 32 layers together, <= 8 gates of <= 4 layers and <= 16
 *   together, <= 64 members in all, while a tile of 16 rows fits 160 KiB of LDS.  Everything else answers DCTR_E_UNSUPPORTED there and
 *   DCTR_MTL_ROUTE_LAYERED from dctr_mtl_route: the host then runs the DNNs through dctr_mlp_fwd and the mixtures through dctr_mtl_mix.
 * ------------------------------------------------------------------------------------------------ */
enum { DCTR_MTL_LEVEL = 0, DCTR_MTL_TOWERS = 1 };
enum { DCTR_MTL_ROUTE_AUTO = 0, DCTR_MTL_ROUTE_FUSED = 1, DCTR_MTL_ROUTE_LAYERED = 2 };
typedef struct {
    int64_t batch;
    const float* x;                       /* [B, x_stride] fp32 */
    int64_t x_stride;
    const int64_t* x_offsets;             /* HOST [n_slots]: first column of every slot */
    int32_t n_slots;
    int32_t in_dim;                       /* width of every slot */
    int32_t n_experts;                    /* E (towers: T) */
    int32_t n_layers;                     /* level: >= 1; towers: >= 0 */
    const int32_t* units;                 /* HOST [n_layers] */
    const int32_t* expert_src;            /* HOST [E]: slot of every expert / tower */
    const float* const* expert_w;         /* HOST [E * n_layers] of DEVICE pointers */
    const float* const* expert_b;
    const float* const* expert_bn_scale;  /* NULL, or [E * n_layers] (entries may be NULL) */
    const float* const* expert_bn_shift;
    int32_t activation;                   /* DCTR_ACT_* (fused: not DICE) */
    int32_t route;                        /* DCTR_MTL_ROUTE_AUTO | _LAYERED (the query answers LAYERED, the launch declines) */
    int32_t n_gates;                      /* level: G >= 1 */
    int32_t n_gate_layers;                /* >= 0 */
    const int32_t* gate_units;            /* HOST [n_gate_layers] */
    const int32_t* gate_src;              /* HOST [G] */
    const int32_t* gate_n;                /* HOST [G]: members per gate, >= 1 */
    const int32_t* members;               /* HOST [sum gate_n]: expert indices */
    const float* const* gate_w;           /* HOST [G * n_gate_layers] */
    const float* const* gate_b;
    const float* const* gate_bn_scale;
    const float* const* gate_bn_shift;
    const float* const* gate_kernel;      /* HOST [G] -> [dz, gate_n[g]] */
    float* out;                           /* level: [B, out_stride] */
    int64_t out_stride;
    int64_t out_offset;
    const float* const* head_w;           /* towers: HOST [T] -> [units[last] or in_dim] */
    const float* const* global_bias;      /* towers: NULL, or HOST [T] of device scalars (entries may be NULL) */
    const int32_t* binary;                /* towers: HOST [T], 1 = sigmoid */
    int32_t esmm;                         /* towers: 0 | 1 */
    int32_t tile_rows;                    /* 0 = the library's choice, or 16 | 32 | 64: at most this many rows per workgroup */
    float* probs;                         /* towers: [T, probs_stride] */
    int64_t probs_stride;                 /* >= batch */
} dctr_mtl_args_t;
/* The route these arguments take for kind = DCTR_MTL_LEVEL | DCTR_MTL_TOWERS (DCTR_MTL_ROUTE_FUSED / _LAYERED), or the DCTR_E_* the size
 * and index checks answer.  Host arrays are read, device pointers are not looked at. */
int dctr_mtl_route(const dctr_mtl_args_t* args, int32_t kind);
int dctr_mtl_level_fwd(const dctr_mtl_args_t* args, void* stream);
int dctr_mtl_towers_fwd(const dctr_mtl_args_t* args, void* stream);
/* The layered route's mixture: expert outputs h [B, h_stride] (expert e in columns [e * width, + width)), per gate its input rows
 * z[g] [B, z_stride[g]] of z_dim columns and its kernel [z_dim, gate_n[g]]:  out columns [out_offset + g * width, + width) =
 * sum_j softmax(z_g kernel_g)[j] * h_{members[g][j]}.  members: HOST array (checked) and the same values on the device (members_dev).
 * Any shape; gates go out eight per launch; no atomics. */
typedef struct {
    int64_t batch;
    const float* h;
    int64_t h_stride;
    int32_t n_experts;
    int32_t width;
    int32_t n_gates;
    int32_t z_dim;
    const float* const* z;                /* HOST [G] of DEVICE pointers */
    const int64_t* z_stride;              /* HOST [G] */
    const float* const* gate_kernel;      /* HOST [G] */
    const int32_t* gate_n;                /* HOST [G] */
    const int32_t* members;               /* HOST [sum gate_n] */
    const int32_t* members_dev;           /* DEVICE copy of members */
    float* out;
    int64_t out_stride;
    int64_t out_offset;
} dctr_mtl_mix_args_t;
int dctr_mtl_mix(const dctr_mtl_mix_args_t* args, void* stream);
/* Backward of dctr_mtl_mix (the multi-task training step).  h, z, gate_kernel, gate_n, members, members_dev as the forward
 * took them; d_out [B, d_out_stride]: gate g's gradient in columns [d_out_offset + g * width, + width).  Per row b and gate g, with
 * p = softmax(z_g kernel_g) recomputed:  a_j = <d_out_g[b,:], h_{members[g][j]}[b,:]>,
 *     ds[b, first_g + j] = p_j (a_j - sum_i p_i a_i)       first_g = sum of gate_n before g: d loss / d (z_g kernel_g)
 *     dh[b, e * width + c] = sum over (g, j) with members[g][j] == e of p_j d_out_g[b, c]   (g ascending, then j; zeros for an expert no
 *                                                                                             gate mixes: all n_experts * width columns are written)
 *     logits (optional) [b, first_g + j] = (z_g kernel_g)[j]
 * No weight gradient and no dz: those are a bias-free linear layer's (dctr_mlp_bwd over z_g with d_out = ds_g).  dh, ds and logits must
 * not overlap the inputs.  Any shape; gates go out eight per launch; no atomics (the same bits on every call). */
typedef struct {
    int64_t batch;
    const float* h;
    int64_t h_stride;
    int32_t n_experts;
    int32_t width;
    int32_t n_gates;
    int32_t z_dim;
    const float* const* z;                /* HOST [G] of DEVICE pointers */
    const int64_t* z_stride;              /* HOST [G] */
    const float* const* gate_kernel;      /* HOST [G] */
    const int32_t* gate_n;                /* HOST [G] */
    const int32_t* members;               /* HOST [sum gate_n] */
    const int32_t* members_dev;           /* DEVICE copy of members */
    const float* d_out;
    int64_t d_out_stride;
    int64_t d_out_offset;
    float* dh;                            /* [B, dh_stride], dh_stride >= n_experts * width */
    int64_t dh_stride;
    float* ds;                            /* [B, ds_stride], ds_stride >= sum gate_n */
    int64_t ds_stride;
    float* logits;                        /* NULL, or [B, logits_stride >= sum gate_n] */
    int64_t logits_stride;
} dctr_mtl_mix_bwd_args_t;
int dctr_mtl_mix_bwd(const dctr_mtl_mix_bwd_args_t* args, void* stream);
/* The multi-task loss gradient.  pred [T, pred_stride]: the towers' outputs — sigmoid(logit_t) where binary[t], else logit_t; with esmm
 * (two binary tasks) row 1 is sigmoid(l_cvr), NOT the product.  y [T, y_stride] labels.  Writes
 *     dlogit[t * dlogit_stride + b] = d (sum_t loss_weight[t] * mean_b loss_t) / d logit_t[b]
 * and ADDS  loss_sum[t] += sum_b (reported loss of task t),  dbias[t][0] += sum_b dlogit[t, b]  (where dbias and dbias[t] are not NULL).
 *     binary + DCTR_MTL_LOSS_BCE:      gradient w (p - y) / B (the logit form); reported: -(y log pc + (1 - y) log(1 - pc)), pc = p
 *                                      clipped to [1e-7, 1 - 1e-7] (Keras' epsilon; in float32 the upper bound is 1 - 2^-23)
 *     regression + DCTR_MTL_LOSS_MSE:  gradient 2 w (l - y) / B; reported (l - y)^2
 *     esmm: p0 = pred[0], c = pred[1], p1 = p0 c.  Task 0 as above; task 1 reports the clipped form on p1 and takes its gradient from it:
 *           g = w_1 (-y / pc + (1 - y) / (1 - pc)) / B where 1e-7 <= p1 <= 1 - 1e-7, else 0;  dlogit[0] += g p1 (1 - p0),
 *           dlogit[1] = g p1 (1 - c).
 * Every other (binary, loss kind) pair answers DCTR_E_UNSUPPORTED, an unknown loss kind DCTR_E_ENUM.  One workgroup per task reduces in a
 * fixed order: no atomics. */
enum { DCTR_MTL_LOSS_BCE = 0, DCTR_MTL_LOSS_MSE = 1 };
typedef struct {
    int64_t batch;
    int32_t n_tasks;
    int32_t esmm;                         /* 0 | 1 */
    const float* pred;
    int64_t pred_stride;                  /* >= batch */
    const float* y;
    int64_t y_stride;
    const int32_t* loss_kind;             /* HOST [T]: DCTR_MTL_LOSS_* */
    const int32_t* binary;                /* HOST [T] */
    const float* loss_weight;             /* HOST [T] */
    float* dlogit;                        /* [T, dlogit_stride] */
    int64_t dlogit_stride;
    float* loss_sum;                      /* DEVICE [T], added to */
    float* const* dbias;                  /* NULL, or HOST [T] of device scalars (entries may be NULL), added to */
} dctr_mtl_loss_args_t;
int dctr_mtl_loss_grad(const dctr_mtl_loss_args_t* args, void* stream);
/* dst[b, dst_offset + c] = (accumulate ? dst[b, dst_offset + c] : 0) + src[0][b, c] + src[1][b, c] + ... for c < n, summed in that order.
 * src / src_stride: HOST arrays of n_src <= 16 device pointers and their row strides (>= n).  The gradient of a slot that several DNNs
 * read: dctr_mlp_bwd WRITES dx, so each reader writes to scratch and this launch forms the sum.  dst must not overlap a source. */
int dctr_mtl_sum_slots(const float* const* src, const int64_t* src_stride, int32_t n_src, int64_t batch, int32_t n, float* dst,
                       int64_t dst_stride, int64_t dst_offset, int32_t accumulate, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Transformer.call x n_layers — deepctr/layers/sequence.py:523-635 with PositionEncoding (:683-689) and LayerNormalization
 * (layers/normalization.py:34-43), stacked as deepctr/models/sequence/bst.py:84-92 stacks it, one launch
 *     queries [B, T, E] (sample stride q_stride, position stride q_row_stride, elements); keys the same shape (NULL: the queries).
 *     Per layer, with the layer's nine pointers query, key, value [E, E], fw1 [E, 4E], fw2 [4E, E] (Keras layout), ln_gamma, ln_beta
 *     [E], pe_q, pe_k [T, E] (the lookup tables ALREADY multiplied by float32(sqrt(E)), sequence.py:687-688):
 *       Xq = x + pe_q, Xk = keys + pe_k                               (use_positional_encoding; sequence.py:540-542)
 *       Q = Xq query, K = Xk key, V = Xk value, split into H heads of width d = E / H          (:544-552)
 *       s = Q_h K_h^T / float32(sqrt(d)); s = -2^32 + 1 where the key is masked, and on the diagonal with blinding   (:556-598)
 *       p = softmax(s - max s) * query mask;  r = concat_h(p V_h) (+ Xq with use_res)            (:600-617)
 *       r = LN(r)                                                       (use_layer_norm; :618-619)
 *       r = r + relu(r fw1) fw2 (use_feed_forward and use_res), then LN(r) again (use_feed_forward and use_layer_norm)   (:621-628)
 *       LN(x) = (x - mean) / sqrt(var + ln_eps) * ln_gamma + ln_beta, var the biased variance of the row (normalization.py:35-43)
 *     The next layer's queries and keys are r.  Masks: int32 lengths [B] (position t counts while t < length: tf.sequence_mask,
 *     :533-536) or uint8 [B, T]; at most one form per side, neither = every position counts.  A sample whose keys are all masked
 *     has a uniform softmax; with a zero query mask its attention output is 0 (no NaN).
 *     out: output_type NONE [B, T, E] at out_stride / out_row_stride (may alias queries: in place), MEAN / SUM [B, E] at out_stride
 *     over ALL T rows (:630-633).  key_mask_out: NULL, or uint8 [B, T] that receives the key mask of the first layer.
 *     Exact fp32 on v_mfma_f32_16x16x4_f32, no atomics: the same bits on every call.  FUSED route: the activations of a tile of samples
 *     stay in LDS (<= 160 KiB for one sample); larger samples take the GENERAL route through a workspace of
 *     dctr_transformer_workspace_bytes() (room for <= 256 workgroups), which is then REQUIRED (DCTR_E_NULL without, before anything is
 *     launched).  route = FUSED for a sample that does not fit answers DCTR_E_UNSUPPORTED.  No shape is refused for its size.
 *     Argument errors (nothing launched): NULL queries / layers / out or a NULL weight a flag needs (DCTR_E_NULL), seq_len or dim < 1,
 *     att_embedding_size * head_num != dim, strides smaller than the block (DCTR_E_DIM), both mask forms on one side, flags not 0 / 1,
 *     unknown output_type / route (DCTR_E_ENUM).
 * ------------------------------------------------------------------------------------------------ */
enum { DCTR_TRANSFORMER_OUT_NONE = 0, DCTR_TRANSFORMER_OUT_MEAN = 1, DCTR_TRANSFORMER_OUT_SUM = 2 };
enum { DCTR_TRANSFORMER_ROUTE_AUTO = 0, DCTR_TRANSFORMER_ROUTE_FUSED = 1, DCTR_TRANSFORMER_ROUTE_GENERAL = 2 };
#define DCTR_TRANSFORMER_LAYER_PTRS 9
typedef struct {
    int64_t batch;
    const float* queries;            /* [B, T, E] fp32 */
    int64_t q_stride;                /* elements between samples */
    int64_t q_row_stride;            /* elements between positions, >= dim */
    const float* keys;               /* NULL (= queries), or [B, T, E] */
    int64_t k_stride;
    int64_t k_row_stride;
    int32_t seq_len;                 /* T >= 1 (queries and keys share it: the reference's seq_len_max) */
    int32_t dim;                     /* E >= 1 */
    int32_t att_embedding_size;      /* d, d * head_num == dim */
    int32_t head_num;                /* H */
    int32_t n_layers;                /* >= 1 */
    int32_t use_positional_encoding; /* 0 | 1 */
    int32_t use_res;
    int32_t use_feed_forward;
    int32_t use_layer_norm;
    int32_t blinding;
    int32_t output_type;             /* DCTR_TRANSFORMER_OUT_* */
    int32_t route;                   /* DCTR_TRANSFORMER_ROUTE_AUTO | _FUSED | _GENERAL */
    float ln_eps;                    /* the reference's 1e-9 */
    int32_t reserved;
    const float* const* layers;      /* HOST array [n_layers * 9] of DEVICE pointers (unused ones may be NULL) */
    const int32_t* query_lengths;    /* NULL or [B] */
    const int32_t* key_lengths;
    const uint8_t* query_mask;       /* NULL or [B, T] */
    const uint8_t* key_mask;
    float* out;
    int64_t out_stride;
    int64_t out_row_stride;          /* output_type NONE only */
    uint8_t* key_mask_out;           /* NULL or [B, T] */
    void* workspace;                 /* NULL, or device scratch of dctr_transformer_workspace_bytes() bytes, 16-B aligned */
    size_t workspace_bytes;
} dctr_transformer_args_t;
/* Bytes dctr_transformer_fwd needs (sizes, flags and route are read, pointers are not): 0 on the fused route up to 16 layers. */
size_t dctr_transformer_workspace_bytes(const dctr_transformer_args_t* args);
/* The route these arguments take (DCTR_TRANSFORMER_ROUTE_FUSED / _GENERAL), or the DCTR_E_* the checks answer. */
int dctr_transformer_route(const dctr_transformer_args_t* args);
int dctr_transformer_fwd(const dctr_transformer_args_t* args, void* stream);
/* The Transformer stack of a training step: dctr_transformer_train_fwd is dctr_transformer_fwd (the same kernel under one more
 * template flag, the same bits in out) that also writes a tape; dctr_transformer_bwd is the backward of the whole stack in one call.
 * fwd: as dctr_transformer_fwd (queries = x, layers, masks in either form, sizes, flags, route; out is written by the forward and
 *   ignored by the backward; fwd.workspace is the forward's alone).
 * tape: caller-allocated, dctr_transformer_tape_bytes(&fwd) bytes, written by the forward and read by the backward:
 *   float [n_layers - 1][B][T][E] contiguous: entry l - 1 is the input of layer l >= 1 (= the output of layer l - 1), the bits the
 *   forward produced.  Layer 0 reads x.  One layer: 0 bytes, the pointer may be NULL.  Everything else is recomputed in the backward
 *   with the forward's own arithmetic (the same device functions), so the recomputed activations are the forward's bits.
 * The backward.  d_out: the gradient of out: [B, T, E] at d_out_stride / d_out_row_stride for output NONE, [B, E] at d_out_stride for
 *   MEAN / SUM, which spread it over ALL T rows (d_out / T for MEAN).  Per layer, last to first, dy the gradient of its output:
 *     df = LNbwd(dy) (use_feed_forward and use_layer_norm), else dy
 *     use_feed_forward and use_res: h = relu(r fw1);  dh = (df fw2^T) [h > 0];  d_fw2 += h^T df;  d_fw1 += r^T dh;  dr = df + dh fw1^T
 *     da = LNbwd(dr) (use_layer_norm), else dr.   LNbwd(g) at the row x it normalised, xh = (x - mean) / sd, sd = sqrt(var + ln_eps):
 *       d_ln_gamma += sum_rows g xh;  d_ln_beta += sum_rows g;  gh = g gamma;  dx = (gh - mean(gh) - xh mean(gh xh)) / sd.
 *       Both LayerNorm applications share gamma / beta, so d_ln_gamma / d_ln_beta are the sum of both.  An all-zero row (use_res = 0
 *       and a masked query) has xh = 0 and sd = sqrt(ln_eps): its dx is finite.
 *     attention, per head, p~ = p * query mask (the mask multiplies p AFTER the softmax):  dV_j = sum_i p~_ij da_i;  dP_ij = da_i . V_j;
 *       ds_ij = p~_ij (dP_ij - sum_k p~_ik dP_ik) / sqrt(d) at keys that count, and 0 at a masked key and on the blinded diagonal
 *       (where(mask, s, -2^32+1) passes no gradient there).  A row whose keys are all masked has a uniform softmax: every ds is 0,
 *       dV still receives p~ da.   dQ_i = sum_j ds_ij K_j;  dK_j = sum_i ds_ij Q_i.
 *     dXq = dQ Wq^T (+ da with use_res);  dXk = dK Wk^T + dV Wv^T;  d_query += Xq^T dQ;  d_key += Xk^T dK;  d_value += Xk^T dV
 *     d_pe_q += sum over samples of dXq, d_pe_k of dXk ([T, E], in the units of the PRE-SCALED tables the op reads: the caller
 *       multiplies by float32(sqrt(E)) for the lookup tables);  the layer's dx = dXq + dXk is the dy of the layer before.
 *   One persistent launch: a workgroup owns a tile of samples; the layer's recomputed activations, the gradient rows and the three
 *   numbers per (row, head) of the attention (max, query mask / sum, sum p~ dP) live in LDS, or in a per-workgroup workspace slice when
 *   a sample does not fit 160 KiB or fwd.route is GENERAL.  Every matrix product is exact fp32 on v_mfma_f32_16x16x4_f32; the
 *   attention backward is a thread per (row, head), one walk for dQ and one for dK / dV, no [T, T] matrix anywhere.  Each workgroup
 *   adds its weight-gradient partials tile after tile into its own workspace slice and a second launch sums the slices in workgroup
 *   order: no atomics, dx and every weight gradient repeat bit for bit from call to call.
 * dx: NULL, or [B, T, E] at its strides, written, or added to with accumulate.  d_layers: NULL, or a HOST array [9 * n_layers] of
 *   DEVICE pointers of the weights' shapes in fwd.layers' order (d_pe_q / d_pe_k [T, E]), ACCUMULATED into; any entry may be NULL,
 *   and an entry whose weight the flags switch off is left untouched.
 * max_blocks: 0, or the most workgroups of the persistent launch (at most 256 either way; each walks its tiles).
 * workspace: dctr_transformer_bwd_workspace_bytes() bytes, 16-B aligned (DCTR_E_NULL without, nothing launched); it depends on batch
 *   and max_blocks.
 * dctr_transformer_bwd_supported answers 1 or 0 from sizes and flags only: self-attention (fwd.keys NULL or the queries), n_layers
 *   <= DCTR_TRANSFORMER_BWD_MAX_LAYERS; every seq_len, dim, head_num, flag set, output type and mask form the forward takes.
 *   Separate keys and more layers answer DCTR_E_UNSUPPORTED from dctr_transformer_bwd with nothing launched.  Dropout has no operand:
 *   a step with an active dropout does not use this op.
 * Argument errors answer the codes of dctr_transformer_fwd (plus DCTR_E_NULL for a missing x, d_out or tape, DCTR_E_DIM for d_out / dx
 *   strides smaller than their blocks, DCTR_E_ENUM for accumulate not 0 / 1 or max_blocks < 0); nothing is launched or written then. */
#define DCTR_TRANSFORMER_BWD_MAX_LAYERS 8
typedef struct {
    dctr_transformer_args_t fwd;
    void* tape;                      /* dctr_transformer_tape_bytes() bytes (NULL when that is 0) */
    size_t tape_bytes;
    const float* d_out;              /* [B, T, E] (output NONE) or [B, E] (MEAN / SUM) */
    int64_t d_out_stride;
    int64_t d_out_row_stride;        /* output NONE only */
    float* dx;                       /* NULL, or [B, T, E] */
    int64_t dx_stride;
    int64_t dx_row_stride;
    float* const* d_layers;          /* NULL, or HOST array [n_layers * 9] of DEVICE pointers; each may be NULL */
    int32_t accumulate;              /* 0 | 1: dx written | added to */
    int32_t max_blocks;
    void* workspace;                 /* the backward's: dctr_transformer_bwd_workspace_bytes() bytes, 16-B aligned */
    size_t workspace_bytes;
} dctr_transformer_train_args_t;
size_t dctr_transformer_tape_bytes(const dctr_transformer_args_t* args);                    /* host only; 0 for refused arguments */
int dctr_transformer_train_fwd(const dctr_transformer_train_args_t* args, void* stream);
int dctr_transformer_bwd_supported(const dctr_transformer_train_args_t* args);              /* host only */
size_t dctr_transformer_bwd_workspace_bytes(const dctr_transformer_train_args_t* args);     /* host only */
int dctr_transformer_bwd(const dctr_transformer_train_args_t* args, void* stream);
/* LayerNormalization.call alone (layers/normalization.py:34-43) over the rows of x [rows, dim]: (x - mean) / sqrt(var + eps) * gamma +
 * beta with the biased variance; gamma / beta NULL = scale / center off.  out may be x. */
int dctr_layer_norm_fwd(const float* x, int64_t rows, int32_t dim, int64_t x_stride, const float* gamma, const float* beta, float eps,
                        float* out, int64_t out_stride, void* stream);

/* ------------------------------------------------------------------------------------------------
 * DynamicGRU.call — deepctr/layers/sequence.py:760-815 over tf.nn.rnn_cell.GRUCell and the attention-gated cells of
 * deepctr/contrib/utils.py (QAAttGRUCell :208-261 "AGRU", VecAttGRUCell :327-378 "AUGRU") under dynamic_rnn(sequence_length=...)
 * (contrib/rnn_v2.py:1324-1401): the whole time loop in one launch, one or two stacked layers (DIEN's gru1 -> gru2)
 *     x [B, T, E] (sample stride x_stride, step stride x_row_stride, elements); inputs and units share the width E.
 *     Per layer its four pointers gate kernel [2E, 2E], gate bias [2E], candidate kernel [2E, E], candidate bias [E] (Keras layout):
 *       [r | u] = sigmoid([x_t | h] gate_kernel + gate_bias)              (gate order r then u)
 *       c = tanh([x_t | r * h] candidate_kernel + candidate_bias)
 *       GRU:   h' = u h + (1 - u) c
 *       AGRU:  h' = (1 - a) h + a c
 *       AUGRU: u <- (1 - a) u, then the GRU form                            a = att_scores[b, t]
 *     h_0 = 0.  lengths [B] int32: at steps t >= length the state is copied through and the emitted row is zero; the final state
 *     is the state at min(length, T); lengths <= 0 give a zero final state and all-zero rows, lengths > T behave as T.
 *     scale_input: x_t is multiplied by att_scores[b, t] first (AIGRU's multiply([rnn_outputs, scores]) folded in).
 *     n_layers = 2 (cell GRU only): layer 2's step t consumes layer 1's h_t on chip; layer 1's [B, T, E] is never written.
 *     out: return_sequence 1 -> [B, T, E] at out_stride / out_row_stride, 0 -> the final state [B, E] at out_stride (so that it can
 *     be written straight into its columns of a wider buffer).
 *     Exact-fp32 products on v_mfma_f32_16x16x4_f32, sigmoid / tanh on the hardware exp and rcp (they saturate to 0 / 1 / -1 without
 *     NaN), no atomics: the same bits on every call.  RESIDENT route: the weights of every layer stay in LDS for all T steps
 *     (6 E^2 floats per layer next to the tiles within 160 KiB: E <= 74 for one layer, E <= 51 for two); STREAMED route: the same
 *     step code with the weights read from global / L2 each step, and from E = 497 (308 for two layers) the tiles of a workgroup in a workspace of
 *     dctr_gru_workspace_bytes() (room for <= 256 workgroups), which is then REQUIRED (DCTR_E_NULL without, before anything is
 *     launched).  route = RESIDENT for weights that do not fit answers DCTR_E_UNSUPPORTED.  No shape is refused for its size.
 *     Argument errors (nothing launched): NULL x / lengths / layers / out / a layer's pointer, NULL att_scores with an attention-gated
 *     cell or scale_input (DCTR_E_NULL), seq_len or dim < 1, n_layers outside 1..2, strides smaller than the block (DCTR_E_DIM),
 *     unknown cell / route, flags not 0 / 1, two layers with an attention-gated cell (DCTR_E_ENUM).
 * ------------------------------------------------------------------------------------------------ */
enum { DCTR_GRU_CELL_GRU = 0, DCTR_GRU_CELL_AGRU = 1, DCTR_GRU_CELL_AUGRU = 2 };
enum { DCTR_GRU_ROUTE_AUTO = 0, DCTR_GRU_ROUTE_RESIDENT = 1, DCTR_GRU_ROUTE_STREAMED = 2 };
#define DCTR_GRU_LAYER_PTRS 4
typedef struct {
    int64_t batch;
    const float* x;                  /* [B, T, E] fp32 */
    int64_t x_stride;                /* elements between samples */
    int64_t x_row_stride;            /* elements between steps, >= dim */
    const int32_t* lengths;          /* [B] */
    const float* att_scores;         /* NULL, or [B, T] at att_stride (AGRU / AUGRU / scale_input) */
    int64_t att_stride;              /* elements between samples, >= seq_len */
    int32_t seq_len;                 /* T >= 1 */
    int32_t dim;                     /* E >= 1 */
    int32_t n_layers;                /* 1 | 2 */
    int32_t cell;                    /* DCTR_GRU_CELL_* */
    int32_t scale_input;             /* 0 | 1 */
    int32_t return_sequence;         /* 0 | 1 */
    int32_t route;                   /* DCTR_GRU_ROUTE_AUTO | _RESIDENT | _STREAMED */
    int32_t reserved;
    const float* const* layers;      /* HOST array [n_layers * 4] of DEVICE pointers */
    float* out;
    int64_t out_stride;
    int64_t out_row_stride;          /* return_sequence only */
    void* workspace;                 /* NULL, or device scratch of dctr_gru_workspace_bytes() bytes, 16-B aligned */
    size_t workspace_bytes;
} dctr_gru_args_t;
/* Bytes dctr_gru_fwd needs (sizes, flags and route are read, pointers are not): 0 while a workgroup's tiles fit the LDS. */
size_t dctr_gru_workspace_bytes(const dctr_gru_args_t* args);
/* The route these arguments take (DCTR_GRU_ROUTE_RESIDENT / _STREAMED), or the DCTR_E_* the checks answer. */
int dctr_gru_route(const dctr_gru_args_t* args);
int dctr_gru_fwd(const dctr_gru_args_t* args, void* stream);

/* Backward of ONE DynamicGRU layer over all T steps, one launch (backpropagation through time).  fwd: batch, x (+ strides), lengths,
 * att_scores (+ stride), seq_len, dim, cell, scale_input, return_sequence, route and layers[0..3] are read; n_layers must be 1 (a
 * stack is one call per layer, last to first), out / out strides / workspace are ignored.  h_seq is the forward's return_sequence = 1
 * output of this layer: row t holds h_t for t < length, h_{t-1} is read from it (h_{-1} = 0) and rows at t >= length are never read.
 * d_out: the gradient of the forward's output, [B, T, E] at d_out_stride / d_out_row_stride with fwd.return_sequence, else the
 * gradient of the final state [B, E] at d_out_stride (injected at t = length - 1).  lengths are clamped to [0, T] as the forward does.
 * Per live step, last to first, with dh the gradient reaching h_t (from step t + 1, plus d_out):
 *     [r | u] and c recomputed from x_t and h_{t-1} with the forward's arithmetic;
 *     GRU / AUGRU (u' = u, or (1 - a) u):  dc = dh (1 - u');  du' = dh (h_{t-1} - c);  dh_prev = dh u'
 *                 AUGRU:  du = du' (1 - a);  da_t += -sum_e du' u                  GRU: du = du'
 *     AGRU:       dc = dh a;  dh_prev = dh (1 - a);  da_t += sum_e dh (c - h_{t-1});  du = 0
 *     dzc = dc (1 - c^2);   [dx_c | d(rh)] = dzc Wc^T;   dWc += [x_t | r h_{t-1}]^T dzc;   dbc += sum_rows dzc
 *     dr = d(rh) h_{t-1};   dh_prev += d(rh) r
 *     dzg = [dr r (1 - r) | du u (1 - u)];   [dx_g | dh_g] = dzg Wg^T;   dWg += [x_t | h_{t-1}]^T dzg;   dbg += sum_rows dzg
 *     dx_t = dx_c + dx_g;   dh_prev += dh_g;       scale_input:  da_t += sum_e dx_t x_raw,t;  dx_raw,t = a_t dx_t
 * A row at t >= length passes dh through and contributes nothing else; rows of length <= 0 contribute nothing.
 * Outputs, each may be NULL: dx [B, T, E] at its strides, written (exact zeros at t >= length) or, with accumulate, added to;
 * d_att [B, T] at d_att_stride, written (zeros at t >= length; NULL or a plain GRU without scale_input: not touched);
 * d_layers: HOST array of 4 DEVICE pointers of the weights' shapes, ACCUMULATED into (the array or any entry may be NULL) — summed
 * on chip per workgroup over all steps and tiles, one atomic per workgroup and element.  dx, d_att and the dh chain use no atomics:
 * the same bits on every call.  All products are exact fp32 on v_mfma_f32_16x16x4_f32.  The weights stay in LDS next to the
 * weight-gradient sums and the tiles while all fit the 160 KiB (E <= 48), else they are read from global / L2 each step (route
 * STREAMED forces that); from E = 66 the sums and the tiles alone exceed the LDS: DCTR_E_UNSUPPORTED, as two layers and scale_input
 * with an attention-gated cell (dctr_gru_bwd_supported: 1 / 0, sizes and flags only).  No workspace is needed
 * (dctr_gru_bwd_workspace_bytes answers 0).  Argument errors as dctr_gru_fwd; nothing is launched or written then. */
typedef struct {
    dctr_gru_args_t fwd;
    const float* h_seq;              /* [B, T, E] */
    int64_t h_stride;                /* elements between samples */
    int64_t h_row_stride;            /* elements between steps, >= dim */
    const float* d_out;              /* [B, T, E] (fwd.return_sequence) or [B, E] */
    int64_t d_out_stride;
    int64_t d_out_row_stride;        /* fwd.return_sequence only */
    float* dx;                       /* NULL, or [B, T, E] */
    int64_t dx_stride;
    int64_t dx_row_stride;
    float* d_att;                    /* NULL, or [B, T] */
    int64_t d_att_stride;            /* >= seq_len */
    float* const* d_layers;          /* NULL, or HOST array [4] of DEVICE pointers, shapes of fwd.layers; each may be NULL */
    int32_t accumulate;              /* 0 | 1: dx written | added to */
    int32_t max_blocks;              /* 0 = 2 per compute unit, else the most workgroups to launch (each walks its tiles) */
} dctr_gru_bwd_args_t;
int dctr_gru_bwd_supported(const dctr_gru_bwd_args_t* args);          /* host only */
size_t dctr_gru_bwd_workspace_bytes(const dctr_gru_bwd_args_t* args); /* host only; 0: none */
int dctr_gru_bwd(const dctr_gru_bwd_args_t* args, void* stream);

/* ------------------------------------------------------------------------------------------------
 * BiLSTM.call — deepctr/layers/sequence.py:318-428 over tf.keras.layers.LSTM as documented: two independent stacks of n_layers LSTMs,
 * the whole of both in one launch (DSIN's session-interest interaction, models/sequence/dsin.py:121-122)
 *     x [B, T, in_dim] (sample stride x_stride, step stride x_row_stride, elements).
 *     Per layer its six pointers fw kernel [D, 4u], fw recurrent kernel [u, 4u], fw bias [4u], then the same three of the backward
 *     stack (Keras layout; D = in_dim for layer 0, units after it), gate order i | f | c~ | o:
 *       z = x_t W + h U + b;  i, f, o = sigma(z_i, z_f, z_o);  g = tanh(z_c);  c' = f c + i g;  h' = o tanh(c');  h_0 = c_0 = 0
 *     The forward stack walks t = 0 .. T-1, the backward stack t = T-1 .. 0 with every layer's output back in time order before it
 *     feeds the next.  No mask, no lengths: every step runs.  Layer l >= n_layers - res_layers adds its input to its output, in each
 *     stack (res_layers > n_layers behaves as n_layers; a residual over layer 0 needs in_dim == units).
 *     recurrent_activation: sigma = sigmoid (0, the TF 2.x default) or hard_sigmoid clip(0.2 z + 0.5, 0, 1) (1, the TF 1.x default).
 *     merge_mode: out [B, T, u] = fw | bw | fw + bw | fw * bw | (fw + bw) / 2, CONCAT out [B, T, 2u] = [fw | bw], NONE fw -> out and
 *     bw -> out_bw.  out at out_stride / out_row_stride: columns beside the written ones are left alone.
 *     Exact-fp32 products on v_mfma_f32_16x16x4_f32, sigmoid / tanh on the hardware exp and rcp (they saturate without NaN), no
 *     atomics: the same bits on every call.  RESIDENT route: the current layer's kernels of both directions stay in LDS for its T
 *     steps (next to the tiles within 160 KiB); STREAMED route: the same step code with the kernels read from global / L2;
 *     WORKSPACE: streamed, with a workgroup's tiles in a workspace of dctr_bilstm_workspace_bytes() (room for <= 256 workgroups) —
 *     taken by AUTO when the tiles exceed the LDS — which is then REQUIRED (DCTR_E_NULL without, before anything is launched).
 *     route = RESIDENT for kernels that do not fit answers DCTR_E_UNSUPPORTED.  No shape is refused for its size.
 *     Argument errors (nothing launched): NULL x / layers / out / a layer's pointer, NULL out_bw with NONE (DCTR_E_NULL), sizes < 1,
 *     n_layers outside 1..DCTR_LSTM_MAX_LAYERS, res_layers < 0, a residual over in_dim != units, strides smaller than the block
 *     (DCTR_E_DIM), unknown merge_mode / recurrent_activation / route (DCTR_E_ENUM), on the RESIDENT route a kernel or recurrent
 *     kernel that is not 16-byte aligned (DCTR_E_ALIGN: the copy into LDS reads them 16 bytes at a time).
 * ------------------------------------------------------------------------------------------------ */
enum { DCTR_LSTM_MERGE_FW = 0, DCTR_LSTM_MERGE_BW = 1, DCTR_LSTM_MERGE_SUM = 2, DCTR_LSTM_MERGE_MUL = 3, DCTR_LSTM_MERGE_AVE = 4,
       DCTR_LSTM_MERGE_CONCAT = 5, DCTR_LSTM_MERGE_NONE = 6 };
enum { DCTR_LSTM_ROUTE_AUTO = 0, DCTR_LSTM_ROUTE_RESIDENT = 1, DCTR_LSTM_ROUTE_STREAMED = 2, DCTR_LSTM_ROUTE_WORKSPACE = 3 };
#define DCTR_LSTM_LAYER_PTRS 6
#define DCTR_LSTM_MAX_LAYERS 8
typedef struct {
    int64_t batch;
    const float* x;                  /* [B, T, in_dim] fp32 */
    int64_t x_stride;                /* elements between samples */
    int64_t x_row_stride;            /* elements between steps, >= in_dim */
    int32_t seq_len;                 /* T >= 1 */
    int32_t in_dim;                  /* >= 1 */
    int32_t units;                   /* u >= 1 */
    int32_t n_layers;                /* 1 .. DCTR_LSTM_MAX_LAYERS */
    int32_t res_layers;              /* >= 0 */
    int32_t merge_mode;              /* DCTR_LSTM_MERGE_* */
    int32_t recurrent_activation;    /* 0 sigmoid | 1 hard_sigmoid */
    int32_t route;                   /* DCTR_LSTM_ROUTE_* */
    const float* const* layers;      /* HOST array [n_layers * 6] of DEVICE pointers */
    float* out;
    int64_t out_stride;
    int64_t out_row_stride;
    float* out_bw;                   /* DCTR_LSTM_MERGE_NONE only */
    int64_t out_bw_stride;
    int64_t out_bw_row_stride;
    void* workspace;                 /* NULL, or device scratch of dctr_bilstm_workspace_bytes() bytes, 16-B aligned */
    size_t workspace_bytes;
} dctr_lstm_args_t;
/* Bytes dctr_bilstm_fwd needs (sizes, flags and route are read, pointers are not): 0 while a workgroup's tiles fit the LDS. */
size_t dctr_bilstm_workspace_bytes(const dctr_lstm_args_t* args);
/* The route these arguments take (DCTR_LSTM_ROUTE_RESIDENT, or _STREAMED with or without a workspace), or the DCTR_E_* the checks answer. */
int dctr_bilstm_route(const dctr_lstm_args_t* args);
int dctr_bilstm_fwd(const dctr_lstm_args_t* args, void* stream);
/* The BiLSTM of a training step: dctr_bilstm_train_fwd is dctr_bilstm_fwd (the same kernel, the same bits without masks) with the
 * input dropout of every LSTM and a tape, dctr_bilstm_bwd backpropagation through time of both stacks, all layers and all steps.
 * fwd: as dctr_bilstm_fwd (x, layers, sizes, flags, route; out / out_bw are written by the forward and ignored by the backward;
 * fwd.workspace is not used by either).
 * masks: NULL, or a HOST array [2 * n_layers] of DEVICE pointers in the order fw layer 0, bw layer 0, fw layer 1, ...; each NULL (no
 *   dropout for that LSTM) or [B, D_l] contiguous floats that already hold 0 or 1 / (1 - rate) (D_0 = in_dim, units after it).  A mask
 *   multiplies its LSTM's input where it enters x_t W, the same for every step; the residual adds the unmasked input.
 * tape: caller-allocated, dctr_bilstm_tape_bytes(&fwd) bytes, written by the forward and read by the backward:
 *   float [n_layers][2 directions][T][2][B][units]: for layer l, direction d (0 fw, 1 bw) and TIME position t, [0] is h_t and [1] is
 *   c_t, the bits the forward produced (h before the residual is added).  A direction the merge_mode never reads is not written.
 * The backward.  d_out: the gradient of out ([B, T, u], [B, T, 2u] for CONCAT) at its strides; d_out_bw: that of out_bw (NONE only).
 *   Merge: AVE d_fw = d_bw = d_out / 2;  SUM d_out;  MUL d_fw = d_out y_bw, d_bw = d_out y_fw (the stacks' outputs rebuilt from the
 *   tape);  CONCAT the two halves;  FW / BW that stack alone (the other is neither walked nor given gradients);  NONE d_out, d_out_bw.
 *   Per stack, layer (last to first) and step (the reverse of the direction's walk), dh the gradient reaching h_t:
 *     i, f, g, o recomputed from [in_t * m | h_prev] [W; U] + b with the forward's arithmetic;  c_prev, c_t from the tape
 *     tc = tanh(c_t);  do = dh tc;  dc = dc_next + dh o (1 - tc^2);  di = dc g;  df = dc c_prev;  dg = dc i;  dc_prev = dc f
 *     dz = [di i (1 - i) | df f (1 - f) | dg (1 - g^2) | do o (1 - o)];   [d(in * m)_t | dh_prev] = dz [W; U]^T
 *     dW += (in_t * m)^T dz;  dU += h_prev^T dz;  db += sum_rows dz;   d_in_t = d(in * m)_t * m (+ d_y_t when the layer is residual)
 *   One recurrent launch: a workgroup owns (16 samples, direction) with the layer's gradient and input sequences in LDS; exact fp32
 *   on v_mfma_f32_16x16x4_f32, the dz [W; U]^T products read the forward's weight copy (resident in LDS while it fits next to the
 *   tiles, else streamed from global / L2; fwd.route forces either for the backward, whatever route the forward took).  It stores dz and the rows [in * m | h_prev] to the workspace,
 *   one grouped GEMM launch forms every [dW; dU; db] in stored k-slices, and a last launch sums the slices into d_layers and the
 *   two directions' input gradients into dx: no atomics anywhere, the same bits on every call.
 * dx: NULL, or [B, T, in_dim] at its strides, written, or added to with accumulate.  d_layers: NULL, or a HOST array [6 * n_layers]
 *   of DEVICE pointers of the weights' shapes in fwd.layers' order, ACCUMULATED into; any entry may be NULL.
 * max_blocks: 0, or the most workgroups of the recurrent launch (each walks its tiles).
 * workspace: dctr_bilstm_bwd_workspace_bytes() bytes, 16-B aligned (the backward's; DCTR_E_NULL without, nothing launched).
 * dctr_bilstm_bwd_supported answers 1 or 0 from sizes and flags only: sigmoid recurrent activation (hard_sigmoid has kinks and no
 *   model here trains under it), n_layers <= 4 (the grouped GEMM's eight groups), every merge_mode and res_layers, in_dim != units,
 *   every units and seq_len whose per-workgroup tiles fit the 160 KiB in both kernels; everything else answers
 *   DCTR_E_UNSUPPORTED from dctr_bilstm_bwd with nothing written (dctr_bilstm_train_fwd refuses only the tiles that do not fit).
 * Argument errors answer the codes of dctr_bilstm_fwd; nothing is launched or written then. */
typedef struct {
    dctr_lstm_args_t fwd;
    const float* const* masks;       /* NULL, or HOST array [2 * n_layers] of DEVICE pointers, each NULL or [B, D_l] */
    void* tape;                      /* dctr_bilstm_tape_bytes() bytes */
    size_t tape_bytes;
    const float* d_out;              /* [B, T, u] ([B, T, 2u] for CONCAT) */
    int64_t d_out_stride;
    int64_t d_out_row_stride;
    const float* d_out_bw;           /* DCTR_LSTM_MERGE_NONE only */
    int64_t d_out_bw_stride;
    int64_t d_out_bw_row_stride;
    float* dx;                       /* NULL, or [B, T, in_dim] */
    int64_t dx_stride;
    int64_t dx_row_stride;
    float* const* d_layers;          /* NULL, or HOST array [n_layers * 6] of DEVICE pointers; each may be NULL */
    int32_t accumulate;              /* 0 | 1: dx written | added to */
    int32_t max_blocks;
    void* workspace;                 /* the backward's: dctr_bilstm_bwd_workspace_bytes() bytes, 16-B aligned */
    size_t workspace_bytes;
} dctr_lstm_train_args_t;
size_t dctr_bilstm_tape_bytes(const dctr_lstm_args_t* args);                 /* host only; 0 for arguments the checks refuse */
int dctr_bilstm_train_fwd(const dctr_lstm_train_args_t* args, void* stream);
int dctr_bilstm_bwd_supported(const dctr_lstm_train_args_t* args);           /* host only */
size_t dctr_bilstm_bwd_workspace_bytes(const dctr_lstm_train_args_t* args);  /* host only */
int dctr_bilstm_bwd(const dctr_lstm_train_args_t* args, void* stream);
/* BiasEncoding.call — deepctr/layers/sequence.py:735-744, in place over a [B, S, T, E] view (sample / session / step strides in
 * elements, unit stride on the last axis): x[b, s, t, e] += item_bias[e] + seq_bias[t] + sess_bias[s]. */
int dctr_bias_encoding_fwd(float* x, int64_t batch, int32_t sess, int32_t seq_len, int32_t dim, int64_t x_stride, int64_t sess_stride,
                           int64_t row_stride, const float* sess_bias, const float* seq_bias, const float* item_bias, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The field-axis convolution stack of CCPM (deepctr/models/ccpm.py:62-70) and FGCNNLayer (deepctr/layers/interaction.py:1022-1047):
 * n_stages x [Conv2D(C_out, (w, 1), padding='same', activation='tanh', use_bias=True), then a pooling along the field axis], the
 * whole stack in one launch.
 *     x [B, F, E, C_0] channel-last (C_0 = in_channels, 1 for an embedding block), read in place: the F E C_0 columns from x_offset of a
 *     [B, x_stride] buffer.  Stage s: kernel [w, C_in, C_out] (keras' [w, 1, C_in, C_out]), bias [C_out]; rows = F for stage 0.
 *       y[b, r, e, co] = tanh(bias[co] + sum_{d, ci} xpad[b, r + d, e, ci] K[d, ci, co])
 *     a cross-correlation (K is not flipped); 'same' puts (w - 1) / 2 zero rows before the first row and w - 1 - (w - 1) / 2 after
 *     the last (w = 6: 2 and 3).  Pooling of a stage:
 *       DCTR_FIELDCONV_POOL_KMAX, arg k: the k largest of the rows for every (b, e, channel) in DESCENDING order of value
 *         (tf.nn.top_k(sorted=True), as KMaxPooling calls it; not the order-preserving variant), 1 <= k <= rows -> k rows
 *       DCTR_FIELDCONV_POOL_MAX, arg p: max over windows of p rows at stride p, 'valid': rows / p rows, the trailing rows % p dropped,
 *         1 <= p <= rows.
 *     out: the last stage's pooled map [rows, E, C] (what Flatten sees) in the columns from out_offset of a [B, out_stride] buffer;
 *     columns beside them are left alone.  stage_outs: NULL, or per stage NULL or a [B, stage_out_strides[s]] buffer that receives
 *     that stage's pooled map [rows_s, E, C_s] from column 0 (FGCNN's recombination Dense reads each).
 *     Exact-fp32 products on v_mfma_f32_16x16x4_f32 (M = 16 (sample, e) columns at one row, K over (d, ci), N a 16-wide slice of
 *     C_out), tanh on the hardware exp and rcp (it saturates to +-1 without NaN), k-max by rank counting, no atomics: the same bits
 *     on every call while the operands are finite.  RESIDENT route: a tile's maps and every stage's kernel stay in LDS; AUTO takes
 *     it while both fit 64 KiB (two workgroups per CU), a forced RESIDENT holds up to 160 KiB.  STREAMED route: the same step code
 *     with the kernels read from global / L2.  WORKSPACE: streamed, with a workgroup's maps in a workspace of
 *     dctr_fieldconv_workspace_bytes() (room for <= 256 workgroups); AUTO takes it when 16 columns' maps exceed the LDS, and the
 *     workspace is then REQUIRED (DCTR_E_NULL without, before anything is launched).  route = RESIDENT for shapes that do not fit
 *     answers DCTR_E_UNSUPPORTED.  No shape is refused for its size below 2^20 per extent.
 *     Argument errors (nothing launched): NULL x / out / arrays / a stage's kernel or bias (DCTR_E_NULL), sizes < 1, n_stages outside
 *     1..DCTR_FIELDCONV_MAX_STAGES, k or p outside 1..rows, strides smaller than offset + block (DCTR_E_DIM), unknown pooling / route
 *     (DCTR_E_ENUM).
 * ------------------------------------------------------------------------------------------------ */
enum { DCTR_FIELDCONV_POOL_KMAX = 0, DCTR_FIELDCONV_POOL_MAX = 1 };
enum { DCTR_FIELDCONV_ROUTE_AUTO = 0, DCTR_FIELDCONV_ROUTE_RESIDENT = 1, DCTR_FIELDCONV_ROUTE_STREAMED = 2, DCTR_FIELDCONV_ROUTE_WORKSPACE = 3 };
#define DCTR_FIELDCONV_MAX_STAGES 8
typedef struct {
    int64_t batch;
    const float* x;                  /* [B, x_stride] fp32; the block is [F, E, in_channels] from x_offset */
    int64_t x_stride;                /* elements between samples */
    int64_t x_offset;
    int32_t fields;                  /* F >= 1 */
    int32_t dim;                     /* E >= 1 */
    int32_t in_channels;             /* C_0 >= 1 */
    int32_t n_stages;                /* 1 .. DCTR_FIELDCONV_MAX_STAGES */
    int32_t route;                   /* DCTR_FIELDCONV_ROUTE_* */
    int32_t reserved;
    const int32_t* widths;           /* HOST [n_stages] */
    const int32_t* channels;         /* HOST [n_stages]: C_out */
    const int32_t* pool_kinds;       /* HOST [n_stages]: DCTR_FIELDCONV_POOL_* */
    const int32_t* pool_args;        /* HOST [n_stages]: k or p */
    const float* const* kernels;     /* HOST array [n_stages] of DEVICE pointers, [w, C_in, C_out] */
    const float* const* biases;      /* HOST array [n_stages] of DEVICE pointers, [C_out] */
    float* out;
    int64_t out_stride;
    int64_t out_offset;
    float* const* stage_outs;        /* NULL, or HOST array [n_stages] of DEVICE pointers (entries may be NULL) */
    const int64_t* stage_out_strides; /* HOST [n_stages], read where stage_outs[s] is set */
    void* workspace;                 /* NULL, or device scratch of dctr_fieldconv_workspace_bytes() bytes, 16-B aligned */
    size_t workspace_bytes;
} dctr_fieldconv_args_t;
/* Bytes dctr_fieldconv_fwd needs (sizes and route are read, device pointers are not): 0 while a workgroup's maps fit the LDS. */
size_t dctr_fieldconv_workspace_bytes(const dctr_fieldconv_args_t* args);
/* The route these arguments take (DCTR_FIELDCONV_ROUTE_RESIDENT, or _STREAMED with or without a workspace), or the DCTR_E_* the checks
 * answer. */
int dctr_fieldconv_route(const dctr_fieldconv_args_t* args);
int dctr_fieldconv_fwd(const dctr_fieldconv_args_t* args, void* stream);
/* KMaxPooling.call — deepctr/layers/sequence.py:853-864 over a contiguous [outer, n, inner] view: y [outer, k, inner] holds the k
 * largest along the middle axis in descending order of value, 1 <= k <= n (DCTR_E_DIM otherwise). */
int dctr_kmax_pool_fwd(const float* x, int64_t outer, int32_t n, int64_t inner, int32_t k, float* y, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a11 AFMLayer.call — deepctr/layers/interaction.py:116-146 (inference: dropout inactive)
 *     x [B,F,E] (sample stride x_stride); W [E,A]; b [A]; h [A]; p [E]  ->  y [B]
 * ------------------------------------------------------------------------------------------------ */
int dctr_afm_fwd(const float* x, int64_t batch, int64_t x_stride, int32_t fields, int32_t dim, const float* att_w,
                 const float* att_b, const float* proj_h, const float* proj_p, int32_t att_factor, float* y,
                 void* stream);

/* ------------------------------------------------------------------------------------------------
 * a12 InnerProductLayer.call — deepctr/layers/interaction.py:655-678
 *     x [B,F,E] (sample stride x_stride) -> y [B, F(F-1)/2] (reduce_sum) or [B, F(F-1)/2, E], sample stride y_stride;
 *     pair order (i<j) row-major.
 * ------------------------------------------------------------------------------------------------ */
int dctr_inner_product_fwd(const float* x, int64_t batch, int64_t x_stride, int32_t fields, int32_t dim,
                           int32_t reduce_sum, float* y, int64_t y_stride, void* stream);

/* ------------------------------------------------------------------------------------------------
 * sibling: CrossNetMix.call — deepctr/layers/interaction.py:511-549 (DCNMix)
 *     x [B, dim] (row stride x_stride) -> y [B, dim] (row stride y_stride)
 *     U, V [layers, experts, dim, low_rank], C [layers, experts, low_rank, low_rank] (U_list / V_list / C_list stacked
 *     over layers, :481-500), gating [experts, dim] (the experts' Dense(1, use_bias=False) kernels, shared by every
 *     layer, :502), bias [layers, dim].  layers == 0 copies x to y.  workspace: DEVICE scratch of
 *     dctr_crossnet_mix_workspace_bytes() bytes (U transposed per call so that the projection back reads it coalesced).
 * ------------------------------------------------------------------------------------------------ */
size_t dctr_crossnet_mix_workspace_bytes(int32_t dim, int32_t layers, int32_t experts, int32_t low_rank);
int dctr_crossnet_mix_fwd(const float* x, int64_t batch, int32_t dim, int64_t x_stride, const float* U, const float* V,
                          const float* C, const float* gating, const float* bias, int32_t layers, int32_t experts,
                          int32_t low_rank, float* y, int64_t y_stride, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * sibling: BiInteractionPooling.call — deepctr/layers/interaction.py:190-203 (NFM)
 *     x [B,F,E] (sample stride x_stride) -> y [B,E] (sample stride y_stride) = 0.5 ((sum_f e)^2 - sum_f e^2)
 * ------------------------------------------------------------------------------------------------ */
int dctr_bi_interaction_fwd(const float* x, int64_t batch, int64_t x_stride, int32_t fields, int32_t dim, float* y,
                            int64_t y_stride, void* stream);

/* ------------------------------------------------------------------------------------------------
 * adjacent  DNN.call (+ Dense(1, use_bias=False) head, add_func, PredictionLayer.call)
 *     deepctr/layers/core.py:189-208, :250-259; layers/utils.py:328-333.
 *     y = x; for each layer: y = act(y W_l + b_l).  Optional head: logit = y . head_w (+ add0 + add1
 *     + global_bias), sigmoid if binary.  W_l: [in_l, out_l] row-major (Keras kernel layout).
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    const float* x;               /* [B, x_stride] */
    int64_t batch;
    int64_t x_stride;
    int32_t in_dim;
    int32_t n_layers;
    const int32_t* units;         /* HOST array [n_layers] */
    const float* const* kernels;  /* HOST array of DEVICE pointers */
    const float* const* biases;   /* HOST array of DEVICE pointers */
    int32_t activation;           /* DCTR_ACT_LINEAR .. DCTR_ACT_GELU (DICE: dice_* arrays below).  ELU .. GELU: every route but the
                                     row-chained and streaming kernels, which decline them (the tile kernels take the launch) */
    int32_t has_head;
    const float* const* dice_alpha;   /* HOST arrays of DEVICE pointers [n_layers] or NULL */
    const float* const* dice_mean;
    const float* const* dice_var;
    float dice_eps;
    int32_t sigmoid_out;          /* PredictionLayer task == "binary" */
    const float* head_w;          /* [units[last]] or NULL */
    const float* add[4];          /* up to four [B] extra logit vectors (linear, FM, CIN ...) or NULL */
    const float* global_bias;     /* [1] device or NULL */
    float* y;                     /* has_head ? [B] : [B, y_stride] */
    int64_t y_stride;
    void* workspace;
    size_t workspace_bytes;
    float* const* save_acts;      /* training: HOST array [n_layers] of DEVICE pointers; layer l's activations
                                     [B, units[l]] (row stride units[l]) are also written there.  NULL = inference. */
    int32_t tile_rows;            /* batch rows per workgroup: 0 = auto, or 16 / 32 / 64.  Larger tiles re-use every
                                     weight fragment for more rows (less L2->CU weight traffic per row, the bound of
                                     this kernel) at the price of fewer workgroups; results are bit-identical.
                                     dctr_embed_mlp_fwd only: 64 = the streaming kernel (64-row tiles, LDS-DMA gather ring),
                                     128 / 256 = the row-chained kernel in one launch shape (waves own batch rows end to
                                     end; needs uniform_dim 16 / 32, a head, units as listed at uniform_dim; 128: units
                                     256-128-64 only).  0 (auto) sends launches of >= 64 rows per CU of such a model to the
                                     row-chained kernel as ONE launch: 256-row passes for the whole multiples of 256 rows x CUs,
                                     64-row units inside the same kernel for what is left; a row's result does not depend on
                                     the shape, the phase or the row's position in the launch. */
    int32_t precision;            /* must be 0: exact fp32 (v_mfma_f32_16x16x4_f32 = an fmaf chain) is the library's only arithmetic.  (ABI <= 11
                                     carried an exploratory bf16x3 mode here; removed — DESIGN.md §9 — anything but 0 is DCTR_E_UNSUPPORTED.) */
    unsigned long long* probe;    /* measurement aid, normally NULL: DEVICE uint64[2]; every workgroup does
                                     atomicMin(probe[0], t_start) / atomicMax(probe[1], t_end) with the constant-rate
                                     wall clock (dctr_wall_clock_khz()), so probe[1] - probe[0] is this launch's duration
                                     even inside a hipGraph, where event pairs cannot be attached.  Caller initialises
                                     to {UINT64_MAX, 0}. */
    const float* const* bn_scale; /* DNN(use_bn=True), inference form of keras BatchNormalization between bias_add and the
                                     activation (layers/core.py:200-201): HOST arrays [n_layers] of DEVICE pointers (entries or
                                     the arrays may be NULL = no BN on that layer): y = act((x W + b) * bn_scale + bn_shift) with
                                     bn_scale = gamma * rsqrt(moving_variance + epsilon), bn_shift = beta - moving_mean * bn_scale */
    const float* const* bn_shift;
    /* ABI 7 — CrossNet, vector parameterization (deepctr/layers/interaction.py:405-424), and the cross branch's share of DCN's
     * Dense(1) over Concatenate([cross_out, deep_out]) (deepctr/models/dcn.py:61-64), folded into the forward: with cross_layers = L
     * in 1 .. 3 the head also adds x_L . cross_head, where x_0 = the row the DNN reads (the gathered row of dctr_embed_mlp_fwd, or x)
     * and x_{l+1} = x_0 (x_l . cross_w[l]) + cross_b[l] + x_l.  Every x_l = a_l x_0 + (b_0 + .. + b_{l-1}), so the kernels take
     * L + 1 dot products of the row while it is on chip and run the scalar recurrence — the same real-number function as
     * dctr_crossnet_head_fwd, rounded differently (fp32 fmaf chains over the same products).  Needs has_head; not with save_acts or
     * precision != 0.  cross_w, cross_b: DEVICE [L, in_dim] row-major; cross_head: DEVICE [in_dim]. */
    const float* cross_w;
    const float* cross_b;
    const float* cross_head;
    int32_t cross_layers;         /* 0 (default): none */
    const float* cross_const;     /* NULL, or DEVICE float[4] written by dctr_crossnet_fold_consts() for THESE cross_w / cross_b /
                                   * cross_head: the L + 1 row-independent constants of the recurrence, which the kernels otherwise
                                   * compute at the start of every launch (one wave, ~7 dependent L2 round trips: a few us of a
                                   * 4096-row launch) */
} dctr_mlp_args_t;
/* Scratch dctr_mlp_fwd needs for these arguments (0 for most): a DNN with a layer wider
 * than any LDS tile holds (> 1,216 units — the reference's DNN takes any hidden_units, layers/core.py:160-175) -> two activation
 * buffers of [min(batch, 65536) rounded up to 64 rows, widest layer] floats: such a DNN runs layer by layer (own f32-MFMA GEMM +
 * one bias / BatchNormalization / activation launch per layer, rows in chunks of what the workspace holds; any workspace of >= 64
 * rows works), the head through the no-hidden-layer form of the same entry point. */
size_t dctr_mlp_workspace_bytes(const dctr_mlp_args_t* args);
/* Would dctr_mlp_fwd (g == NULL) / dctr_embed_mlp_fwd (g != NULL) take these arguments?  Runs every argument check and kernel-shape
 * decision of the launch without launching: 1 = yes, 0 = no (dctr_last_error() carries the reason).  Hosts ask this instead of
 * re-deriving the library's shape limits. */
int dctr_mlp_fwd_supported(const dctr_gather_fm_args_t* g, const dctr_mlp_args_t* m, int32_t add_fm_logit, int32_t add_lin_logit);
/* consts[l] = (cross_b[0] + .. + cross_b[l-1]) . v_l with v_l = cross_w[l] for l < layers and cross_head for l = layers (consts has
 * room for 4 floats; layers in 1 .. 3).  One tiny launch per change of the weights, not per batch. */
int dctr_crossnet_fold_consts(const float* cross_w, const float* cross_b, const float* cross_head, int32_t layers, int32_t dim,
                              float* consts, void* stream);
int dctr_mlp_fwd(const dctr_mlp_args_t* args, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a3-a8 + DNN fused: dctr_embed_gather_fm feeding dctr_mlp_fwd inside ONE launch.  The DNN-input tile is gathered
 * straight into LDS (g->dnn_in is ignored; m->x is ignored; m->in_dim must equal the gathered row width =
 * sum of the fields' dims at their out_offsets + dense_copy_cols), and the gather's FM / linear logits are added to
 * the head when the flags say so (they are also written to g->fm_logit / g->lin_logit when those are non-NULL).
 * Requirements: g->all_dim4, embedding_dim <= 64.  This is DeepFM's whole forward as a single kernel
 * (deepctr/models/deepfm.py:42-65).
 * ------------------------------------------------------------------------------------------------ */
int dctr_embed_mlp_fwd(const dctr_gather_fm_args_t* g, const dctr_mlp_args_t* m, int32_t add_fm_logit,
                       int32_t add_lin_logit, void* stream);

/* How dctr_embed_mlp_fwd would run this call.  Every path is ONE kernel launch; the row-chained kernel runs a call in up to two
 * phases inside that launch (256-row passes for the whole multiples of 256 rows x CUs, 64-row units for what is left).  Writes up
 * to `max` entries (rows, DCTR_FWD_KERNEL_* id, batch rows per workgroup) — one per phase, in order — and returns their number
 * (<= 0: error, see dctr_last_error).  Needs a current HIP device (CU count).
 * dctr_embed_mlp_fwd_last_kernel(): the DCTR_FWD_KERNEL_* id the calling thread's last successful dctr_embed_mlp_fwd call
 * launched (-1 before the first one).  DCTR_FWD_KERNEL_TILE covers both forms of the tile family: 16- / 32-row workgroups whose waves
 * stream their weight slices into registers, and — launches of at most 16 rows per CU (or tile_rows 16) with every layer width a
 * multiple of 16 — 16-row workgroups whose waves pull them by LDS-DMA (csrc/mlp_device.h: mlp_ring_kernel; same bits). */
enum { DCTR_FWD_KERNEL_TILE = 0, DCTR_FWD_KERNEL_STREAM = 1, DCTR_FWD_KERNEL_CHAIN = 2 };
int dctr_embed_mlp_fwd_plan(const dctr_gather_fm_args_t* g, const dctr_mlp_args_t* m, int64_t* rows, int32_t* kernel,
                            int32_t* rows_per_workgroup, int32_t max);
int dctr_embed_mlp_fwd_last_kernel(void);

/* ------------------------------------------------------------------------------------------------
 * a13 AttentionSequencePoolingLayer.call + LocalActivationUnit.call (DIN)
 *     deepctr/layers/sequence.py:261-298, layers/core.py:94-108, activation.py:59-64.
 *     query [B,E]; keys [B,T,E]; key_mask [B,T] bytes; att MLP over [q,k,q-k,q*k] (4E -> h1 -> .. -> 1)
 *     out [B,E] = sum_t score_t * k_t.
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
    const float* query;
    const float* keys;
    const uint8_t* key_mask;
    int64_t batch;
    int32_t maxlen;
    int32_t dim;                  /* E (query / key width) */
    int32_t n_layers;
    int32_t activation;           /* DCTR_ACT_SIGMOID | RELU | DICE ... */
    const int32_t* units;         /* HOST */
    const float* const* kernels;  /* HOST array of DEVICE ptrs; kernels[0]: [4E, units[0]] */
    const float* const* biases;
    const float* const* dice_alpha;
    const float* const* dice_mean;
    const float* const* dice_var;
    float dice_eps;
    int32_t weight_normalization;
    const float* out_kernel;      /* [units[last]] */
    const float* out_bias;        /* [1] */
    float* out;                   /* [B, out_stride] */
    int64_t out_stride;
    float* scores;                /* optional [B,T] (return_score) */
    void* workspace;              /* optional device scratch of dctr_din_attn_workspace_bytes() bytes, 16-B aligned.
                                     With it (and dim % 16 == 0 and <= 64, layer widths <= 96, query / keys 16-B aligned) the
                                     attention MLP runs as one row problem over the B*T positions with the weights
                                     resident in LDS; without it, one workgroup per sample.  Layout (ABI 8): [B*T] raw scores,
                                     then the list of the positions that COUNT (masked positions are skipped by the row-chained
                                     score kernel: their scores never reach the output, sequence.py:280-285), then the
                                     workgroups' LDS image.  A workspace of only B*T floats (ABI <= 7 callers) still works: every
                                     position is scored and each workgroup folds the weights itself. */
    size_t workspace_bytes;
} dctr_din_attn_args_t;
size_t dctr_din_attn_workspace_bytes(const dctr_din_attn_args_t* args);
int dctr_din_attn_pool_fwd(const dctr_din_attn_args_t* args, void* stream);

/* ABI 7 — a13 with the lookups of the behaviour sequences and of the query features folded in (deepctr/models/sequence/din.py:62-76
 * embedding_lookup of query / keys + concat_func, layers/sequence.py:261-298): key row (b, t) = concat_h hist_table[h][hist_ids[h][b, t]],
 * query row b = concat_h query_table[h][query_ids[h][b]], read inside the score and pooling kernels — the [B, T, dim] key tensor and
 * the key mask never exist in HBM.  args->query / keys / key_mask are ignored; args->workspace ([B * T] floats) is required.
 * Position t of sample b counts iff hist_ids[h][b, t] != 0 for every feature with mask_zero[h] (keras Concat.compute_mask: the
 * conjunction of the mask_zero embeddings' masks); no mask_zero feature: every position counts.  An id outside its vocabulary reads
 * row 0 and raises DCTR_STATUS_INDEX_OOR in *status.  Plain ids only (hashed features: hash first, or use the lookups).
 * Covered: 1 or 2 features of equal width (dim / n_feats, a multiple of 16), dim in {16, 32, 64}, two-layer attention MLPs of the
 * row-chained score kernel; else DCTR_E_UNSUPPORTED (use dctr_embed_lookup_multi + dctr_din_attn_pool_fwd). */
typedef struct {
    int32_t n_feats;
    int32_t ids_is_i64;
    const void* hist_ids[2];      /* [B, maxlen] ids, row stride hist_stride (elements) */
    int64_t hist_stride;
    const void* query_ids[2];     /* [B] ids, element stride query_stride */
    int64_t query_stride;
    const float* hist_table[2];   /* [hist_vocab, dim / n_feats] fp32, 16-B aligned */
    const float* query_table[2];  /* [query_vocab, dim / n_feats] (usually the same table: shared embedding_name) */
    int64_t hist_vocab[2];
    int64_t query_vocab[2];
    int32_t mask_zero[2];
    int32_t* status;              /* DEVICE int or NULL */
} dctr_din_gather_t;
int dctr_din_attn_gather_fwd(const dctr_din_attn_args_t* args, const dctr_din_gather_t* gather, void* stream);

/* ================================================================================================
 * SURVEY.md §8(f) rank 1 — backward + optimizer of the hot path ("next" row; forward entry points above are
 * unchanged).  The reference has no code for these (Keras autodiff, tf.keras.optimizers.Adam): each entry is the
 * derivative of the forward expression of the cited lines.  Gradient tables are dense fp32 buffers of the same shape as
 * the parameter, ACCUMULATED into (atomics); dctr_adam_step consumes and clears them.
 * ================================================================================================ */

/* loss of PredictionLayer + compile(loss=...): task 0 = binary_crossentropy on sigmoid outputs (value with Keras'
 * 1e-7 clip), task 1 = mse.  dlogit[b] = d(mean loss)/d(logit_b); optional device floats: loss_sum += sum_b loss_b,
 * dlogit_sum += sum_b dlogit[b] (= gradient of PredictionLayer's global_bias, layers/core.py:250-259). */
int dctr_bce_grad(const float* pred, const float* y, int64_t batch, int32_t task, float* dlogit, float* loss_sum,
                  float* dlogit_sum, void* stream);
/* ABI 9 — the same with tf.keras' per-sample weights (Model.fit(sample_weight=, class_weight=), which the reference's models inherit):
 * loss = sum_b weight[b] * loss_b / batch (Keras' SUM_OVER_BATCH_SIZE reduction divides by the batch size, not by the summed weights),
 * so loss_sum += sum_b weight[b] loss_b and dlogit[b] = weight[b] * d(loss_b)/d(logit_b) / batch.  weight == NULL: dctr_bce_grad. */
int dctr_bce_grad_w(const float* pred, const float* y, const float* weight, int64_t batch, int32_t task, float* dlogit,
                    float* loss_sum, float* dlogit_sum, void* stream);

/* `touched` (ABI 6; optional, tables with dim % 4 == 0): one byte per 16-B group of g_table ([vocab * dim / 4] bytes, zero-initialised
 * by the caller).  The scatter kernels set the bytes of the groups they add to; dctr_opt_multi then treats groups with a clear byte as a
 * ZERO gradient it neither reads nor clears (see dctr_adam_seg_t).  Invariant the caller keeps: g_table is zero wherever its byte is. */
typedef struct {
    float* g_table;       /* [vocab, dim] gradient of the field's table, or NULL (frozen / absent)  */
    float* g_lin_table;   /* [vocab] gradient of its 1-wide linear table, or NULL                   */
    uint8_t* touched;     /* [vocab * dim / 4] bytes beside g_table, or NULL                        */
} dctr_field_grad_t;

/* backward of dctr_embed_gather_fm (inputs.py:101-117, layers/utils.py:336-346, feature_column.py:171-210,
 * layers/interaction.py:588-604):  d e_f = d_dnn_in[b, off_f..] + d_fm[b] * (sum_f' e_f' - e_f);  d lin_f[row] += d_lin[b];
 * d dense_lin_w[k] += d_lin[b] * dense[b,k]. */
typedef struct {
    const dctr_gather_fm_args_t* fwd;   /* the forward call's arguments (descriptors, ids, dense).  fwd->dnn_in, when not NULL, must
                                           still hold what that forward wrote in the fields' columns: the FM term reads e_f from
                                           there (coalesced) instead of the tables (a second random row read); NULL: from the tables */
    const dctr_field_grad_t* grads;     /* DEVICE array [n_fields], parallel to fwd->fields                  */
    const float* d_dnn_in;              /* [B, d_stride] gradient w.r.t. dnn_in, or NULL                      */
    int64_t d_stride;
    const float* d_fm;                  /* [B] gradient w.r.t. fm_logit, or NULL (model without FM)           */
    const float* d_lin;                 /* [B] gradient w.r.t. lin_logit, or NULL                             */
    float* g_dense_lin_w;               /* gradient of Linear.kernel, or NULL                                 */
    const int32_t* dense_lin_rows;      /* DEVICE [n_dense]: row of Linear.kernel fed by dense column k (-1: none);
                                           NULL = identity (fwd->dense_lin_w is the kernel itself)            */
} dctr_gather_fm_bwd_args_t;
int dctr_embed_gather_fm_bwd(const dctr_gather_fm_bwd_args_t* args, void* stream);

/* backward of dctr_embed_pool (inputs.py:120-158, layers/sequence.py:76-106, :155-183): the gradient of a pooled vector
 * (and of the pooled 1-wide linear term) scattered to the rows of the sequence with the forward's factors — weight *
 * mask (sum), / length (mean), or to the first position attaining each dimension's maximum (max). */
typedef struct {
    const dctr_pool_args_t* fwd;   /* the forward call's arguments                                      */
    const float* d_out;            /* [B, d_stride] gradient w.r.t. the pooled vectors, or NULL         */
    int64_t d_stride;
    const float* d_lin_out;        /* [B] gradient w.r.t. lin_out, or NULL                              */
    float* g_table;                /* [vocab, dim] accumulated, or NULL                                 */
    float* g_lin_table;            /* [vocab] accumulated, or NULL                                      */
    uint8_t* touched;              /* touched bytes of g_table (dctr_field_grad_t), or NULL (ABI 6)     */
} dctr_pool_bwd_args_t;
int dctr_embed_pool_bwd(const dctr_pool_bwd_args_t* args, void* stream);

/* backward of dctr_mlp_fwd with has_head (layers/core.py:189-208 + Dense(1, use_bias=False)): needs the activations the
 * forward saved through save_acts.  relu / linear / sigmoid / tanh and the six activations whose derivative can be written in the
 * OUTPUT (elu: h > 0 ? 1 : h + 1; selu: h > 0 ? s : h + s a; softplus: -expm1(-h); softsign: (1 - |h|)^2; exponential: h;
 * hard_sigmoid: 0 < h < 1 ? 0.2 : 0): FIVE launches whatever the depth — head, W_l^T of every layer,
 * the backward chain (every dZ_l and dX in one launch on the forward's whole-MLP kernel), the dW_l (+ d_bias_l) row slices of every
 * layer as one grouped GEMM, the slice sum.  Dice, swish and gelu (act' needs the pre-activation): layer by layer (two GEMMs + the
 * recomputed pre-activations per layer, or saved_z) on dctr_sgemm's kernel. */
typedef struct {
    const float* x;               /* [B, x_stride] the forward's input (dnn_in)                          */
    int64_t batch;
    int64_t x_stride;
    int32_t in_dim;
    int32_t n_layers;             /* >= 1                                                                */
    const int32_t* units;         /* HOST [n_layers]                                                     */
    const float* const* kernels;  /* HOST array of DEVICE pointers, as in the forward                    */
    const float* const* acts;     /* HOST array of DEVICE pointers: saved activations [B, units[l]]      */
    int32_t activation;           /* DCTR_ACT_LINEAR .. DCTR_ACT_GELU                                    */
    int32_t pad_;
    const float* head_w;          /* [units[last]]                                                       */
    const float* dlogit;          /* [B]                                                                 */
    float* const* d_kernels;      /* HOST array of DEVICE pointers [in_l, out_l], accumulated into       */
    float* const* d_biases;       /* HOST array of DEVICE pointers [out_l] (or NULL entries), accumulated */
    float* d_head_w;              /* [units[last]], accumulated                                          */
    float* dx;                    /* [B, dx_stride] gradient w.r.t. x (written), or NULL                 */
    int64_t dx_stride;
    void* workspace;              /* dctr_mlp_bwd_workspace_bytes() bytes, 16-B aligned                  */
    size_t workspace_bytes;
    const float* d_out;           /* headless form (head_w == NULL): [B, d_out_stride] gradient w.r.t. the last
                                     layer's activations (the DNN branch of DCN feeds a wider Dense(1))  */
    int64_t d_out_stride;
    /* DCTR_ACT_DICE (layers/activation.py:59-64 with the moving statistics), DCTR_ACT_SWISH, DCTR_ACT_GELU: not invertible from the
     * output, so the pre-activations are recomputed (one more GEMM per layer) from `biases` and the layer inputs. */
    const float* const* biases;       /* HOST array of DEVICE pointers [out_l] (entries may be NULL), as in the forward */
    const float* const* dice_alpha;   /* HOST arrays of DEVICE pointers [out_l]                           */
    const float* const* dice_mean;
    const float* const* dice_var;
    float* const* d_dice_alpha;       /* accumulated; array or entries may be NULL                        */
    float dice_eps;
    int32_t pad2_;
    const float* const* dice_batch_mean;  /* Dice under training=True: HOST arrays of DEVICE pointers [out_l] with THIS batch's */
    const float* const* dice_batch_var;   /* statistics as dctr_dice_train_fwd returned them; the gradient then flows through
                                             them (BatchNormalization backward).  NULL (arrays or entries): dice_mean / dice_var
                                             are constants (inference statistics)                                            */
    void* dw_stream;              /* ABI 6.  NULL, or a second hipStream_t: the weight-gradient half of the chained form (the grouped
                                     dW / d_bias GEMM and its slice sum) is launched there behind an event on `stream`, so that it
                                     runs beside what the caller launches next on `stream` (the embedding scatter, atomics-bound).
                                     The CALLER joins the two streams (dctr_mlp_bwd_join) before it reads d_kernels / d_biases or
                                     reuses the workspace — and before anything on `stream` OVERWRITES what the side stream still
                                     reads: x, acts[l] (the layers' inputs X_l) and the dZ_l slices inside the workspace. */
    const float* const* saved_z;  /* ABI 6, DCTR_ACT_DICE / SWISH / GELU.  NULL, or HOST array of DEVICE pointers [out_l] (entries may be NULL): layer l's
                                     pre-activations z_l = x_l W_l + b_l, dense [B, units[l]], as a forward launch wrote them (training-mode
                                     Dice runs the layers one by one and has them): the recompute GEMM of that layer is skipped         */
} dctr_mlp_bwd_args_t;
size_t dctr_mlp_bwd_workspace_bytes(const dctr_mlp_bwd_args_t* args);
/* `stream` waits (event record + wait, no host synchronisation) for everything issued to `dw_stream` so far.  No-op for NULL / equal streams. */
int dctr_mlp_bwd_join(void* stream, void* dw_stream);

/* Dice.call under training=True (deepctr/layers/activation.py:51-64: BatchNormalization(center=False, scale=False,
 * epsilon) with the training flag, then alpha (1 - p) z + p z):  z [rows, z_stride] pre-activations (+ bias[n] when bias !=
 * NULL); statistics = those of this batch over all rows (biased variance), written to batch_mean / batch_var [n]; the stored
 * statistics move towards them (moving = moving * momentum + batch * (1 - momentum); either may be NULL); h [rows, h_stride]
 * receives the activations.  The matching backward is dctr_mlp_bwd with dice_batch_mean / dice_batch_var. */
int dctr_dice_train_fwd(const float* z, int64_t z_stride, const float* bias, int64_t rows, int32_t n, const float* alpha,
                        float eps, float momentum, float* moving_mean, float* moving_var, float* batch_mean, float* batch_var,
                        float* h, int64_t h_stride, void* stream);
int dctr_mlp_bwd(const dctr_mlp_bwd_args_t* args, void* stream);

/* One DNN layer under training=True with the regularisers of the reference's DNN.call (deepctr/layers/core.py:196-208):
 *     fc = x W + b  ->  BatchNormalization(training) when use_bn  ->  activation  ->  Dropout(training) when dropout_rate > 0.
 * The dense part (z = x W + b) is a one-layer linear dctr_mlp_fwd; these two entries are what sits behind it and its backward:
 *   fwd:  [use_bn: batch mean / biased variance of z over all rows -> bn_batch_mean / bn_batch_var, stored statistics moved with
 *         bn_momentum (tf.keras: moving = moving * momentum + batch * (1 - momentum))]
 *         y = gamma (z - mean) rsqrt(var + eps) + beta   (y = z without BatchNormalization)
 *         h = keep(b, n) ? act(y) / (1 - rate) : 0        (keras' inverted dropout; keep = counter-based generator over
 *                                                          (dropout_seed, b * n + column): the backward regenerates it)
 *   bwd:  dy = dh * keep / (1 - rate) * act'(y);  d_beta += sum_b dy;  d_gamma += sum_b dy xhat;
 *         dz = gamma rsqrt(var + eps) (dy - mean_b(dy) - xhat mean_b(dy xhat))    (dz = dy without BatchNormalization)
 * The generator is this library's, not TensorFlow's: masks differ from a TF run with the same seed (as any two TF versions do). */
typedef struct {
    const float* z;               /* [rows, z_stride] pre-activations x W + b                              */
    int64_t z_stride;
    int64_t rows;
    int32_t n;                    /* columns (units of the layer)                                          */
    int32_t activation;           /* DCTR_ACT_LINEAR | RELU | SIGMOID | TANH | ELU .. GELU (not DICE); act' from y */
    int32_t use_bn;
    float bn_eps;
    float bn_momentum;
    float dropout_rate;           /* in [0, 1); 0 = no dropout                                             */
    unsigned long long dropout_seed;
    const float* bn_gamma;        /* [n] or NULL (scale=False: 1)                                          */
    const float* bn_beta;         /* [n] or NULL (center=False: 0)                                         */
    float* bn_moving_mean;        /* [n] updated by the forward; NULL = leave                              */
    float* bn_moving_var;
    float* bn_batch_mean;         /* [n] written by the forward, read by the backward (use_bn)             */
    float* bn_batch_var;
    float* h;                     /* forward: [rows, h_stride] out                                         */
    int64_t h_stride;
    const float* dh;              /* backward: [rows, dh_stride] gradient w.r.t. h                         */
    int64_t dh_stride;
    float* dz;                    /* backward: [rows, n] contiguous out (may alias dh when dh_stride == n) */
    float* d_gamma;               /* backward: accumulated [n]; NULL ok                                    */
    float* d_beta;
    float* workspace;             /* backward with use_bn: 2 * n floats                                    */
} dctr_dnn_train_layer_t;
int dctr_dnn_train_layer_fwd(const dctr_dnn_train_layer_t* a, void* stream);
int dctr_dnn_train_layer_bwd(const dctr_dnn_train_layer_t* a, void* stream);

/* DIN's LocalActivationUnit as a training step (layers/core.py:94-108, layers/sequence.py:261-298, att_weight_normalization
 * = False): the attention input a[b*T+t, :] = [q_b, k_bt, q_b - k_bt, q_b * k_bt] ([B*T, 4*dim]) is materialised so that the
 * unit's MLP runs through dctr_mlp_fwd (save_acts) / dctr_mlp_bwd; out[b,:] = sum_t (mask ? score : 0) k[b,t,:].
 *   dctr_din_wsum_bwd:   d_score [B*T], dk [B,T,dim] WRITTEN (= masked score * d_out), d_bias += sum d_score (or NULL)
 *   dctr_din_att_in_bwd: da [B*T, 4*dim] -> dk ADDED to, dq added into dx[b, qcol[e]] (qcol: DEVICE int32 [dim], the columns of
 *                        the query embeddings inside the DNN input)
 *   dctr_embed_lookup_bwd: g_table[row(idx[i]), :] += d_out[i, :dim] with the forward's id resolution (hash, range check);
 *                        touched: the touched bytes of g_table (dctr_field_grad_t), or NULL (ABI 6) */
int dctr_din_att_in_fwd(const float* q, const float* k, int64_t batch, int32_t maxlen, int32_t dim, float* a, void* stream);
int dctr_din_wsum_fwd(const float* score, const uint8_t* mask, const float* k, int64_t batch, int32_t maxlen, int32_t dim,
                      float* out, int64_t out_stride, void* stream);
int dctr_din_wsum_bwd(const float* d_out, int64_t d_stride, const float* score, const uint8_t* mask, const float* k, int64_t batch,
                      int32_t maxlen, int32_t dim, float* d_score, float* dk, float* d_bias, void* stream);
/* att_weight_normalization=True (layers/sequence.py:283-289): p [B, T] = softmax over all T positions of where(mask, score, -2^32 + 1);
 * the weighted sum over the keys then takes p with an all-ones mask (dctr_din_wsum_fwd / _bwd).  Backward: d_score = mask ? p (dp - <p, dp>)
 * : 0 (d_score may alias dp), d_bias (NULL ok) += sum d_score. */
int dctr_din_softmax_fwd(const float* score, const uint8_t* mask, int64_t batch, int32_t maxlen, float* p, void* stream);
int dctr_din_softmax_bwd(const float* p, const uint8_t* mask, const float* dp, int64_t batch, int32_t maxlen, float* d_score, float* d_bias,
                         void* stream);
int dctr_din_att_in_bwd(const float* da, const float* q, const float* k, int64_t batch, int32_t maxlen, int32_t dim, float* dk,
                        float* dx, int64_t dx_stride, const int32_t* qcol, void* stream);
int dctr_embed_lookup_bwd(const dctr_lookup_args_t* fwd, const float* d_out, int64_t d_stride, float* g_table, uint8_t* touched,
                          void* stream);

/* backward of Dense(1, use_bias=False) on a strided [B, n] input: dx[b,:] = dlogit[b] * w (written), d_w += x^T dlogit. */
int dctr_dense1_bwd(const float* x, int64_t x_stride, int64_t batch, int32_t n, const float* w, const float* dlogit, float* dx,
                    int64_t dx_stride, float* d_w, void* stream);

/* backward of dctr_bi_interaction_fwd (interaction.py:190-203): dx[b,f,:] = dy[b,:] * (sum_f' x[b,f',:] - x[b,f,:]),
 * and of dctr_inner_product_fwd with reduce_sum (interaction.py:655-678): dx[b,i,:] = sum_{j != i} dy[b,pair(i,j)] x[b,j,:].
 * x as in the forward; dy [B, dy_stride]; dx [B, dx_stride] first F*E columns written, or added to with accumulate=1. */
int dctr_bi_interaction_bwd(const float* x, int64_t batch, int64_t x_stride, int32_t fields, int32_t dim, const float* dy,
                            int64_t dy_stride, float* dx, int64_t dx_stride, int32_t accumulate, void* stream);
int dctr_inner_product_bwd(const float* x, int64_t batch, int64_t x_stride, int32_t fields, int32_t dim, const float* dy,
                           int64_t dy_stride, float* dx, int64_t dx_stride, int32_t accumulate, void* stream);
/* backward of FM.call (interaction.py:588-604; dctr_fm_fwd / the gather's FM epilogue) for an FM group that is a slice of the DNN input
 * (DeepFM(fm_group=...) beyond the first group): dx[b,f,:] = dlogit[b] * (sum_f' x[b,f',:] - x[b,f,:]), written or added to. */
int dctr_fm_bwd(const float* x, int64_t batch, int64_t x_stride, int32_t fields, int32_t dim, const float* dlogit, float* dx,
                int64_t dx_stride, int32_t accumulate, void* stream);

/* backward of dctr_afm_fwd (AFMLayer.call, interaction.py:116-146); the attention is recomputed, nothing is saved by the
 * forward.  dy [B] = gradient w.r.t. the layer's [B,1] output; dx [B, dx_stride]: first fields*dim columns written (or
 * added to); d_att_w [dim, att_factor], d_att_b [att_factor], d_proj_h [att_factor], d_proj_p [dim] are ACCUMULATED. */
typedef struct {
    const float* x;               /* as in the forward: [B, x_stride], fields*dim used                    */
    int64_t batch;
    int64_t x_stride;
    int32_t fields, dim, att_factor, dx_accumulate;
    const float* att_w;
    const float* att_b;
    const float* proj_h;
    const float* proj_p;
    const float* dy;
    float* dx;
    int64_t dx_stride;
    float* d_att_w;
    float* d_att_b;
    float* d_proj_h;
    float* d_proj_p;
} dctr_afm_bwd_args_t;
int dctr_afm_bwd(const dctr_afm_bwd_args_t* args, void* stream);
/* 1: dctr_afm_bwd takes these sizes; 0: it answers DCTR_E_DIM or, past 160 KiB of LDS for the weights and four samples' tiles
 * ((2 (dim att_factor + 2 att_factor + dim) + 4 (2 fields dim + fields (fields - 1) / 2)) * 4 bytes), DCTR_E_UNSUPPORTED — the forward
 * streams such shapes, the backward does not.  Host arithmetic, the op's own predicate. */
int dctr_afm_bwd_supported(int32_t fields, int32_t dim, int32_t att_factor);

/* backward of dctr_crossnet_fwd (interaction.py:405-424).  vector: one fused kernel (x_l recomputed) while a wave's x_l and its d w / d b
 * accumulators fit the LDS and a row's gradient the registers (dim <= 2048, 48 * layers * dim bytes <= 160 KiB); wider inputs (ABI 13: any
 * dim — Criteo at embedding_dim 64 is 1,677 columns) run the same recurrence layer by layer over the batch through the workspace.
 * matrix: GEMMs on dctr_sgemm's kernel + elementwise kernels through the workspace; u_l / x_l recomputed unless the forward saved
 * them (saved_u / saved_x).  dctr_crossnet_bwd_workspace_bytes() says what a call needs (0 for the on-chip vector form). */
typedef struct {
    const float* x;               /* [B, x_stride] the forward's input x_0                               */
    int64_t x_stride;
    int64_t batch;
    int32_t dim, layers, mode, dx_accumulate;   /* dx_accumulate: 1 = add into dx, 0 = overwrite          */
    const float* kernels;         /* as in the forward                                                   */
    const float* bias;
    const float* dy;              /* [B, dy_stride] gradient w.r.t. the output                           */
    int64_t dy_stride;
    float* d_kernels;             /* accumulated, same shape as kernels                                  */
    float* d_bias;                /* accumulated [layers, dim]                                           */
    float* dx;                    /* [B, dx_stride] gradient w.r.t. x_0                                  */
    int64_t dx_stride;
    void* workspace;              /* dctr_crossnet_bwd_workspace_bytes() bytes (matrix form; wide vector form), 16-B aligned */
    size_t workspace_bytes;
    const float* saved_u;         /* ABI 6, matrix form: NULL (u_l and x_l are recomputed: one GEMM + one elementwise launch per layer),   */
    const float* saved_x;         /* or what the forward wrote through dctr_crossnet_args_t.save_u / save_x (saved_x may be NULL: 1 layer) */
} dctr_crossnet_bwd_args_t;
size_t dctr_crossnet_bwd_workspace_bytes(const dctr_crossnet_bwd_args_t* args);
int dctr_crossnet_bwd(const dctr_crossnet_bwd_args_t* args, void* stream);

/* CrossNetMix backward (DCNMix; forward: dctr_crossnet_mix_fwd, deepctr/layers/interaction.py:511-549).  Nothing is saved by
 * the forward: x_l, the low-rank projections and the gate are recomputed into the workspace.  Weights as in the forward
 * (U, V [layers, experts, dim, low_rank], C [layers, experts, low_rank, low_rank], gating [experts, dim], bias [layers, dim]);
 * dU / dV / dC / dgating / dbias have the same shapes and are ACCUMULATED into; dx [B, dx_stride] = gradient w.r.t. x_0. */
typedef struct {
    const float* x;               /* [B, x_stride] the forward's input x_0                               */
    int64_t x_stride;
    int64_t batch;
    int32_t dim, layers, experts, low_rank;
    const float* U;
    const float* V;
    const float* C;
    const float* gating;
    const float* bias;
    const float* dy;              /* [B, dy_stride] gradient w.r.t. the output                           */
    int64_t dy_stride;
    float* dU;
    float* dV;
    float* dC;
    float* dgating;
    float* dbias;
    float* dx;                    /* [B, dx_stride]                                                      */
    int64_t dx_stride;
    int32_t dx_accumulate;        /* 1 = add into dx, 0 = overwrite                                      */
    int32_t pad_;
    void* workspace;              /* dctr_crossnet_mix_bwd_workspace_bytes() bytes, 16-B aligned         */
    size_t workspace_bytes;
} dctr_crossnet_mix_bwd_args_t;
size_t dctr_crossnet_mix_bwd_workspace_bytes(const dctr_crossnet_mix_bwd_args_t* args);
int dctr_crossnet_mix_bwd(const dctr_crossnet_mix_bwd_args_t* args, void* stream);
/* 1: dctr_crossnet_mix_bwd takes these sizes; 0: it answers DCTR_E_DIM (more than 16 experts: the forward takes any number).  Host
 * arithmetic, the op's own predicate. */
int dctr_crossnet_mix_bwd_supported(int32_t dim, int32_t layers, int32_t experts, int32_t low_rank);

/* backward of dctr_cin_fwd (interaction.py:277-325).  Layers with H % 16 == 0, H <= 128, F0 <= 32, Fk <= 64 run z-free on two
 * MFMA kernels (filter gradient with x0*xk formed in registers; dz = dpre W^T contracted with x0 / xk tile by tile); other
 * shapes materialise z in the workspace and use dctr_sgemm's kernel.  The layer activations come from the forward call
 * (fwd->save_y -> saved_y) or are recomputed by re-running the forward kernel into the workspace. */
typedef struct {
    const dctr_cin_args_t* fwd;   /* the forward call's arguments (out / workspace unused)                */
    const float* d_out;           /* [B, out_dim] gradient w.r.t. the CIN output                          */
    int32_t out_dim;              /* featuremap_num                                                       */
    int32_t dx_accumulate;
    float* const* d_filters;      /* HOST array of DEVICE pointers, accumulated, shapes of fwd->filters   */
    float* const* d_bias;         /* HOST array of DEVICE pointers, accumulated                           */
    float* dx;                    /* [B, dx_stride] gradient w.r.t. x (first F0*D columns), or NULL       */
    int64_t dx_stride;
    void* workspace;              /* dctr_cin_bwd_workspace_bytes() bytes, 16-B aligned                   */
    size_t workspace_bytes;
    const float* const* saved_y;  /* NULL (the layer activations are recomputed), or HOST array of n_layers DEVICE
                                   * pointers to what the forward call wrote through fwd->save_y (ABI 4)   */
} dctr_cin_bwd_args_t;
size_t dctr_cin_bwd_workspace_bytes(const dctr_cin_bwd_args_t* args);
int dctr_cin_bwd(const dctr_cin_bwd_args_t* args, void* stream);

/* Keras Adam step over n contiguous floats (a whole table or weight): g' = g + 2*l2*w;  m = b1 m + (1-b1) g';
 * v = b2 v + (1-b2) g'^2;  w -= alpha * m / (sqrt(v) + eps) with alpha = lr*sqrt(1-b2^t)/(1-b1^t) from the caller.
 * Non-lazy like tf.keras' sparse apply: rows without a gradient still decay.  zero_grad clears g. */
int dctr_adam_step(float* w, float* m, float* v, float* g, int64_t n, float alpha, float beta1, float beta2, float eps,
                   float l2, int32_t zero_grad, void* stream);

/* the same for every parameter of a model in ONE launch: a DEVICE array of segments (16-B aligned buffers);
 * max_n = the largest segment's n (sizes the grid).  touched (ABI 6): NULL, or [n / 4] bytes — byte i clear means g[4i .. 4i+3] is
 * zero: the step does not read it (nor clear it); set bytes are cleared together with their gradient (zero_grad).  The update is the
 * same non-lazy one either way — every element of w / m / v moves. */
typedef struct {
    float* w;
    float* m;
    float* v;
    float* g;
    int64_t n;
    float l2;
    int32_t pad_;
    uint8_t* touched;
} dctr_adam_seg_t;
int dctr_adam_multi(const dctr_adam_seg_t* segs, int32_t n_segs, int64_t max_n, float alpha, float beta1, float beta2,
                    float eps, int32_t zero_grad, void* stream);

/* the other optimizers model.compile() accepts by name in the reference's examples, same segment array (tf.keras
 * formulas): ADAGRAD v += g^2, w -= lr g/(sqrt(v)+eps) (v starts at initial_accumulator_value, caller-filled);
 * RMSPROP (beta2 = rho) v = rho v + (1-rho) g^2, w -= lr g/(sqrt(v)+eps); SGD w -= lr g.  ADAM as dctr_adam_multi. */
enum { DCTR_OPT_ADAM = 0, DCTR_OPT_ADAGRAD = 1, DCTR_OPT_RMSPROP = 2, DCTR_OPT_SGD = 3 };
int dctr_opt_multi(int32_t kind, const dctr_adam_seg_t* segs, int32_t n_segs, int64_t max_n, float lr, float beta1,
                   float beta2, float eps, int32_t zero_grad, void* stream);
/* ABI 13 — the same step; with l2_penalty != NULL (a DEVICE double, accumulated into) the launch also adds
 *     penalty_scale * sum over the segments of l2 * sum(w^2),   taken on the weights BEFORE the update:
 * the regularisation losses tf.keras adds to that batch's reported loss (kernel_regularizer=l2(...) of inputs.py:22, layers/core.py:170,
 * interaction.py:100,258,387; tf.keras.Model.fit's `loss` is the batch-size-weighted mean of data loss + penalties: penalty_scale = the
 * batch's rows).  The weights pass through the step's registers anyway: no further pass over the tables. */
int dctr_opt_multi_l2(int32_t kind, const dctr_adam_seg_t* segs, int32_t n_segs, int64_t max_n, float lr, float beta1,
                      float beta2, float eps, int32_t zero_grad, double* l2_penalty, float penalty_scale, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Optimizer OBJECTS (deepctr_amd/optimizers.py): every tf.keras rule and variant in one multi-segment launch of its own; the entry
 * points above are untouched.  g below is  clip(g_raw + 2*l2*w):  times clip_scale[segment] when given, then clamped to
 * [-clipvalue, clipvalue] when clipvalue > 0.  State slots of a segment, in order (NULL beyond what the rule needs):
 *   SGD       momentum == 0: w -= lr g.              else s0 = a:  a = momentum a - lr g;  w += nesterov ? momentum a - lr g : a
 *   ADAGRAD   s0 = v (caller-filled with initial_accumulator_value):  v += g^2;  w -= lr g / (sqrt(v) + eps)
 *   RMSPROP   s0 = ms, then mg when centered, then mom when momentum > 0 (beta2 = rho):  ms = rho ms + (1-rho) g^2;
 *             mg = rho mg + (1-rho) g;  den = centered ? ms - mg^2 : ms;
 *             momentum == 0: w -= lr g / (sqrt(den) + eps);   else mom = momentum mom + lr g / sqrt(den + eps);  w -= mom
 *   ADAM      s0 = m, s1 = v, s2 = vhat when amsgrad; lr = lr0 sqrt(1-b2^t)/(1-b1^t) from the caller, as dctr_adam_multi:
 *             m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;  vhat = max(vhat, v);  w -= lr m / (sqrt(amsgrad ? vhat : v) + eps)
 *   ADAMAX    s0 = m, s1 = u; lr = lr0 / (1-b1^t) from the caller:  m = b1 m + (1-b1) g;  u = max(b2 u, |g|);  w -= lr m / (u + eps)
 *   ADADELTA  s0 = a, s1 = s (beta2 = rho):  a = rho a + (1-rho) g^2;  d = sqrt(s+eps)/sqrt(a+eps) g;  s = rho s + (1-rho) d^2;  w -= lr d
 *   FTRL      s0 = n (caller-filled), s1 = z;  p = -lr_power;  gs = g + 2 l2_shrinkage w;  n' = n + g^2;
 *             z += gs - (n'^p - n^p)/lr w;  q = n'^p/lr + 2 l2_ftrl (the caller folds beta/(2 lr) into l2_ftrl);
 *             w = |z| > l1 ? (sign(z) l1 - z)/q : 0;  n = n'   (p == 0.5: sqrt, not pow)
 * Non-lazy like the entry points above; `touched` as dctr_adam_seg_t documents it.
 * ------------------------------------------------------------------------------------------------ */
enum { DCTR_OPT_ADAMAX = 4, DCTR_OPT_ADADELTA = 5, DCTR_OPT_FTRL = 6 };
typedef struct {
    float* w;
    float* g;
    float* s0;
    float* s1;
    float* s2;
    int64_t n;
    float l2;
    int32_t pad_;
    uint8_t* touched;
} dctr_opt_seg_t;
typedef struct {
    int32_t kind;                 /* DCTR_OPT_*                                                           */
    float lr;
    float beta1;
    float beta2;                  /* rho of RMSPROP / ADADELTA                                            */
    float eps;
    float momentum;               /* SGD, RMSPROP                                                         */
    float lr_power;               /* FTRL: learning_rate_power (<= 0)                                     */
    float l1;
    float l2_ftrl;
    float l2_shrinkage;
    int32_t nesterov;
    int32_t centered;
    int32_t amsgrad;
    float clipvalue;              /* <= 0: off                                                            */
    const float* clip_scale;      /* NULL, or DEVICE float [n_segs] (dctr_grad_clip_scales)               */
    int32_t zero_grad;
    float penalty_scale;          /* with l2_penalty: exactly as dctr_opt_multi_l2                        */
    double* l2_penalty;           /* NULL, or a DEVICE double accumulated into                            */
} dctr_opt_args_t;
/* segs: DEVICE array, 8-B aligned.  A segment whose w / g / slots are all 16-B aligned takes 16-byte accesses for its n / 4 groups and
 * a scalar tail; any other segment (which must not carry `touched`) runs element by element.  A segment that lacks a slot its rule
 * needs is left untouched.  DCTR_E_ENUM: kind (or lr_power > 0);  DCTR_E_NULL: args / segs;  DCTR_E_ALIGN: segs, clip_scale, l2_penalty. */
int dctr_opt_apply(const dctr_opt_args_t* args, const dctr_opt_seg_t* segs, int32_t n_segs, int64_t max_n, void* stream);

/* Keras' clipnorm / global_clipnorm as a pre-pass: clip_scale[i] = clip / max(norm, clip) with norm = ||g + 2 l2 w|| of segment i
 * (PER_SEGMENT) or of all segments together (GLOBAL).  Sums of squares go per workgroup into the workspace in float64 and a second
 * launch adds them in a fixed order: no float atomics, the same bits on every call.  A segment with l2 == 0 skips the groups whose
 * `touched` byte is clear.  Everything stays on the device.  DCTR_E_NULL also answers a workspace smaller than the query's. */
enum { DCTR_CLIP_PER_SEGMENT = 0, DCTR_CLIP_GLOBAL = 1 };
size_t dctr_grad_clip_scales_workspace_bytes(int32_t n_segs, int64_t max_n);
int dctr_grad_clip_scales(const dctr_opt_seg_t* segs, int32_t n_segs, int64_t max_n, int32_t mode, float clip, void* workspace,
                          size_t workspace_bytes, float* clip_scale, void* stream);

/* ------------------------------------------------------------------------------------------------
 * the plain fp32 contractions of the backward step — dW = X^T dZ, dH = dZ W^T of DNN.call
 * (deepctr/layers/core.py:189-208 under Keras autodiff), the matrix CrossNet and CrossNetMix projections
 * (layers/interaction.py:405-424, :511-549) — on the library's own v_mfma_f32_16x16x4_f32 GEMM (csrc/gemm_kernels.hip; no BLAS
 * library behind this ABI).  Column-major BLAS semantics:  C (m x n, ldc) = op(A) (m x k) * op(B) (k x n) + beta * C, beta in {0, 1},
 * trans_x != 0: op = transpose; `batch` problems at the given element strides (batch 1: strides unused).  Exact fp32 products.
 * ------------------------------------------------------------------------------------------------ */
int dctr_sgemm(int32_t trans_a, int32_t trans_b, int32_t m, int32_t n, int32_t k, const float* A, int32_t lda, int64_t stride_a,
               const float* B, int32_t ldb, int64_t stride_b, float beta, float* C, int32_t ldc, int64_t stride_c, int32_t batch,
               void* stream);

/* What a dctr_sgemm call of these sizes runs on (host arithmetic only, no device call unless n_cus == 0; the launcher plans through
 * this same function): *tile = edge of the square output tile, 64 or 128 — 128 when ceil(m/128) ceil(n/128) batch >= 2 n_cus;
 * *k_slices > 1: the reduction is cut into that many slices of *k_chunk (a multiple of 32; the last one shorter) which ADD their
 * products with float atomics — chosen when the tiles fill at most half the CUs and k >= 1024 (>= 256 k per slice, <= 32 slices);
 * otherwise 1 and *k_chunk = k.  n_cus: the compute-unit count to plan for, 0 = the current device's.  DCTR_E_DIM / DCTR_E_NULL. */
int dctr_sgemm_plan(int32_t m, int32_t n, int32_t k, int32_t batch, int32_t n_cus, int32_t* tile, int32_t* k_slices, int32_t* k_chunk);

/* Slices a reduction of length k is cut into at about rows_per_slice each: want = min(32, ceil(k / rows_per_slice)),
 * chunk = ceil(ceil(k / want) / 32) * 32, slices = ceil(k / chunk).  The k_slices a dctr_gemm_group_t takes.  k <= 0: 1. */
int32_t dctr_gemm_k_slices(int32_t k, int32_t rows_per_slice);

/* Up to 8 independent products in ONE launch (64 x 64 tiles), each C (m x n, ldc) = op(A) op(B) as in dctr_sgemm (the dW products of
 * every layer of a DNN, the gate products of a BiLSTM backward).  A group with m, n or batch 0 is skipped.
 *   ones_last   op(B) holds only n - 1 columns in memory; column n - 1 reads as 1.0 for every k, so that column n - 1 of C is
 *               sum_k op(A)(:, k) (a bias gradient beside its dW).
 *   accumulate  C += the product (beta = 1).
 *   k_slices    > 1: must equal ceil(k / chunk) with chunk = ceil(ceil(k / k_slices) / 32) * 32 (dctr_gemm_k_slices gives such a count).
 *               With slice_stride_c != 0 and no accumulate, slice s STORES the product of its own k range [s chunk, (s + 1) chunk) at
 *               C + s * slice_stride_c — the caller sums them: no atomics, the same bits on every call.  With slice_stride_c == 0 and
 *               accumulate the slices add to the one C with float atomics.  Any other pairing: DCTR_E_UNSUPPORTED.
 * DCTR_E_DIM: n_groups outside 1..8, a negative size, ldc < m, a k_slices the rule does not give;  DCTR_E_NULL: groups, or A / B / C
 * of a group that is not empty.  All of these are answered before any device call. */
typedef struct {
    const float* A;
    const float* B;
    float* C;
    int64_t stride_a;             /* element strides between the `batch` problems of the group             */
    int64_t stride_b;
    int64_t stride_c;
    int64_t slice_stride_c;
    int32_t trans_a;
    int32_t trans_b;
    int32_t m;
    int32_t n;
    int32_t k;
    int32_t lda;
    int32_t ldb;
    int32_t ldc;
    int32_t batch;
    int32_t ones_last;
    int32_t accumulate;
    int32_t k_slices;             /* 0 / 1: one slice                                                       */
} dctr_gemm_group_t;
int dctr_sgemm_grouped(const dctr_gemm_group_t* groups, int32_t n_groups, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DCTR_H_ */
