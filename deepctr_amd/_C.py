"""ctypes binding of ``libdctr_hip.so`` (C ABI declared in ``include/dctr.h``).

The HIP extension IS the product path: there is no CPU or eager-PyTorch fallback.  ``lib()``
raises ``DctrExtensionError`` when the shared library is missing or cannot be loaded, and every
op raises when asked to run without a HIP device.
"""
import ctypes
import os

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "lib", "libdctr_hip.so")

c_i32, c_i64, c_f32 = ctypes.c_int32, ctypes.c_int64, ctypes.c_float
c_vp, c_sz = ctypes.c_void_p, ctypes.c_size_t

ABI_VERSION = 13

E_NULL = -1                      # DCTR_E_NULL: a required pointer (or required workspace) is missing
E_UNSUPPORTED = -5               # DCTR_E_UNSUPPORTED: valid request this build does not implement
POOL_SUM, POOL_MEAN, POOL_MAX = 0, 1, 2
CROSS_VECTOR, CROSS_MATRIX = 0, 1
OPT_CODES = {"adam": 0, "adagrad": 1, "rmsprop": 2, "sgd": 3}
ACT_LINEAR, ACT_RELU, ACT_SIGMOID, ACT_TANH, ACT_DICE = 0, 1, 2, 3, 4
ACT_ELU, ACT_SELU, ACT_SOFTPLUS, ACT_SOFTSIGN, ACT_EXPONENTIAL, ACT_HARD_SIGMOID, ACT_SWISH, ACT_GELU = 5, 6, 7, 8, 9, 10, 11, 12
STATUS_INDEX_OOR = 1
STATUS_TIMEOUT = 2

ACT_CODES = {None: ACT_LINEAR, "linear": ACT_LINEAR, "relu": ACT_RELU, "sigmoid": ACT_SIGMOID, "tanh": ACT_TANH,
             "dice": ACT_DICE, "Dice": ACT_DICE}
# The tf.keras 2.x activation names the DNN entry points take beside ACT_CODES (dctr_mlp_fwd / dctr_embed_mlp_fwd, dctr_mlp_bwd,
# dctr_dnn_train_layer_*).  Every other op keeps ACT_CODES: to it these names are unknown.
KERAS_ACT_CODES = {"elu": ACT_ELU, "selu": ACT_SELU, "softplus": ACT_SOFTPLUS, "softsign": ACT_SOFTSIGN, "exponential": ACT_EXPONENTIAL,
                   "hard_sigmoid": ACT_HARD_SIGMOID, "swish": ACT_SWISH, "silu": ACT_SWISH, "gelu": ACT_GELU}
DNN_ACT_CODES = dict(ACT_CODES, **KERAS_ACT_CODES)
ACT_FROM_Z = (ACT_DICE, ACT_SWISH, ACT_GELU)      # act' needs the pre-activation: dctr_mlp_bwd recomputes it or takes saved_z
POOL_CODES = {"sum": POOL_SUM, "mean": POOL_MEAN, "max": POOL_MAX}


class DctrExtensionError(RuntimeError):
    pass


class DctrError(RuntimeError):
    """A dctr_* entry point returned non-zero (``rc``: its return code, e.g. E_UNSUPPORTED)."""
    rc = None


# ---------------------------------------------------------------------------------------------
# struct mirrors (field order and types must match include/dctr.h)
# ---------------------------------------------------------------------------------------------
class FieldDesc(ctypes.Structure):
    _fields_ = [("table", c_vp), ("lin_table", c_vp), ("vocab", c_i64), ("dim", c_i32), ("out_offset", c_i32),
                ("in_fm", c_i32), ("hash_mode", c_i32), ("identity", c_i32), ("row_pitch", c_i32)]


class GatherFmArgs(ctypes.Structure):
    _fields_ = [("fields", c_vp), ("ids", c_vp), ("ids_stride_f", c_i64), ("ids_stride_b", c_i64),
                ("ids_is_i64", c_i32), ("n_fields", c_i32), ("max_dim", c_i32), ("all_dim4", c_i32),
                ("any_hash", c_i32), ("n_dense", c_i32), ("dense", c_vp), ("dense_stride", c_i64),
                ("dense_lin_w", c_vp), ("dense_out_offset", c_i32), ("dense_copy_cols", c_i32), ("batch", c_i64),
                ("dnn_in", c_vp), ("out_stride", c_i64), ("fm_logit", c_vp), ("lin_logit", c_vp), ("status", c_vp),
                ("split_col", c_i32), ("split_field", c_i32), ("uniform_dim", c_i32), ("any_identity", c_i32),
                ("any_pitch", c_i32), ("n_pools", c_i32), ("pools", c_vp), ("pool_row0", c_i64), ("pool_pieces", c_i32), ("pool_flags", c_i32)]


class PoolSeq(ctypes.Structure):       # dctr_pool_seq_t: a sequence feature pooled inside dctr_embed_mlp_fwd (DEVICE array)
    _fields_ = [("idx", c_vp), ("length", c_vp), ("idx_stride", c_i64), ("maxlen", c_i32), ("combiner", c_i32)]


class PoolArgs(ctypes.Structure):
    _fields_ = [("idx", c_vp), ("table", c_vp), ("lin_table", c_vp), ("length", c_vp), ("weight", c_vp),
                ("vocab", c_i64), ("idx_stride", c_i64), ("batch", c_i64), ("idx_is_i64", c_i32), ("maxlen", c_i32),
                ("dim", c_i32), ("combiner", c_i32), ("weight_norm", c_i32), ("hash_mode", c_i32), ("out", c_vp),
                ("out_stride", c_i64), ("lin_out", c_vp), ("status", c_vp)]


class LookupArgs(ctypes.Structure):
    _fields_ = [("idx", c_vp), ("table", c_vp), ("vocab", c_i64), ("n", c_i64), ("idx_is_i64", c_i32), ("dim", c_i32),
                ("hash_mode", c_i32), ("pad_", c_i32), ("out", c_vp), ("out_stride", c_i64), ("mask", c_vp),
                ("status", c_vp)]


class CinArgs(ctypes.Structure):
    _fields_ = [("x", c_vp), ("batch", c_i64), ("x_stride", c_i64), ("fields", c_i32), ("dim", c_i32),
                ("n_layers", c_i32), ("split_half", c_i32), ("activation", c_i32), ("workspace_ready", c_i32), ("layer_size", c_vp),
                ("filters", c_vp), ("bias", c_vp), ("out", c_vp), ("workspace", c_vp), ("workspace_bytes", c_sz),
                ("save_y", c_vp)]


class MlpArgs(ctypes.Structure):
    _fields_ = [("x", c_vp), ("batch", c_i64), ("x_stride", c_i64), ("in_dim", c_i32), ("n_layers", c_i32),
                ("units", c_vp), ("kernels", c_vp), ("biases", c_vp), ("activation", c_i32), ("has_head", c_i32),
                ("dice_alpha", c_vp), ("dice_mean", c_vp), ("dice_var", c_vp), ("dice_eps", c_f32),
                ("sigmoid_out", c_i32), ("head_w", c_vp), ("add", c_vp * 4), ("global_bias", c_vp),
                ("y", c_vp), ("y_stride", c_i64), ("workspace", c_vp), ("workspace_bytes", c_sz),
                ("save_acts", c_vp), ("tile_rows", c_i32), ("precision", c_i32), ("probe", c_vp), ("bn_scale", c_vp), ("bn_shift", c_vp),
                ("cross_w", c_vp), ("cross_b", c_vp), ("cross_head", c_vp), ("cross_layers", c_i32), ("cross_const", c_vp)]


class FieldGrad(ctypes.Structure):
    _fields_ = [("g_table", c_vp), ("g_lin_table", c_vp), ("touched", c_vp)]


class GatherFmBwdArgs(ctypes.Structure):
    _fields_ = [("fwd", ctypes.POINTER(GatherFmArgs)), ("grads", c_vp), ("d_dnn_in", c_vp), ("d_stride", c_i64),
                ("d_fm", c_vp), ("d_lin", c_vp), ("g_dense_lin_w", c_vp), ("dense_lin_rows", c_vp)]


class PoolBwdArgs(ctypes.Structure):
    _fields_ = [("fwd", ctypes.POINTER(PoolArgs)), ("d_out", c_vp), ("d_stride", c_i64), ("d_lin_out", c_vp),
                ("g_table", c_vp), ("g_lin_table", c_vp), ("touched", c_vp)]


class DnnTrainLayer(ctypes.Structure):
    _fields_ = [("z", c_vp), ("z_stride", c_i64), ("rows", c_i64), ("n", c_i32), ("activation", c_i32), ("use_bn", c_i32),
                ("bn_eps", c_f32), ("bn_momentum", c_f32), ("dropout_rate", c_f32), ("dropout_seed", ctypes.c_uint64),
                ("bn_gamma", c_vp), ("bn_beta", c_vp), ("bn_moving_mean", c_vp), ("bn_moving_var", c_vp), ("bn_batch_mean", c_vp),
                ("bn_batch_var", c_vp), ("h", c_vp), ("h_stride", c_i64), ("dh", c_vp), ("dh_stride", c_i64), ("dz", c_vp),
                ("d_gamma", c_vp), ("d_beta", c_vp), ("workspace", c_vp)]


class MlpBwdArgs(ctypes.Structure):
    _fields_ = [("x", c_vp), ("batch", c_i64), ("x_stride", c_i64), ("in_dim", c_i32), ("n_layers", c_i32),
                ("units", c_vp), ("kernels", c_vp), ("acts", c_vp), ("activation", c_i32), ("pad_", c_i32),
                ("head_w", c_vp), ("dlogit", c_vp), ("d_kernels", c_vp), ("d_biases", c_vp), ("d_head_w", c_vp),
                ("dx", c_vp), ("dx_stride", c_i64), ("workspace", c_vp), ("workspace_bytes", c_sz),
                ("d_out", c_vp), ("d_out_stride", c_i64), ("biases", c_vp), ("dice_alpha", c_vp), ("dice_mean", c_vp),
                ("dice_var", c_vp), ("d_dice_alpha", c_vp), ("dice_eps", c_f32), ("pad2_", c_i32),
                ("dice_batch_mean", c_vp), ("dice_batch_var", c_vp), ("dw_stream", c_vp), ("saved_z", c_vp)]


class CrossMixBwdArgs(ctypes.Structure):
    _fields_ = [("x", c_vp), ("x_stride", c_i64), ("batch", c_i64), ("dim", c_i32), ("layers", c_i32), ("experts", c_i32),
                ("low_rank", c_i32), ("U", c_vp), ("V", c_vp), ("C", c_vp), ("gating", c_vp), ("bias", c_vp), ("dy", c_vp),
                ("dy_stride", c_i64), ("dU", c_vp), ("dV", c_vp), ("dC", c_vp), ("dgating", c_vp), ("dbias", c_vp), ("dx", c_vp),
                ("dx_stride", c_i64), ("dx_accumulate", c_i32), ("pad_", c_i32), ("workspace", c_vp), ("workspace_bytes", c_sz)]


class gemm(object):
    """dctr_gemm_group_t (dctr_sgemm_grouped), one level down for the same reason as interacting.Args (tests/test_gemm_cpu.py checks
    its layout)."""
    MAX_GROUPS = 8

    class Group(ctypes.Structure):
        _fields_ = [("A", c_vp), ("B", c_vp), ("C", c_vp), ("stride_a", c_i64), ("stride_b", c_i64), ("stride_c", c_i64),
                    ("slice_stride_c", c_i64), ("trans_a", c_i32), ("trans_b", c_i32), ("m", c_i32), ("n", c_i32), ("k", c_i32),
                    ("lda", c_i32), ("ldb", c_i32), ("ldc", c_i32), ("batch", c_i32), ("ones_last", c_i32), ("accumulate", c_i32),
                    ("k_slices", c_i32)]


class interacting(object):
    """dctr_interacting_args_t.  Its mirror sits one level down (interacting.Args): tests/test_cabi.py pairs the module-level mirrors
    with header structs by a fixed list, and tests/test_autoint_cpu.py checks this one against the C compiler's layout the same way."""

    class Args(ctypes.Structure):
        _fields_ = [("x", c_vp), ("batch", c_i64), ("x_stride", c_i64), ("fields", c_i32), ("dim", c_i32), ("n_layers", c_i32),
                    ("att_embedding_size", c_i32), ("head_num", c_i32), ("use_res", c_i32), ("scaling", c_i32), ("layers", c_vp),
                    ("out", c_vp), ("out_stride", c_i64), ("head_w", c_vp), ("logit", c_vp), ("workspace", c_vp), ("workspace_bytes", c_sz)]


# dctr_interacting_bwd_args_t (tests/test_interacting_bwd_oracle_cpu.py checks the layout)
interacting.BwdArgs = type("BwdArgs", (ctypes.Structure,), {"_fields_": [
    ("fwd", interacting.Args), ("dy", c_vp), ("dy_stride", c_i64), ("dx", c_vp), ("dx_stride", c_i64), ("d_layers", c_vp),
    ("accumulate", c_i32), ("max_blocks", c_i32)]})


class bilinear(object):
    """dctr_bilinear_args_t, one level down for the same reason as interacting.Args (tests/test_fibinet_cpu.py checks its layout)."""
    ALL, EACH, INTERACTION = 0, 1, 2
    TYPES = {"all": ALL, "each": EACH, "interaction": INTERACTION}
    MODE_MODEL, MODE_SENET, MODE_LAYER = 0, 1, 2

    class Args(ctypes.Structure):
        _fields_ = [("x", c_vp), ("batch", c_i64), ("x_stride", c_i64), ("fields", c_i32), ("dim", c_i32), ("bilinear_type", c_i32),
                    ("mode", c_i32), ("reduction_size", c_i32), ("dense_cols", c_i32), ("senet_w1", c_vp), ("senet_w2", c_vp),
                    ("senet_bilinear_w", c_vp), ("bilinear_w", c_vp), ("out", c_vp), ("out_stride", c_i64), ("workspace", c_vp),
                    ("workspace_bytes", c_sz)]


# dctr_bilinear_bwd_args_t (tests/test_bilinear_bwd_oracle_cpu.py checks the layout)
bilinear.BwdArgs = type("BwdArgs", (ctypes.Structure,), {"_fields_": [
    ("fwd", bilinear.Args), ("d_out", c_vp), ("d_out_stride", c_i64), ("d_out_offset", c_i64), ("dx", c_vp), ("dx_stride", c_i64),
    ("dx_offset", c_i64), ("accumulate", c_i32), ("max_blocks", c_i32), ("d_senet_w1", c_vp), ("d_senet_w2", c_vp),
    ("d_senet_bilinear_w", c_vp), ("d_bilinear_w", c_vp), ("workspace", c_vp), ("workspace_bytes", c_sz)]})


class fieldpair(object):
    """dctr_fieldpair_args_t, one level down for the same reason as interacting.Args (tests/test_fefm_cpu.py checks its layout)."""
    FEFM, FWFM = 0, 1

    class Args(ctypes.Structure):
        _fields_ = [("x", c_vp), ("batch", c_i64), ("x_stride", c_i64), ("x_offset", c_i64), ("fields", c_i32), ("dim", c_i32),
                    ("kind", c_i32), ("reserved", c_i32), ("weights", c_vp), ("pairs_out", c_vp), ("pairs_stride", c_i64),
                    ("pairs_offset", c_i64), ("add", c_vp), ("logit_out", c_vp), ("workspace", c_vp), ("workspace_bytes", c_sz)]


# dctr_fieldpair_bwd_args_t (tests/test_fieldpair_bwd_oracle_cpu.py checks the layout)
fieldpair.BwdArgs = type("BwdArgs", (ctypes.Structure,), {"_fields_": [
    ("fwd", fieldpair.Args), ("d_pairs", c_vp), ("d_pairs_stride", c_i64), ("d_pairs_offset", c_i64), ("d_logit", c_vp), ("dx", c_vp),
    ("dx_stride", c_i64), ("dx_offset", c_i64), ("accumulate", c_i32), ("reserved", c_i32), ("d_weights", c_vp), ("max_blocks", c_i32),
    ("reserved2", c_i32)]})


class ffm(object):
    """dctr_ffm_field_t / dctr_ffm_args_t, one level down for the same reason as interacting.Args (tests/test_onn_cpu.py checks the layout)."""
    ROUTE_AUTO, ROUTE_DIRECT, ROUTE_LDS = 0, 1, 2

    class Field(ctypes.Structure):
        _fields_ = [("rows", c_vp), ("ids", c_vp), ("vocab", c_i64), ("row_pitch", c_i64), ("ids_stride", c_i64), ("ids_is_i64", c_i32),
                    ("identity", c_i32)]

    class Args(ctypes.Structure):
        _fields_ = [("fields", c_vp), ("batch", c_i64), ("n_fields", c_i32), ("dim", c_i32), ("reduce_sum", c_i32), ("n_dense", c_i32),
                    ("scale", c_vp), ("shift", c_vp), ("dense", c_vp), ("dense_stride", c_i64), ("out", c_vp), ("out_stride", c_i64),
                    ("out_offset", c_i64), ("status", c_vp), ("route", c_i32), ("reserved", c_i32), ("workspace", c_vp),
                    ("workspace_bytes", c_sz)]

    class Grad(ctypes.Structure):
        _fields_ = [("grad", c_vp), ("row_stride", c_i64)]


# dctr_ffm_bwd_args_t (tests/test_ffm_bwd_oracle_cpu.py checks the layout)
ffm.BwdArgs = type("BwdArgs", (ctypes.Structure,), {"_fields_": [
    ("fwd", ffm.Args), ("d_out", c_vp), ("d_out_stride", c_i64), ("d_out_offset", c_i64), ("grads", c_vp), ("max_blocks", c_i32),
    ("reserved", c_i32), ("workspace", c_vp), ("workspace_bytes", c_sz)]})


class mlr(object):
    """dctr_mlr_field_t / dctr_mlr_args_t / dctr_mlr_grad_t / dctr_mlr_bwd_args_t, one level down for the same reason as
    interacting.Args (tests/test_mlr_cpu.py checks the layout)."""
    LEARNER_SIGMOID, LEARNER_LINEAR = 0, 1
    MAX_COLUMNS = 64

    class Field(ctypes.Structure):
        _fields_ = [("rows", c_vp), ("ids", c_vp), ("vocab", c_i64), ("row_pitch", c_i64), ("ids_stride", c_i64), ("ids_is_i64", c_i32),
                    ("identity", c_i32), ("col0", c_i32), ("width", c_i32)]

    class Args(ctypes.Structure):
        _fields_ = [("fields", c_vp), ("batch", c_i64), ("n_fields", c_i32), ("region_num", c_i32), ("has_bias", c_i32),
                    ("learner_act", c_i32), ("n_dense", c_i32), ("reserved", c_i32), ("dense", c_vp), ("dense_stride", c_i64),
                    ("dense_w", c_vp), ("out", c_vp), ("out_stride", c_i64), ("z", c_vp), ("z_stride", c_i64), ("z_offset", c_i64),
                    ("status", c_vp)]

    class Grad(ctypes.Structure):
        _fields_ = [("grad", c_vp), ("row_stride", c_i64)]


mlr.BwdArgs = type("BwdArgs", (ctypes.Structure,), {"_fields_": [
    ("fwd", mlr.Args), ("d_out", c_vp), ("d_out_stride", c_i64), ("dz", c_vp), ("dz_stride", c_i64), ("grads", c_vp)]})


class ifm(object):
    """dctr_ifm_src_t / dctr_ifm_lin_t / dctr_ifm_args_t, one level down for the same reason as interacting.Args (tests/test_ifm_cpu.py
    checks the layout)."""
    ROUTE_AUTO, ROUTE_WORKSPACE, ROUTE_LDS = 0, 1, 2

    class Src(ctypes.Structure):
        _fields_ = [("act", c_vp), ("kernel", c_vp), ("act_stride", c_i64), ("K", c_i32), ("reserved", c_i32)]

    class Lin(ctypes.Structure):
        _fields_ = [("table", c_vp), ("ids", c_vp), ("vec", c_vp), ("vocab", c_i64), ("ids_stride", c_i64), ("vec_stride", c_i64),
                    ("ids_is_i64", c_i32), ("reserved", c_i32)]


ifm.Args = type("Args", (ctypes.Structure,), {"_fields_": [
    ("batch", c_i64), ("n_fields", c_i32), ("dim", c_i32), ("x", c_vp), ("x_stride", c_i64), ("n_src", c_i32), ("softmax", c_i32),
    ("src", ifm.Src * 2), ("mprime", c_vp), ("mprime_stride", c_i64), ("lin", c_vp), ("n_lin", c_i32), ("n_add", c_i32),
    ("add", c_vp * 4), ("global_bias", c_vp), ("sigmoid_out", c_i32), ("route", c_i32), ("out", c_vp), ("factor_out", c_vp),
    ("factor_stride", c_i64), ("status", c_vp), ("workspace", c_vp), ("workspace_bytes", c_sz)]})


# dctr_ifm_bwd_args_t (tests/test_ifm_bwd_oracle_cpu.py checks the layout)
ifm.BwdArgs = type("BwdArgs", (ctypes.Structure,), {"_fields_": [
    ("batch", c_i64), ("n_fields", c_i32), ("dim", c_i32), ("x", c_vp), ("x_stride", c_i64), ("factor", c_vp), ("factor_stride", c_i64),
    ("terms", c_vp), ("terms_stride", c_i64), ("d_out", c_vp), ("n_src", c_i32), ("softmax", c_i32), ("src", ifm.Src * 2),
    ("dx", c_vp), ("dx_stride", c_i64), ("dterms", c_vp), ("dterms_stride", c_i64), ("dmprime", c_vp), ("dmprime_stride", c_i64),
    ("dact", c_vp * 2), ("dact_stride", c_i64 * 2), ("dkernel", c_vp * 2), ("dkernel_stride", c_i64 * 2), ("slices", c_i32),
    ("reserved", c_i32), ("workspace", c_vp), ("workspace_bytes", c_sz)]})


class fieldwise(object):
    """dctr_fieldwise_group_t / dctr_fieldwise_args_t / dctr_fieldwise_bwd_args_t, one level down for the same reason as
    interacting.Args (tests/test_flen_cpu.py checks the layout)."""
    ROUTE_AUTO, ROUTE_ON_CHIP, ROUTE_REREAD = 0, 1, 2

    class Group(ctypes.Structure):
        _fields_ = [("first", c_i64), ("n_fields", c_i32), ("reserved", c_i32)]

    class Args(ctypes.Structure):
        _fields_ = [("batch", c_i64), ("x", c_vp), ("x_stride", c_i64), ("x_offset", c_i64), ("groups", c_vp), ("groups_host", c_vp),
                    ("n_groups", c_i32), ("dim", c_i32), ("kernel_mf", c_vp), ("kernel_fm", c_vp), ("bias_mf", c_vp), ("bias_fm", c_vp),
                    ("y", c_vp), ("y_stride", c_i64), ("y_offset", c_i64), ("head_w", c_vp), ("add", c_vp), ("logit", c_vp),
                    ("route", c_i32), ("max_blocks", c_i32)]


fieldwise.BwdArgs = type("BwdArgs", (ctypes.Structure,), {"_fields_": [
    ("fwd", fieldwise.Args), ("dy", c_vp), ("dy_stride", c_i64), ("dlogit", c_vp), ("dx", c_vp), ("dx_stride", c_i64),
    ("dx_offset", c_i64), ("accumulate", c_i32), ("reserved", c_i32), ("d_kernel_mf", c_vp), ("d_kernel_fm", c_vp),
    ("d_bias_mf", c_vp), ("d_bias_fm", c_vp), ("d_head_w", c_vp)]})


class edcn(object):
    """dctr_edcn_args_t, one level down for the same reason as interacting.Args (tests/test_edcn_cpu.py checks the layout)."""
    BRIDGE_ADD, BRIDGE_HADAMARD, BRIDGE_CONCAT, BRIDGE_ATTENTION = 0, 1, 2, 3
    BRIDGES = {"pointwise_addition": BRIDGE_ADD, "hadamard_product": BRIDGE_HADAMARD, "concatenation": BRIDGE_CONCAT,
               "attention_pooling": BRIDGE_ATTENTION}
    ROUTE_AUTO, ROUTE_FUSED, ROUTE_LAYERED = 0, 1, 2

    class Args(ctypes.Structure):
        _fields_ = [("batch", c_i64), ("x", c_vp), ("x_stride", c_i64), ("x_offset", c_i64), ("fields", c_i32), ("dim", c_i32),
                    ("cross_num", c_i32), ("mode", c_i32), ("bridge", c_i32), ("activation", c_i32), ("bridge_activation", c_i32),
                    ("inv_tau", c_f32), ("gates", c_vp), ("cross_w", c_vp), ("cross_b", c_vp), ("dnn_w", c_vp), ("dnn_b", c_vp),
                    ("bn_scale", c_vp), ("bn_shift", c_vp), ("bridge_w", c_vp), ("bridge_b", c_vp), ("head_w", c_vp), ("add", c_vp * 4),
                    ("global_bias", c_vp), ("sigmoid_out", c_i32), ("route", c_i32), ("logit", c_vp), ("out", c_vp), ("out_stride", c_i64),
                    ("out_offset", c_i64), ("workspace", c_vp), ("workspace_bytes", c_sz)]


# dctr_edcn_train_args_t (tests/test_edcn_bwd_oracle_cpu.py checks the layout)
edcn.BWD_MAX_ROUNDS = 32
edcn.TrainArgs = type("TrainArgs", (ctypes.Structure,), {"_fields_": [
    ("fwd", edcn.Args), ("tape", c_vp), ("d_logit", c_vp), ("d_out", c_vp), ("d_out_stride", c_i64), ("dx", c_vp), ("dx_stride", c_i64),
    ("dx_offset", c_i64), ("accumulate", c_i32), ("slices", c_i32), ("d_gates", c_vp), ("d_cross_w", c_vp), ("d_cross_b", c_vp),
    ("d_dnn_w", c_vp), ("d_dnn_b", c_vp), ("d_bridge_w", c_vp), ("d_bridge_b", c_vp), ("d_head_w", c_vp), ("workspace", c_vp),
    ("workspace_bytes", c_sz)]})


class transformer(object):
    """dctr_transformer_args_t, one level down for the same reason as interacting.Args (tests/test_bst_cpu.py checks the layout)."""
    OUT_NONE, OUT_MEAN, OUT_SUM = 0, 1, 2
    OUTPUTS = {None: OUT_NONE, "mean": OUT_MEAN, "sum": OUT_SUM}
    ROUTE_AUTO, ROUTE_FUSED, ROUTE_GENERAL = 0, 1, 2
    LAYER_PTRS = 9      # query, key, value, fw1, fw2, ln_gamma, ln_beta, pe_q, pe_k

    class Args(ctypes.Structure):
        _fields_ = [("batch", c_i64), ("queries", c_vp), ("q_stride", c_i64), ("q_row_stride", c_i64), ("keys", c_vp), ("k_stride", c_i64),
                    ("k_row_stride", c_i64), ("seq_len", c_i32), ("dim", c_i32), ("att_embedding_size", c_i32), ("head_num", c_i32),
                    ("n_layers", c_i32), ("use_positional_encoding", c_i32), ("use_res", c_i32), ("use_feed_forward", c_i32),
                    ("use_layer_norm", c_i32), ("blinding", c_i32), ("output_type", c_i32), ("route", c_i32), ("ln_eps", c_f32),
                    ("reserved", c_i32), ("layers", c_vp), ("query_lengths", c_vp), ("key_lengths", c_vp), ("query_mask", c_vp),
                    ("key_mask", c_vp), ("out", c_vp), ("out_stride", c_i64), ("out_row_stride", c_i64), ("key_mask_out", c_vp),
                    ("workspace", c_vp), ("workspace_bytes", c_sz)]


# dctr_transformer_train_args_t (tests/test_transformer_bwd_oracle_cpu.py checks the layout)
transformer.BWD_MAX_LAYERS = 8
transformer.TrainArgs = type("TrainArgs", (ctypes.Structure,), {"_fields_": [
    ("fwd", transformer.Args), ("tape", c_vp), ("tape_bytes", c_sz), ("d_out", c_vp), ("d_out_stride", c_i64), ("d_out_row_stride", c_i64),
    ("dx", c_vp), ("dx_stride", c_i64), ("dx_row_stride", c_i64), ("d_layers", c_vp), ("accumulate", c_i32), ("max_blocks", c_i32),
    ("workspace", c_vp), ("workspace_bytes", c_sz)]})


class gru(object):
    """dctr_gru_args_t, one level down for the same reason as interacting.Args (tests/test_dien_cpu.py checks the layout)."""
    CELL_GRU, CELL_AGRU, CELL_AUGRU = 0, 1, 2
    CELLS = {"GRU": CELL_GRU, "AGRU": CELL_AGRU, "AUGRU": CELL_AUGRU}
    ROUTE_AUTO, ROUTE_RESIDENT, ROUTE_STREAMED = 0, 1, 2
    ROUTES = {None: ROUTE_AUTO, "resident": ROUTE_RESIDENT, "streamed": ROUTE_STREAMED}
    LAYER_PTRS = 4      # gate kernel, gate bias, candidate kernel, candidate bias

    class Args(ctypes.Structure):
        _fields_ = [("batch", c_i64), ("x", c_vp), ("x_stride", c_i64), ("x_row_stride", c_i64), ("lengths", c_vp), ("att_scores", c_vp),
                    ("att_stride", c_i64), ("seq_len", c_i32), ("dim", c_i32), ("n_layers", c_i32), ("cell", c_i32), ("scale_input", c_i32),
                    ("return_sequence", c_i32), ("route", c_i32), ("reserved", c_i32), ("layers", c_vp), ("out", c_vp),
                    ("out_stride", c_i64), ("out_row_stride", c_i64), ("workspace", c_vp), ("workspace_bytes", c_sz)]


# dctr_gru_bwd_args_t (tests/test_gru_bwd_oracle_cpu.py checks the layout)
gru.BwdArgs = type("BwdArgs", (ctypes.Structure,), {"_fields_": [
    ("fwd", gru.Args), ("h_seq", c_vp), ("h_stride", c_i64), ("h_row_stride", c_i64), ("d_out", c_vp), ("d_out_stride", c_i64),
    ("d_out_row_stride", c_i64), ("dx", c_vp), ("dx_stride", c_i64), ("dx_row_stride", c_i64), ("d_att", c_vp), ("d_att_stride", c_i64),
    ("d_layers", c_vp), ("accumulate", c_i32), ("max_blocks", c_i32)]})


class lstm(object):
    """dctr_lstm_args_t, one level down for the same reason as interacting.Args (tests/test_dsin_cpu.py checks the layout)."""
    MERGES = {"fw": 0, "bw": 1, "sum": 2, "mul": 3, "ave": 4, "concat": 5, None: 6}
    ACTIVATIONS = {"sigmoid": 0, "hard_sigmoid": 1}
    ROUTE_AUTO, ROUTE_RESIDENT, ROUTE_STREAMED, ROUTE_WORKSPACE = 0, 1, 2, 3
    ROUTES = {None: ROUTE_AUTO, "resident": ROUTE_RESIDENT, "streamed": ROUTE_STREAMED, "workspace": ROUTE_WORKSPACE}
    LAYER_PTRS = 6      # fw kernel, fw recurrent kernel, fw bias, bw kernel, bw recurrent kernel, bw bias
    MAX_LAYERS = 8

    class Args(ctypes.Structure):
        _fields_ = [("batch", c_i64), ("x", c_vp), ("x_stride", c_i64), ("x_row_stride", c_i64), ("seq_len", c_i32), ("in_dim", c_i32),
                    ("units", c_i32), ("n_layers", c_i32), ("res_layers", c_i32), ("merge_mode", c_i32), ("recurrent_activation", c_i32),
                    ("route", c_i32), ("layers", c_vp), ("out", c_vp), ("out_stride", c_i64), ("out_row_stride", c_i64), ("out_bw", c_vp),
                    ("out_bw_stride", c_i64), ("out_bw_row_stride", c_i64), ("workspace", c_vp), ("workspace_bytes", c_sz)]


# dctr_lstm_train_args_t (tests/test_bilstm_bwd_oracle_cpu.py checks the layout)
lstm.TrainArgs = type("TrainArgs", (ctypes.Structure,), {"_fields_": [
    ("fwd", lstm.Args), ("masks", c_vp), ("tape", c_vp), ("tape_bytes", c_sz), ("d_out", c_vp), ("d_out_stride", c_i64),
    ("d_out_row_stride", c_i64), ("d_out_bw", c_vp), ("d_out_bw_stride", c_i64), ("d_out_bw_row_stride", c_i64), ("dx", c_vp),
    ("dx_stride", c_i64), ("dx_row_stride", c_i64), ("d_layers", c_vp), ("accumulate", c_i32), ("max_blocks", c_i32), ("workspace", c_vp),
    ("workspace_bytes", c_sz)]})


class fieldconv(object):
    """dctr_fieldconv_args_t, one level down for the same reason as interacting.Args (tests/test_ccpm_fgcnn_cpu.py checks the layout)."""
    POOL_KMAX, POOL_MAX = 0, 1
    POOLS = {"kmax": POOL_KMAX, "max": POOL_MAX}
    ROUTE_AUTO, ROUTE_RESIDENT, ROUTE_STREAMED, ROUTE_WORKSPACE = 0, 1, 2, 3
    ROUTES = {None: ROUTE_AUTO, "resident": ROUTE_RESIDENT, "streamed": ROUTE_STREAMED, "workspace": ROUTE_WORKSPACE}
    MAX_STAGES = 8

    class Args(ctypes.Structure):
        _fields_ = [("batch", c_i64), ("x", c_vp), ("x_stride", c_i64), ("x_offset", c_i64), ("fields", c_i32), ("dim", c_i32),
                    ("in_channels", c_i32), ("n_stages", c_i32), ("route", c_i32), ("reserved", c_i32), ("widths", c_vp),
                    ("channels", c_vp), ("pool_kinds", c_vp), ("pool_args", c_vp), ("kernels", c_vp), ("biases", c_vp), ("out", c_vp),
                    ("out_stride", c_i64), ("out_offset", c_i64), ("stage_outs", c_vp), ("stage_out_strides", c_vp), ("workspace", c_vp),
                    ("workspace_bytes", c_sz)]


class mtl(object):
    """dctr_mtl_args_t / dctr_mtl_mix_args_t / dctr_mtl_mix_bwd_args_t / dctr_mtl_loss_args_t, one level down for the same reason as interacting.Args (tests/test_mtl_cpu.py checks the
    layout)."""
    LEVEL, TOWERS = 0, 1
    ROUTE_AUTO, ROUTE_FUSED, ROUTE_LAYERED = 0, 1, 2

    class Args(ctypes.Structure):
        _fields_ = [("batch", c_i64), ("x", c_vp), ("x_stride", c_i64), ("x_offsets", c_vp), ("n_slots", c_i32), ("in_dim", c_i32),
                    ("n_experts", c_i32), ("n_layers", c_i32), ("units", c_vp), ("expert_src", c_vp), ("expert_w", c_vp), ("expert_b", c_vp),
                    ("expert_bn_scale", c_vp), ("expert_bn_shift", c_vp), ("activation", c_i32), ("route", c_i32), ("n_gates", c_i32),
                    ("n_gate_layers", c_i32), ("gate_units", c_vp), ("gate_src", c_vp), ("gate_n", c_vp), ("members", c_vp), ("gate_w", c_vp),
                    ("gate_b", c_vp), ("gate_bn_scale", c_vp), ("gate_bn_shift", c_vp), ("gate_kernel", c_vp), ("out", c_vp),
                    ("out_stride", c_i64), ("out_offset", c_i64), ("head_w", c_vp), ("global_bias", c_vp), ("binary", c_vp), ("esmm", c_i32),
                    ("tile_rows", c_i32), ("probs", c_vp), ("probs_stride", c_i64)]

    class MixArgs(ctypes.Structure):
        _fields_ = [("batch", c_i64), ("h", c_vp), ("h_stride", c_i64), ("n_experts", c_i32), ("width", c_i32), ("n_gates", c_i32),
                    ("z_dim", c_i32), ("z", c_vp), ("z_stride", c_vp), ("gate_kernel", c_vp), ("gate_n", c_vp), ("members", c_vp),
                    ("members_dev", c_vp), ("out", c_vp), ("out_stride", c_i64), ("out_offset", c_i64)]

    LOSS_BCE, LOSS_MSE = 0, 1

    class MixBwdArgs(ctypes.Structure):
        _fields_ = [("batch", c_i64), ("h", c_vp), ("h_stride", c_i64), ("n_experts", c_i32), ("width", c_i32), ("n_gates", c_i32),
                    ("z_dim", c_i32), ("z", c_vp), ("z_stride", c_vp), ("gate_kernel", c_vp), ("gate_n", c_vp), ("members", c_vp),
                    ("members_dev", c_vp), ("d_out", c_vp), ("d_out_stride", c_i64), ("d_out_offset", c_i64), ("dh", c_vp),
                    ("dh_stride", c_i64), ("ds", c_vp), ("ds_stride", c_i64), ("logits", c_vp), ("logits_stride", c_i64)]

    class LossArgs(ctypes.Structure):
        _fields_ = [("batch", c_i64), ("n_tasks", c_i32), ("esmm", c_i32), ("pred", c_vp), ("pred_stride", c_i64), ("y", c_vp),
                    ("y_stride", c_i64), ("loss_kind", c_vp), ("binary", c_vp), ("loss_weight", c_vp), ("dlogit", c_vp),
                    ("dlogit_stride", c_i64), ("loss_sum", c_vp), ("dbias", c_vp)]


class CinBwdArgs(ctypes.Structure):
    _fields_ = [("fwd", ctypes.POINTER(CinArgs)), ("d_out", c_vp), ("out_dim", c_i32), ("dx_accumulate", c_i32),
                ("d_filters", c_vp), ("d_bias", c_vp), ("dx", c_vp), ("dx_stride", c_i64), ("workspace", c_vp),
                ("workspace_bytes", c_sz), ("saved_y", c_vp)]


class CrossBwdArgs(ctypes.Structure):
    _fields_ = [("x", c_vp), ("x_stride", c_i64), ("batch", c_i64), ("dim", c_i32), ("layers", c_i32), ("mode", c_i32),
                ("dx_accumulate", c_i32), ("kernels", c_vp), ("bias", c_vp), ("dy", c_vp), ("dy_stride", c_i64),
                ("d_kernels", c_vp), ("d_bias", c_vp), ("dx", c_vp), ("dx_stride", c_i64), ("workspace", c_vp),
                ("workspace_bytes", c_sz), ("saved_u", c_vp), ("saved_x", c_vp)]


class AfmBwdArgs(ctypes.Structure):
    _fields_ = [("x", c_vp), ("batch", c_i64), ("x_stride", c_i64), ("fields", c_i32), ("dim", c_i32), ("att_factor", c_i32),
                ("dx_accumulate", c_i32), ("att_w", c_vp), ("att_b", c_vp), ("proj_h", c_vp), ("proj_p", c_vp), ("dy", c_vp),
                ("dx", c_vp), ("dx_stride", c_i64), ("d_att_w", c_vp), ("d_att_b", c_vp), ("d_proj_h", c_vp), ("d_proj_p", c_vp)]


class HostCol(ctypes.Structure):
    _fields_ = [("src", c_vp), ("stride_bytes", c_i64), ("kind", c_i32), ("reserved_", c_i32)]


HOST_KINDS = {"int32": 0, "int64": 1, "float32": 2, "float64": 3}


class CrossnetArgs(ctypes.Structure):
    _fields_ = [("x", c_vp), ("batch", c_i64), ("x_stride", c_i64), ("dim", c_i32), ("layers", c_i32), ("mode", c_i32),
                ("workspace_ready", c_i32), ("kernels", c_vp), ("bias", c_vp), ("y", c_vp), ("y_stride", c_i64), ("workspace", c_vp),
                ("workspace_bytes", c_sz), ("head_w", c_vp), ("logit", c_vp), ("save_u", c_vp), ("save_x", c_vp)]


class AdamSeg(ctypes.Structure):
    _fields_ = [("w", c_vp), ("m", c_vp), ("v", c_vp), ("g", c_vp), ("n", c_i64), ("l2", c_f32), ("pad_", c_i32), ("touched", c_vp)]


class opt(object):
    """dctr_opt_seg_t / dctr_opt_args_t of dctr_opt_apply and dctr_grad_clip_scales, one level down like interacting.Args
    (tests/test_optimizers_cpu.py checks the layout)."""
    ADAM, ADAGRAD, RMSPROP, SGD, ADAMAX, ADADELTA, FTRL = range(7)
    CLIP_PER_SEGMENT, CLIP_GLOBAL = 0, 1

    class Seg(ctypes.Structure):
        _fields_ = [("w", c_vp), ("g", c_vp), ("s0", c_vp), ("s1", c_vp), ("s2", c_vp), ("n", c_i64), ("l2", c_f32), ("pad_", c_i32),
                    ("touched", c_vp)]

    class Args(ctypes.Structure):
        _fields_ = [("kind", c_i32), ("lr", c_f32), ("beta1", c_f32), ("beta2", c_f32), ("eps", c_f32), ("momentum", c_f32),
                    ("lr_power", c_f32), ("l1", c_f32), ("l2_ftrl", c_f32), ("l2_shrinkage", c_f32), ("nesterov", c_i32),
                    ("centered", c_i32), ("amsgrad", c_i32), ("clipvalue", c_f32), ("clip_scale", c_vp), ("zero_grad", c_i32),
                    ("penalty_scale", c_f32), ("l2_penalty", c_vp)]


class DinAttnArgs(ctypes.Structure):
    _fields_ = [("query", c_vp), ("keys", c_vp), ("key_mask", c_vp), ("batch", c_i64), ("maxlen", c_i32),
                ("dim", c_i32), ("n_layers", c_i32), ("activation", c_i32), ("units", c_vp), ("kernels", c_vp),
                ("biases", c_vp), ("dice_alpha", c_vp), ("dice_mean", c_vp), ("dice_var", c_vp), ("dice_eps", c_f32),
                ("weight_normalization", c_i32), ("out_kernel", c_vp), ("out_bias", c_vp), ("out", c_vp),
                ("out_stride", c_i64), ("scores", c_vp), ("workspace", c_vp), ("workspace_bytes", c_sz)]


class DinGatherArgs(ctypes.Structure):
    _fields_ = [("n_feats", c_i32), ("ids_is_i64", c_i32), ("hist_ids", c_vp * 2), ("hist_stride", c_i64), ("query_ids", c_vp * 2),
                ("query_stride", c_i64), ("hist_table", c_vp * 2), ("query_table", c_vp * 2), ("hist_vocab", c_i64 * 2),
                ("query_vocab", c_i64 * 2), ("mask_zero", c_i32 * 2), ("status", c_vp)]


# every symbol include/dctr.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "dctr_abi_version": (ctypes.c_int, []),
    "dctr_last_error": (ctypes.c_char_p, []),
    "dctr_target_arch": (ctypes.c_char_p, []),
    "dctr_profile_next_launch": (ctypes.c_int, []),
    "dctr_profile_last_ms": (ctypes.c_float, []),
    "dctr_wall_clock_khz": (ctypes.c_int, []),
    "dctr_profile_arm": (ctypes.c_int, [c_i32]),
    "dctr_profile_collect": (ctypes.c_int, [c_vp, c_i32]),
    "dctr_hash_bucket_i32": (ctypes.c_int, [c_vp, c_i64, c_i64, ctypes.c_int, c_vp, c_vp]),
    "dctr_hash_bucket_i64": (ctypes.c_int, [c_vp, c_i64, c_i64, ctypes.c_int, c_vp, c_vp]),
    "dctr_hash_bucket_bytes": (ctypes.c_int, [c_vp, c_vp, c_i64, c_i64, ctypes.c_int, c_vp, c_vp]),
    "dctr_embed_gather_fm": (ctypes.c_int, [ctypes.POINTER(GatherFmArgs), c_vp]),
    "dctr_sgemm": (ctypes.c_int, [c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_i32, c_i64, c_vp, c_i32, c_i64, ctypes.c_float, c_vp, c_i32,
                                  c_i64, c_i32, c_vp]),
    "dctr_sgemm_plan": (ctypes.c_int, [c_i32, c_i32, c_i32, c_i32, c_i32, ctypes.POINTER(c_i32), ctypes.POINTER(c_i32),
                                       ctypes.POINTER(c_i32)]),
    "dctr_gemm_k_slices": (c_i32, [c_i32, c_i32]),
    "dctr_sgemm_grouped": (ctypes.c_int, [ctypes.POINTER(gemm.Group), c_i32, c_vp]),
    "dctr_hash_fields": (ctypes.c_int, [c_vp, c_i32, c_vp, c_i64, c_i64, c_i32, c_i64, c_vp, c_i64, c_i32, c_vp]),
    "dctr_embed_pool": (ctypes.c_int, [ctypes.POINTER(PoolArgs), c_vp]),
    "dctr_embed_lookup": (ctypes.c_int, [ctypes.POINTER(LookupArgs), c_vp]),
    "dctr_embed_lookup_multi": (ctypes.c_int, [ctypes.POINTER(LookupArgs), c_i32, c_vp, c_vp, c_i32, c_vp]),
    "dctr_seq_weight_fwd": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp, c_i64, c_i32, c_i32, c_i32, c_vp, c_vp]),
    "dctr_fm_fwd": (ctypes.c_int, [c_vp, c_i64, c_i64, c_i32, c_i32, c_vp, c_vp]),
    "dctr_crossnet_workspace_bytes": (c_sz, [c_i32, c_i32, c_i32, c_vp]),
    "dctr_crossnet_fwd": (ctypes.c_int, [c_vp, c_i64, c_i32, c_i64, c_vp, c_vp, c_i32, c_i32, c_vp, c_i64, c_vp, c_sz, c_vp]),
    "dctr_crossnet_head_fwd": (ctypes.c_int, [ctypes.POINTER(CrossnetArgs), c_vp]),
    "dctr_crossnet_gather_head_fwd": (ctypes.c_int, [ctypes.POINTER(CrossnetArgs), ctypes.POINTER(GatherFmArgs), c_vp]),
    "dctr_crossnet_fwd_supported": (ctypes.c_int, [ctypes.POINTER(CrossnetArgs), ctypes.POINTER(GatherFmArgs)]),
    "dctr_crossnet_matrix_step": (ctypes.c_int, [c_vp, c_i64, c_vp, c_i64, c_vp, c_vp, c_i64, c_i32, c_vp, c_i64, c_vp]),
    "dctr_cin_workspace_bytes": (c_sz, [ctypes.POINTER(CinArgs)]),
    "dctr_cin_fwd": (ctypes.c_int, [ctypes.POINTER(CinArgs), c_vp]),
    "dctr_cin_fwd_supported": (ctypes.c_int, [ctypes.POINTER(CinArgs), ctypes.POINTER(GatherFmArgs), ctypes.c_int32]),
    "dctr_cin_gather_fwd": (ctypes.c_int, [ctypes.POINTER(CinArgs), ctypes.POINTER(GatherFmArgs), c_vp, c_vp, c_vp]),
    "dctr_interacting_workspace_bytes": (c_sz, [ctypes.POINTER(interacting.Args)]),
    "dctr_interacting_fwd": (ctypes.c_int, [ctypes.POINTER(interacting.Args), c_vp]),
    "dctr_interacting_bwd_supported": (ctypes.c_int, [ctypes.POINTER(interacting.BwdArgs)]),
    "dctr_interacting_bwd_workspace_bytes": (c_sz, [ctypes.POINTER(interacting.BwdArgs)]),
    "dctr_interacting_bwd": (ctypes.c_int, [ctypes.POINTER(interacting.BwdArgs), c_vp]),
    "dctr_bilinear_workspace_bytes": (c_sz, [ctypes.POINTER(bilinear.Args)]),
    "dctr_bilinear_fwd": (ctypes.c_int, [ctypes.POINTER(bilinear.Args), c_vp]),
    "dctr_bilinear_bwd_workspace_bytes": (c_sz, [ctypes.POINTER(bilinear.BwdArgs)]),
    "dctr_bilinear_bwd_supported": (ctypes.c_int, [ctypes.POINTER(bilinear.BwdArgs)]),
    "dctr_bilinear_bwd": (ctypes.c_int, [ctypes.POINTER(bilinear.BwdArgs), c_vp]),
    "dctr_fieldpair_workspace_bytes": (c_sz, [ctypes.POINTER(fieldpair.Args)]),
    "dctr_fieldpair_fwd": (ctypes.c_int, [ctypes.POINTER(fieldpair.Args), c_vp]),
    "dctr_fieldpair_bwd_workspace_bytes": (c_sz, [ctypes.POINTER(fieldpair.BwdArgs)]),
    "dctr_fieldpair_bwd_supported": (ctypes.c_int, [ctypes.POINTER(fieldpair.BwdArgs)]),
    "dctr_fieldpair_bwd": (ctypes.c_int, [ctypes.POINTER(fieldpair.BwdArgs), c_vp]),
    "dctr_ffm_workspace_bytes": (c_sz, [ctypes.POINTER(ffm.Args)]),
    "dctr_ffm_route": (ctypes.c_int, [ctypes.POINTER(ffm.Args)]),
    "dctr_ffm_fwd": (ctypes.c_int, [ctypes.POINTER(ffm.Args), c_vp]),
    "dctr_ffm_bwd_workspace_bytes": (c_sz, [ctypes.POINTER(ffm.BwdArgs)]),
    "dctr_ffm_bwd_route": (ctypes.c_int, [ctypes.POINTER(ffm.BwdArgs)]),
    "dctr_ffm_bwd": (ctypes.c_int, [ctypes.POINTER(ffm.BwdArgs), c_vp]),
    "dctr_mlr_supported": (ctypes.c_int, [ctypes.POINTER(mlr.Args)]),
    "dctr_mlr_fwd": (ctypes.c_int, [ctypes.POINTER(mlr.Args), c_vp]),
    "dctr_mlr_bwd": (ctypes.c_int, [ctypes.POINTER(mlr.BwdArgs), c_vp]),
    "dctr_ifm_workspace_bytes": (c_sz, [ctypes.POINTER(ifm.Args)]),
    "dctr_ifm_route": (ctypes.c_int, [ctypes.POINTER(ifm.Args)]),
    "dctr_ifm_fwd": (ctypes.c_int, [ctypes.POINTER(ifm.Args), c_vp]),
    "dctr_ifm_bwd_supported": (ctypes.c_int, [ctypes.POINTER(ifm.BwdArgs)]),
    "dctr_ifm_bwd_workspace_bytes": (c_sz, [ctypes.POINTER(ifm.BwdArgs)]),
    "dctr_ifm_bwd": (ctypes.c_int, [ctypes.POINTER(ifm.BwdArgs), c_vp]),
    "dctr_fieldwise_route": (ctypes.c_int, [ctypes.POINTER(fieldwise.Args)]),
    "dctr_fieldwise_fwd": (ctypes.c_int, [ctypes.POINTER(fieldwise.Args), c_vp]),
    "dctr_fieldwise_bwd_supported": (ctypes.c_int, [ctypes.POINTER(fieldwise.BwdArgs)]),
    "dctr_fieldwise_bwd": (ctypes.c_int, [ctypes.POINTER(fieldwise.BwdArgs), c_vp]),
    "dctr_edcn_workspace_bytes": (c_sz, [ctypes.POINTER(edcn.Args)]),
    "dctr_edcn_route": (ctypes.c_int, [ctypes.POINTER(edcn.Args)]),
    "dctr_edcn_fwd": (ctypes.c_int, [ctypes.POINTER(edcn.Args), c_vp]),
    "dctr_edcn_bwd_supported": (ctypes.c_int, [ctypes.POINTER(edcn.TrainArgs)]),
    "dctr_edcn_tape_bytes": (c_sz, [ctypes.POINTER(edcn.TrainArgs)]),
    "dctr_edcn_bwd_workspace_bytes": (c_sz, [ctypes.POINTER(edcn.TrainArgs)]),
    "dctr_edcn_train_fwd": (ctypes.c_int, [ctypes.POINTER(edcn.TrainArgs), c_vp]),
    "dctr_edcn_bwd": (ctypes.c_int, [ctypes.POINTER(edcn.TrainArgs), c_vp]),
    "dctr_transformer_workspace_bytes": (c_sz, [ctypes.POINTER(transformer.Args)]),
    "dctr_transformer_route": (ctypes.c_int, [ctypes.POINTER(transformer.Args)]),
    "dctr_transformer_fwd": (ctypes.c_int, [ctypes.POINTER(transformer.Args), c_vp]),
    "dctr_transformer_tape_bytes": (c_sz, [ctypes.POINTER(transformer.Args)]),
    "dctr_transformer_train_fwd": (ctypes.c_int, [ctypes.POINTER(transformer.TrainArgs), c_vp]),
    "dctr_transformer_bwd_supported": (ctypes.c_int, [ctypes.POINTER(transformer.TrainArgs)]),
    "dctr_transformer_bwd_workspace_bytes": (c_sz, [ctypes.POINTER(transformer.TrainArgs)]),
    "dctr_transformer_bwd": (ctypes.c_int, [ctypes.POINTER(transformer.TrainArgs), c_vp]),
    "dctr_gru_workspace_bytes": (c_sz, [ctypes.POINTER(gru.Args)]),
    "dctr_gru_route": (ctypes.c_int, [ctypes.POINTER(gru.Args)]),
    "dctr_gru_fwd": (ctypes.c_int, [ctypes.POINTER(gru.Args), c_vp]),
    "dctr_gru_bwd_supported": (ctypes.c_int, [ctypes.POINTER(gru.BwdArgs)]),
    "dctr_gru_bwd_workspace_bytes": (c_sz, [ctypes.POINTER(gru.BwdArgs)]),
    "dctr_gru_bwd": (ctypes.c_int, [ctypes.POINTER(gru.BwdArgs), c_vp]),
    "dctr_bilstm_workspace_bytes": (c_sz, [ctypes.POINTER(lstm.Args)]),
    "dctr_bilstm_route": (ctypes.c_int, [ctypes.POINTER(lstm.Args)]),
    "dctr_bilstm_fwd": (ctypes.c_int, [ctypes.POINTER(lstm.Args), c_vp]),
    "dctr_bilstm_tape_bytes": (c_sz, [ctypes.POINTER(lstm.Args)]),
    "dctr_bilstm_train_fwd": (ctypes.c_int, [ctypes.POINTER(lstm.TrainArgs), c_vp]),
    "dctr_bilstm_bwd_supported": (ctypes.c_int, [ctypes.POINTER(lstm.TrainArgs)]),
    "dctr_bilstm_bwd_workspace_bytes": (c_sz, [ctypes.POINTER(lstm.TrainArgs)]),
    "dctr_bilstm_bwd": (ctypes.c_int, [ctypes.POINTER(lstm.TrainArgs), c_vp]),
    "dctr_bias_encoding_fwd": (ctypes.c_int, [c_vp, c_i64, c_i32, c_i32, c_i32, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp]),
    "dctr_fieldconv_workspace_bytes": (c_sz, [ctypes.POINTER(fieldconv.Args)]),
    "dctr_fieldconv_route": (ctypes.c_int, [ctypes.POINTER(fieldconv.Args)]),
    "dctr_fieldconv_fwd": (ctypes.c_int, [ctypes.POINTER(fieldconv.Args), c_vp]),
    "dctr_kmax_pool_fwd": (ctypes.c_int, [c_vp, c_i64, c_i32, c_i64, c_i32, c_vp, c_vp]),
    "dctr_layer_norm_fwd": (ctypes.c_int, [c_vp, c_i64, c_i32, c_i64, c_vp, c_vp, c_f32, c_vp, c_i64, c_vp]),
    "dctr_mtl_route": (ctypes.c_int, [ctypes.POINTER(mtl.Args), c_i32]),
    "dctr_mtl_level_fwd": (ctypes.c_int, [ctypes.POINTER(mtl.Args), c_vp]),
    "dctr_mtl_towers_fwd": (ctypes.c_int, [ctypes.POINTER(mtl.Args), c_vp]),
    "dctr_mtl_mix": (ctypes.c_int, [ctypes.POINTER(mtl.MixArgs), c_vp]),
    "dctr_mtl_mix_bwd": (ctypes.c_int, [ctypes.POINTER(mtl.MixBwdArgs), c_vp]),
    "dctr_mtl_loss_grad": (ctypes.c_int, [ctypes.POINTER(mtl.LossArgs), c_vp]),
    "dctr_mtl_sum_slots": (ctypes.c_int, [c_vp, c_vp, c_i32, c_i64, c_i32, c_vp, c_i64, c_i64, c_i32, c_vp]),
    "dctr_edcn_regulate": (ctypes.c_int, [c_vp, c_i64, c_i64, c_i32, c_i32, c_vp, c_vp, c_f32, c_vp, c_i64, c_vp, c_i64, c_vp]),
    "dctr_edcn_bridge": (ctypes.c_int, [c_i32, c_vp, c_i64, c_vp, c_i64, c_vp, c_i64, c_vp, c_i64, c_i64, c_i32, c_vp, c_i64, c_vp]),
    "dctr_afm_fwd": (ctypes.c_int, [c_vp, c_i64, c_i64, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_vp]),
    "dctr_host_pack_columns": (ctypes.c_int, [c_vp, c_i32, c_i64, c_i64, c_vp, c_i64, c_i32, c_i32]),
    "dctr_crossnet_mix_workspace_bytes": (ctypes.c_size_t, [c_i32, c_i32, c_i32, c_i32]),
    "dctr_crossnet_mix_fwd": (ctypes.c_int, [c_vp, c_i64, c_i32, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp,
                                             c_i64, c_vp, ctypes.c_size_t, c_vp]),
    "dctr_bi_interaction_fwd": (ctypes.c_int, [c_vp, c_i64, c_i64, c_i32, c_i32, c_vp, c_i64, c_vp]),
    "dctr_inner_product_fwd": (ctypes.c_int, [c_vp, c_i64, c_i64, c_i32, c_i32, c_i32, c_vp, c_i64, c_vp]),
    "dctr_mlp_workspace_bytes": (c_sz, [ctypes.POINTER(MlpArgs)]),
    "dctr_mlp_fwd_supported": (ctypes.c_int, [ctypes.POINTER(GatherFmArgs), ctypes.POINTER(MlpArgs), ctypes.c_int32, ctypes.c_int32]),
    "dctr_crossnet_fold_consts": (ctypes.c_int, [c_vp, c_vp, c_vp, c_i32, c_i32, c_vp, c_vp]),
    "dctr_mlp_fwd": (ctypes.c_int, [ctypes.POINTER(MlpArgs), c_vp]),
    "dctr_embed_mlp_fwd": (ctypes.c_int, [ctypes.POINTER(GatherFmArgs), ctypes.POINTER(MlpArgs), c_i32, c_i32, c_vp]),
    "dctr_embed_mlp_fwd_last_kernel": (ctypes.c_int, []),
    "dctr_embed_mlp_fwd_plan": (ctypes.c_int, [ctypes.POINTER(GatherFmArgs), ctypes.POINTER(MlpArgs), ctypes.POINTER(ctypes.c_int64),
                                               ctypes.POINTER(c_i32), ctypes.POINTER(c_i32), c_i32]),
    "dctr_bce_grad": (ctypes.c_int, [c_vp, c_vp, c_i64, c_i32, c_vp, c_vp, c_vp, c_vp]),
    "dctr_bce_grad_w": (ctypes.c_int, [c_vp, c_vp, c_vp, c_i64, c_i32, c_vp, c_vp, c_vp, c_vp]),
    "dctr_embed_gather_fm_bwd": (ctypes.c_int, [ctypes.POINTER(GatherFmBwdArgs), c_vp]),
    "dctr_embed_pool_bwd": (ctypes.c_int, [ctypes.POINTER(PoolBwdArgs), c_vp]),
    "dctr_afm_bwd": (ctypes.c_int, [c_vp, c_vp]),
    "dctr_afm_bwd_supported": (ctypes.c_int, [c_i32, c_i32, c_i32]),
    "dctr_din_att_in_fwd": (ctypes.c_int, [c_vp, c_vp, c_i64, c_i32, c_i32, c_vp, c_vp]),
    "dctr_din_wsum_fwd": (ctypes.c_int, [c_vp, c_vp, c_vp, c_i64, c_i32, c_i32, c_vp, c_i64, c_vp]),
    "dctr_din_wsum_bwd": (ctypes.c_int, [c_vp, c_i64, c_vp, c_vp, c_vp, c_i64, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp]),
    "dctr_din_att_in_bwd": (ctypes.c_int, [c_vp, c_vp, c_vp, c_i64, c_i32, c_i32, c_vp, c_vp, c_i64, c_vp, c_vp]),
    "dctr_embed_lookup_bwd": (ctypes.c_int, [c_vp, c_vp, c_i64, c_vp, c_vp, c_vp]),
    "dctr_bi_interaction_bwd": (ctypes.c_int, [c_vp, c_i64, c_i64, c_i32, c_i32, c_vp, c_i64, c_vp, c_i64, c_i32, c_vp]),
    "dctr_inner_product_bwd": (ctypes.c_int, [c_vp, c_i64, c_i64, c_i32, c_i32, c_vp, c_i64, c_vp, c_i64, c_i32, c_vp]),
    "dctr_dense1_bwd": (ctypes.c_int, [c_vp, c_i64, c_i64, c_i32, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp]),
    "dctr_crossnet_bwd_workspace_bytes": (c_sz, [ctypes.POINTER(CrossBwdArgs)]),
    "dctr_crossnet_bwd": (ctypes.c_int, [ctypes.POINTER(CrossBwdArgs), c_vp]),
    "dctr_cin_bwd_workspace_bytes": (c_sz, [ctypes.POINTER(CinBwdArgs)]),
    "dctr_cin_bwd": (ctypes.c_int, [ctypes.POINTER(CinBwdArgs), c_vp]),
    "dctr_mlp_bwd_workspace_bytes": (c_sz, [ctypes.POINTER(MlpBwdArgs)]),
    "dctr_mlp_bwd_join": (ctypes.c_int, [c_vp, c_vp]),
    "dctr_mlp_bwd": (ctypes.c_int, [ctypes.POINTER(MlpBwdArgs), c_vp]),
    "dctr_crossnet_mix_bwd_workspace_bytes": (c_sz, [ctypes.POINTER(CrossMixBwdArgs)]),
    "dctr_crossnet_mix_bwd": (ctypes.c_int, [ctypes.POINTER(CrossMixBwdArgs), c_vp]),
    "dctr_crossnet_mix_bwd_supported": (ctypes.c_int, [c_i32, c_i32, c_i32, c_i32]),
    "dctr_fm_bwd": (ctypes.c_int, [c_vp, c_i64, c_i64, c_i32, c_i32, c_vp, c_vp, c_i64, c_i32, c_vp]),
    "dctr_din_softmax_fwd": (ctypes.c_int, [c_vp, c_vp, c_i64, c_i32, c_vp, c_vp]),
    "dctr_din_softmax_bwd": (ctypes.c_int, [c_vp, c_vp, c_vp, c_i64, c_i32, c_vp, c_vp, c_vp]),
    "dctr_dnn_train_layer_fwd": (ctypes.c_int, [ctypes.POINTER(DnnTrainLayer), c_vp]),
    "dctr_dnn_train_layer_bwd": (ctypes.c_int, [ctypes.POINTER(DnnTrainLayer), c_vp]),
    "dctr_dice_train_fwd": (ctypes.c_int, [c_vp, c_i64, c_vp, c_i64, c_i32, c_vp, c_f32, c_f32, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp]),
    "dctr_adam_step": (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp, c_i64, c_f32, c_f32, c_f32, c_f32, c_f32, c_i32, c_vp]),
    "dctr_adam_multi": (ctypes.c_int, [c_vp, c_i32, c_i64, c_f32, c_f32, c_f32, c_f32, c_i32, c_vp]),
    "dctr_opt_multi": (ctypes.c_int, [c_i32, c_vp, c_i32, c_i64, c_f32, c_f32, c_f32, c_f32, c_i32, c_vp]),
    "dctr_opt_multi_l2": (ctypes.c_int, [ctypes.c_int32, c_vp, c_i32, c_i64, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                          c_i32, c_vp, ctypes.c_float, c_vp]),
    "dctr_opt_apply": (ctypes.c_int, [ctypes.POINTER(opt.Args), c_vp, c_i32, c_i64, c_vp]),
    "dctr_grad_clip_scales_workspace_bytes": (c_sz, [c_i32, c_i64]),
    "dctr_grad_clip_scales": (ctypes.c_int, [c_vp, c_i32, c_i64, c_i32, c_f32, c_vp, c_sz, c_vp, c_vp]),
    "dctr_din_attn_workspace_bytes": (c_sz, [ctypes.POINTER(DinAttnArgs)]),
    "dctr_din_attn_pool_fwd": (ctypes.c_int, [ctypes.POINTER(DinAttnArgs), c_vp]),
    "dctr_din_attn_gather_fwd": (ctypes.c_int, [ctypes.POINTER(DinAttnArgs), ctypes.POINTER(DinGatherArgs), c_vp]),
}

_LIB = None


def lib():
    """Load (once) and return the ctypes handle.  torch is imported FIRST so that the library's
    ``NEEDED libamdhip64.so.7`` binds to the HIP runtime PyTorch already loaded."""
    global _LIB
    if _LIB is not None:
        return _LIB
    import torch  # noqa: F401  (must precede CDLL: one HIP runtime per process)
    if not os.path.exists(LIB_PATH):
        raise DctrExtensionError(
            "HIP extension %s is not built. Run `python -m deepctr_amd.build` (needs hipcc; target gfx950). "
            "There is no CPU / PyTorch fallback for this path." % LIB_PATH)
    try:
        handle = ctypes.CDLL(LIB_PATH)
    except OSError as e:
        raise DctrExtensionError("cannot load %s: %s" % (LIB_PATH, e))
    for name, (res, args) in SYMBOLS.items():
        try:
            fn = getattr(handle, name)
        except AttributeError:
            raise DctrExtensionError("%s does not export %s (stale build? run python -m deepctr_amd.build --force)"
                                     % (LIB_PATH, name))
        fn.restype = res
        fn.argtypes = args
    ver = handle.dctr_abi_version()
    if ver != ABI_VERSION:
        raise DctrExtensionError("ABI mismatch: library %d, python %d" % (ver, ABI_VERSION))
    _LIB = handle
    return _LIB


def check(rc, what):
    if rc != 0:
        msg = lib().dctr_last_error()
        err = DctrError("%s failed (rc=%d): %s" % (what, rc, msg.decode() if msg else ""))
        err.rc = int(rc)
        raise err


def require_device():
    """Return the torch HIP device or raise: the path never runs on the CPU."""
    import torch
    if not torch.cuda.is_available():
        raise DctrExtensionError("no HIP device visible: deepctr_amd's forward path only runs on an AMD GPU "
                                 "(MI355X / gfx950); there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def stream_ptr():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
