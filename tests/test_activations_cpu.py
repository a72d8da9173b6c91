"""CPU: the tf.keras 2.x activation names of the DNN (elu, selu, softplus, softsign, exponential, hard_sigmoid, swish / silu, gelu).
  1. tests/ref_activations.py, the float64 oracle of the GPU tests, pinned without TensorFlow: known values, torch's float64
     functions, and both derivative forms against central differences;
  2. the host surface: activation_layer, DNN, every model constructor that takes ``dnn_activation``, the callers that keep refusing;
  3. training.dnn_forward (the autograd step's restatement) against the oracle, values and gradients;
  4. training_hip.supported / HipTrainer with the new names;
  5. the C ABI's argument checks, which run without a launch."""
import ctypes
import inspect
import math
import types

import numpy as np
import pytest
import torch

from tests import ref_activations as RA

NAMES = RA.NAMES + ("silu",)
GRID = np.concatenate([np.linspace(-30.0, 30.0, 2401), [-2.5, 2.5, 0.0, -1e-3, 1e-3, -1e-8, 1e-8]])


# ---- 1. the oracle --------------------------------------------------------------------------------------------------------------------
def test_known_values():
    assert RA.SELU_SCALE == 1.0507009873554805 and RA.SELU_ALPHA == 1.6732632423543772          # (tf.nn.selu's constants)
    one = lambda name, z: float(RA.value(name, z))                                               # noqa: E731
    assert one("gelu", 1.0) == pytest.approx(0.8413447460685429, abs=1e-15)
    assert one("swish", 1.0) == pytest.approx(0.7310585786300049, abs=1e-15) and one("silu", 1.0) == one("swish", 1.0)
    assert one("softplus", 0.0) == pytest.approx(math.log(2.0), abs=1e-15)
    assert one("softsign", 3.0) == 0.75
    assert one("elu", -1.0) == pytest.approx(math.exp(-1.0) - 1.0, abs=1e-15)
    assert one("hard_sigmoid", 2.5) == 1.0 and one("hard_sigmoid", -2.5) == 0.0 and one("hard_sigmoid", 0.0) == 0.5
    assert one("hard_sigmoid", 1.0) == pytest.approx(0.7, abs=1e-15)        # (0.2 z + 0.5: not torch's / Keras 3's relu6(z + 3) / 6 = 2 / 3)
    assert one("selu", 1.0) == RA.SELU_SCALE and one("selu", -1.0) == pytest.approx(RA.SELU_SCALE * RA.SELU_ALPHA * (math.exp(-1.0) - 1.0), abs=1e-15)
    assert one("exponential", 1.0) == pytest.approx(math.e, abs=1e-15) and one("elu", 2.0) == 2.0
    # the tails stay finite and keep their relative accuracy
    assert one("gelu", -30.0) < 0 and one("gelu", -30.0) > -1e-190 and one("softplus", -30.0) == pytest.approx(math.exp(-30.0), rel=1e-12)
    assert float(RA.deriv_from_z("softplus", -30.0)) == pytest.approx(math.exp(-30.0), rel=1e-12)
    assert float(RA.deriv_from_output("softplus", RA.value("softplus", -30.0))) == pytest.approx(math.exp(-30.0), rel=1e-12)


@pytest.mark.parametrize("name", ["elu", "selu", "softplus", "softsign", "swish", "gelu", "exponential"])
def test_values_agree_with_torch_in_float64(name):
    F = torch.nn.functional
    fn = {"elu": F.elu, "selu": F.selu, "softplus": lambda t: F.softplus(t, threshold=50.0), "softsign": F.softsign, "swish": F.silu,
          "gelu": F.gelu, "exponential": torch.exp}[name]           # (threshold: torch's shortcut softplus(z) = z beyond it, not a definition)
    ref = fn(torch.from_numpy(GRID)).numpy()
    got = RA.value(name, GRID)
    assert got.dtype == np.float64 and np.isfinite(got).all()
    assert (np.abs(got - ref) <= 1e-12 * np.abs(ref) + 1e-12).all(), float(np.abs(got - ref).max())


@pytest.mark.parametrize("name", RA.NAMES)
def test_both_derivative_forms_agree_with_central_differences(name):
    z = GRID[np.all([np.abs(GRID - k) > 0.01 for k in RA.KINKS.get(name, ())] + [np.ones_like(GRID, bool)], axis=0)]
    h = 1e-4
    cd = (RA.value(name, z + h) - RA.value(name, z - h)) / (2 * h)
    scale = np.maximum(np.abs(cd), np.abs(RA.value(name, z))) + 1e-300
    dz = RA.deriv_from_z(name, z)
    assert (np.abs(dz - cd) <= 1e-6 * scale + 1e-9).all(), float((np.abs(dz - cd) / scale).max())
    if name in RA.FROM_OUTPUT:
        do = RA.deriv_from_output(name, RA.value(name, z))
        assert (np.abs(do - cd) <= 1e-6 * scale + 1e-9).all(), float((np.abs(do - cd) / scale).max())
        # the two forms are the same function wherever the output determines it (everywhere but hard_sigmoid's ends, where both are 0)
        assert (np.abs(do - dz) <= 1e-12 * np.abs(dz) + 1e-15).all()
    else:
        assert name in RA.FROM_Z
    assert set(RA.FROM_OUTPUT) | set(RA.FROM_Z) == set(RA.NAMES) and RA.ALIASES == {"silu": "swish"}


def test_codes_are_the_abis():
    from deepctr_amd import _C
    assert {n: _C.DNN_ACT_CODES[n] for n in RA.NAMES} == RA.CODES and _C.DNN_ACT_CODES["silu"] == RA.CODES["swish"]
    assert sorted(RA.CODES.values()) == list(range(5, 13)) and _C.ABI_VERSION == 13 and _C.lib().dctr_abi_version() == 13
    assert all(n not in _C.ACT_CODES for n in NAMES)                 # every other op: still unknown names


# ---- 2. host surface -------------------------------------------------------------------------------------------------------------------
def _cols():
    from deepctr_amd.feature_column import DenseFeat, SparseFeat, VarLenSparseFeat
    E = 4
    sparse = [SparseFeat("user", 20, E), SparseFeat("item_id", 31, E), SparseFeat("cate_id", 11, E)]
    seq = [VarLenSparseFeat(SparseFeat("hist_item_id", 31, E, embedding_name="item_id"), maxlen=4, length_name="seq_length"),
           VarLenSparseFeat(SparseFeat("hist_cate_id", 11, E, embedding_name="cate_id"), maxlen=4, length_name="seq_length")]
    return sparse, [DenseFeat("score", 1)], seq


def _constructors():
    """name -> callable(dnn_activation, **kw) for every model constructor of the package that takes ``dnn_activation``."""
    from deepctr_amd import models
    sparse, dense, seq = _cols()
    flat = sparse + dense
    hist = ["item_id", "cate_id"]
    kw = dict(dnn_hidden_units=(8, 4), device="cpu")
    from deepctr_amd.feature_column import SparseFeat, VarLenSparseFeat
    sess = sparse + dense + [VarLenSparseFeat(SparseFeat("sess_%d_%s" % (i, n), v, 4, embedding_name=n), maxlen=4, length_name="seq_length%d" % i)
                             for i in range(2) for n, v in (("item_id", 31), ("cate_id", 11))]
    two = lambda C: (lambda a, **k: C(flat, flat, dnn_activation=a, **dict(kw, **k)))            # noqa: E731
    one = lambda C, cols=flat: (lambda a, **k: C(cols, dnn_activation=a, **dict(kw, **k)))       # noqa: E731
    out = {n: two(getattr(models, n)) for n in ("AutoInt", "DCN", "DCNMix", "DeepFEFM", "DeepFM", "FiBiNET", "NFM", "WDL", "xDeepFM")}
    grouped = [SparseFeat(fc.name, fc.vocabulary_size, 4, group_name="g%d" % (i % 2)) for i, fc in enumerate(sparse)] + dense
    out["FLEN"] = lambda a, **k: models.FLEN(grouped, grouped, dnn_activation=a, **dict(kw, **k))
    out.update({n: (lambda C: (lambda a, **k: C(flat, sparse, dnn_activation=a, **dict(kw, **k))))(getattr(models, n)) for n in ("FwFM", "IFM", "DIFM")})
    out.update(FNN=two(models.FNN), PNN=one(models.PNN))
    out.update({n: (lambda C: (lambda a, **k: C(sparse + dense + seq, hist, dnn_activation=a, **dict(kw, **k))))(getattr(models, n))
                for n in ("DIN", "DIEN", "BST")})
    out["DSIN"] = lambda a, **k: models.DSIN(sess, hist, sess_max_count=2, dnn_activation=a, **dict(kw, **k))
    refusing = {n: (lambda C: (lambda a, **k: C(flat, dnn_activation=a, device="cpu", **k)))(getattr(models, n))
                for n in ("SharedBottom", "ESMM", "MMOE", "PLE")}
    refusing["EDCN"] = lambda a, **k: models.EDCN(sparse, sparse, dnn_activation=a, device="cpu", **k)
    taking = sorted(n for n in dir(models) if callable(getattr(models, n)) and not n.startswith("_")
                    and "dnn_activation" in inspect.signature(getattr(models, n)).parameters)
    assert taking == sorted(list(out) + list(refusing)), taking
    return out, refusing


def test_names_are_accepted_by_activation_layer_and_dnn():
    from deepctr_amd.layers.activation import KERAS_ACTIVATIONS, SUPPORTED, activation_layer
    from deepctr_amd.layers.core import DNN
    assert sorted(KERAS_ACTIVATIONS) == sorted(NAMES) and set(NAMES) < set(SUPPORTED)
    for name in NAMES:
        assert activation_layer(name) == name
        d = DNN((6, 3), activation=name, output_activation=name, device="cpu").build_for(5)
        assert d.activation == name and d.layer_activation(1) == name and not d.dice_layers
        cfg = d.get_config()
        assert cfg["activation"] == name and cfg["output_activation"] == name
        again = DNN(**{k: v for k, v in cfg.items() if k in inspect.signature(DNN.__init__).parameters})
        assert again.get_config()["activation"] == name and again.hidden_units == d.hidden_units
        assert DNN((6, 3), activation="relu", output_activation=name, device="cpu").layer_activation(1) == name
    for bad in ("softmax", "leaky_relu", "relu6", "mish", "no_such_activation", "GELU"):
        with pytest.raises(ValueError, match="Invalid activation"):
            activation_layer(bad)
        with pytest.raises(ValueError, match="Invalid activation"):
            DNN((4,), activation=bad, device="cpu")
        with pytest.raises(ValueError, match="Invalid activation"):
            DNN((4,), output_activation=bad, device="cpu")


@pytest.mark.parametrize("name", NAMES)
def test_every_covered_constructor_builds_and_the_others_refuse(name):
    from deepctr_amd.layers.core import LocalActivationUnit
    from deepctr_amd.layers.sequence import AttentionSequencePoolingLayer
    from deepctr_amd import models
    builds, refusing = _constructors()
    assert len(builds) == 19 and len(refusing) == 5
    for kind, make in builds.items():
        m = make(name)
        assert m.dnn.activation == name, kind
    for kind, make in refusing.items():
        with pytest.raises(ValueError, match="Invalid activation"):
            make(name)
        assert make("relu") is not None, kind
    sparse, dense, seq = _cols()
    for ctor in (lambda: LocalActivationUnit((4, 2), name, device="cpu"), lambda: AttentionSequencePoolingLayer((4, 2), name, device="cpu"),
                 lambda: models.DIN(sparse + dense + seq, ["item_id", "cate_id"], att_activation=name, device="cpu"),
                 lambda: models.DIEN(sparse + dense + seq, ["item_id", "cate_id"], att_activation=name, device="cpu")):
        with pytest.raises(ValueError, match="Invalid activation"):
            ctor()


def test_ops_keep_their_sets():
    from deepctr_amd import ops
    for name in ("gelu", "selu"):
        with pytest.raises(ValueError, match="unknown activation"):
            ops.edcn_route(3, 4, activation=name)
        with pytest.raises(ValueError, match="unknown activation"):
            ops.mtl_route(6, [3], 2, members=[[0, 1]], activation=name)
        assert not ops.cin_supported(3, 4, [4], activation=name)
    for op in ("mlp", "mlp_bwd", "dnn_train_layer"):
        with pytest.raises(ValueError, match="unknown activation"):
            ops._dnn_act_code(op, "softmax")
    assert [ops._dnn_act_code("mlp", n) for n in RA.NAMES] == list(range(5, 13)) and ops._dnn_act_code("mlp", "silu") == 11


# ---- 3. the autograd step's restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_dnn_forward_restates_the_oracle(name):
    from deepctr_amd import training
    rng = np.random.RandomState(5)
    z = np.concatenate([GRID[::7], rng.standard_normal(40) * 3])
    z = z[np.all([np.abs(z - k) > 1e-6 for k in RA.KINKS.get(RA.ALIASES.get(name, name), ())] + [np.ones_like(z, bool)], axis=0)]
    x = torch.tensor(z.reshape(-1, 1) * np.ones((1, 3)), requires_grad=True)                 # float64
    dnn = types.SimpleNamespace(kernels=[torch.eye(3, dtype=torch.float64)], biases=[torch.zeros(3, dtype=torch.float64)], activation=name,
                                dropout_rate=0)
    y = training.dnn_forward(dnn, x)
    ref = RA.value(name, x.detach().numpy())
    assert (np.abs(y.detach().numpy() - ref) <= 1e-12 * np.abs(ref) + 1e-12).all()
    y.sum().backward()
    dref = RA.deriv_from_z(name, x.detach().numpy())
    assert (np.abs(x.grad.numpy() - dref) <= 1e-10 * np.abs(dref) + 1e-12).all()
    # two layers with a bias, against the oracle's DNN
    W = [rng.standard_normal((3, 5)) * 0.7, rng.standard_normal((5, 2)) * 0.5]
    b = [rng.standard_normal(5) * 0.3, rng.standard_normal(2) * 0.3]
    xin = rng.standard_normal((17, 3))
    dnn2 = types.SimpleNamespace(kernels=[torch.tensor(w) for w in W], biases=[torch.tensor(v) for v in b], activation=name, dropout_rate=0)
    got = training.dnn_forward(dnn2, torch.tensor(xin)).numpy()
    ref2 = RA.dnn(xin, W, b, name)[1][-1]
    assert (np.abs(got - ref2) <= 1e-12 * np.abs(ref2) + 1e-12).all()


# ---- 4. the HIP training step admits them --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_hip_step_is_supported_with_the_new_names(name):
    from deepctr_amd import training_hip
    builds, _ = _constructors()
    for kind in ("DeepFM", "DCN", "xDeepFM", "FLEN", "DIN"):
        extras = [dict()] + ([dict(dnn_dropout=0.3), dict(dnn_use_bn=True), dict(dnn_dropout=0.2, dnn_use_bn=True)] if kind != "DIN" else
                             [dict(dnn_dropout=0.3), dict(dnn_use_bn=True)])
        for kw in extras:
            m = builds[kind](name, **kw)
            assert training_hip.supported(m), (kind, kw)
            tr = training_hip.HipTrainer(m)
            assert tr.zact_dnn == (name in ("swish", "silu", "gelu")) and tr.slow_dnn == bool(kw) and not tr.dice_dnn
    for kind in ("AutoInt", "FiBiNET", "FwFM", "DeepFEFM", "IFM", "DIFM", "BST", "DIEN", "DSIN"):        # unchanged: the autograd step
        assert training_hip.supported(builds[kind](name)) == training_hip.supported(builds[kind]("relu")), kind
        assert not training_hip.supported(builds[kind](name)), kind


@pytest.mark.parametrize("kind", ["DeepFM", "xDeepFM", "DIN", "DeepFM-reg"])
@pytest.mark.parametrize("name", RA.NAMES)
def test_the_autograd_step_of_the_gpu_fit_cases_stays_finite_and_learns(name, kind):
    """The cases tests/test_gpu_activations.py compares the two steps on (default initialisers, labels computed from the features),
    on the CPU: plain SGD at the GPU test's rate over training.model_logits, the three batches of an epoch — every loss and gradient
    finite, the epoch loss lower after twelve epochs than after the first (with dropout: the last ten of sixty against the first ten), and no row's probability within 1e-3 of 0 or 1 in the epoch
    the GPU test runs.  (One case is let off the last point: exponential behind a BatchNormalization is exp of a unit-variance normal
    under a Glorot head, whose logits reach +-10 at the default initialisers before any update.)"""
    from deepctr_amd import engine, training
    from tests.test_gpu_activations import FIT_BATCH, FIT_LR, FIT_ROWS, fit_case
    torch.manual_seed(0)
    make, feed, y = fit_case(kind, name, "cpu")
    model = make()
    staged = engine.Staged(FIT_ROWS)
    model._stage_inputs(feed, staged)
    params = [t for k, t in model.named_weights() if "moving_" not in k]
    yt = torch.from_numpy(y)
    epochs = []
    n_epochs, k = (60, 10) if kind == "DeepFM-reg" else (12, 1)      # (dropout on 70 rows: the epoch loss is noisy — averages of ten)
    for epoch in range(n_epochs):
        tot = 0.0
        for lo in range(0, FIT_ROWS, FIT_BATCH):
            hi = min(FIT_ROWS, lo + FIT_BATCH)
            for t in params:
                t.requires_grad_(True)
            try:
                model._begin()
                logit = training.model_logits(model, staged, lo, hi, training=True)
                loss = torch.nn.functional.binary_cross_entropy_with_logits(logit, yt[lo:hi])
                grads = torch.autograd.grad(loss, params, allow_unused=True)
            finally:
                for t in params:
                    t.requires_grad_(False)
            assert bool(torch.isfinite(loss)) and all(g is None or bool(torch.isfinite(g).all()) for g in grads), (kind, name)
            with torch.no_grad():
                for t, g in zip(params, grads):
                    if g is not None:
                        t.sub_(FIT_LR * g)
            tot += float(loss.detach()) * (hi - lo)
            p = torch.sigmoid(logit.detach())
            if epoch == 0 and (name, kind) != ("exponential", "DeepFM-reg"):
                assert float(p.min()) > 1e-3 and float(p.max()) < 1 - 1e-3, "a row saturates"
        epochs.append(tot / FIT_ROWS)
    assert np.mean(epochs[-k:]) < np.mean(epochs[:k]), (kind, name, epochs)


# ---- 5. C ABI, no launch ------------------------------------------------------------------------------------------------------------
def _mlp_args(act, **kw):
    from deepctr_amd import _C
    units = (ctypes.c_int32 * 2)(24, 8)
    ptrs = (ctypes.c_void_p * 2)(4096, 8192)
    base = dict(x=4096, batch=33, x_stride=20, in_dim=20, n_layers=2, units=ctypes.cast(units, ctypes.c_void_p),
                kernels=ctypes.cast(ptrs, ctypes.c_void_p), biases=ctypes.cast(ptrs, ctypes.c_void_p), activation=act, y=4096, y_stride=8)
    base.update(kw)
    return _C.MlpArgs(**base), (units, ptrs)


def test_the_dnn_entry_points_take_the_new_codes():
    from deepctr_amd import _C
    lib = _C.lib()
    for act in range(5, 13):
        for tile in (0, 16, 32, 64):
            a, keep = _mlp_args(act, tile_rows=tile)
            assert lib.dctr_mlp_fwd_supported(None, ctypes.byref(a), 0, 0) == 1, (act, tile, lib.dctr_last_error())
        a, keep = _mlp_args(act)
        assert lib.dctr_mlp_workspace_bytes(ctypes.byref(a)) == 0
        wide_units = (ctypes.c_int32 * 1)(1300)
        a, keep = _mlp_args(act, n_layers=1, units=ctypes.cast(wide_units, ctypes.c_void_p), batch=65)
        assert lib.dctr_mlp_workspace_bytes(ctypes.byref(a)) == 2 * 128 * 1300 * 4            # the layered route
        a.workspace, a.workspace_bytes = 4096, 2 * 128 * 1300 * 4
        assert lib.dctr_mlp_fwd_supported(None, ctypes.byref(a), 0, 0) == 1
    for act in (13, -1, 64, 65):
        a, keep = _mlp_args(act)
        assert lib.dctr_mlp_fwd_supported(None, ctypes.byref(a), 0, 0) == 0 and b"activation" in lib.dctr_last_error()
        assert lib.dctr_mlp_fwd(ctypes.byref(a), None) == -4                                  # DCTR_E_ENUM, before any launch
    # dctr_dnn_train_layer_*: the argument checks, then an empty batch returns
    for fn in (lib.dctr_dnn_train_layer_fwd, lib.dctr_dnn_train_layer_bwd):
        for act in list(range(0, 4)) + list(range(5, 13)):
            assert fn(ctypes.byref(_C.DnnTrainLayer(z=4096, z_stride=8, rows=0, n=8, activation=act)), None) == 0, act
        for act in (4, 13, -1):
            assert fn(ctypes.byref(_C.DnnTrainLayer(z=4096, z_stride=8, rows=0, n=8, activation=act)), None) == -4, act
    # dctr_mlp_bwd: past the activation check, the next one (no workspace) answers; code 13 stops at the activation
    units = (ctypes.c_int32 * 2)(24, 8)
    ptrs = ctypes.cast((ctypes.c_void_p * 2)(4096, 8192), ctypes.c_void_p)
    bwd = lambda act: _C.MlpBwdArgs(x=4096, batch=33, x_stride=20, in_dim=20, n_layers=2, units=ctypes.cast(units, ctypes.c_void_p), kernels=ptrs,   # noqa: E731
                                    acts=ptrs, activation=act, head_w=4096, dlogit=4096, d_kernels=ptrs, d_biases=ptrs, d_head_w=4096)
    from tests import ref_mlp_bwd as RM
    for act in range(5, 13):
        a = bwd(act)
        assert lib.dctr_mlp_bwd(ctypes.byref(a), None) == -1 and b"workspace" in lib.dctr_last_error(), act
        # swish / gelu keep a third buffer for the pre-activations (the layered form, as Dice without its 2 x widest column sums)
        want = 4 * ((3 * 33 * 24 + 3) // 4 * 4) if act in (11, 12) else RM.workspace_bytes(33, [20, 24, 8])
        assert lib.dctr_mlp_bwd_workspace_bytes(ctypes.byref(a)) == want, act
    assert lib.dctr_mlp_bwd(ctypes.byref(bwd(13)), None) == -5 and b"no backward" in lib.dctr_last_error()


def test_the_other_families_refuse_code_5():
    from deepctr_amd import _C
    from tests.test_edcn_cpu import _abi_args as edcn_args
    from tests.test_mtl_cpu import _abi_args as mtl_args
    lib = _C.lib()
    ptrs = (ctypes.c_void_p * 4)(16, 16, 16, 16)
    arr = ctypes.cast(ptrs, ctypes.c_void_p)
    # EDCN's tower
    full = dict(x=16, gates=arr, cross_w=arr, cross_b=arr, dnn_w=arr, dnn_b=arr, head_w=16, logit=16)
    assert lib.dctr_edcn_fwd(ctypes.byref(edcn_args(**dict(full, activation=5))), None) == -4
    assert lib.dctr_edcn_fwd(ctypes.byref(edcn_args(**dict(full, bridge_activation=12))), None) == -4
    # the multi-task level kernel
    a, keep = mtl_args(0, x=16, expert_w=arr, expert_b=arr, gate_kernel=arr, out=16, out_stride=6)
    assert lib.dctr_mtl_level_fwd(ctypes.byref(a), None) == 0
    a.activation = 5
    assert lib.dctr_mtl_level_fwd(ctypes.byref(a), None) == -4 and b"unknown activation" in lib.dctr_last_error()
    # DIN's attention
    units = (ctypes.c_int32 * 2)(4, 2)
    d = _C.DinAttnArgs(query=16, keys=16, key_mask=16, batch=3, maxlen=4, dim=4, n_layers=2, activation=2, units=ctypes.cast(units, ctypes.c_void_p),
                       kernels=arr, biases=arr, out_kernel=16, out_bias=16, out=16, out_stride=4)
    d.activation = 5
    assert lib.dctr_din_attn_pool_fwd(ctypes.byref(d), None) == -4 and b"activation 5" in lib.dctr_last_error()
    # CIN
    ls = (ctypes.c_int32 * 1)(4)
    c = _C.CinArgs(x=16, batch=2, x_stride=12, fields=3, dim=4, n_layers=1, split_half=0, activation=5, layer_size=ctypes.cast(ls, ctypes.c_void_p),
                   filters=arr, bias=arr, out=16)
    assert lib.dctr_cin_fwd(ctypes.byref(c), None) == -4 and b"activation 5" in lib.dctr_last_error()
