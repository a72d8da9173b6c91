"""CPU: EDCN / BridgeModule / RegulationModule — the NumPy oracle (tests/ref_edcn.py) against the reference's own outputs
(tests/golden/model_edcn_*.npz, edcn_layer.npz; scripts/make_golden_edcn.py), what the fixtures can see, the float32-vs-float64 run that
sets the bar of the GPU tower tests, the torch restatement the training path uses, the API contract, and the argument checks of the ops
and of the C ABI (no launch)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import ref_edcn as RE
from tests.spec import columns_from_spec
from tests.test_autoint_cpu import att_rows
from tests.util import assert_close, assert_close_terms, golden_meta, load_golden

FIXTURES = ["model_edcn_%s_%s" % (b, p) for b in ("add", "had", "cat", "att") for p in ("vec", "mat")] + [
    "model_edcn_c1", "model_edcn_tau2", "model_edcn_regression", "model_edcn_bn", "model_edcn_nolin", "model_edcn_hash", "model_edcn_nomax"]
REG_TAGS = ["reg_3_4", "reg_9_4"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUSED_BRIDGES = ("pointwise_addition", "hadamard_product", "concatenation")

# (F, d, cross_num, B): the smallest shapes at which the tower kernel can still go wrong
SWEEP = [
    (1, 1, 1, 5),           # minimal, D = 1
    (2, 3, 2, 17),          # D = 6, scalar loads
    (3, 4, 1, 65),          # one full tile plus one row
    (9, 4, 3, 33),          # the fixtures' shape
    (5, 17, 2, 40),         # odd D = 85
    (26, 16, 2, 130),       # Criteo, ragged last tile
    (39, 16, 4, 20),        # D = 624, near the LDS limit
    (64, 16, 2, 19),        # D = 1024: the layered route
]


def build_model(meta, device, **more):
    from deepctr_amd import models
    kw = dict(meta["kwargs"])
    kw.update(more)
    return models.EDCN(columns_from_spec(meta["linear"]), columns_from_spec(meta["dnn"]), device=device, **kw)


def _has_hash(meta):
    return any(d.get("use_hash") or d.get("sparsefeat", {}).get("use_hash") for d in meta["dnn"] + meta["linear"])


def _feed(g):
    return {k[5:]: v for k, v in g.items() if k.startswith("feed/")}


def tower_case(F, d, L, B, bridge_type, parameterization, off, tau, seed, bn=False, dice=False):
    """Seeded operands of ops.edcn / RE.tower_op as NumPy arrays: gates N(0, 1), kernels scaled by 1 / sqrt(fan-in)."""
    rng = np.random.RandomState(seed)
    D = F * d
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)       # noqa: E731
    # (trailing columns; a slice at a multiple of 4 floats sits in rows of a multiple of 4 floats, as dnn_in does)
    case = dict(xbuf=f32(rng.standard_normal((B, off + D + (5 if off % 4 else 8 - D % 4))) * 0.5),
                gates=[f32(rng.standard_normal((1, F, 1))) for _ in range(2 * L)],
                cross_kernels=[f32(rng.standard_normal((D, 1) if parameterization == "vector" else (D, D)) / np.sqrt(D)) for _ in range(L)],
                cross_biases=[f32(rng.standard_normal((D, 1)) * 0.1) for _ in range(L)],
                dnn_kernels=[f32(rng.standard_normal((D, D)) / np.sqrt(D)) for _ in range(L)],
                dnn_biases=[f32(rng.standard_normal(D) * 0.1) for _ in range(L)],
                head=f32(rng.standard_normal((3 * D, 1))), add=f32(rng.standard_normal(B)), bias=f32(rng.standard_normal(1)),
                bridge_weights=None, bn=None, dice=None, tau=tau, off=off)
    if bridge_type == "concatenation":
        case["bridge_weights"] = [(f32(rng.standard_normal((2 * D, D)) / np.sqrt(2 * D)), f32(rng.standard_normal(D) * 0.1)) for _ in range(L)]
    elif bridge_type == "attention_pooling":
        case["bridge_weights"] = [tuple((f32(rng.standard_normal((D, D)) / np.sqrt(D)), f32(rng.standard_normal(D) * 0.1),
                                         f32(rng.standard_normal((D, D)) / np.sqrt(D)), f32(rng.standard_normal(D) * 0.1)) for _ in range(2))
                                  for _ in range(L)]
    if bn:
        case["bn"] = [(f32(1.0 + 0.2 * rng.standard_normal(D)), f32(0.1 * rng.standard_normal(D))) for _ in range(L)]
    if dice:
        case["dice"] = [(f32(0.3 * rng.standard_normal(D)), f32(0.1 * rng.standard_normal(D)), f32(rng.uniform(0.5, 1.5, D))) for _ in range(L)]
    return case


def ref_tower(case, F, d, bridge_type, parameterization, activation="relu", head=True, extras=True, **kw):
    return RE.tower_op(case["xbuf"], F, d, case["gates"], case["cross_kernels"], case["cross_biases"], case["dnn_kernels"], case["dnn_biases"],
                       bridge_type=bridge_type, parameterization=parameterization, tau=case["tau"], activation=activation, bn=case["bn"],
                       dice_params=case["dice"], bridge_weights=case["bridge_weights"], x_offset=case["off"],
                       head_w=case["head"] if head else None, add=[case["add"]] if head and extras else (),
                       global_bias=case["bias"] if head and extras else None, **kw)


def _miss(y, ref):
    """Per row: off the fixture by more than the probability bar of check_probs (1e-4 relative + 1e-6)."""
    y, ref = np.asarray(y, dtype=np.float64).reshape(-1), np.asarray(ref, dtype=np.float64).reshape(-1)
    return np.abs(y - ref) > 1e-4 * np.abs(ref) + 1e-6


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_matches_reference_code(name):
    from tests.test_gpu_models import check_probs
    g = load_golden(name)
    meta = golden_meta(g)
    assert meta["model"] == "EDCN"
    n = g["y"].shape[0]
    rows = att_rows(meta, _feed(g), n)
    assert rows.sum() >= 0.5 * n                   # at least half of the rows carry no all-padding max-pooled sequence
    y, ref = RE.run_fixture(g), g["y"]
    assert y.shape == ref.shape == (n, 1)
    check_probs(y.astype(np.float32), ref, name, rows)
    if meta["kwargs"].get("task") != "regression":
        assert ((ref[rows] > 1e-3) & (ref[rows] < 1 - 1e-3)).all()         # none of the compared rows is saturated
    assert_close(RE.run_fixture(g, np.float64)[rows], ref[rows], rtol=1e-4, atol=1e-6, what=name + " float64 prob")


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_sees_the_tower(name):
    """A tower with the WRONG bridge, and one whose head rows are zeroed, each miss the fixture on at least half of the kept rows."""
    g = load_golden(name)
    meta = golden_meta(g)
    rows = att_rows(meta, _feed(g), g["y"].shape[0])
    wrong = "hadamard_product" if meta["kwargs"]["bridge_type"] == "pointwise_addition" else "pointwise_addition"
    y = RE.run_fixture(g, np.float64, compute_bridge=wrong)
    assert _miss(y[rows], g["y"][rows]).sum() >= 0.5 * rows.sum(), "blind to the bridge"
    w = {k[2:]: v for k, v in g.items() if k.startswith("w/")}
    head = [k for k in w if re.match(r"dense(_\d+)?/kernel$", k) and w[k].shape[1] == 1]
    assert len(head) == 1
    w[head[0]] = np.zeros_like(w[head[0]])
    y = RE.run_fixture(g, np.float64, weights=w)
    assert _miss(y[rows], g["y"][rows]).sum() >= 0.5 * rows.sum(), "blind to the tower"


def test_fixtures_cover_what_they_are_for():
    kw = lambda name: golden_meta(load_golden(name))["kwargs"]      # noqa: E731
    seen = set((kw(n)["bridge_type"], kw(n)["cross_parameterization"]) for n in FIXTURES[:8])
    assert seen == set((b, p) for b in RE.BRIDGES for p in ("vector", "matrix"))
    assert all(kw(n)["cross_num"] == 3 and kw(n)["tau"] == 0.5 for n in FIXTURES[:8])
    assert kw("model_edcn_c1")["cross_num"] == 1 and kw("model_edcn_tau2")["tau"] == 2.0
    assert kw("model_edcn_regression")["task"] == "regression" and kw("model_edcn_bn")["dnn_use_bn"] is True
    assert golden_meta(load_golden("model_edcn_nolin"))["linear"] == []
    assert _has_hash(golden_meta(load_golden("model_edcn_hash")))
    nomax = golden_meta(load_golden("model_edcn_nomax"))
    assert not any(d["type"] == "varlen" and d["combiner"] == "max" for d in nomax["dnn"])
    for name in FIXTURES:
        meta = golden_meta(load_golden(name))
        assert not any(d["type"] == "dense" for d in meta["dnn"] + meta["linear"])
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) < 359 * 1024
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "edcn_layer.npz")) < 359 * 1024


@pytest.mark.parametrize("tag", REG_TAGS)
def test_regulation_oracle_matches_reference_code_and_uniform_gates_miss(tag):
    g = load_golden("edcn_layer")
    x, w, tau, y = g[tag + "/x"], g[tag + "/g"], float(g[tag + "/tau"]), g[tag + "/y"]
    F, d = x.shape[1:]
    assert w.shape == (1, F, 1) and y.shape == (x.shape[0], F * d)
    mag = np.abs(x.astype(np.float64)).reshape(x.shape[0], -1) * np.repeat(RE.gate(w, tau), d)[None, :]
    for dt in (np.float32, np.float64):
        assert_close_terms(RE.regulation(x, w, tau, dt), y, mag, what="RegulationModule " + tag)
    uni = RE.regulation(x, w, tau, uniform=True)
    assert (np.abs(uni - y) > 1e-4 * np.abs(y) + 2e-6 * mag).mean() > 0.5


@pytest.mark.parametrize("bridge_type", RE.BRIDGES)
def test_bridge_oracle_matches_reference_code(bridge_type):
    x, h, w, y = bridge_case(load_golden("edcn_layer"), bridge_type)
    assert y.shape == x.shape == h.shape == (6, 12)
    mag = RE.bridge(x, h, bridge_type, w, absolute=True)
    for dt in (np.float32, np.float64):
        assert_close_terms(RE.bridge(x, h, bridge_type, w, dtype=dt), y, mag, what="BridgeModule " + bridge_type)
    other = RE.bridge(x, h, "hadamard_product" if bridge_type != "hadamard_product" else "pointwise_addition")
    assert (np.abs(other - y) > 1e-4 * np.abs(y) + 2e-6 * mag).mean() > 0.5


def bridge_case(g, bridge_type):
    """(x, h, the weights as RE.bridge / ops take them, y) of one bridge type of edcn_layer.npz."""
    tag = "bridge_" + bridge_type
    w = {k[len(tag) + 3:]: v for k, v in g.items() if k.startswith(tag + "/w/")}
    weights = None
    if bridge_type == "concatenation":
        assert sorted(w) == ["dense/bias", "dense/kernel"] and w["dense/kernel"].shape == (24, 12)
        weights = (w["dense/kernel"], w["dense/bias"])
    elif bridge_type == "attention_pooling":
        assert sorted(w) == sorted("%s/%s" % (n, k) for n in ("dnn", "dnn_1") for k in ("kernel0", "bias0", "kernel1", "bias1"))
        weights = tuple(tuple(w["%s/%s" % (n, k)] for k in ("kernel0", "bias0", "kernel1", "bias1")) for n in ("dnn", "dnn_1"))
    else:
        assert not w
    return g[tag + "/x"], g[tag + "/h"], weights, g[tag + "/y"]


def test_float32_tower_against_float64_sets_the_bar():
    """The float32 NumPy run of the tower against its float64 run over the sweep of the GPU tests: the worst error in units of the
    summed magnitude (4.46e-7 when the bar was set), times two (the MFMA tile sums k in another order) and rounded up to one digit, is
    RE.TOWER_RTOL_TERMS.  Asserted here with room for another BLAS: the float32 run passes the bar, and the bar is within 4x of it."""
    worst = 0.0
    for F, d, L, B in SWEEP:
        for bridge_type in FUSED_BRIDGES:
            for par in ("vector", "matrix"):
                for off in (3, 4):
                    for act, bn in (("relu", False), ("linear", True)):
                        case = tower_case(F, d, L, B, bridge_type, par, off, (0.5, 2.0)[(F + off) % 2], F * 100 + d + off, bn=bn)
                        l64, o64 = ref_tower(case, F, d, bridge_type, par, act)
                        l32, o32 = ref_tower(case, F, d, bridge_type, par, act, dtype=np.float32)
                        lm, om = ref_tower(case, F, d, bridge_type, par, act, absolute=True)
                        worst = max(worst, float((np.abs(o32 - o64) / om).max()), float((np.abs(l32 - l64) / lm).max()))
    print("float32 vs float64 tower: worst error / summed magnitude = %.3g" % worst)
    assert worst <= RE.TOWER_RTOL_TERMS <= 4 * worst, worst


def test_magnitude_mode_bounds_the_plain_run():
    case = tower_case(3, 4, 2, 7, "concatenation", "matrix", 3, 0.5, 11)
    l, o = ref_tower(case, 3, 4, "concatenation", "matrix")
    lm, om = ref_tower(case, 3, 4, "concatenation", "matrix", absolute=True)
    assert (om >= np.abs(o)).all() and (lm >= np.abs(l)).all()
    la, _ = ref_tower(case, 3, 4, "concatenation", "matrix", extras=False)
    assert np.allclose(l - la, case["add"].astype(np.float64) + float(case["bias"][0]))


@pytest.mark.parametrize("name", FIXTURES)
def test_torch_restatement_matches_oracle(name):
    from deepctr_amd import engine, training
    g = load_golden(name)
    meta = golden_meta(g)
    if _has_hash(meta):
        pytest.skip("integer Hash runs inside the HIP gather kernel; the GPU suite covers this fixture")
    model = build_model(meta, torch.device("cpu"))
    model.set_weights_by_name({k[2:]: v for k, v in g.items() if k.startswith("w/")})
    feed = _feed(g)
    n = g["y"].shape[0]
    staged = engine.Staged(n)
    model._stage_inputs(feed, staged)
    model._begin()
    with torch.no_grad():
        logit = training.model_logits(model, staged, 0, n).numpy().astype(np.float64).reshape(-1)
    ref = RE.run_fixture(g, np.float64, task="regression").reshape(-1)
    rows = att_rows(meta, feed, n)
    assert_close(logit[rows], ref[rows], rtol=1e-4, atol=2e-5, what=name + " model_logits")


def test_the_gates_and_the_bridge_are_differentiable():
    from deepctr_amd import engine, training
    g = load_golden("model_edcn_nomax")             # (no -1e9 rows of an all-padding max-pooled sequence in the sum)
    model = build_model(golden_meta(g), torch.device("cpu"))
    model.set_weights_by_name({k[2:]: v for k, v in g.items() if k.startswith("w/")})
    leaves = [r.g for r in model.regulations] + [model.bridges[0].dense.w("kernel")]
    for t in leaves:
        t.requires_grad_(True)
    n = g["y"].shape[0]
    staged = engine.Staged(n)
    model._stage_inputs(_feed(g), staged)
    model._begin()
    training.model_logits(model, staged, 0, n).sum().backward()
    assert all(t.grad is not None and 0 < float(t.grad.abs().max()) < float("inf") for t in leaves)


def test_signature_defaults_match_the_reference():
    from deepctr_amd.layers import BridgeModule, RegulationModule
    from deepctr_amd.models import EDCN
    params = inspect.signature(EDCN).parameters
    want = dict(cross_num=2, cross_parameterization='vector', bridge_type='concatenation', tau=1.0, l2_reg_linear=1e-5, l2_reg_embedding=1e-5,
                l2_reg_cross=1e-5, l2_reg_dnn=0, seed=1024, dnn_dropout=0, dnn_use_bn=False, dnn_activation='relu', task='binary', device=None)
    assert list(params) == ["linear_feature_columns", "dnn_feature_columns"] + list(want)
    for k, v in want.items():
        assert params[k].default == v, k
    bp = inspect.signature(BridgeModule.__init__).parameters
    assert [(k, bp[k].default) for k in ("bridge_type", "activation")] == [("bridge_type", "hadamard_product"), ("activation", "relu")]
    assert inspect.signature(RegulationModule.__init__).parameters["tau"].default == 1.0


def test_construction_errors():
    from deepctr_amd.feature_column import DenseFeat, SparseFeat, VarLenSparseFeat
    from deepctr_amd.layers import BridgeModule, RegulationModule
    from deepctr_amd.models import EDCN
    cols = [SparseFeat("a", 5, 4), SparseFeat("b", 5, 4)]
    with pytest.raises(ValueError, match="Cross layer num must > 0"):
        EDCN(cols, cols, cross_num=0, device="cpu")
    with pytest.raises(ValueError, match="RegulationModule tau can not be zero"):
        EDCN(cols, cols, tau=0, device="cpu")
    with pytest.raises(ValueError, match="bridge_type"):
        EDCN(cols, cols, bridge_type="sum", device="cpu")
    mixed = [SparseFeat("a", 5, 4), VarLenSparseFeat(SparseFeat("s", 6, 8), maxlen=3)]
    with pytest.raises(ValueError, match=r"embedding_dim, got \[4, 8\]"):
        EDCN(mixed, mixed, device="cpu")
    with pytest.raises(ValueError, match="DenseFeat is not supported in dnn_feature_columns"):
        EDCN(cols, cols + [DenseFeat("c", 1)], device="cpu")
    with pytest.raises(ValueError, match=r"linear columns \['z'\] are not among them"):       # (the reference: KeyError)
        EDCN(cols + [SparseFeat("z", 3, 4)], cols, device="cpu")
    with pytest.raises(ValueError, match="parameterization should be 'vector' or 'matrix'"):
        EDCN(cols, cols, cross_parameterization="tensor", device="cpu")
    with pytest.raises(ValueError, match="tau can not be zero"):
        RegulationModule(0)
    with pytest.raises(ValueError, match="expect to be 3 dimensions"):
        RegulationModule(device="cpu").build((None, 12))
    with pytest.raises(ValueError, match="on a list of 2 inputs"):
        BridgeModule(device="cpu").build((None, 12))
    m = EDCN([], cols, cross_num=1, device="cpu")                                           # an empty linear list is fine
    assert tuple(m.dense.w("kernel").shape) == (24, 1)


def test_layer_contract():
    from deepctr_amd.layers import BridgeModule, RegulationModule, custom_objects
    assert custom_objects["BridgeModule"] is BridgeModule and custom_objects["RegulationModule"] is RegulationModule
    r = RegulationModule(0.5, device="cpu")
    r.build((None, 3, 4))
    assert r.name.startswith("regulation_module")
    assert [(n, tuple(t.shape)) for n, t in r.named_weights()] == [("%s/%s_field_weight" % (r.name, r.name), (1, 3, 1))]
    assert torch.equal(r.g, torch.ones(1, 3, 1)) and r.tau == 2.0 and r.get_config()["tau"] == 2.0     # (the reciprocal, as the reference)
    assert r.compute_output_shape((None, 3, 4)) == (None, 12)
    for bt, n_w in (("pointwise_addition", 0), ("hadamard_product", 0), ("concatenation", 2), ("attention_pooling", 8)):
        b = BridgeModule(bt, device="cpu")
        b.build([(None, 12), (None, 12)])
        assert len(b.named_weights()) == n_w and b.compute_output_shape([(None, 12)] * 2) == (None, 12)
        assert {k: b.get_config()[k] for k in ("bridge_type", "activation")} == dict(bridge_type=bt, activation="relu")
    cat = BridgeModule("concatenation", device="cpu")
    cat.build([(None, 5), (None, 5)])
    assert [(n.split("/")[1], tuple(t.shape)) for n, t in cat.named_weights()] == [("kernel", (10, 5)), ("bias", (5,))]


@pytest.mark.parametrize("name", FIXTURES)
def test_weight_names_and_shapes_match_the_fixture(name):
    g = load_golden(name)
    model = build_model(golden_meta(g), torch.device("cpu"))
    mine = {k: tuple(v.shape) for k, v in model.get_weights_by_name().items()}
    ref = {k[2:]: tuple(v.shape) for k, v in g.items() if k.startswith("w/") and not k.startswith("w/linearsparse_")}
    assert mine == ref


def test_reference_import_names():
    import deepctr
    import deepctr_amd.models
    from deepctr.layers import BridgeModule, RegulationModule
    from deepctr.layers.core import RegulationModule as R2
    from deepctr.layers.interaction import BridgeModule as B2
    from deepctr.models import EDCN
    from deepctr.models.edcn import EDCN as E2
    assert EDCN is deepctr_amd.models.EDCN is E2 is deepctr.models.EDCN is deepctr.models.edcn.EDCN
    assert BridgeModule is B2 is deepctr_amd.layers.BridgeModule and RegulationModule is R2 is deepctr_amd.layers.RegulationModule


def test_regularisers_and_training_route():
    from deepctr_amd import training, training_hip
    g = load_golden("model_edcn_cat_mat")
    model = build_model(golden_meta(g), "cpu", l2_reg_linear=0.1, l2_reg_embedding=0.2, l2_reg_dnn=0.3, l2_reg_cross=0.4)
    assert training_hip.supported(model) is False            # the tower has no HIP backward: fit() takes the autograd step
    names = {t.data_ptr(): n for n, t in model.named_weights()}
    got = sorted((names[t.data_ptr()], l2) for t, l2 in training.regularized_weights(model))
    tower_dnns = [dn.name for dn in model.dnn_layers]
    want = sorted([(n, 0.2) for n, _ in model.named_weights() if n.startswith("sparse_")] +
                  [(n, 0.1) for n, _ in model.named_weights() if n.startswith("linear")] +
                  [("%s/kernel0" % n, 0.3) for n in tower_dnns] + [("%s/kernel0" % c.name, 0.4) for c in model.cross_layers])
    assert got == want


def _cpu_case(bridge_type="concatenation", par="vector", **kw):
    case = tower_case(3, 4, 2, 5, bridge_type, par, 3, 0.5, 1, **kw)
    t = lambda a: torch.from_numpy(a)       # noqa: E731
    args = [t(case["xbuf"]), 3, 4, [t(a) for a in case["gates"]], [t(a) for a in case["cross_kernels"]], [t(a) for a in case["cross_biases"]],
            [t(a) for a in case["dnn_kernels"]], [t(a) for a in case["dnn_biases"]]]
    deep = lambda v: tuple(deep(e) for e in v) if isinstance(v, tuple) else t(v)       # noqa: E731
    kwargs = dict(bridge_type=bridge_type, parameterization=par, tau=0.5, x_offset=3, head_w=t(case["head"]),
                  bridge_weights=None if case["bridge_weights"] is None else [deep(bw) for bw in case["bridge_weights"]])
    return args, kwargs


def test_ops_operand_checks_raise_before_any_launch():
    from deepctr_amd import _C, ops
    args, kw = _cpu_case()

    def refused(match, exc=ValueError, a=None, **more):
        k = dict(kw)
        k.update(more)
        with pytest.raises(exc, match=match):
            ops.edcn(*(a or args), **k)

    refused("no CPU path", exc=_C.DctrExtensionError)                       # every operand passes: the device check is the last
    refused("x .* must be a float32", x_offset=9)                            # the columns end past the row
    refused("x .* must be a float32", a=[args[0].double()] + args[1:])
    refused("bridge_type 'sum'", bridge_type="sum")
    refused("parameterization should be", parameterization="tensor")
    refused("tau can not be zero", tau=0)
    refused("route 'fused'", route="fused")
    refused("unknown activation", activation="gelu")
    refused("2 rounds take 4 gates", a=args[:3] + [args[3][:3]] + args[4:])
    refused(r"gates\[1\] must be a contiguous float32 tensor of 3 elements", a=args[:3] + [[args[3][0], torch.zeros(4)] + args[3][2:]] + args[4:])
    refused(r"cross_kernels\[0\] must be a contiguous float32 tensor of 12 elements", a=args[:4] + [[torch.zeros(12, 12)] + args[4][1:]] + args[5:])
    refused(r"dnn_kernels\[1\] .* of 144 elements", a=args[:6] + [[args[6][0], torch.zeros(12, 11)]] + args[7:])
    refused(r"dnn_biases\[0\] .* of 12 elements", a=args[:7] + [[torch.zeros(13), args[7][1]]])
    refused("takes bridge_weights per round", bridge_weights=None)
    refused(r"bridge_weights\[0\] kernel .* of 288 elements", bridge_weights=[(torch.zeros(12, 12), torch.zeros(12))] * 2)
    refused("bn holds one entry", bn=[None])
    refused(r"bn\[1\] shift", bn=[None, (torch.ones(12), torch.ones(11))])
    refused("activation 'dice' takes dice", activation="dice")
    refused("head_w must be a contiguous float32 tensor of 36 elements", head_w=torch.zeros(24))
    refused("a logit needs head_w", head_w=None, logit=True)
    refused("need a logit output", head_w=None, out=True, sigmoid_out=True)
    refused("logit must be a contiguous float32 tensor of 5", logit=torch.zeros(6))
    refused("add must be a contiguous float32 tensor of 5", add=[torch.zeros(4)])
    refused("at most four logits", add=[torch.zeros(5)] * 5)
    refused("out must be a float32", out=torch.zeros(5, 36), out_offset=1)
    att_args, att_kw = _cpu_case("attention_pooling")
    with pytest.raises(ValueError, match=r"bridge_weights\[0\]"):
        ops.edcn(*att_args, **dict(att_kw, bridge_weights=[((torch.zeros(12, 12),) * 4,) * 2] * 2))
    # the two elementwise ops
    x3 = torch.zeros(5, 3, 4)
    with pytest.raises(_C.DctrExtensionError, match="no CPU path"):
        ops.edcn_regulate(x3, torch.ones(1, 3, 1), torch.ones(3))
    with pytest.raises(ValueError, match="g_deep must be a contiguous float32 tensor of 3"):
        ops.edcn_regulate(x3, torch.ones(4))
    with pytest.raises(ValueError, match="expect to be 3 dimensions"):
        ops.edcn_regulate(torch.zeros(5, 12), torch.ones(3))
    with pytest.raises(ValueError, match="tau can not be zero"):
        ops.edcn_regulate(x3, torch.ones(3), tau=0)
    with pytest.raises(ValueError, match="a cross output needs g_cross"):
        ops.edcn_regulate(x3, torch.ones(3), cross=torch.zeros(5, 12))
    with pytest.raises(ValueError, match="deep must be a float32"):
        ops.edcn_regulate(x3, torch.ones(3), deep=torch.zeros(5, 11))
    c, h = torch.zeros(5, 12), torch.zeros(5, 12)
    with pytest.raises(_C.DctrExtensionError, match="no CPU path"):
        ops.edcn_bridge(c, h, "hadamard_product")
    with pytest.raises(ValueError, match="no elementwise bridge"):
        ops.edcn_bridge(c, h, "concatenation")
    with pytest.raises(ValueError, match="h must be a float32"):
        ops.edcn_bridge(c, torch.zeros(5, 11), "pointwise_addition")
    with pytest.raises(ValueError, match="needs the scores ax and ah"):
        ops.edcn_bridge(c, h, "attention_pooling", ax=c)
    with pytest.raises(ValueError, match="ah must be a float32"):
        ops.edcn_bridge(c, h, "attention_pooling", ax=c, ah=torch.zeros(4, 12))


def test_routes_without_a_gpu():
    """The library answers what its LDS holds: four [16, pad16(D) + 4] tiles and the gates in 160 KiB."""
    from deepctr_amd import ops
    for F, d, L, _ in SWEEP[:-1]:
        for bt in FUSED_BRIDGES:
            for par in ("vector", "matrix"):
                assert ops.edcn_route(F, d, L, bt, par) == "fused", (F, d, bt, par)
                assert ops.edcn_route(F, d, L, bt, par, route="layered") == "layered"
        assert ops.edcn_route(F, d, L, "attention_pooling") == "layered"
        for act in ("dice", "sigmoid", "tanh"):
            assert ops.edcn_route(F, d, L, "hadamard_product", activation=act) == "layered"
        assert ops.edcn_route(F, d, L, "hadamard_product", activation="linear") == "fused"
        assert ops.edcn_route(F, d, L, "concatenation", bridge_activation="sigmoid") == "layered"
        assert ops.edcn_route(F, d, L, "hadamard_product", bridge_activation="sigmoid") == "fused"       # (no Dense in that bridge)
    assert ops.edcn_route(39, 16) == "fused" and ops.edcn_route(40, 16) == "layered"                     # D = 624 | 640
    assert ops.edcn_route(64, 16) == "layered" and ops.edcn_route(1, 1, 100) == "fused"
    with pytest.raises(ValueError):
        ops.edcn_route(3, 4, route="lds")
    with pytest.raises(ValueError):
        ops.edcn_route(3, 4, 0)


def _abi_args(**kw):
    from deepctr_amd import _C
    base = dict(batch=4, x_stride=15, x_offset=3, fields=3, dim=4, cross_num=2, mode=0, bridge=1, activation=1, bridge_activation=1, inv_tau=2.0)
    base.update(kw)
    return _C.edcn.Args(**base)


def test_abi_argument_errors_without_a_gpu():
    from deepctr_amd import _C
    lib = _C.lib()
    f = lambda a: lib.dctr_edcn_fwd(ctypes.byref(a), None)   # noqa: E731
    ptrs = (ctypes.c_void_p * 4)(16, 16, 16, 16)
    arr = ctypes.cast(ptrs, ctypes.c_void_p)
    full = dict(x=16, gates=arr, cross_w=arr, cross_b=arr, dnn_w=arr, dnn_b=arr, head_w=16, logit=16)
    assert lib.dctr_edcn_fwd(None, None) == -1 and lib.dctr_edcn_route(None) == -1
    assert f(_abi_args()) == -1                                      # pointers missing
    assert b"edcn" in lib.dctr_last_error()
    for k, v in (("fields", 0), ("dim", 0), ("cross_num", 0), ("batch", -1), ("x_stride", 14), ("x_offset", -1)):
        assert f(_abi_args(**dict(full, **{k: v}))) == -2, k
    for k, v in (("mode", 2), ("bridge", 4), ("activation", 5), ("bridge_activation", -1), ("route", 3), ("sigmoid_out", 2)):
        assert f(_abi_args(**dict(full, **{k: v}))) == -4, k
    assert f(_abi_args(**dict(full, inv_tau=float("inf")))) == -2
    for k in ("x", "gates", "cross_w", "cross_b", "dnn_w", "dnn_b", "head_w"):
        a = dict(full)
        del a[k]
        assert f(_abi_args(**a)) == -1, k
    assert f(_abi_args(**dict(full, logit=None))) == -1                                       # no output at all
    assert f(_abi_args(**dict(full, bridge=2))) == -1                                         # concatenation without its weights
    assert f(_abi_args(**dict(full, bn_scale=arr))) == -1                                     # scale without shift
    assert f(_abi_args(**dict(full, out=16, out_stride=35))) == -2                            # 3 D = 36 columns do not fit
    assert f(_abi_args(**dict(full, out=16, out_stride=38, out_offset=3))) == -2
    assert f(_abi_args(**dict(full, bridge=3))) == -5 and f(_abi_args(**dict(full, activation=4))) == -5   # the layered route's
    assert f(_abi_args(**dict(full, route=2))) == -5 and f(_abi_args(**dict(full, fields=64, dim=16, x_stride=1027))) == -5
    assert f(_abi_args(**dict(full, batch=0))) == 0                                           # empty batch: a no-op
    assert f(_abi_args(**dict(full, batch=0, out=16, out_stride=36, bridge=2, bridge_w=arr, bridge_b=arr))) == 0
    # more than 32 rounds chain launches through a workspace that carries br
    assert lib.dctr_edcn_workspace_bytes(ctypes.byref(_abi_args(cross_num=32))) == 0
    assert lib.dctr_edcn_workspace_bytes(ctypes.byref(_abi_args(cross_num=33))) == 4 * 12 * 4
    assert lib.dctr_edcn_workspace_bytes(ctypes.byref(_abi_args(cross_num=33, bridge=3))) == 0
    def reg(**kw):
        a = dict(x=16, x_stride=12, batch=0, fields=3, dim=4, g_deep=16, g_cross=None, inv_tau=1.0, deep=16, deep_stride=12, cross=None,
                 cross_stride=0, stream=None)
        a.update(kw)
        return lib.dctr_edcn_regulate(*[a[k] for k in ("x", "x_stride", "batch", "fields", "dim", "g_deep", "g_cross", "inv_tau", "deep",
                                                       "deep_stride", "cross", "cross_stride", "stream")])

    assert reg() == 0 and reg(deep=None) == -1 and reg(g_deep=None) == -1 and reg(cross=16, cross_stride=12) == -1
    assert reg(x_stride=11) == -2 and reg(deep_stride=11) == -2 and reg(fields=0) == -2 and reg(inv_tau=float("nan")) == -2
    def br(kind=0, **kw):
        a = dict(c=16, c_stride=12, h=16, h_stride=12, ax=None, ax_stride=0, ah=None, ah_stride=0, batch=0, dim=12, out=16, out_stride=12,
                 stream=None)
        a.update(kw)
        return lib.dctr_edcn_bridge(kind, *[a[k] for k in ("c", "c_stride", "h", "h_stride", "ax", "ax_stride", "ah", "ah_stride", "batch",
                                                           "dim", "out", "out_stride", "stream")])

    assert br() == 0 and br(1) == 0 and br(2) == -4 and br(3) == -1 and br(3, ax=16, ax_stride=12, ah=16, ah_stride=12) == 0
    assert br(h=None) == -1 and br(out_stride=11) == -2 and br(dim=0) == -2 and br(3, ax=16, ax_stride=11, ah=16, ah_stride=12) == -2


def test_header_declares_the_entry_points_and_the_mirror_matches_the_c_layout(tmp_path):
    import shutil
    import subprocess
    from deepctr_amd import _C
    header = open(os.path.join(ROOT, "include", "dctr.h")).read()
    assert "#define DCTR_ABI_VERSION 13" in header and _C.ABI_VERSION == 13              # no existing struct changed
    for sym in ("dctr_edcn_fwd", "dctr_edcn_route", "dctr_edcn_workspace_bytes"):
        assert re.search(r"\b(int|size_t) %s\(const dctr_edcn_args_t\* args" % sym, header), sym
    assert _C.SYMBOLS["dctr_edcn_fwd"] == (ctypes.c_int, [ctypes.POINTER(_C.edcn.Args), ctypes.c_void_p])
    assert "dctr_edcn_regulate" in _C.SYMBOLS and "dctr_edcn_bridge" in _C.SYMBOLS
    assert "edcn_kernels.hip" in __import__("deepctr_amd.build", fromlist=["SOURCES"]).SOURCES
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    cls, cname = _C.edcn.Args, "dctr_edcn_args_t"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dctr.h"', "int main(void) {",
             '    printf("enums %d %d %d %d %d %d %d\\n", DCTR_EDCN_BRIDGE_ADD, DCTR_EDCN_BRIDGE_HADAMARD, DCTR_EDCN_BRIDGE_CONCAT, '
             'DCTR_EDCN_BRIDGE_ATTENTION, DCTR_EDCN_ROUTE_AUTO, DCTR_EDCN_ROUTE_FUSED, DCTR_EDCN_ROUTE_LAYERED);',
             '    printf("sizeof %%zu\\n", sizeof(%s));' % cname]
    for fname, _ in cls._fields_:
        lines.append('    printf("%s %%zu\\n", offsetof(%s, %s));' % (fname, cname, fname))
    lines += ["    return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    seen = 0
    for line in filter(None, out):
        field, *vals = line.split()
        if field == "enums":
            e = _C.edcn
            assert [int(v) for v in vals] == [e.BRIDGE_ADD, e.BRIDGE_HADAMARD, e.BRIDGE_CONCAT, e.BRIDGE_ATTENTION, e.ROUTE_AUTO, e.ROUTE_FUSED,
                                              e.ROUTE_LAYERED]
            continue
        want = ctypes.sizeof(cls) if field == "sizeof" else getattr(cls, field).offset
        assert int(vals[0]) == want, "%s: C says %s, ctypes %d" % (field, vals[0], want)
        seen += 1
    assert seen == 1 + len(cls._fields_)
