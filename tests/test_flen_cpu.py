"""CPU: FLEN / FieldWiseBiInteraction — the NumPy oracle (tests/ref_flen.py) against the reference's own outputs
(tests/golden/model_flen*.npz, flen_layer.npz; scripts/make_golden_flen.py), the torch restatement the training path uses
(training.model_logits) against the oracle, its gradients against the closed forms, the API contract, and the C ABI's argument checks
(no launch)."""
import ctypes
import inspect
import itertools
import os
import re

import numpy as np
import pytest
import torch

from tests import ref_flen as RL
from tests.spec import columns_from_spec
from tests.test_autoint_cpu import att_rows
from tests.util import assert_close, golden_meta, load_golden, sigmoid_inv

FIXTURES = ["model_flen", "model_flen_hash", "model_flen_nomax", "model_flen_fixed", "model_flen_regression", "model_flen_bn",
            "model_flen_nodnn", "model_flen_denselin", "model_flen_avazu_sample"]
LAYER_TAGS = ["g2", "g3", "g4nb"]      # group sizes (1,1) d 4; (3,1,2) d 5; (2,2,1,3) d 8 without biases
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_model(meta, device, **more):
    from deepctr_amd import models
    kw = dict(meta["kwargs"])
    kw.update(more)
    return models.FLEN(columns_from_spec(meta["linear"]), columns_from_spec(meta["dnn"]), device=device, **kw)


def _has_hash(meta):
    return any(d.get("use_hash") or d.get("sparsefeat", {}).get("use_hash") for d in meta["dnn"] + meta["linear"])


def _feed(g):
    return {k[5:]: v for k, v in g.items() if k.startswith("feed/")}


def layer_case(g, tag):
    """(inputs, weights by short name, y, use_bias) of one tag of flen_layer.npz."""
    xs = [g["%s/x%d" % (tag, k)] for k in range(sum(1 for n in g if re.match(r"%s/x\d+$" % tag, n)))]
    w = {k.rsplit("/", 1)[1]: v for k, v in g.items() if k.startswith(tag + "/w/")}
    return xs, w, g[tag + "/y"], bool(g[tag + "/use_bias"])


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_matches_reference_code(name):
    g = load_golden(name)
    meta = golden_meta(g)
    assert meta["model"] == "FLEN"
    n = g["y"].shape[0]
    rows = att_rows(meta, _feed(g), n)
    assert rows.sum() >= 0.5 * n                   # at least half of the rows carry no all-padding max-pooled sequence
    y, ref = RL.run_fixture(g), g["y"]
    assert y.shape == ref.shape == (n, 1)
    y, ref = y[rows], ref[rows]
    assert_close(y, ref, rtol=1e-4, atol=1e-6, what=name + " prob")
    if meta["kwargs"].get("task") != "regression":
        assert ((ref > 1e-3) & (ref < 1 - 1e-3)).all()         # none of the compared rows is saturated
        assert_close(sigmoid_inv(y), sigmoid_inv(ref), rtol=1e-4, atol=2e-5, what=name + " logit")
    y64 = RL.run_fixture(g, np.float64)[rows]
    assert_close(y64, ref, rtol=1e-4, atol=1e-6, what=name + " float64 prob")


def test_fixtures_cover_what_they_are_for():
    groups = lambda name: [len(v) for v in _groups(golden_meta(load_golden(name))["dnn"]).values()]      # noqa: E731
    assert groups("model_flen") == [8, 1] and groups("model_flen_fixed") == [3, 2, 2]
    assert sorted(groups("model_flen_avazu_sample")) == [3, 6, 12]        # item, context, user of the example's field_info
    meta = golden_meta(load_golden("model_flen_avazu_sample"))
    assert [d["name"] for d in meta["linear"] if d["type"] == "dense"] == ["day"]
    assert golden_meta(load_golden("model_flen_nodnn"))["kwargs"]["dnn_hidden_units"] == []
    assert all(d["type"] == "dense" for d in golden_meta(load_golden("model_flen_denselin"))["linear"])
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "avazu_sample.txt")) == 15694
    for name in FIXTURES:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) < 359 * 1024


def _groups(spec):
    out = {}
    for d in spec:
        if d["type"] != "dense":
            out.setdefault((d.get("sparsefeat") or d).get("group_name", "default_group"), []).append(d)
    return out


@pytest.mark.parametrize("tag", LAYER_TAGS)
def test_layer_oracle_matches_reference_code(tag):
    xs, w, y, use_bias = layer_case(load_golden("flen_layer"), tag)
    G, d = len(xs), xs[0].shape[2]
    assert w["kernel_mf"].shape == (G * (G - 1) // 2, 1) and w["kernel_fm"].shape == (G, 1)
    assert (set(w) == {"kernel_mf", "kernel_fm", "bias_mf", "bias_fm"}) == use_bias
    if use_bias:
        assert w["bias_mf"].shape == w["bias_fm"].shape == (d,)
    for dt in (np.float32, np.float64):
        got = RL.fieldwise_layer(xs, w["kernel_mf"], w["kernel_fm"], w.get("bias_mf"), w.get("bias_fm"), dtype=dt)
        assert got.shape == y.shape == (xs[0].shape[0], d)
        assert_close(got, y, rtol=1e-4, atol=1e-5, what="FieldWiseBiInteraction " + tag)


def test_pair_order_and_magnitude_mode():
    """kernel_mf's rows meet the group pairs in itertools.combinations order; one field per group leaves no FM part; the magnitude
    mode bounds the plain result and does not cancel."""
    rng = np.random.RandomState(1)
    xs = [rng.standard_normal((3, 1, 2)) for _ in range(4)]
    assert RL.pairs(4) == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    for p, (i, j) in enumerate(RL.pairs(4)):
        w = np.zeros(6)
        w[p] = 2.0
        got = RL.fieldwise_layer(xs, w, np.full(4, 0.5))
        assert np.allclose(got, 2.0 * xs[i][:, 0] * xs[j][:, 0])
    x2 = [rng.standard_normal((3, 3, 2)) for _ in range(2)]
    y = RL.fieldwise_layer(x2, np.ones(1), np.full(2, 0.5), np.ones(2), -np.ones(2))
    mag = RL.fieldwise_layer(x2, np.ones(1), np.full(2, 0.5), np.ones(2), -np.ones(2), absolute=True)
    s = [np.abs(x).sum(1) for x in x2]
    want = s[0] * s[1] + 0.5 * sum(v * v + (x * x).sum(1) for v, x in zip(s, x2)) + 2.0
    assert np.allclose(mag, want) and (mag >= np.abs(y)).all()


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
    ref = RL.run_fixture(g, np.float64, task="regression").reshape(-1)
    rows = att_rows(meta, feed, n)
    assert rows.sum() >= n // 2
    assert_close(logit[rows], ref[rows], rtol=1e-4, atol=2e-5, what=name + " model_logits")


def test_signature_defaults_match_the_reference():
    from deepctr_amd.layers import FieldWiseBiInteraction
    from deepctr_amd.models import FLEN
    params = inspect.signature(FLEN).parameters
    want = dict(dnn_hidden_units=(256, 128, 64), l2_reg_linear=0.00001, l2_reg_embedding=0.00001, l2_reg_dnn=0, seed=1024, dnn_dropout=0.0,
                dnn_activation='relu', dnn_use_bn=False, task='binary', device=None)
    assert list(params) == ["linear_feature_columns", "dnn_feature_columns"] + list(want)
    for k, v in want.items():
        assert params[k].default == v, k
    lp = inspect.signature(FieldWiseBiInteraction.__init__).parameters
    assert [(k, lp[k].default) for k in ("use_bias", "seed")] == [("use_bias", True), ("seed", 1024)]


def test_construction_errors_match_the_reference():
    from deepctr_amd.feature_column import DenseFeat, SparseFeat, VarLenSparseFeat
    from deepctr_amd.layers import FieldWiseBiInteraction
    from deepctr_amd.models import FLEN
    one = [SparseFeat("a", 5, 4), SparseFeat("b", 5, 4), DenseFeat("c", 1)]
    with pytest.raises(ValueError, match="at least 2 inputs"):           # one embedding group
        FLEN(one, one, device="cpu")
    dense_group = [SparseFeat("a", 5, 4), DenseFeat("c", 1)]             # (DenseFeat carry no group: still one)
    with pytest.raises(ValueError, match="at least 2 inputs"):
        FLEN(dense_group, dense_group, device="cpu")
    mixed = [SparseFeat("a", 5, 4, group_name="u"), VarLenSparseFeat(SparseFeat("s", 6, 8, group_name="i"), maxlen=3)]
    with pytest.raises(ValueError, match=r"embedding_dim, got \[4, 8\]"):
        FLEN(mixed, mixed, device="cpu")
    two = [SparseFeat("a", 5, 4, group_name="u"), VarLenSparseFeat(SparseFeat("s", 6, 4, group_name="i"), maxlen=3), DenseFeat("c", 1)]
    m = FLEN(two, two, dnn_hidden_units=(), device="cpu")
    assert tuple(m.dense.w("kernel").shape) == (4 + 9, 1)                # without hidden units the DNN is the identity: H = in_dim
    with pytest.raises(ValueError, match="at least 2 inputs"):
        FieldWiseBiInteraction(device="cpu").build([(None, 3, 4)])
    with pytest.raises(ValueError, match="at least 2 inputs"):
        FieldWiseBiInteraction(device="cpu").build((None, 3, 4))
    layer = FieldWiseBiInteraction(device="cpu")
    layer.build([(None, 3, 4), (None, 1, 4)])
    with pytest.raises(ValueError, match="expect to be 3 dimensions"):
        layer.call([torch.zeros(2, 12), torch.zeros(2, 4)])


def test_layer_contract():
    from deepctr_amd.layers import FieldWiseBiInteraction, custom_objects
    assert custom_objects["FieldWiseBiInteraction"] is FieldWiseBiInteraction
    s = FieldWiseBiInteraction(device="cpu")
    s.build([(None, 3, 6), (None, 1, 6), (None, 2, 6)])
    assert s.name.startswith("field_wise_bi_interaction")
    assert [(n.rsplit("/", 1)[1], tuple(t.shape)) for n, t in s.named_weights()] == [
        ("kernel_mf", (3, 1)), ("kernel_fm", (3, 1)), ("bias_mf", (6,)), ("bias_fm", (6,))]
    assert torch.equal(s.w("kernel_mf"), torch.ones(3, 1)) and torch.equal(s.w("kernel_fm"), torch.full((3, 1), 0.5))
    assert not s.w("bias_mf").any() and not s.w("bias_fm").any()
    assert s.compute_output_shape([(None, 3, 6), (None, 1, 6), (None, 2, 6)]) == (None, 6)
    assert {k: s.get_config()[k] for k in ("use_bias", "seed")} == dict(use_bias=True, seed=1024)
    nb = FieldWiseBiInteraction(use_bias=False, seed=7, device="cpu")
    nb.build([(None, 1, 2), (None, 1, 2)])
    assert [n.rsplit("/", 1)[1] for n, _ in nb.named_weights()] == ["kernel_mf", "kernel_fm"]
    assert {k: nb.get_config()[k] for k in ("use_bias", "seed")} == dict(use_bias=False, seed=7)


@pytest.mark.parametrize("name", FIXTURES)
def test_weight_names_and_shapes_match_the_fixture(name):
    g = load_golden(name)
    model = build_model(golden_meta(g), torch.device("cpu"))
    mine = {k: tuple(v.shape) for k, v in model.get_weights_by_name().items()}
    ref = {k[2:]: tuple(v.shape) for k, v in g.items() if k.startswith("w/") and not k.startswith("w/linearsparse_")}
    assert mine == ref
    d = model.emb_dim
    assert ref["dense/kernel"][0] == d + (meta_last(golden_meta(g)) or model.stage_plan.in_dim)


def meta_last(meta):
    units = meta["kwargs"].get("dnn_hidden_units")
    return units[-1] if units else None


def test_reference_import_names():
    import deepctr
    import deepctr_amd.models
    from deepctr.layers import FieldWiseBiInteraction
    from deepctr.layers.interaction import FieldWiseBiInteraction as L2
    from deepctr.models import FLEN
    from deepctr.models.flen import FLEN as F2
    assert FLEN is deepctr_amd.models.FLEN is F2 is deepctr.models.FLEN is deepctr.models.flen.FLEN
    assert FieldWiseBiInteraction is L2 is deepctr_amd.layers.FieldWiseBiInteraction


def test_no_regulariser_reaches_the_layer_weights_or_the_head():
    from deepctr_amd import training
    g = load_golden("model_flen_fixed")
    model = build_model(golden_meta(g), "cpu", l2_reg_linear=0.1, l2_reg_embedding=0.2, l2_reg_dnn=0.3)
    names = {t.data_ptr(): n for n, t in model.named_weights()}
    got = sorted((names[t.data_ptr()], l2) for t, l2 in training.regularized_weights(model))
    want = sorted([(n, 0.2) for n, _ in model.named_weights() if n.startswith("sparse_")] +
                  [(n, 0.1) for n, _ in model.named_weights() if n.startswith("linear")] +
                  [(n, 0.3) for n, _ in model.named_weights() if n.startswith("dnn/kernel")])
    assert got == want


def test_autograd_step_gradients_match_the_closed_forms():
    """d kernel_mf[p] = sum dy s_i s_j, d kernel_fm[g] = sum dy (s_g^2 - q_g), d bias = sum_b dy, dy = dlogit * dense/kernel[:d],
    d dense/kernel[:d] = sum_b dlogit y — on a tiny FLEN without a DNN term in the way (the head's rows behind d are zeroed)."""
    from deepctr_amd import engine, training
    from deepctr_amd.feature_column import DenseFeat, SparseFeat
    from deepctr_amd.models import FLEN
    rng = np.random.RandomState(5)
    grp = ["u", "i", "u", "c"]
    cols = [SparseFeat("C%d" % k, 7, 3, group_name=grp[k]) for k in range(4)] + [DenseFeat("I0", 1)]
    n = 6
    feed = {"C%d" % k: rng.randint(0, 7, n).astype(np.int32) for k in range(4)}
    feed["I0"] = rng.rand(n).astype(np.float32)
    model = FLEN(cols, cols, dnn_hidden_units=(5,), device="cpu")
    w = {k: (rng.standard_normal(v.shape) * 0.4).astype(np.float32) for k, v in model.get_weights_by_name().items()}
    model.set_weights_by_name(w)
    layer = model.fieldwise
    leaves = [layer.w(k) for k in ("kernel_mf", "kernel_fm", "bias_mf", "bias_fm")] + [model.dense.w("kernel")]
    for t in leaves:
        t.requires_grad_(True)
    staged = engine.Staged(n)
    model._stage_inputs(feed, staged)
    model._begin()
    logit = training.model_logits(model, staged, 0, n)
    coef = torch.from_numpy(rng.standard_normal(n).astype(np.float32))
    (logit * coef).sum().backward()
    # closed forms in float64 from the embeddings themselves
    emb = lambda k: w["sparse_emb_C%d/embeddings" % k].astype(np.float64)[feed["C%d" % k]]       # noqa: E731
    xs = [np.stack([emb(0), emb(2)], 1), emb(1)[:, None], emb(3)[:, None]]                      # groups u, i, c in first-appearance order
    s = [x.sum(1) for x in xs]
    q = [(x * x).sum(1) for x in xs]
    head = w["dense/kernel"].astype(np.float64)[:3, 0]
    dy = coef.numpy().astype(np.float64)[:, None] * head[None, :]
    want_mf = np.array([(dy * s[i] * s[j]).sum() for i, j in itertools.combinations(range(3), 2)])
    want_fm = np.array([(dy * (s[g] ** 2 - q[g])).sum() for g in range(3)])
    y = RL.fieldwise_layer(xs, w["field_wise_bi_interaction/kernel_mf"], w["field_wise_bi_interaction/kernel_fm"],
                           w["field_wise_bi_interaction/bias_mf"], w["field_wise_bi_interaction/bias_fm"])
    got = [t.grad.numpy().astype(np.float64) for t in leaves]
    assert_close(got[0].reshape(-1), want_mf, rtol=1e-4, atol=1e-5, what="d kernel_mf")
    assert_close(got[1].reshape(-1), want_fm, rtol=1e-4, atol=1e-5, what="d kernel_fm")
    assert_close(got[2], dy.sum(0), rtol=1e-4, atol=1e-5, what="d bias_mf")
    assert_close(got[3], dy.sum(0), rtol=1e-4, atol=1e-5, what="d bias_fm")
    assert_close(got[4][:3, 0], (coef.numpy().astype(np.float64)[:, None] * y).sum(0), rtol=1e-4, atol=1e-5, what="d dense/kernel[:d]")


def test_hip_step_support_and_the_head_row_handle():
    """FLEN brings a HIP step: supported with a relu / BatchNorm + dropout / dice DNN, not without hidden units or with dice + dropout; the
    trainer's head handle is a view of dense/kernel's rows behind the field-wise vector's (one optimizer segment for the kernel)."""
    from deepctr_amd import training_hip
    g = load_golden("model_flen_fixed")
    meta = golden_meta(g)
    for kw, want in ((dict(), True), (dict(dnn_use_bn=True, dnn_dropout=0.3), True), (dict(dnn_activation="dice"), True),
                     (dict(dnn_hidden_units=()), False), (dict(dnn_activation="dice", dnn_dropout=0.3), False)):
        assert training_hip.supported(build_model(meta, "cpu", **kw)) == want, kw
    p = training_hip._Param(torch.arange(6, dtype=torch.float32).reshape(6, 1))
    rows = training_hip._ParamRows(p, 2, None)
    assert rows.w.data_ptr() == p.w.data_ptr() + 8 and rows.g.data_ptr() == p.g.data_ptr() + 8 and tuple(rows.w.shape) == (4, 1)
    rows.g.add_(1.0)
    assert p.g.reshape(-1).tolist() == [0, 0, 1, 1, 1, 1]


def _args(table=((0, 2), (6, 2)), **kw):
    from deepctr_amd import _C
    host = (_C.fieldwise.Group * len(table))()
    for i, (f, n) in enumerate(table):
        host[i].first, host[i].n_fields = f, n
    base = dict(batch=4, x_stride=12, x_offset=0, n_groups=len(table), dim=3, groups_host=ctypes.addressof(host))
    base.update(kw)
    a = _C.fieldwise.Args(**base)
    a._keep = host
    return a


def test_abi_argument_errors_without_a_gpu():
    from deepctr_amd import _C
    lib = _C.lib()
    f = lambda a: lib.dctr_fieldwise_fwd(ctypes.byref(a), None)   # noqa: E731
    full = dict(x=16, groups=16, kernel_mf=16, kernel_fm=16, y=16, y_stride=3)
    assert lib.dctr_fieldwise_fwd(None, None) == -1
    assert f(_args()) == -1                                          # pointers missing
    assert f(_args(table=((0, 4),), **full)) == -2                  # fewer than two groups
    assert f(_args(dim=0, **full)) == -2
    assert f(_args(x_stride=11, **full)) == -2                       # the second group ends past the row
    assert f(_args(x_offset=1, **full)) == -2
    assert f(_args(x_offset=-1, **full)) == -2
    assert f(_args(table=((0, 2), (6, 0)), **full)) == -2           # an empty group
    assert f(_args(table=((-3, 2), (6, 2)), **full)) == -2
    assert f(_args(route=7, **full)) == -4
    assert f(_args(batch=-1, **full)) == -2
    assert b"fieldwise" in lib.dctr_last_error()
    assert f(_args(y_stride=2, x=16, groups=16, kernel_mf=16, kernel_fm=16, y=16)) == -2
    for k in ("x", "groups", "kernel_mf", "kernel_fm"):
        a = dict(full)
        del a[k]
        assert f(_args(**a)) == -1, k
    assert f(_args(x=16, groups=16, kernel_mf=16, kernel_fm=16)) == -1                       # no output at all
    assert f(_args(x=16, groups=16, kernel_mf=16, kernel_fm=16, logit=16)) == -1             # a logit without head_w
    assert f(_args(add=16, **full)) == -1                                                     # add without a logit
    assert f(_args(batch=0, **full)) == 0                                                     # empty batch: a no-op
    assert f(_args(batch=0, x=16, groups=16, kernel_mf=16, kernel_fm=16, logit=16, head_w=16, add=16)) == 0
    # backward: exactly one upstream form, d_head_w with dlogit only
    b = _C.fieldwise.BwdArgs()
    fwd = _args(batch=0, **full)            # (kept: it owns the host group table b.fwd points at)
    b.fwd = fwd
    assert lib.dctr_fieldwise_bwd(ctypes.byref(b), None) == -1
    b.dy, b.dy_stride = 16, 3
    assert lib.dctr_fieldwise_bwd(ctypes.byref(b), None) == 0
    b.d_head_w = 16
    assert lib.dctr_fieldwise_bwd(ctypes.byref(b), None) == -1
    b.d_head_w, b.dy_stride = None, 2
    assert lib.dctr_fieldwise_bwd(ctypes.byref(b), None) == -2
    b.dy_stride, b.dlogit = 3, 16
    assert lib.dctr_fieldwise_bwd(ctypes.byref(b), None) == -1
    b.dy, b.accumulate = None, 2
    assert lib.dctr_fieldwise_bwd(ctypes.byref(b), None) == -4
    assert lib.dctr_fieldwise_bwd(None, None) == -1


def test_routes_without_a_gpu():
    """No shape is refused: the group sums wait in LDS up to 128 KiB per workgroup of 64 threads, beyond that they are re-read.  The
    backward keeps its accumulators there too and declines what does not fit (the model then trains on the autograd step)."""
    from deepctr_amd import ops
    ones = lambda G: [(k * 16, 1) for k in range(G)]      # noqa: E731
    for groups, d in (([(0, 13), (208, 5), (288, 3)], 16), ([(0, 1), (1, 1)], 1), ([(0, 1), (3, 3)], 3), ([(k * 1600, 50) for k in range(4)], 32),
                      (ones(21), 16), ([(0, 2), (128, 3)], 64)):
        assert ops.fieldwise_route(groups, d) == "on_chip", (groups, d)
        assert ops.fieldwise_route(groups, d, route="reread") == "reread"
        assert ops.fieldwise_bwd_supported(groups, d)
    assert ops.fieldwise_route(ones(128), 16) == "on_chip" and not ops.fieldwise_bwd_supported(ones(128), 16)      # (+ 8,128 pair sums)
    assert ops.fieldwise_route(ones(129), 16) == "reread"                              # 129 groups x 64 threads x 16 B > 128 KiB
    assert ops.fieldwise_route([(k * 3, 1) for k in range(512)], 3) == "on_chip"       # scalar columns: four times the groups
    assert ops.fieldwise_route([(k * 3, 1) for k in range(513)], 3) == "reread"
    assert ops.fieldwise_route([(k * 4, 1) for k in range(700)], 4) == "reread"
    assert not ops.fieldwise_bwd_supported(ones(129), 16) and not ops.fieldwise_bwd_supported([(k * 4, 1) for k in range(700)], 4)
    with pytest.raises(ValueError):
        ops.fieldwise_route(ones(3), 16, route="lds")


def test_header_declares_the_entry_points_and_the_mirrors_match_the_c_layout(tmp_path):
    import shutil
    import subprocess
    from deepctr_amd import _C
    header = open(os.path.join(ROOT, "include", "dctr.h")).read()
    assert "#define DCTR_ABI_VERSION 13" in header and _C.ABI_VERSION == 13
    for sym in ("dctr_fieldwise_fwd", "dctr_fieldwise_bwd", "dctr_fieldwise_route", "dctr_fieldwise_bwd_supported"):
        assert re.search(r"\bint %s\(const dctr_fieldwise_(bwd_)?args_t\* args" % sym, header), sym
        assert sym in _C.SYMBOLS and _C.SYMBOLS[sym][0] is ctypes.c_int
    assert _C.SYMBOLS["dctr_fieldwise_fwd"][1] == [ctypes.POINTER(_C.fieldwise.Args), ctypes.c_void_p]
    assert _C.SYMBOLS["dctr_fieldwise_bwd"][1] == [ctypes.POINTER(_C.fieldwise.BwdArgs), ctypes.c_void_p]
    assert "fieldwise_kernels.hip" in __import__("deepctr_amd.build", fromlist=["SOURCES"]).SOURCES
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    structs = (("dctr_fieldwise_group_t", _C.fieldwise.Group), ("dctr_fieldwise_args_t", _C.fieldwise.Args),
               ("dctr_fieldwise_bwd_args_t", _C.fieldwise.BwdArgs))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dctr.h"', "int main(void) {",
             '    printf("enums %d %d %d %d\\n", DCTR_FIELDWISE_ROUTE_AUTO, DCTR_FIELDWISE_ROUTE_ON_CHIP, DCTR_FIELDWISE_ROUTE_REREAD, '
             'DCTR_ABI_VERSION);']
    for cname, cls in structs:
        lines.append('    printf("%s.sizeof %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in cls._fields_:
            lines.append('    printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines += ["    return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    by_name = dict(structs)
    seen = 0
    for line in filter(None, out):
        field, *vals = line.split()
        if field == "enums":
            assert [int(v) for v in vals] == [_C.fieldwise.ROUTE_AUTO, _C.fieldwise.ROUTE_ON_CHIP, _C.fieldwise.ROUTE_REREAD, 13]
            continue
        cname, fname = field.split(".")
        cls = by_name[cname]
        want = ctypes.sizeof(cls) if fname == "sizeof" else getattr(cls, fname).offset
        assert int(vals[0]) == want, "%s: C says %s, ctypes %d" % (field, vals[0], want)
        seen += 1
    assert seen == sum(1 + len(cls._fields_) for _, cls in structs)
