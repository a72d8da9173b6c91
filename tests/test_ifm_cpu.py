"""CPU: IFM and DIFM — the NumPy oracle (tests/ref_ifm.py) against the reference's own outputs (tests/golden/model_ifm*.npz,
model_difm*.npz; scripts/make_golden_ifm.py), the torch restatement the training path uses (training.model_logits) against the oracle,
the API contract (signatures, weight names, input names, the pairing by position, the refusals), the ctypes mirrors' layout, the C
ABI's argument checks (no launch) and a CPU fit() on the autograd step."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from tests import ref_ifm as RI
from tests.spec import columns_from_spec
from tests.test_autoint_cpu import att_rows
from tests.util import assert_close, golden_meta, load_golden, sigmoid_inv

IFM_FIXTURES = ["model_ifm", "model_ifm_hash", "model_ifm_nomax", "model_ifm_fixed", "model_ifm_regression", "model_ifm_bn",
                "model_ifm_reorder", "model_ifm_denselin"]
DIFM_FIXTURES = ["model_difm", "model_difm_hash", "model_difm_nomax", "model_difm_fixed", "model_difm_regression", "model_difm_bn",
                 "model_difm_reorder", "model_difm_denselin", "model_difm_nores", "model_difm_h3"]
FIXTURES = IFM_FIXTURES + DIFM_FIXTURES


def build_model(meta, device, **more):
    from deepctr_amd import models
    kw = dict(meta["kwargs"])
    kw.update(more)
    return getattr(models, meta["model"])(columns_from_spec(meta["linear"]), columns_from_spec(meta["dnn"]), device=device, **kw)


def _has_hash(meta):
    return any(d.get("use_hash") or d.get("sparsefeat", {}).get("use_hash") for d in meta["dnn"] + meta["linear"])


def _feed(g):
    return {k[5:]: v for k, v in g.items() if k.startswith("feed/")}


def _weights(g):
    return {k[2:]: v for k, v in g.items() if k.startswith("w/")}


def kept_rows(meta, feed, n):
    """att_rows (an all-padding max-pooled sequence puts the reference's -1e9 embedding into the FM term), asserted to keep at least
    half of the fixture."""
    rows = att_rows(meta, feed, n)
    assert rows.sum() * 2 >= n
    return rows


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_matches_reference_code(name):
    g = load_golden(name)
    meta = golden_meta(g)
    assert meta["model"] == ("DIFM" if "difm" in name else "IFM")
    n = g["y"].shape[0]
    assert g["y"].shape == (n, 1)
    rows = kept_rows(meta, _feed(g), n)
    y, ref = RI.run_fixture(g), g["y"]
    assert y.shape == ref.shape
    y, ref = y[rows], ref[rows]
    if meta["kwargs"].get("task") != "regression":
        assert ((ref > 1e-3) & (ref < 1 - 1e-3)).all()         # none of the compared rows is saturated
    assert_close(y, ref, rtol=1e-4, atol=1e-6, what=name + " prob")
    if meta["kwargs"].get("task") != "regression":
        assert_close(sigmoid_inv(y), sigmoid_inv(ref), rtol=1e-4, atol=2e-5, what=name + " logit")
    y64 = RI.run_fixture(g, np.float64)[rows]
    assert_close(y64, ref, rtol=1e-4, atol=1e-6, what=name + " float64 prob")
    if meta["kwargs"].get("task") != "regression":
        assert_close(sigmoid_inv(y64), sigmoid_inv(ref), rtol=1e-4, atol=2e-5, what=name + " float64 logit")


def test_fixture_set_is_what_the_recipe_lists():
    names = lambda spec: [d.get("name") or d["sparsefeat"]["name"] for d in spec]     # noqa: E731
    g = load_golden("model_ifm")
    assert g["w/dense/kernel"].shape == (8, 9) and "w/dense_1/kernel" not in g                     # [H, F], no bias
    g = load_golden("model_difm")
    assert g["w/dense/kernel"].shape == (9 * 4 * 2, 9) and g["w/dense_1/kernel"].shape == (8, 9)   # [F d_att heads, F], [H, F]
    assert {k for k in g if k.startswith("w/interacting_layer/")} == {"w/interacting_layer/" + n for n in ("query", "key", "value", "res")}
    assert "w/interacting_layer/res" not in load_golden("model_difm_nores")
    assert load_golden("model_difm_h3")["w/interacting_layer/query"].shape == (4, 15)
    for tag in ("ifm", "difm"):
        meta = golden_meta(load_golden("model_%s_reorder" % tag))
        assert names(meta["linear"]) == names(meta["dnn"])[::-1]
        meta = golden_meta(load_golden("model_%s_denselin" % tag))
        assert all(d["type"] == "dense" for d in meta["linear"])
        meta = golden_meta(load_golden("model_%s_nomax" % tag))
        assert not [d for d in meta["dnn"] if d.get("combiner") == "max"]
        meta = golden_meta(load_golden("model_%s_fixed" % tag))
        assert not [d for d in meta["dnn"] if d["type"] == "varlen"]
        assert golden_meta(load_golden("model_%s_bn" % tag))["kwargs"]["dnn_use_bn"] is True


def test_reordered_linear_list_pairs_by_position_not_by_name():
    """The oracle pairs m[k] with the k-th first-order term; pairing by name instead would miss the reference's outputs."""
    g = load_golden("model_ifm_reorder")
    meta = golden_meta(g)
    rows = kept_rows(meta, _feed(g), 32)
    by_name = dict(meta, linear=[d for d in meta["dnn"]])                       # the deep list's order: each term under its own factor
    g2 = dict(g, meta=np.frombuffer(__import__("json").dumps(by_name).encode(), dtype=np.uint8))
    y = RI.run_fixture(g2, np.float64)[rows]
    assert np.abs(y - g["y"][rows]).max() > 1e-3


@pytest.mark.parametrize("name", FIXTURES)
def test_torch_restatement_matches_oracle(name):
    from deepctr_amd import engine, training
    g = load_golden(name)
    meta = golden_meta(g)
    if _has_hash(meta):
        pytest.skip("integer Hash runs in a HIP kernel; the GPU suite covers this fixture")
    model = build_model(meta, torch.device("cpu"))
    model.set_weights_by_name(_weights(g))
    feed = _feed(g)
    n = g["y"].shape[0]
    staged = engine.Staged(n)
    model._stage_inputs(feed, staged)
    model._begin()
    with torch.no_grad():
        logit = training.model_logits(model, staged, 0, n).numpy().astype(np.float64).reshape(-1)
    ref = RI.run_fixture(g, np.float64, task="regression").reshape(-1)
    rows = kept_rows(meta, feed, n)
    assert_close(logit[rows], ref[rows], rtol=1e-4, atol=2e-5, what=name + " model_logits")


def test_signature_defaults_match_the_reference():
    from deepctr_amd.models import DIFM, IFM
    common = dict(dnn_hidden_units=(256, 128, 64), l2_reg_linear=0.00001, l2_reg_embedding=0.00001, l2_reg_dnn=0, seed=1024, dnn_dropout=0,
                  dnn_activation='relu', dnn_use_bn=False, task='binary', device=None)
    for ctor, want in ((IFM, common), (DIFM, dict(dict(att_embedding_size=8, att_head_num=8, att_res=True), **common))):
        params = inspect.signature(ctor).parameters
        assert list(params) == ["linear_feature_columns", "dnn_feature_columns"] + list(want)
        for k, v in want.items():
            assert params[k].default == v, k


@pytest.mark.parametrize("name", FIXTURES)
def test_weight_names_and_shapes_match_the_fixture(name):
    g = load_golden(name)
    model = build_model(golden_meta(g), torch.device("cpu"))
    mine = {k: tuple(v.shape) for k, v in model.get_weights_by_name().items()}
    # (get_linear_logit builds a second, unused set of tables under the prefix "linear" for its dense inputs: feature_column.py:185)
    ref = {k: tuple(v.shape) for k, v in _weights(g).items() if not k.startswith("linearsparse_")}
    assert mine == ref
    assert model.count_params() == sum(int(np.prod(s)) for s in ref.values())
    model.set_weights_by_name(_weights(g))                       # a reference checkpoint loads by name, strictly
    for k, v in model.get_weights_by_name().items():
        assert np.array_equal(v, g["w/" + k]), k


def test_deep_only_dense_feature_is_an_input_and_feeds_nothing():
    from deepctr_amd.feature_column import DenseFeat, SparseFeat
    from deepctr_amd.models import DIFM, IFM
    sparse = [SparseFeat("a", 5, 4), SparseFeat("b", 6, 4)]
    for ctor in (IFM, DIFM):
        m = ctor(sparse, sparse + [DenseFeat("x", 3)], dnn_hidden_units=(8,), device="cpu")
        assert "x" in m.input_names
        assert m.stage_plan.in_dim == 8 and tuple(m.dnn.kernels[0].shape) == (8, 8)          # F*d: the dense width does not enter
        assert not [k for k in m.get_weights_by_name() if k.startswith("linear/")]            # no dense linear term either
        m2 = ctor(sparse + [DenseFeat("x", 3)], sparse + [DenseFeat("x", 3)], dnn_hidden_units=(8,), device="cpu")
        assert m2.stage_plan.in_dim == 8 and tuple(m2.get_weights_by_name()["linear/linear_kernel"].shape) == (3, 1)


def test_construction_errors():
    from deepctr_amd.feature_column import DenseFeat, SparseFeat, VarLenSparseFeat
    from deepctr_amd.models import DIFM, IFM
    ab = [SparseFeat("a", 5, 4), SparseFeat("b", 6, 4)]
    for ctor in (IFM, DIFM):
        with pytest.raises(ValueError, match="dnn_hidden_units is null!"):
            ctor(ab, ab, dnn_hidden_units=(), device="cpu")
        with pytest.raises(ValueError, match="there are no sparse features"):
            ctor(ab, [DenseFeat("x", 1)], device="cpu")
        with pytest.raises(ValueError, match="there are no sparse features"):
            ctor(ab, [], device="cpu")
        mixed = [SparseFeat("a", 5, 4), VarLenSparseFeat(SparseFeat("s", 6, 8), maxlen=3)]
        with pytest.raises(ValueError, match=r"embedding_dim, got \[4, 8\]"):
            ctor(mixed, mixed, device="cpu")
        abc = ab + [SparseFeat("c", 7, 4)]
        with pytest.raises(ValueError, match=r"holds 2 sparse / sequence feature\(s\), dnn_feature_columns 3"):
            ctor(ab, abc, device="cpu")                               # a linear subset: the reference's broadcast error
        with pytest.raises(ValueError, match=r"holds 1 sparse / sequence feature\(s\), dnn_feature_columns 3"):
            ctor(ab[:1], abc, device="cpu")                           # TF would broadcast the single term: refused on purpose
        with pytest.raises(ValueError, match=r"holds 3 sparse / sequence feature\(s\), dnn_feature_columns 1"):
            ctor(abc, ab[:1], device="cpu")
        ctor([], abc, dnn_hidden_units=(4,), device="cpu")            # no linear part at all
        ctor([DenseFeat("x", 2)], abc, dnn_hidden_units=(4,), device="cpu")
    with pytest.raises(ValueError, match="head_num"):
        DIFM(ab, ab, att_head_num=0, device="cpu")


def test_regularizers_leave_the_factor_projections_and_the_attention_alone():
    from deepctr_amd import training
    g = load_golden("model_difm_fixed")
    model = build_model(golden_meta(g), "cpu", l2_reg_linear=0.1, l2_reg_embedding=0.2, l2_reg_dnn=0.3)
    names = {t.data_ptr(): n for n, t in model.named_weights()}
    got = sorted((names[t.data_ptr()], l2) for t, l2 in training.regularized_weights(model))
    want = sorted([(n, 0.2) for n, _ in model.named_weights() if n.startswith("sparse_emb_")] +
                  [(n, 0.1) for n, _ in model.named_weights() if n.startswith("linear")] +
                  [(n, 0.3) for n, _ in model.named_weights() if n.startswith("dnn/kernel")])
    assert got == want
    assert not [n for n, _ in got if n.startswith(("dense", "interacting_layer"))]


def test_the_hip_trainer_declines_both_models():
    from deepctr_amd import training_hip
    for name in ("model_ifm_fixed", "model_difm_fixed"):
        assert training_hip.supported(build_model(golden_meta(load_golden(name)), "cpu")) is False


def test_reference_import_names():
    import deepctr
    import deepctr_amd.models
    from deepctr.models import DIFM, IFM
    from deepctr.models.difm import DIFM as D2
    from deepctr.models.ifm import IFM as I2
    assert IFM is deepctr_amd.models.IFM is I2 is deepctr.models.IFM
    assert DIFM is deepctr_amd.models.DIFM is D2 is deepctr.models.DIFM


def test_op_oracle_bounds_and_factor():
    rng = np.random.RandomState(3)
    B, F, d, K = 7, 5, 3, 11
    x, act, w = rng.standard_normal((B, F * d + 2)), rng.standard_normal((B, K)), rng.standard_normal((K, F))
    lin, add = rng.standard_normal((B, F)), [rng.standard_normal(B)]
    for softmax in (False, True):
        out, m = RI.ifm_op(x, F, d, sources=[(act, w)], softmax=softmax, lin=lin, add=add, bias=0.3)
        if softmax:
            assert np.allclose(m.sum(1), F) and (m > 0).all()
        else:
            assert np.allclose(m, act @ w)
        r = x[:, :F * d].reshape(B, F, d) * m[:, :, None]
        pairs = sum((r[:, i] * r[:, j]).sum(-1) for i in range(F) for j in range(i + 1, F))
        assert np.allclose(out, pairs + (lin * m).sum(1) + add[0] + 0.3)
        bound, _ = RI.ifm_op(x, F, d, sources=[(act, w)], softmax=softmax, lin=lin, add=add, bias=0.3, absolute=True)
        assert (bound >= np.abs(out)).all()
    o2, m2 = RI.ifm_op(x, F, d, mprime=act @ w, lin=lin, add=add, bias=0.3)
    o1, m1 = RI.ifm_op(x, F, d, sources=[(act, w)], lin=lin, add=add, bias=0.3)
    assert np.allclose(o1, o2) and np.allclose(m1, m2)


def test_cost_model():
    """The counts DESIGN.md §4.12 quotes (Criteo defaults: 39 fields of embedding_dim 4, DNN 256-128-64, 8 heads of 8)."""
    F, d, H = 39, 4, 64
    assert F * d * 4 == 624 and H * 4 == 256 and F * 8 * 8 == 2496 and 2496 * 4 == 9984
    assert 2 * H * F == 4992 and 2 * 2496 * F == 194688 and 4 * F * d + 2 * F == 702
    assert 2496 * F * 4 == 389376 and H * F * 4 == 9984
    assert 4 * 16 * 68 * 4 == 17408 and 4 * 16 * (48 + 4) * 4 == 13312 and 4 * 16 * (208 + 4) * 4 == 54272
    assert 17408 + 4 * 16 * (560 + 4) * 4 <= 160 * 1024 < 17408 + 4 * 16 * (576 + 4) * 4


def _args(**kw):
    from deepctr_amd import _C
    base = dict(batch=4, n_fields=5, dim=3, x_stride=16, n_src=0, mprime_stride=5, route=0)
    src = kw.pop("src", ())
    base.update(kw)
    a = _C.ifm.Args(**base)
    for i, s in enumerate(src):
        a.src[i].act, a.src[i].kernel, a.src[i].act_stride, a.src[i].K = s
    return a


def test_abi_argument_errors_without_a_gpu():
    from deepctr_amd import _C
    lib = _C.lib()
    f = lambda a: lib.dctr_ifm_fwd(ctypes.byref(a), None)   # noqa: E731
    full = dict(x=16, out=16, mprime=16)
    assert lib.dctr_ifm_fwd(None, None) == -1
    for k in full:
        a = dict(full)
        del a[k]
        assert f(_args(**a)) == -1, k
    assert f(_args(n_fields=0, **full)) == -2
    assert f(_args(dim=0, **full)) == -2
    assert f(_args(batch=-1, **full)) == -2
    assert f(_args(x_stride=14, **full)) == -2                       # 5 fields x 3 = 15 columns
    assert f(_args(mprime_stride=4, **full)) == -2
    assert f(_args(n_src=3, **full)) == -2
    assert f(_args(n_src=-1, **full)) == -2
    assert f(_args(n_src=1, src=[(16, 16, 8, 0)], **full)) == -2     # K = 0
    assert f(_args(n_src=1, src=[(16, 16, 7, 8)], **full)) == -2     # act_stride < K
    assert f(_args(n_src=1, src=[(0, 16, 8, 8)], **full)) == -1      # null act
    assert f(_args(n_src=2, src=[(16, 16, 8, 8), (16, 0, 8, 8)], **full)) == -1
    assert f(_args(n_src=1, src=[(16, 16, 8, 8)], mprime_stride=1, mprime=16, x=16, out=16)) == -2   # mprime beside a source: its stride counts
    assert f(_args(n_lin=4, lin=16, **full)) == -2                   # 0 or n_fields first-order terms
    assert f(_args(n_lin=5, **full)) == -1                           # terms without descriptors
    assert f(_args(n_add=5, **full)) == -2
    assert f(_args(n_add=1, **full)) == -1                           # a null add vector
    assert f(_args(factor_out=16, factor_stride=4, **full)) == -2
    assert f(_args(route=2, **full)) == -4                           # the LDS route cannot be forced
    assert f(_args(route=-1, **full)) == -4
    assert f(_args(route=1, n_src=1, src=[(16, 16, 8, 8)], **full)) == -1            # workspace route without a workspace
    assert f(_args(route=1, n_src=1, src=[(16, 16, 8, 8)], workspace=4096 + 4, workspace_bytes=4096, **full)) == -3
    assert f(_args(route=1, n_src=1, src=[(16, 16, 8, 8)], workspace=4096, workspace_bytes=64, **full)) == -2
    assert b"ifm_fwd" in lib.dctr_last_error()
    assert f(_args(batch=0, **full)) == 0                            # empty batch: a no-op
    assert f(_args(batch=0, n_src=2, src=[(16, 16, 8, 8), (16, 16, 9, 9)], n_lin=5, lin=16, softmax=1, **full)) == 0


def test_abi_first_source_check_reads_mprime_only_when_given():
    from deepctr_amd import _C
    lib = _C.lib()
    a = _args(batch=0, n_src=1, src=[(16, 16, 8, 8)], mprime_stride=0, x=16, out=16)
    assert lib.dctr_ifm_fwd(ctypes.byref(a), None) == 0


def test_routes_and_workspace_without_a_gpu():
    from deepctr_amd import _C, ops
    for F, d in ((1, 1), (26, 16), (39, 4), (39, 64), (200, 8), (560, 300)):
        for n in (3, 4096, 65536):
            assert ops.ifm_route(n, F, d) == "lds", (F, d)
            assert ops.ifm_workspace_bytes(n, F, d) == 0 and ops.ifm_workspace_bytes(n, F, d, n_src=2) == 0
            assert ops.ifm_route(n, F, d, route="workspace") == "workspace"
            assert ops.ifm_workspace_bytes(n, F, d, route="workspace") == (n * F * 4 + 15) // 16 * 16
            # m' handed over: nothing to project, nothing to keep
            assert ops.ifm_route(n, F, d, n_src=0, route="workspace") == "lds" and ops.ifm_workspace_bytes(n, F, d, n_src=0, route="workspace") == 0
    for F in (561, 577, 1000, 5000):                       # the [16, F] tile of m' of four waves no longer fits 160 KiB
        assert ops.ifm_route(100, F, 2) == "workspace" and ops.ifm_workspace_bytes(100, F, 2) == (100 * F * 4 + 15) // 16 * 16
    with pytest.raises(ValueError, match="fields"):
        ops.ifm_route(5, 0, 4)
    with pytest.raises(ValueError, match="route"):
        ops.ifm_route(5, 4, 4, route="lds")
    with pytest.raises(ValueError, match="sources"):
        ops.ifm_route(5, 4, 4, n_src=3)
    with pytest.raises(_C.DctrError):
        ops.ifm_route(5, 1 << 20, 1 << 10)


def test_args_mirrors_have_the_layout_the_c_compiler_gives_the_header(tmp_path):
    import os
    import shutil
    import subprocess
    from deepctr_amd import _C
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    structs = (("dctr_ifm_args_t", _C.ifm.Args), ("dctr_ifm_src_t", _C.ifm.Src), ("dctr_ifm_lin_t", _C.ifm.Lin))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dctr.h"', "int main(void) {",
             '    printf("enums %d %d %d %d\\n", DCTR_IFM_ROUTE_AUTO, DCTR_IFM_ROUTE_WORKSPACE, DCTR_IFM_ROUTE_LDS, DCTR_ABI_VERSION);']
    for cname, cls in structs:
        lines.append('    printf("%s.sizeof %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in cls._fields_:
            lines.append('    printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines += ["    return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    by_name = dict(structs)
    seen = set()
    for line in filter(None, out):
        field, *vals = line.split()
        if field == "enums":
            assert [int(v) for v in vals] == [_C.ifm.ROUTE_AUTO, _C.ifm.ROUTE_WORKSPACE, _C.ifm.ROUTE_LDS, 13]   # additions only
            continue
        cname, fname = field.split(".")
        cls = by_name[cname]
        want = ctypes.sizeof(cls) if fname == "sizeof" else getattr(cls, fname).offset
        assert int(vals[0]) == want, "%s: C says %s, ctypes %d" % (field, vals[0], want)
        seen.add(field)
    assert seen == {"%s.%s" % (c, f) for c, cls in structs for f in ["sizeof"] + [n for n, _ in cls._fields_]}


@pytest.mark.parametrize("kind", ["IFM", "DIFM"])
def test_cpu_fit_on_the_autograd_step_lowers_the_loss(kind):
    """training._fit_torch is device-agnostic torch code: a CPU-built model trains on a planted signal, sequences, a reordered linear
    list and BatchNormalization included; the factor projections and (DIFM) the attention weights move."""
    from deepctr_amd import engine, models, training
    from deepctr_amd.feature_column import DenseFeat, SparseFeat, VarLenSparseFeat
    rng = np.random.RandomState(4)
    n = 1024
    cols = [SparseFeat("a", 8, 4), SparseFeat("b", 6, 4), VarLenSparseFeat(SparseFeat("s", 7, 4), maxlen=3, combiner="mean"),
            DenseFeat("x", 1)]
    feed = {"a": rng.randint(0, 8, n).astype(np.int32), "b": rng.randint(0, 6, n).astype(np.int32),
            "s": rng.randint(0, 7, (n, 3)).astype(np.int32), "x": rng.rand(n).astype(np.float32)}
    y = ((feed["a"] % 2) ^ (feed["b"] % 3 == 0)).astype(np.float32)
    torch.manual_seed(0)
    np.random.seed(0)
    kw = dict(dnn_hidden_units=(16, 8), dnn_dropout=0.1, dnn_use_bn=True, device="cpu")
    if kind == "DIFM":
        kw.update(att_embedding_size=4, att_head_num=2)
    model = getattr(models, kind)([cols[1], cols[0], cols[3], cols[2]], cols, **kw)
    model.compile(lambda ps: torch.optim.Adam(ps, lr=0.01), "binary_crossentropy")
    staged = engine.Staged(n)
    model._stage_inputs(feed, staged)
    yt = torch.from_numpy(y)
    w0 = {k: v.copy() for k, v in model.get_weights_by_name().items()}
    losses = []

    class End(object):
        def __call__(self, ep, loss):
            losses.append(loss)
            return False

        def finish(self):
            return losses

    training._fit_torch(model, staged, yt, n, 128, 6, True, End())
    assert losses[-1] < losses[0] - 0.05
    w1 = model.get_weights_by_name()
    moved = {k for k in w0 if not np.array_equal(w0[k], w1[k])}
    want = {"dense/kernel", "dnn/kernel0", "sparse_emb_a/embeddings", "sparse_seq_emb_s/embeddings", "linear0sparse_emb_a/embeddings",
            "linear0sparse_seq_emb_s/embeddings", "linear/linear_kernel", "batch_normalization/moving_mean", "batch_normalization/gamma"}
    if kind == "DIFM":
        want |= {"dense_1/kernel", "interacting_layer/query", "interacting_layer/res"}
    assert want <= moved, want - moved
    assert all(not t.requires_grad for t in model.weights)
