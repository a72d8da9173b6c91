"""CPU: MLR — the NumPy oracle (tests/ref_mlr.py) against the reference's own outputs (tests/golden/model_mlr*.npz;
scripts/make_golden_mlr.py), the torch restatement (training._mlr_output) against the oracle, the API contract (signature, weight names
and order, the fused per-name tables behind the per-name views, freezing, regularisers, the refusals, the import names), the C ABI's
argument checks (no launch), the probability-loss rule of the autograd step and a CPU fit()."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from tests import ref_mlr as RM
from tests.spec import columns_from_spec
from tests.test_autoint_cpu import att_rows
from tests.util import assert_close, golden_meta, load_golden

FIXTURES = ["model_mlr", "model_mlr_hash", "model_mlr_r2", "model_mlr_r7", "model_mlr_base_overlap", "model_mlr_base_disjoint",
            "model_mlr_bias", "model_mlr_bias_split", "model_mlr_regression", "model_mlr_fixed"]


def build_model(meta, device, **more):
    from deepctr_amd.models.mlr import MLR
    kw = dict(meta["kwargs"])
    kw.update(more)
    cols = lambda key: columns_from_spec(meta[key]) if meta.get(key) else None     # noqa: E731
    return MLR(cols("region"), cols("base"), bias_feature_columns=cols("bias"), device=device, **kw)


def _has_hash(meta):
    return any(d.get("use_hash") or d.get("sparsefeat", {}).get("use_hash") for d in meta["dnn"])


def _feed(g):
    return {k[5:]: v for k, v in g.items() if k.startswith("feed/")}


def _weights(g):
    return {k[2:]: v for k, v in g.items() if k.startswith("w/")}


def kept_rows(meta, feed, n):
    """att_rows, asserted to keep at least half of the fixture."""
    rows = att_rows(meta, feed, n)
    assert rows.sum() * 2 >= n
    return rows


def _binary(meta):
    return meta["kwargs"].get("task", "binary") == "binary"


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_matches_reference_code(name):
    g = load_golden(name)
    meta = golden_meta(g)
    assert meta["model"] == "MLR"
    n = g["y"].shape[0]
    assert g["y"].shape == (n, 1)
    rows = kept_rows(meta, _feed(g), n)
    ref = g["y"][rows]
    if _binary(meta):
        assert ((ref > 1e-3) & (ref < 1 - 1e-3)).all()         # none of the compared rows is saturated
    assert_close(RM.run_fixture(g, np.float32)[rows], ref, rtol=1e-4, atol=2e-5, what=name + " float32")
    assert_close(RM.run_fixture(g, np.float64)[rows], ref, rtol=1e-4, atol=2e-5, what=name + " float64")


@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_would_notice_a_wrong_graph(name):
    """From the float64 oracle alone (scripts/make_golden_mlr.py asserts the same): on at least half of the compared rows each
    applicable mutation moves the output by >= 100 x (1e-4 of it)."""
    g = load_golden(name)
    meta = golden_meta(g)
    rows = kept_rows(meta, _feed(g), g["y"].shape[0])
    y = RM.run_fixture(g).reshape(-1)[rows]
    muts = RM.mutations(meta)
    assert "uniform" in muts and ("no_sigmoid" in muts) == _binary(meta)
    for mutate in muts:
        ym = RM.run_fixture(g, mutate=mutate).reshape(-1)[rows]
        moved = np.abs(ym - y) >= 100 * 1e-4 * np.abs(y)
        assert moved.sum() * 2 >= moved.size, (name, mutate, int(moved.sum()), moved.size)


def test_fixture_set_is_what_the_recipe_lists():
    seen = set()
    for name in FIXTURES:
        meta = golden_meta(load_golden(name))
        seen |= set(RM.mutations(meta))
        for key in ("region", "base", "bias"):                    # the shim quirk: every column list carries a DenseFeat
            assert meta[key] is None or any(d["type"] == "dense" for d in meta[key]), (name, key)
    assert seen == {"uniform", "no_sigmoid", "swap", "no_bias"}
    names = lambda spec: {d.get("name") or d["sparsefeat"]["name"] for d in spec}     # noqa: E731
    m = golden_meta(load_golden("model_mlr_base_overlap"))
    assert names(m["region"]) & names(m["base"]) and names(m["region"]) - names(m["base"])
    m = golden_meta(load_golden("model_mlr_base_disjoint"))
    assert not names(m["region"]) & names(m["base"])
    m = golden_meta(load_golden("model_mlr_bias"))
    assert names(m["bias"]) < names(m["region"]) and m["base"] is None
    m = golden_meta(load_golden("model_mlr_bias_split"))
    assert "sparse_feature_0" in (names(m["region"]) & names(m["bias"])) - names(m["base"])        # region + bias only
    assert golden_meta(load_golden("model_mlr_r2"))["kwargs"]["region_num"] == 2
    assert golden_meta(load_golden("model_mlr_r7"))["kwargs"]["region_num"] == 7
    assert _has_hash(golden_meta(load_golden("model_mlr_hash")))
    assert all(d["type"] != "varlen" for d in golden_meta(load_golden("model_mlr_fixed"))["region"])


def _staged_cpu(model, feed, n):
    from deepctr_amd import engine
    staged = engine.Staged(n)
    model._stage_inputs(feed, staged)
    model._begin()
    return staged


@pytest.mark.parametrize("name", FIXTURES)
def test_torch_restatement_matches_oracle(name):
    from deepctr_amd import training
    g = load_golden(name)
    meta = golden_meta(g)
    if _has_hash(meta):
        pytest.skip("integer Hash runs in a HIP kernel; the GPU suite covers this fixture")
    model = build_model(meta, torch.device("cpu"))
    model.set_weights_by_name(_weights(g))
    feed = _feed(g)
    n = g["y"].shape[0]
    staged = _staged_cpu(model, feed, n)
    rows = kept_rows(meta, feed, n)
    ref = RM.run_fixture(g, np.float64).reshape(-1)
    with torch.no_grad():
        y64 = training._mlr_output(model, staged, 0, n, dtype=torch.float64).numpy()
        y32 = training.model_logits(model, staged, 0, n).numpy()
    # float64 against float64: only the float32 weights and inputs are shared, the two codes agree to rounding
    assert np.abs(y64[rows] - ref[rows]).max() <= 1e-12 * max(1.0, np.abs(ref[rows]).max())
    assert_close(y32[rows], ref[rows], rtol=1e-4, atol=2e-5, what=name + " float32")


def test_no_dense_feature_against_the_oracle():
    """The case the fixtures cannot hold (the shim's linear part needs a DenseFeat): no dense value in any list."""
    from deepctr_amd import training
    from deepctr_amd.feature_column import SparseFeat, VarLenSparseFeat
    from deepctr_amd.models.mlr import MLR
    rng = np.random.RandomState(3)
    cols = [SparseFeat("a", 9, 4), SparseFeat("b", 5, 4), VarLenSparseFeat(SparseFeat("s", 7, 4), maxlen=4, combiner="sum")]
    m = MLR(cols, region_num=3, bias_feature_columns=cols[:1], device="cpu")
    assert m.n_dense == 0 and all(not lin.weights for lin in m.mlr_linears)
    w = {k: rng.standard_normal(v.shape).astype(np.float32) for k, v in m.get_weights_by_name().items()}
    m.set_weights_by_name(w)
    n = 16
    feed = {"a": rng.randint(0, 9, n).astype(np.int32), "b": rng.randint(0, 5, n).astype(np.int32),
            "s": rng.randint(0, 7, (n, 4)).astype(np.int32)}
    staged = _staged_cpu(m, feed, n)
    with torch.no_grad():
        y = training._mlr_output(m, staged, 0, n, dtype=torch.float64).numpy()
    ref, _ = RM.mlr_model(cols, None, cols[:1], w, feed, region_num=3)
    assert np.abs(y - ref.reshape(-1)).max() <= 1e-12


def test_dense_only_model_against_the_oracle():
    """No sparse or sequence feature in any list: the reference allows it; the model has no field entry and no table."""
    from deepctr_amd import training
    from deepctr_amd.feature_column import DenseFeat
    from deepctr_amd.models.mlr import MLR
    rng = np.random.RandomState(6)
    cols = [DenseFeat("x", 3), DenseFeat("y", 1)]
    m = MLR(cols, region_num=3, bias_feature_columns=cols[1:], device="cpu")
    assert not m.entries and not m.masters and m.n_dense == 4
    w = {k: rng.standard_normal(v.shape).astype(np.float32) for k, v in m.get_weights_by_name().items()}
    m.set_weights_by_name(w)
    n = 9
    feed = {"x": rng.standard_normal((n, 3)).astype(np.float32), "y": rng.standard_normal(n).astype(np.float32)}
    staged = _staged_cpu(m, feed, n)
    with torch.no_grad():
        y = training._mlr_output(m, staged, 0, n, dtype=torch.float64).numpy()
    ref, _ = RM.mlr_model(cols, None, cols[1:], w, feed, region_num=3)
    assert np.abs(y - ref.reshape(-1)).max() <= 1e-12


def test_signature_defaults_match_the_reference():
    from deepctr_amd.models.mlr import MLR
    params = inspect.signature(MLR).parameters
    want = dict(base_feature_columns=None, region_num=4, l2_reg_linear=1e-5, seed=1024, task='binary', bias_feature_columns=None,
                device=None)
    assert list(params) == ["region_feature_columns"] + list(want)
    for k, v in want.items():
        assert params[k].default == v, k


def _dangling(key):
    """The reference's second, never-used table set (get_linear_logit's extra input_from_feature_columns call with the bare prefix)."""
    import re
    return re.match(r"w/(region|learner|bias)_\d*[1-9]sparse_", key) is not None


@pytest.mark.parametrize("name", FIXTURES)
def test_weight_names_order_and_shapes_match_the_fixture(name):
    g = load_golden(name)
    model = build_model(golden_meta(g), torch.device("cpu"))
    mine = [(k, tuple(v.shape)) for k, v in model.get_weights_by_name().items()]
    ref = [(k[2:], tuple(v.shape)) for k, v in g.items() if k.startswith("w/") and not _dangling(k)]
    assert any(_dangling(k) for k in g) and mine == ref
    assert model.count_params() == sum(int(np.prod(s)) for _, s in ref)
    assert model.input_names == golden_meta(g)["inputs"] and set(model.input_names) == {k[5:] for k in g if k.startswith("feed/")}
    # the fixture's whole weight dict loads (the dangling tables are skipped) and comes back
    model.set_weights_by_name(_weights(g))
    for k, v in model.get_weights_by_name().items():
        assert np.array_equal(v, g["w/" + k]), k
    with pytest.raises(KeyError):
        model.set_weights_by_name({"region_10sparse_emb_nope/embeddings": np.zeros((3, 1), np.float32)})


def test_per_name_weights_are_views_of_one_master_per_feature():
    g = load_golden("model_mlr_bias_split")
    meta = golden_meta(g)
    model = build_model(meta, torch.device("cpu"))
    R = model.region_num
    assert R == 3 and model.n_columns == 7
    w = dict(model.named_weights())
    # region + base: one master over the columns 0 .. 2R-1, pitch rounded up to 4 floats
    (c0, n, m), = model.masters["sparse_feature_1"]
    assert (c0, n) == (0, 2 * R) and tuple(m.shape) == (5, 8) and m.is_contiguous()
    for r in range(R):
        for c, key in ((r, "region_%d0sparse_emb_sparse_feature_1" % (r + 1)), (R + r, "learner_%d0sparse_emb_sparse_feature_1" % (r + 1))):
            t = w[key + "/embeddings"]
            assert t.data_ptr() == m.data_ptr() + 4 * c and tuple(t.shape) == (5, 1) and t.stride(0) == 8
    # region + bias without base: two masters, two field entries
    runs = model.masters["sparse_feature_0"]
    assert [(c0, n, tuple(m.shape)) for c0, n, m in runs] == [(0, 3, (9, 4)), (6, 1, (9, 4))]
    assert w["bias_10sparse_emb_sparse_feature_0/embeddings"].data_ptr() == runs[1][2].data_ptr()
    assert [(e["col0"], e["width"]) for e in model.entries if e["fc"].name == "sparse_feature_0"] == [(0, 3), (6, 1)]
    # base + bias: columns R .. 2R: one run
    assert [(c0, n) for c0, n, _ in model.masters["sparse_feature_2"]] == [(3, 4)]
    # a write through a view is seen by the master, and only there
    before = {k: [m.clone() for _, _, m in v] for k, v in model.masters.items()}
    new = np.full((5, 1), 2.5, dtype=np.float32)
    model.set_weights_by_name({"learner_20sparse_emb_sparse_feature_1/embeddings": new}, strict=False)
    for k, runs in model.masters.items():
        for (c0, n, m), b in zip(runs, before[k]):
            if k != "sparse_feature_1":
                assert torch.equal(m, b)
            else:
                assert (m != b).any(dim=0).nonzero().reshape(-1).tolist() == [R + 1]
    assert np.array_equal(model.get_weights_by_name()["learner_20sparse_emb_sparse_feature_1/embeddings"], new)
    # every per-name tensor is a distinct column
    ptrs = [t.data_ptr() for k, t in w.items() if k.endswith("/embeddings")]
    assert len(set(ptrs)) == len(ptrs)


def test_shared_embedding_name_shares_the_master():
    g = load_golden("model_mlr")
    model = build_model(golden_meta(g), torch.device("cpu"))
    assert "sequence_len_max" not in model.masters                     # its embedding_name is sparse_feature_2
    es = [e for e in model.entries if e["fc"].name in ("sparse_feature_2", "sequence_len_max")]
    assert len(es) == 2 and es[0]["master"] is es[1]["master"] and model.mlr_tables["region_10sparse_emb_sparse_feature_2"].mask_zero


def test_trainable_false_freezes_every_view_of_the_feature():
    from deepctr_amd import training
    from deepctr_amd.feature_column import DenseFeat, SparseFeat
    from deepctr_amd.models.mlr import MLR
    cols = [SparseFeat("a", 5, 4, trainable=False), SparseFeat("b", 6, 4), DenseFeat("x", 1)]
    m = MLR(cols, region_num=2, bias_feature_columns=cols[:1], device="cpu")
    frozen = training.frozen_weights(m)
    w = dict(m.named_weights())
    assert {n for n, t in w.items() if t.data_ptr() in frozen} == {
        "region_10sparse_emb_a/embeddings", "region_20sparse_emb_a/embeddings", "learner_10sparse_emb_a/embeddings",
        "learner_20sparse_emb_a/embeddings", "bias_10sparse_emb_a/embeddings"}


def test_regularized_weights_cover_every_table_and_linear_kernel():
    from deepctr_amd import training
    g = load_golden("model_mlr_bias")
    model = build_model(golden_meta(g), "cpu", l2_reg_linear=0.25)
    names = {t.data_ptr(): n for n, t in model.named_weights()}
    got = sorted((names[t.data_ptr()], l2) for t, l2 in training.regularized_weights(model))
    assert got == sorted((n, 0.25) for n, _ in model.named_weights())
    assert sum(1 for n, _ in got if n.endswith("linear_kernel")) == 9
    assert training.regularized_weights(build_model(golden_meta(g), "cpu", l2_reg_linear=0)) == []


def test_construction_errors():
    from deepctr_amd.feature_column import DenseFeat, SparseFeat
    from deepctr_amd.models.mlr import MLR
    cols = [SparseFeat("a", 5, 4), DenseFeat("x", 1)]
    for r in (1, 0, -2):
        with pytest.raises(ValueError, match="region_num must > 1"):
            MLR(cols, region_num=r, device="cpu")
    for empty in ([], None):
        with pytest.raises(ValueError, match="region_feature_columns"):
            MLR(empty, device="cpu")
    with pytest.raises(ValueError, match="same embedding_name"):
        MLR(cols, base_feature_columns=[SparseFeat("a", 6, 4)], device="cpu")
    m = MLR(cols, base_feature_columns=[], device="cpu")           # empty base: the region columns
    assert [fc.name for fc in m.groups[4].features] == ["a"] and not m.has_bias and m.n_columns == 8


def test_predict_logits_raises_and_the_learners_do_not_follow_task():
    from deepctr_amd.feature_column import DenseFeat, SparseFeat
    from deepctr_amd.models.mlr import MLR
    m = MLR([SparseFeat("a", 5, 4), DenseFeat("x", 1)], device="cpu")
    with pytest.raises(NotImplementedError, match="not the sigmoid of a logit"):
        m.predict_logits({"a": np.zeros(2, np.int32), "x": np.zeros(2, np.float32)})
    m.task = "regression"
    assert m.learner_task == "binary" and m.output_kind == "prediction"
    from deepctr_amd.models._common import FeatureModel
    assert FeatureModel.output_kind == "logit"


def test_import_names():
    import deepctr
    import deepctr.models
    import deepctr_amd.models
    from deepctr.models import MLR
    import deepctr.models.mlr
    from deepctr.models.mlr import MLR as M2
    from deepctr_amd.models import MLR as M3
    assert MLR is M2 is M3 is deepctr.models.MLR is deepctr_amd.models.MLR is deepctr.models.mlr.MLR
    assert deepctr.models is deepctr_amd.models
    assert "MLR" not in dir(deepctr.models) and "MLR" not in vars(deepctr_amd.models)      # lazy: see models/__init__.py
    with pytest.raises(AttributeError):
        deepctr.models.NoSuchModel


def _args(**kw):
    from deepctr_amd import _C
    base = dict(batch=4, n_fields=2, region_num=4, has_bias=1, learner_act=0, out_stride=1)
    base.update(kw)
    return _C.mlr.Args(**base)


def test_abi_argument_errors_without_a_gpu():
    from deepctr_amd import _C
    lib = _C.lib()
    f = lambda a: lib.dctr_mlr_fwd(ctypes.byref(a), None)   # noqa: E731
    full = dict(fields=16, out=16)
    assert lib.dctr_mlr_fwd(None, None) == -1
    assert f(_args()) == -1                                          # fields / out missing
    for k in full:
        a = dict(full)
        del a[k]
        assert f(_args(**a)) == -1, k
    for r in (1, 0, -1):
        assert f(_args(region_num=r, **full)) == -2
    assert f(_args(batch=-1, **full)) == -2
    assert f(_args(n_fields=-1, **full)) == -2
    assert f(_args(n_dense=-1, **full)) == -2
    assert f(_args(out_stride=0, **full)) == -2
    assert f(_args(has_bias=2, **full)) == -4
    assert f(_args(learner_act=2, **full)) == -4
    assert f(_args(learner_act=-1, **full)) == -4
    assert f(_args(n_dense=2, dense_stride=2, **full)) == -1         # dense values without dense / dense_w
    assert f(_args(n_dense=2, dense=16, dense_stride=2, **full)) == -1
    assert f(_args(n_dense=2, dense=16, dense_w=16, dense_stride=1, **full)) == -2
    assert f(_args(z=16, z_stride=8, **full)) == -2                  # K = 9 columns
    assert f(_args(z=16, z_stride=12, z_offset=4, **full)) == -2
    assert f(_args(z=16, z_stride=12, z_offset=-1, **full)) == -2
    assert f(_args(fields=20, out=16)) == -3                         # the descriptor array holds pointers
    assert b"mlr_fwd" in lib.dctr_last_error()
    assert f(_args(batch=0, **full)) == 0                            # empty batch: a no-op
    assert f(_args(batch=0, n_fields=0, out=16)) == 0                # no sparse feature at all is legal
    assert f(_args(batch=0, z=16, z_stride=16, z_offset=7, n_dense=2, dense=16, dense_w=16, dense_stride=2, status=16, **full)) == 0
    # the backward: the forward's checks, then its own operands
    b = lambda **kw: lib.dctr_mlr_bwd(ctypes.byref(_C.mlr.BwdArgs(**kw)), None)   # noqa: E731
    fz = _args(z=16, z_stride=9, **full)
    assert lib.dctr_mlr_bwd(None, None) == -1
    assert b(fwd=_args(region_num=1, **full), d_out=16, d_out_stride=1, dz=16, dz_stride=9) == -2
    assert b(fwd=_args(**full), d_out=16, d_out_stride=1, dz=16, dz_stride=9) == -1          # no saved z
    assert b(fwd=fz, d_out_stride=1, dz=16, dz_stride=9) == -1
    assert b(fwd=fz, d_out=16, d_out_stride=1, dz_stride=9) == -1
    assert b(fwd=fz, d_out=16, d_out_stride=0, dz=16, dz_stride=9) == -2
    assert b(fwd=fz, d_out=16, d_out_stride=1, dz=16, dz_stride=8) == -2
    assert b(fwd=fz, d_out=16, d_out_stride=1, dz=16, dz_stride=9, grads=12) == -3
    assert b"mlr_bwd" in lib.dctr_last_error()
    fz.batch = 0
    assert b(fwd=fz, d_out=16, d_out_stride=1, dz=16, dz_stride=9, grads=16) == 0


def test_supported_at_64_and_65_columns_without_a_gpu():
    from deepctr_amd import _C, ops
    lib = _C.lib()
    assert ops.mlr_supported(4) and ops.mlr_supported(4, True) and ops.mlr_supported(2)
    assert ops.mlr_supported(32, False) and not ops.mlr_supported(32, True)          # K = 64 / 65
    assert ops.mlr_supported(31, True) and not ops.mlr_supported(33, False)          # K = 63 / 66
    assert not ops.mlr_supported(1)
    full = dict(fields=16, out=16, batch=0)
    assert lib.dctr_mlr_fwd(ctypes.byref(_args(region_num=32, has_bias=0, **full)), None) == 0
    assert lib.dctr_mlr_fwd(ctypes.byref(_args(region_num=32, has_bias=1, **full)), None) == _C.E_UNSUPPORTED
    assert lib.dctr_mlr_fwd(ctypes.byref(_args(region_num=32, has_bias=1)), None) == _C.E_UNSUPPORTED     # before the pointers
    b = _C.mlr.BwdArgs(fwd=_args(region_num=40, has_bias=0, **full), d_out=16, d_out_stride=1, dz=16, dz_stride=80)
    assert lib.dctr_mlr_bwd(ctypes.byref(b), None) == _C.E_UNSUPPORTED


def test_args_mirrors_have_the_layout_the_c_compiler_gives_the_header(tmp_path):
    import os
    import shutil
    import subprocess
    from deepctr_amd import _C
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    structs = (("dctr_mlr_args_t", _C.mlr.Args), ("dctr_mlr_field_t", _C.mlr.Field), ("dctr_mlr_grad_t", _C.mlr.Grad),
               ("dctr_mlr_bwd_args_t", _C.mlr.BwdArgs))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dctr.h"', "int main(void) {",
             '    printf("enums %d %d %d %d\\n", DCTR_MLR_LEARNER_SIGMOID, DCTR_MLR_LEARNER_LINEAR, DCTR_MLR_MAX_COLUMNS, DCTR_ABI_VERSION);']
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
            assert [int(v) for v in vals] == [_C.mlr.LEARNER_SIGMOID, _C.mlr.LEARNER_LINEAR, _C.mlr.MAX_COLUMNS, 13]   # additions only
            continue
        cname, fname = field.split(".")
        cls = by_name[cname]
        want = ctypes.sizeof(cls) if fname == "sizeof" else getattr(cls, fname).offset
        assert int(vals[0]) == want, "%s: C says %s, ctypes %d" % (field, vals[0], want)
        seen.add(field)
    assert seen == {"%s.%s" % (c, f) for c, cls in structs for f in ["sizeof"] + [n for n, _ in cls._fields_]}


def test_op_oracle_backward_is_the_derivative_of_its_forward():
    """tests/ref_mlr.py's dz and table gradients against central differences of its own forward (float64)."""
    rng = np.random.RandomState(5)
    B, R = 6, 3
    for bias, task in ((True, "binary"), (False, "regression")):
        K = 2 * R + int(bias)
        fields = [dict(rows=rng.standard_normal((7, 8)), ids=rng.randint(0, 7, B), col0=0, width=2 * R),
                  dict(rows=rng.standard_normal((B, 4)), ids=None, col0=2, width=3)]
        if bias:
            fields.append(dict(rows=rng.standard_normal((5, 4)), ids=rng.randint(0, 5, B), col0=2 * R, width=1))
        dense, dw = rng.standard_normal((B, 2)), rng.standard_normal((2, K))
        d = rng.standard_normal(B)
        res = RM.mlr_op(fields, B, R, bias, task, dense, dw, d_out=d)
        loss = lambda fs: float((RM.mlr_op(fs, B, R, bias, task, dense, dw)["out"] * d).sum())     # noqa: E731
        for j, f in enumerate(fields):
            num = np.zeros((f["rows"].shape[0], f["width"]))
            for idx in np.ndindex(*num.shape):
                fp = [dict(q, rows=q["rows"].copy()) for q in fields]
                fm = [dict(q, rows=q["rows"].copy()) for q in fields]
                fp[j]["rows"][idx] += 1e-6
                fm[j]["rows"][idx] -= 1e-6
                num[idx] = (loss(fp) - loss(fm)) / 2e-6
            assert np.abs(num - res["grads"][j]).max() < 1e-8, (bias, task, j)
        assert (res["dz_terms"] >= np.abs(res["dz"]) - 1e-15).all() and (res["z_terms"] >= np.abs(res["z"]) - 1e-15).all()


class _End(object):
    def __init__(self):
        self.losses = []

    def __call__(self, ep, loss):
        self.losses.append(loss)
        return False

    def finish(self):
        return self.losses


def test_probability_loss_of_the_autograd_step_is_the_clipped_formula():
    """_fit_torch on a model whose output_kind is "prediction": one SGD step equals the clipped binary cross-entropy computed in NumPy,
    and a row whose p is clamped (at either end) contributes exactly zero gradient."""
    from deepctr_amd import training
    from deepctr_amd.feature_column import SparseFeat
    from deepctr_amd.models.mlr import MLR
    cols = [SparseFeat("a", 6, 4)]
    m = MLR(cols, region_num=2, l2_reg_linear=0, device="cpu")
    # ids 0 / 1: saturated towards 1 / towards 0 (clamped at each end); ids 2 .. 5: ordinary rows
    w = {k: np.zeros((6, 1), np.float32) for k in m.get_weights_by_name()}
    rng = np.random.RandomState(2)
    for k in w:
        w[k][2:] = rng.standard_normal((4, 1)).astype(np.float32)
        if k.startswith("learner"):
            w[k][0], w[k][1] = 40.0, -40.0
    m.set_weights_by_name(w)
    ids = np.array([0, 1, 2, 3, 4, 5, 2, 3], dtype=np.int32)
    y = np.array([1, 0, 1, 0, 0, 1, 0, 1], dtype=np.float32)
    n = len(ids)
    lr = 0.5
    m.compile(lambda ps: torch.optim.SGD(ps, lr=lr), "binary_crossentropy")
    staged = _staged_cpu(m, {"a": ids}, n)
    end = _End()
    training._fit_torch(m, staged, torch.from_numpy(y), n, n, 1, False, end)
    # NumPy, float64: forward, clipped loss, gradient
    tabs = sorted(w)                                   # learner_10, learner_20, region_10, region_20
    z = np.stack([w["region_10sparse_emb_a/embeddings"][ids, 0], w["region_20sparse_emb_a/embeddings"][ids, 0],
                  w["learner_10sparse_emb_a/embeddings"][ids, 0], w["learner_20sparse_emb_a/embeddings"][ids, 0]], axis=1).astype(np.float64)
    mx = RM.mix(z, 2, False, "binary")
    p = mx["out"]
    assert p[0] > 1 - 1e-7 and p[1] < 1e-7 and ((p[2:] > 1e-3) & (p[2:] < 1 - 1e-3)).all()
    pc = np.clip(p, 1e-7, 1 - 1e-7)
    loss = -(y * np.log(pc) + (1 - y) * np.log(1 - pc)).mean()
    assert abs(end.losses[0] - loss) <= 1e-5 * loss
    dp = np.where((p > 1e-7) & (p < 1 - 1e-7), -(y / pc - (1 - y) / (1 - pc)), 0.0) / n
    res = RM.mlr_op([dict(rows=np.concatenate([w[k] for k in ("region_10sparse_emb_a/embeddings", "region_20sparse_emb_a/embeddings",
                                                               "learner_10sparse_emb_a/embeddings", "learner_20sparse_emb_a/embeddings")],
                                              axis=1), ids=ids, col0=0, width=4)], n, 2, False, "binary", d_out=dp)
    after = m.get_weights_by_name()
    for c, k in enumerate(("region_10sparse_emb_a/embeddings", "region_20sparse_emb_a/embeddings", "learner_10sparse_emb_a/embeddings",
                           "learner_20sparse_emb_a/embeddings")):
        want = w[k][:, 0] - lr * res["grads"][0][:, c]
        assert np.abs(after[k][:, 0] - want).max() <= 2e-6 * max(1.0, np.abs(want).max()), k
        assert np.array_equal(after[k][:2], w[k][:2]), k               # the clamped rows: exactly zero gradient
        assert not np.array_equal(after[k][2:], w[k][2:]), k
    assert tabs and all(not t.requires_grad for t in m.weights)


def test_mse_on_the_prediction_uses_it_as_it_is():
    from deepctr_amd import training
    from deepctr_amd.feature_column import DenseFeat, SparseFeat
    from deepctr_amd.models.mlr import MLR
    rng = np.random.RandomState(1)
    cols = [SparseFeat("a", 6, 4), DenseFeat("x", 2)]
    m = MLR(cols, region_num=2, l2_reg_linear=0, task="regression", device="cpu")
    w = {k: rng.standard_normal(v.shape).astype(np.float32) for k, v in m.get_weights_by_name().items()}
    m.set_weights_by_name(w)
    n = 8
    feed = {"a": rng.randint(0, 6, n).astype(np.int32), "x": rng.rand(n, 2).astype(np.float32)}
    y = rng.standard_normal(n).astype(np.float32)
    m.compile(lambda ps: torch.optim.SGD(ps, lr=0.0), "mse")
    staged = _staged_cpu(m, feed, n)
    end = _End()
    training._fit_torch(m, staged, torch.from_numpy(y), n, n, 1, False, end)
    ref, _ = RM.mlr_model(cols, None, None, w, feed, region_num=2, task="regression")
    want = float(((ref.reshape(-1) - y) ** 2).mean())
    assert abs(end.losses[0] - want) <= 1e-5 * want


def test_cpu_fit_on_the_autograd_step_lowers_the_loss():
    """training._fit_torch is device-agnostic torch code: a CPU-built MLR trains on a planted signal, sequences, a bias part and dense
    values included, and every table that sees a gradient moves through its view of the fused rows."""
    from deepctr_amd import training
    from deepctr_amd.feature_column import DenseFeat, SparseFeat, VarLenSparseFeat
    from deepctr_amd.models.mlr import MLR
    rng = np.random.RandomState(4)
    n = 1024
    cols = [SparseFeat("a", 8, 4), SparseFeat("b", 6, 4), VarLenSparseFeat(SparseFeat("s", 7, 4), maxlen=3, combiner="mean"),
            DenseFeat("x", 1)]
    feed = {"a": rng.randint(0, 8, n).astype(np.int32), "b": rng.randint(0, 6, n).astype(np.int32),
            "s": rng.randint(0, 7, (n, 3)).astype(np.int32), "x": rng.rand(n).astype(np.float32)}
    y = ((feed["a"] % 2) ^ (feed["b"] % 3 == 0)).astype(np.float32)
    torch.manual_seed(0)
    np.random.seed(0)
    model = MLR(cols, region_num=3, bias_feature_columns=cols[1:2] + cols[3:], device="cpu")
    # (Zeros() tables give every region the same logit and every learner the same gradient: break the symmetry as a user would)
    model.set_weights_by_name({k: (0.1 * rng.standard_normal(v.shape)).astype(np.float32) for k, v in model.get_weights_by_name().items()})
    model.compile(lambda ps: torch.optim.Adam(ps, lr=0.05), "binary_crossentropy")
    staged = _staged_cpu(model, feed, n)
    w0 = {k: v.copy() for k, v in model.get_weights_by_name().items()}
    m0 = [m.clone() for runs in model.masters.values() for _, _, m in runs]
    end = _End()
    training._fit_torch(model, staged, torch.from_numpy(y), n, 128, 6, True, end)
    assert end.losses[-1] < end.losses[0] - 0.05
    w1 = model.get_weights_by_name()
    assert all(not np.array_equal(w0[k], w1[k]) for k in w0)
    m1 = [m for runs in model.masters.values() for _, _, m in runs]
    assert all(not torch.equal(a, b) for a, b in zip(m0, m1))           # the fused rows followed, in place
    assert all(not t.requires_grad for t in model.weights)
