"""CPU: FwFM / DeepFEFM / FwFMLayer / FEFMLayer — the NumPy oracle (tests/ref_fefm.py) against the reference's own outputs
(tests/golden/model_fwfm*.npz, model_fefm*.npz, fwfm_fefm_layer.npz; scripts/make_golden_fefm.py), the torch restatement the training
path uses (training.model_logits) against the oracle, the API contract, and the C ABI's argument checks (no launch)."""
import ctypes
import inspect
import itertools

import numpy as np
import pytest
import torch

from tests import ref_fefm as RF
from tests.spec import columns_from_spec
from tests.test_autoint_cpu import att_rows
from tests.util import assert_close, golden_meta, load_golden, sigmoid_inv

FWFM_FIXTURES = ["model_fwfm", "model_fwfm_two_groups", "model_fwfm_nodnn", "model_fwfm_hash", "model_fwfm_regression", "model_fwfm_bn",
                 "model_fwfm_fixed"]
FEFM_FIXTURES = ["model_fefm", "model_fefm_nofefm", "model_fefm_exclude", "model_fefm_nolinear", "model_fefm_noembed",
                 "model_fefm_deep_only", "model_fefm_nodnn", "model_fefm_shallow", "model_fefm_linear_only", "model_fefm_hash",
                 "model_fefm_bn", "model_fefm_fixed"]
FIXTURES = FWFM_FIXTURES + FEFM_FIXTURES
LAYER_TAGS = ["a", "two", "odd", "c", "wide"]      # (B,F,E) = (5,4,3), (3,2,6), (4,6,5), (3,26,16), (2,3,20)


def build_model(meta, device, **more):
    from deepctr_amd import models
    ctor = getattr(models, meta["model"])
    kw = dict(meta["kwargs"])
    kw.update(more)
    return ctor(columns_from_spec(meta["linear"]), columns_from_spec(meta["dnn"]), device=device, **kw)


def _has_hash(meta):
    return any(d.get("use_hash") or d.get("sparsefeat", {}).get("use_hash") for d in meta["dnn"] + meta["linear"])


def _feed(g):
    return {k[5:]: v for k, v in g.items() if k.startswith("feed/")}


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_matches_reference_code(name):
    g = load_golden(name)
    meta = golden_meta(g)
    assert meta["model"] == ("FwFM" if name in FWFM_FIXTURES else "DeepFEFM")
    n = g["y"].shape[0]
    rows = att_rows(meta, _feed(g), n)
    assert rows.sum() >= 0.5 * n                   # at least half of the rows carry no all-padding max-pooled sequence
    y, ref = RF.run_fixture(g), g["y"]
    assert y.shape == ref.shape
    y, ref = y[rows], ref[rows]
    assert_close(y, ref, rtol=1e-4, atol=1e-6, what=name + " prob")
    if meta["kwargs"].get("task") != "regression":
        assert ((ref > 1e-3) & (ref < 1 - 1e-3)).all()         # none of the compared rows is saturated
        assert_close(sigmoid_inv(y), sigmoid_inv(ref), rtol=1e-4, atol=2e-5, what=name + " logit")
    y64 = RF.run_fixture(g, np.float64)[rows]
    assert_close(y64, ref, rtol=1e-4, atol=1e-6, what=name + " float64 prob")


@pytest.mark.parametrize("tag", LAYER_TAGS)
def test_layer_oracles_match_reference_code(tag):
    g = load_golden("fwfm_fefm_layer")
    x = g["fwfm_%s_x" % tag]
    B, F, E = x.shape
    assert g["fwfm_%s_r" % tag].shape == (F, F) and g["fefm_%s_w" % tag].shape == (F * (F - 1) // 2, E, E)
    for dt in (np.float32, np.float64):
        y = RF.fwfm_layer(x, g["fwfm_%s_r" % tag], dtype=dt)
        assert y.shape == g["fwfm_%s_y" % tag].shape == (B, 1)
        assert_close(y, g["fwfm_%s_y" % tag], rtol=1e-4, atol=1e-5, what="fwfm " + tag)
        y = RF.fefm_layer(g["fefm_%s_x" % tag], list(g["fefm_%s_w" % tag]), dtype=dt)
        assert y.shape == g["fefm_%s_y" % tag].shape == (B, F * (F - 1) // 2)
        assert_close(y, g["fefm_%s_y" % tag], rtol=1e-4, atol=1e-5, what="fefm " + tag)


def test_fwfm_reads_the_strict_upper_triangle_only():
    g = load_golden("fwfm_fefm_layer")
    x, r = g["fwfm_a_x"], g["fwfm_a_r"].copy()
    y = RF.fwfm_layer(x, r)
    r[np.tril_indices(r.shape[0])] = 1e6
    assert np.array_equal(RF.fwfm_layer(x, r), y)


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
    ref = RF.run_fixture(g, np.float64, task="regression").reshape(-1)
    rows = att_rows(meta, feed, n)
    assert rows.sum() >= n // 2
    assert_close(logit[rows], ref[rows], rtol=1e-4, atol=2e-5, what=name + " model_logits")


def test_signature_defaults_match_the_reference():
    from deepctr_amd.models import DeepFEFM, FwFM
    params = inspect.signature(FwFM).parameters
    want = dict(fm_group=("default_group",), dnn_hidden_units=(256, 128, 64), l2_reg_linear=0.00001, l2_reg_embedding=0.00001,
                l2_reg_field_strength=0.00001, l2_reg_dnn=0, seed=1024, dnn_dropout=0, dnn_activation='relu', dnn_use_bn=False,
                task='binary', device=None)
    assert list(params) == ["linear_feature_columns", "dnn_feature_columns"] + list(want)
    for k, v in want.items():
        assert params[k].default == v, k
    params = inspect.signature(DeepFEFM).parameters
    want = dict(use_fefm=True, dnn_hidden_units=(256, 128, 64), l2_reg_linear=0.00001, l2_reg_embedding_feat=0.00001,
                l2_reg_embedding_field=0.00001, l2_reg_dnn=0, seed=1024, dnn_dropout=0.0, exclude_feature_embed_in_dnn=False,
                use_linear=True, use_fefm_embed_in_dnn=True, dnn_activation='relu', dnn_use_bn=False, task='binary', device=None)
    assert list(params) == ["linear_feature_columns", "dnn_feature_columns"] + list(want)
    for k, v in want.items():
        assert params[k].default == v, k
    from deepctr_amd.layers import FEFMLayer, FwFMLayer
    sp = inspect.signature(FwFMLayer.__init__).parameters
    assert [(k, sp[k].default) for k in ("num_fields", "regularizer")] == [("num_fields", 4), ("regularizer", 0.000001)]
    fp = inspect.signature(FEFMLayer.__init__).parameters
    assert list(fp)[:2] == ["self", "regularizer"] and fp["regularizer"].default is inspect.Parameter.empty


def test_construction_errors_match_the_reference():
    from deepctr_amd.feature_column import DenseFeat, SparseFeat, VarLenSparseFeat
    from deepctr_amd.layers import FEFMLayer, FwFMLayer
    from deepctr_amd.models import DeepFEFM, FwFM
    one = [SparseFeat("a", 5, 4), DenseFeat("c", 1)]
    for ctor in (FwFM, DeepFEFM):
        with pytest.raises(ValueError, match="at least 2"):
            ctor(one, one, device="cpu")
    mixed = [SparseFeat("a", 5, 4), VarLenSparseFeat(SparseFeat("s", 6, 8), maxlen=3)]
    for ctor in (FwFM, DeepFEFM):
        with pytest.raises(ValueError, match=r"embedding_dim, got \[4, 8\]"):
            ctor(mixed, mixed, device="cpu")
    cols = [SparseFeat("a", 5, 4), SparseFeat("b", 6, 4), SparseFeat("c", 7, 4, group_name="g1")]
    with pytest.raises(ValueError, match="at least 2"):          # a group of one field in fm_group: tf.add_n([]) in the reference
        FwFM(cols, cols, fm_group=("default_group", "g1"), device="cpu")
    with pytest.raises(ValueError, match="fm_group"):
        FwFM(cols, cols, fm_group=("nope",), device="cpu")
    only_g1 = [SparseFeat("a", 5, 4, group_name="g1"), SparseFeat("b", 6, 4, group_name="g1")]
    with pytest.raises(ValueError, match="at least 2"):          # DeepFEFM pairs the default group only
        DeepFEFM(only_g1, only_g1, device="cpu")
    FwFM(only_g1, only_g1, fm_group=("g1",), device="cpu")
    with pytest.raises(NotImplementedError):                     # the eighth combination of deepfefm.py:84-99
        DeepFEFM(cols, cols, dnn_hidden_units=(), use_fefm=False, use_linear=False, device="cpu")
    for kw in (dict(dnn_hidden_units=(), use_fefm=False), dict(dnn_hidden_units=(), use_linear=False), dict(dnn_hidden_units=()),
               dict(use_fefm=False, use_linear=False), dict(use_linear=False), dict(use_fefm=False), dict()):
        DeepFEFM(cols, cols, device="cpu", **kw)
    with pytest.raises(ValueError, match="expect to be 3 dimensions"):
        FwFMLayer(device="cpu").build((None, 4))
    with pytest.raises(ValueError, match="Mismatch in number of fields"):
        FwFMLayer(num_fields=4, device="cpu").build((None, 5, 3))
    with pytest.raises(ValueError, match="expect to be 3 dimensions"):
        FEFMLayer(1e-5, device="cpu").build((None, 4))
    layer = FwFMLayer(num_fields=4, device="cpu")
    layer.build((None, 4, 3))
    with pytest.raises(ValueError, match="expect to be 3 dimensions"):
        layer.call(torch.zeros(2, 12))
    with pytest.raises(ValueError, match="Mismatch in number of fields"):
        layer.call(torch.zeros(2, 5, 3))
    fl = FEFMLayer(1e-5, device="cpu")
    fl.build((None, 4, 3))
    with pytest.raises(ValueError, match="expect to be 3 dimensions"):
        fl.call(torch.zeros(2, 12))


def test_layer_contract():
    from deepctr_amd.layers import FEFMLayer, FwFMLayer, custom_objects
    assert custom_objects["FwFMLayer"] is FwFMLayer and custom_objects["FEFMLayer"] is FEFMLayer
    g = load_golden("fwfm_fefm_layer")
    s = FwFMLayer(num_fields=5, regularizer=0.25, device="cpu")
    s.build((None, 5, 6))
    assert s.name.startswith("fw_fm_layer")
    assert [(n.rsplit("/", 1)[1], tuple(t.shape)) for n, t in s.named_weights()] == [("field_pair_strengths", (5, 5))]
    assert s.compute_output_shape((None, 5, 6)) == (None, 1)
    assert {k: s.get_config()[k] for k in ("num_fields", "regularizer")} == dict(num_fields=5, regularizer=0.25)
    w = s.w("field_pair_strengths")
    assert float(w.abs().max()) <= 0.1 + 1e-6 and float(w.std()) > 0.01       # TruncatedNormal(): stddev 0.05, cut at two
    b = FEFMLayer(0.5, device="cpu")
    b.build((None, 4, 7))
    assert b.name.startswith("fefm_layer")
    names = ["field_embeddings%d-%d" % p for p in itertools.combinations(range(4), 2)]
    assert names == ["field_embeddings0-1", "field_embeddings0-2", "field_embeddings0-3", "field_embeddings1-2", "field_embeddings1-3",
                     "field_embeddings2-3"]
    assert [(n.rsplit("/", 1)[1], tuple(t.shape)) for n, t in b.named_weights()] == [(n, (7, 7)) for n in names]
    assert b.compute_output_shape((None, 4, 7)) == (None, 6)
    assert b.get_config()["regularizer"] == 0.5
    assert not torch.equal(b.matrices[0], b.matrices[1])         # every pair its own draw
    assert g["fefm_a_w"].shape == (6, 3, 3)


@pytest.mark.parametrize("name", FIXTURES)
def test_weight_names_and_shapes_match_the_fixture(name):
    g = load_golden(name)
    model = build_model(golden_meta(g), torch.device("cpu"))
    mine = {k: tuple(v.shape) for k, v in model.get_weights_by_name().items()}
    ref = {k[2:]: tuple(v.shape) for k, v in g.items() if k.startswith("w/") and not k.startswith("w/linearsparse_")}
    assert mine == ref


def test_fit_loss_carries_the_new_l2_penalties():
    """fit()'s reported loss adds l2 * sum(w^2): l2_reg_field_strength over the WHOLE [F,F] field_pair_strengths (keras regularises the
    variable, not the triangle the forward reads), l2_reg_embedding_field over every pair matrix, beside the embedding / linear / DNN
    penalties."""
    from deepctr_amd import training
    g = load_golden("model_fwfm_two_groups")
    model = build_model(golden_meta(g), "cpu", l2_reg_linear=0.1, l2_reg_embedding=0.2, l2_reg_dnn=0.3, l2_reg_field_strength=0.4)
    names = {t.data_ptr(): n for n, t in model.named_weights()}
    got = sorted((names[t.data_ptr()], l2) for t, l2 in training.regularized_weights(model))
    want = sorted([(n, 0.2) for n, _ in model.named_weights() if n.startswith("sparse_")] +
                  [(n, 0.1) for n, _ in model.named_weights() if n.startswith("linear")] +
                  [(n, 0.3) for n, _ in model.named_weights() if n.startswith("dnn/kernel")] +
                  [("fw_fm_layer/field_pair_strengths", 0.4), ("fw_fm_layer_1/field_pair_strengths", 0.4)])
    assert got == want
    reg = dict((names[t.data_ptr()], t) for t, _ in training.regularized_weights(model))
    assert tuple(reg["fw_fm_layer/field_pair_strengths"].shape) == (7, 7)
    g = load_golden("model_fefm_fixed")
    model = build_model(golden_meta(g), "cpu", l2_reg_linear=0.1, l2_reg_embedding_feat=0.2, l2_reg_dnn=0.3, l2_reg_embedding_field=0.6)
    names = {t.data_ptr(): n for n, t in model.named_weights()}
    got = sorted((names[t.data_ptr()], l2) for t, l2 in training.regularized_weights(model))
    want = sorted([(n, 0.2) for n, _ in model.named_weights() if n.startswith("sparse_")] +
                  [(n, 0.1) for n, _ in model.named_weights() if n.startswith("linear")] +
                  [(n, 0.3) for n, _ in model.named_weights() if n.startswith("dnn/kernel")] +
                  [("fefm_layer/field_embeddings%d-%d" % p, 0.6) for p in itertools.combinations(range(6), 2)])
    assert got == want


def test_reference_import_names():
    import deepctr
    import deepctr_amd.models
    from deepctr.layers import FEFMLayer, FwFMLayer
    from deepctr.layers.interaction import FEFMLayer as E2, FwFMLayer as W2
    from deepctr.models import DeepFEFM, FwFM
    from deepctr.models.deepfefm import DeepFEFM as D2
    from deepctr.models.fwfm import FwFM as F2
    assert FwFM is deepctr_amd.models.FwFM is F2 is deepctr.models.FwFM
    assert DeepFEFM is deepctr_amd.models.DeepFEFM is D2 is deepctr.models.DeepFEFM
    assert FwFMLayer is W2 is deepctr_amd.layers.FwFMLayer
    assert FEFMLayer is E2 is deepctr_amd.layers.FEFMLayer


def test_cost_model():
    """The arithmetic DESIGN.md §4.10 quotes (defaults on Criteo-shaped input: F 26, E 16, 13 dense)."""
    from deepctr_amd.models.deepfefm import fieldpair_flops
    assert fieldpair_flops(26, 16) == 2 * 325 * (256 + 16) == 176800
    assert fieldpair_flops(2, 1) == 4
    dnn = 2 * ((26 * 16 + 13 + 325) * 256 + 256 * 128 + 128 * 64 + 64)
    assert dnn == 468096 and dnn + fieldpair_flops(26, 16) == 644896                 # "about 645 kFLOP per sample"


def test_the_pairs_land_in_the_dnn_input_row():
    """DeepFEFM widens the stage's row stride so that the P scalars sit behind the dense columns (embeddings, dense, pairs: the
    reference's order); the ablations that do not feed them to the DNN leave the stage as it is."""
    g = load_golden("model_fefm_fixed")
    meta = golden_meta(g)
    m = build_model(meta, "cpu")
    sp = m.stage_plan
    assert (sp.in_dim, m.n_pairs, m.dnn_in_dim) == (6 * 8 + 3, 15, 66) and sp.out_stride == 68
    assert tuple(m.dnn.kernels[0].shape) == (66, 32)
    for kw, want in ((dict(use_fefm_embed_in_dnn=False), 51), (dict(exclude_feature_embed_in_dnn=True), 15)):
        m = build_model(meta, "cpu", **kw)
        assert m.dnn_in_dim == want and m.stage_plan.out_stride == 52


def _args(**kw):
    from deepctr_amd import _C
    base = dict(batch=4, x_stride=12, x_offset=0, fields=4, dim=3, kind=0, pairs_stride=6, pairs_offset=0)
    base.update(kw)
    return _C.fieldpair.Args(**base)


def test_abi_argument_errors_without_a_gpu():
    from deepctr_amd import _C
    lib = _C.lib()
    f = lambda a: lib.dctr_fieldpair_fwd(ctypes.byref(a), None)   # noqa: E731
    full = dict(x=16, weights=16, pairs_out=16, logit_out=16)
    assert lib.dctr_fieldpair_fwd(None, None) == -1
    assert f(_args()) == -1                                          # x / weights / outputs missing
    assert f(_args(fields=1, x_stride=3, **full)) == -2              # F < 2
    assert f(_args(fields=0, **full)) == -2
    assert f(_args(kind=2, **full)) == -4                            # unknown kind
    assert f(_args(kind=-1, **full)) == -4
    assert f(_args(dim=0, **full)) == -2                             # E < 1
    assert f(_args(x_stride=11, **full)) == -2
    assert f(_args(x_offset=1, **full)) == -2                        # the group's slice ends past the row
    assert f(_args(x_offset=-1, **full)) == -2
    assert f(_args(pairs_stride=5, **full)) == -2                    # 6 pairs
    assert f(_args(pairs_offset=1, **full)) == -2
    assert f(_args(pairs_offset=-1, pairs_stride=9, **full)) == -2
    assert f(_args(kind=1, **full)) == -2                            # FwFM writes no pairs
    assert b"fieldpair" in lib.dctr_last_error()
    for k in ("x", "weights"):
        a = dict(full)
        del a[k]
        assert f(_args(**a)) == -1, k
    assert f(_args(x=16, weights=16)) == -1                          # FEFM: no output at all
    assert f(_args(kind=1, x=16, weights=16)) == -1                  # FwFM: logit_out missing
    assert f(_args(batch=0, **full)) == 0                            # empty batch: a no-op
    assert f(_args(batch=0, x=16, weights=16, pairs_out=16)) == 0    # either output alone will do
    assert f(_args(batch=0, x=16, weights=16, logit_out=16)) == 0
    assert f(_args(batch=0, kind=1, x=16, weights=16, logit_out=16, add=16)) == 0
    # a tile past the LDS: the workspace is required, and must be aligned
    big = dict(fields=200, dim=64, x_stride=200 * 64, pairs_stride=19900, batch=3, **full)
    need = lib.dctr_fieldpair_workspace_bytes(ctypes.byref(_args(**big)))
    assert need > 0
    assert f(_args(**big)) == -1
    assert f(_args(workspace=4096, workspace_bytes=need - 1, **big)) == -1
    assert f(_args(workspace=4096 + 4, workspace_bytes=need, **big)) == -3


def test_workspace_sizes_without_a_gpu():
    from deepctr_amd import _C, ops
    # the LDS route needs none: Criteo defaults (both kinds, every batch size), the layer fixtures' shapes, F = 2
    for n in (5, 4096, 10000, 65536):
        assert ops.fieldpair_workspace_bytes(n, 26, 16, "fefm") == 0
        assert ops.fieldpair_workspace_bytes(n, 26, 16, "fefm", pairs=False) == 0
        assert ops.fieldpair_workspace_bytes(n, 26, 16, "fwfm") == 0
    for F, E in ((4, 3), (2, 6), (6, 5), (3, 20), (2, 1), (39, 8), (7, 32)):
        assert ops.fieldpair_workspace_bytes(9, F, E, "fefm") == 0 and ops.fieldpair_workspace_bytes(9, F, E, "fwfm") == 0
    # a tile too large for the LDS: the general route's slices, independent of the batch
    for kind in ("fefm", "fwfm"):
        big = ops.fieldpair_workspace_bytes(3, 200, 64, kind)
        assert big > 0 and big % 16 == 0 and big == ops.fieldpair_workspace_bytes(70000, 200, 64, kind)
        assert big <= 256 << 20
    assert ops.fieldpair_workspace_bytes(3, 200, 16, "fefm") > 0 and ops.fieldpair_workspace_bytes(3, 200, 4, "fwfm") == 0
    a = _args(fields=1)
    assert _C.lib().dctr_fieldpair_workspace_bytes(ctypes.byref(a)) == 0


def test_args_mirror_has_the_layout_the_c_compiler_gives_the_header(tmp_path):
    import os
    import shutil
    import subprocess
    from deepctr_amd import _C
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    cls = _C.fieldpair.Args
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dctr.h"', "int main(void) {",
             '    printf("sizeof %zu\\n", sizeof(dctr_fieldpair_args_t));',
             '    printf("enums %d %d %d\\n", DCTR_FIELDPAIR_FEFM, DCTR_FIELDPAIR_FWFM, DCTR_ABI_VERSION);']
    for fname, _ in cls._fields_:
        lines.append('    printf("%s %%zu\\n", offsetof(dctr_fieldpair_args_t, %s));' % (fname, fname))
    lines += ["    return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    seen = set()
    for line in filter(None, out):
        field, *vals = line.split()
        if field == "enums":
            assert [int(v) for v in vals] == [_C.fieldpair.FEFM, _C.fieldpair.FWFM, 13]      # additions only: the ABI version stays
            continue
        want = ctypes.sizeof(cls) if field == "sizeof" else getattr(cls, field).offset
        assert int(vals[0]) == want, "%s: C says %s, ctypes %d" % (field, vals[0], want)
        seen.add(field)
    assert seen == {"sizeof"} | {f for f, _ in cls._fields_}
