"""CPU: ONN — the NumPy oracle (tests/ref_onn.py) against the reference's own outputs (tests/golden/model_onn*.npz;
scripts/make_golden_onn.py), the torch restatement the training path uses (training.model_logits) against the oracle, the API
contract (signature, weight names, the fused per-feature tables behind the per-name views, the refusals), the C ABI's argument checks
(no launch) and a CPU fit() on the autograd step."""
import ctypes
import inspect
import itertools

import numpy as np
import pytest
import torch

from tests import ref_onn as RO
from tests.spec import columns_from_spec
from tests.test_autoint_cpu import att_rows
from tests.util import assert_close, golden_meta, load_golden, sigmoid_inv

FIXTURES = ["model_onn", "model_onn_reduce", "model_onn_nobn", "model_onn_hash", "model_onn_regression", "model_onn_nodnn",
            "model_onn_fixed", "model_onn_two", "model_onn_linear_subset"]


def build_model(meta, device, **more):
    from deepctr_amd.models import ONN
    kw = dict(meta["kwargs"])
    kw.update(more)
    return ONN(columns_from_spec(meta["linear"]), columns_from_spec(meta["dnn"]), device=device, **kw)


def _has_hash(meta):
    return any(d.get("use_hash") or d.get("sparsefeat", {}).get("use_hash") for d in meta["dnn"] + meta["linear"])


def _feed(g):
    return {k[5:]: v for k, v in g.items() if k.startswith("feed/")}


def kept_rows(meta, feed, n):
    """att_rows, asserted to keep at least half of the fixture."""
    rows = att_rows(meta, feed, n)
    assert rows.sum() * 2 >= n
    return rows


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_matches_reference_code(name):
    g = load_golden(name)
    meta = golden_meta(g)
    assert meta["model"] == "ONN"
    n = g["y"].shape[0]
    assert g["y"].shape == (n, 1)
    rows = kept_rows(meta, _feed(g), n)
    y, ref = RO.run_fixture(g), g["y"]
    assert y.shape == ref.shape
    y, ref = y[rows], ref[rows]
    if meta["kwargs"].get("task") != "regression":
        assert ((ref > 1e-3) & (ref < 1 - 1e-3)).all()         # none of the compared rows is saturated
    assert_close(y, ref, rtol=1e-4, atol=1e-6, what=name + " prob")
    if meta["kwargs"].get("task") != "regression":
        assert_close(sigmoid_inv(y), sigmoid_inv(ref), rtol=1e-4, atol=2e-5, what=name + " logit")
    y64 = RO.run_fixture(g, np.float64)[rows]
    assert_close(y64, ref, rtol=1e-4, atol=1e-6, what=name + " float64 prob")


def test_fixture_set_is_what_the_recipe_lists():
    g = load_golden("model_onn")
    ws = [k for k in g if k.startswith("w/sparse_emb_")]
    assert len(ws) == 9 * 8                        # F (F - 1) field-aware tables: the diagonal ones are never built
    assert not [k for k in ws if k.split("/")[1] in ("sparse_emb_%s_%s" % (n, n) for n in ("sparse_feature_0", "sequence_sum"))]
    g = load_golden("model_onn_nodnn")
    assert not [k for k in g if k.startswith("w/dnn/")] and g["w/dense/kernel"].shape == (36 * 4 + 4, 1)
    g = load_golden("model_onn_two")
    assert g["w/batch_normalization/gamma"].shape == (1,)
    meta = golden_meta(load_golden("model_onn_linear_subset"))
    names = lambda spec: {d.get("name") or d["sparsefeat"]["name"] for d in spec}     # noqa: E731
    assert names(meta["linear"]) < names(meta["dnn"])


def test_ffm_pairs_is_the_models_interaction():
    """The layer-level oracle over fused tables assembled from the fixture's per-name weights reproduces the pair block."""
    g = load_golden("model_onn_fixed")
    meta = golden_meta(g)
    cols = [fc for fc in columns_from_spec(meta["dnn"]) if hasattr(fc, "vocabulary_size")]
    F = len(cols)
    feed = _feed(g)
    masters = []
    for j, fj in enumerate(cols):
        masters.append(np.stack([g["w/sparse_emb_%s_%s/embeddings" % (fj.name, fi.name)] for i, fi in enumerate(cols) if i != j], axis=1))
    ids = np.stack([feed[fc.name] for fc in cols])
    out = RO.ffm_pairs(ids, masters)
    assert out.shape == (24, F * (F - 1) // 2 * 8)
    p = 0
    for i, j in itertools.combinations(range(F), 2):
        a = g["w/sparse_emb_%s_%s/embeddings" % (cols[i].name, cols[j].name)][feed[cols[i].name]]
        b = g["w/sparse_emb_%s_%s/embeddings" % (cols[j].name, cols[i].name)][feed[cols[j].name]]
        assert np.allclose(out[:, p * 8:(p + 1) * 8], a.astype(np.float64) * b)
        p += 1
    red = RO.ffm_pairs(ids, masters, reduce_sum=True)
    assert np.allclose(red, out.reshape(24, -1, 8).sum(-1))
    assert (RO.ffm_pairs(ids, masters, absolute=True) >= np.abs(out)).all()


@pytest.mark.parametrize("name", FIXTURES)
def test_torch_restatement_matches_oracle(name):
    from deepctr_amd import engine, training
    g = load_golden(name)
    meta = golden_meta(g)
    if _has_hash(meta):
        pytest.skip("integer Hash runs in a HIP kernel; the GPU suite covers this fixture")
    model = build_model(meta, torch.device("cpu"))
    model.set_weights_by_name({k[2:]: v for k, v in g.items() if k.startswith("w/")})
    feed = _feed(g)
    n = g["y"].shape[0]
    staged = engine.Staged(n)
    model._stage_inputs(feed, staged)
    model._begin()
    with torch.no_grad():
        logit = training.model_logits(model, staged, 0, n).numpy().astype(np.float64).reshape(-1)
    ref = RO.run_fixture(g, np.float64, task="regression").reshape(-1)
    rows = kept_rows(meta, feed, n)
    assert_close(logit[rows], ref[rows], rtol=1e-4, atol=2e-5, what=name + " model_logits")


def test_signature_defaults_match_the_reference():
    from deepctr_amd.models import ONN
    params = inspect.signature(ONN).parameters
    want = dict(dnn_hidden_units=(256, 128, 64), l2_reg_embedding=1e-5, l2_reg_linear=1e-5, l2_reg_dnn=0, dnn_dropout=0, seed=1024,
                use_bn=True, reduce_sum=False, task='binary', device=None)
    assert list(params) == ["linear_feature_columns", "dnn_feature_columns"] + list(want)
    for k, v in want.items():
        assert params[k].default == v, k


@pytest.mark.parametrize("name", FIXTURES)
def test_weight_names_and_shapes_match_the_fixture(name):
    g = load_golden(name)
    model = build_model(golden_meta(g), torch.device("cpu"))
    mine = {k: tuple(v.shape) for k, v in model.get_weights_by_name().items()}
    ref = {k[2:]: tuple(v.shape) for k, v in g.items() if k.startswith("w/") and not k.startswith("w/linearsparse_")}
    assert mine == ref
    assert model.count_params() == sum(int(np.prod(s)) for s in ref.values())


def test_per_name_weights_are_views_of_one_table_per_feature():
    g = load_golden("model_onn")
    meta = golden_meta(g)
    model = build_model(meta, torch.device("cpu"))
    F, d = model.n_fields, model.emb_dim
    assert (F, d) == (9, 4) and len(model.masters) == F
    names = [fc.name for fc in model.deep_cols]
    assert names[:3] == ["sparse_feature_0", "sparse_feature_1", "sparse_feature_2"]          # SparseFeat first, then VarLenSparseFeat
    w = dict(model.named_weights())
    ptrs = set()
    for j, nj in enumerate(names):
        m = model.masters[j]
        assert tuple(m.shape) == (model.deep_cols[j].vocabulary_size, F - 1, d) and m.is_contiguous()
        for i, ni in enumerate(names):
            if i == j:
                assert "sparse_emb_%s_%s/embeddings" % (nj, ni) not in w
                continue
            t = w["sparse_emb_%s_%s/embeddings" % (nj, ni)]
            k = i if i < j else i - 1
            assert t.data_ptr() == m[:, k, :].data_ptr() and t.stride() == (d * (F - 1), 1)
            ptrs.add(t.data_ptr())
    assert len(ptrs) == F * (F - 1)
    # one name written through the API changes exactly that slot of the master
    before = [m.clone() for m in model.masters]
    new = np.full((7, 4), 2.5, dtype=np.float32)
    model.set_weights_by_name({"sparse_emb_sparse_feature_2_sequence_sum/embeddings": new}, strict=False)
    j, i = names.index("sparse_feature_2"), names.index("sequence_sum")
    for q, (m, b) in enumerate(zip(model.masters, before)):
        if q != j:
            assert torch.equal(m, b)
    diff = (model.masters[j] != before[j]).any(dim=0).any(dim=-1)
    assert diff.nonzero().reshape(-1).tolist() == [i - 1]
    assert np.array_equal(model.get_weights_by_name()["sparse_emb_sparse_feature_2_sequence_sum/embeddings"], new)
    # the round trip through every name leaves the model reproducing the fixture's weights
    model.set_weights_by_name({k[2:]: v for k, v in g.items() if k.startswith("w/")})
    for k, v in model.get_weights_by_name().items():
        assert np.array_equal(v, g["w/" + k]), k


def test_trainable_false_freezes_every_table_of_the_feature():
    from deepctr_amd import training
    from deepctr_amd.feature_column import DenseFeat, SparseFeat
    from deepctr_amd.models import ONN
    cols = [SparseFeat("a", 5, 4, trainable=False), SparseFeat("b", 6, 4), SparseFeat("c", 7, 4), DenseFeat("x", 1)]
    m = ONN(cols, cols, dnn_hidden_units=(8,), device="cpu")
    frozen = training.frozen_weights(m)
    w = dict(m.named_weights())
    assert {n for n, t in w.items() if t.data_ptr() in frozen} == {"sparse_emb_a_b/embeddings", "sparse_emb_a_c/embeddings",
                                                                        "linear0sparse_emb_a/embeddings"}


def test_construction_errors_match_the_reference():
    from deepctr_amd.feature_column import DenseFeat, SparseFeat, VarLenSparseFeat
    from deepctr_amd.models import ONN
    one = [SparseFeat("a", 5, 4), DenseFeat("c", 1)]
    with pytest.raises(ValueError, match="at least 2"):
        ONN(one, one, device="cpu")
    with pytest.raises(ValueError, match="at least 2"):
        ONN(one, [DenseFeat("c", 1)], device="cpu")
    mixed = [SparseFeat("a", 5, 4), VarLenSparseFeat(SparseFeat("s", 6, 8), maxlen=3)]
    with pytest.raises(ValueError, match=r"embedding_dim, got \[4, 8\]"):
        ONN(mixed, mixed, device="cpu")
    shared = [SparseFeat("a", 5, 4), VarLenSparseFeat(SparseFeat("s", 5, 4, embedding_name="a"), maxlen=3)]
    with pytest.raises(ValueError, match="embedding_name"):
        ONN(shared, shared, device="cpu")
    ok = [SparseFeat("a", 5, 4), SparseFeat("b", 6, 4)]
    m = ONN([], ok, dnn_hidden_units=(), device="cpu")           # no linear part, no dense value, no hidden layer: runs in the reference
    assert m.dnn_in_dim == 4 and tuple(m.dense.w("kernel").shape) == (4, 1)


def test_regularized_weights_cover_every_field_aware_table():
    from deepctr_amd import training
    g = load_golden("model_onn_fixed")
    model = build_model(golden_meta(g), "cpu", l2_reg_linear=0.1, l2_reg_embedding=0.2, l2_reg_dnn=0.3)
    names = {t.data_ptr(): n for n, t in model.named_weights()}
    got = sorted((names[t.data_ptr()], l2) for t, l2 in training.regularized_weights(model))
    want = sorted([(n, 0.2) for n, _ in model.named_weights() if n.startswith("sparse_emb_")] +
                  [(n, 0.1) for n, _ in model.named_weights() if n.startswith("linear")] +
                  [(n, 0.3) for n, _ in model.named_weights() if n.startswith("dnn/kernel")])
    assert got == want and sum(1 for n, _ in got if n.startswith("sparse_emb_")) == 30


def test_reference_import_names():
    import deepctr
    import deepctr_amd.models
    from deepctr.models import ONN
    from deepctr.models.onn import ONN as O2
    assert ONN is deepctr_amd.models.ONN is O2 is deepctr.models.ONN


def test_cost_model():
    """The byte counts DESIGN.md §4.11 quotes (Criteo shape: 26 fields, 13 dense)."""
    F, P = 26, 325
    for d, read, written, width in ((4, 10400, 5252, 1313), (16, 41600, 20852, 5213)):
        assert F * (F - 1) * d * 4 == read and (P * d + 13) * 4 == written and P * d + 13 == width
    assert 2 * (1313 * 256 + 256 * 128 + 128 * 64 + 64) == 754304 and 2 * (5213 * 256 + 256 * 128 + 128 * 64 + 64) == 2751104


def _args(**kw):
    from deepctr_amd import _C
    base = dict(batch=4, n_fields=4, dim=3, reduce_sum=0, n_dense=0, out_stride=20, out_offset=0, route=0)
    base.update(kw)
    return _C.ffm.Args(**base)


def test_abi_argument_errors_without_a_gpu():
    from deepctr_amd import _C
    lib = _C.lib()
    f = lambda a: lib.dctr_ffm_fwd(ctypes.byref(a), None)   # noqa: E731
    full = dict(fields=16, out=16)
    assert lib.dctr_ffm_fwd(None, None) == -1
    assert f(_args()) == -1                                          # fields / out missing
    for k in full:
        a = dict(full)
        del a[k]
        assert f(_args(**a)) == -1, k
    assert f(_args(n_fields=1, **full)) == -2                        # F < 2
    assert f(_args(n_fields=0, **full)) == -2
    assert f(_args(dim=0, **full)) == -2                             # d <= 0
    assert f(_args(dim=-3, **full)) == -2
    assert f(_args(batch=-1, **full)) == -2
    assert f(_args(out_stride=18, **full)) == -3                     # 18 columns fit, but the row stride must be a multiple of 4
    assert f(_args(out_stride=16, **full)) == -2                     # 6 pairs x 3 = 18 columns
    assert f(_args(out_offset=4, **full)) == -2
    assert f(_args(out_offset=-4, **full)) == -2
    assert f(_args(reduce_sum=1, out_stride=4, **full)) == -2        # 6 scalars
    assert f(_args(n_dense=3, out_stride=20, **full)) == -2          # 18 + 3 columns
    assert f(_args(n_dense=2, dense_stride=2, **full)) == -1         # dense values without a dense matrix
    assert f(_args(n_dense=2, dense=16, dense_stride=1, **full)) == -2
    assert f(_args(scale=16, **full)) == -1                          # scale and shift come together
    assert f(_args(shift=16, **full)) == -1
    assert f(_args(route=3, **full)) == -4
    assert f(_args(route=-1, **full)) == -4
    assert f(_args(workspace=4096 + 4, workspace_bytes=64, **full)) == -3
    assert b"ffm_fwd" in lib.dctr_last_error()
    assert f(_args(batch=0, **full)) == 0                            # empty batch: a no-op
    assert f(_args(batch=0, reduce_sum=1, out_stride=8, n_dense=2, dense=16, dense_stride=2, scale=16, shift=16, status=16, **full)) == 0


def test_routes_and_workspace_without_a_gpu():
    from deepctr_amd import _C, ops
    # neither route keeps state off chip: no shape needs a workspace
    for F, d in ((2, 1), (26, 4), (26, 16), (60, 16), (9, 17), (200, 64)):
        for n in (3, 4096, 65536):
            assert ops.ffm_workspace_bytes(n, F, d) == 0 and ops.ffm_workspace_bytes(n, F, d, route="direct") == 0
    # the LDS route holds whole samples: F (F-1) d 4 bytes each (10.4 KB and 41.6 KB at the Criteo shape; 226 KB at F = 60, d = 16)
    for F, d in ((2, 1), (2, 64), (26, 4), (26, 16), (9, 17), (39, 8), (13, 17), (60, 8)):
        assert ops.ffm_route(1000, F, d) == "lds", (F, d)
        assert ops.ffm_route(1000, F, d, route="direct") == "direct"
        assert ops.ffm_route(1000, F, d, reduce_sum=True) == "lds"
    for F, d in ((60, 16), (200, 4), (100, 32), (30, 64)):
        assert F * (F - 1) * d * 4 > 160 * 1024
        assert ops.ffm_route(5, F, d) == "direct" and ops.ffm_route(70000, F, d) == "direct", (F, d)
    with pytest.raises(_C.DctrError):
        ops.ffm_route(5, 1, 4)
    with pytest.raises(ValueError, match="route"):
        ops.ffm_route(5, 4, 4, route="lds")


def test_args_mirrors_have_the_layout_the_c_compiler_gives_the_header(tmp_path):
    import os
    import shutil
    import subprocess
    from deepctr_amd import _C
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    structs = (("dctr_ffm_args_t", _C.ffm.Args), ("dctr_ffm_field_t", _C.ffm.Field))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dctr.h"', "int main(void) {",
             '    printf("enums %d %d %d %d\\n", DCTR_FFM_ROUTE_AUTO, DCTR_FFM_ROUTE_DIRECT, DCTR_FFM_ROUTE_LDS, DCTR_ABI_VERSION);']
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
            assert [int(v) for v in vals] == [_C.ffm.ROUTE_AUTO, _C.ffm.ROUTE_DIRECT, _C.ffm.ROUTE_LDS, 13]   # additions only
            continue
        cname, fname = field.split(".")
        cls = by_name[cname]
        want = ctypes.sizeof(cls) if fname == "sizeof" else getattr(cls, fname).offset
        assert int(vals[0]) == want, "%s: C says %s, ctypes %d" % (field, vals[0], want)
        seen.add(field)
    assert seen == {"%s.%s" % (c, f) for c, cls in structs for f in ["sizeof"] + [n for n, _ in cls._fields_]}


def test_cpu_fit_on_the_autograd_step_lowers_the_loss():
    """training._fit_torch is device-agnostic torch code: a CPU-built ONN trains on a planted signal, sequences and BatchNormalization
    included, and every field-aware table that sees a gradient moves through its view of the fused table."""
    from deepctr_amd import engine, training
    from deepctr_amd.feature_column import DenseFeat, SparseFeat, VarLenSparseFeat
    from deepctr_amd.models import ONN
    rng = np.random.RandomState(4)
    n = 1024
    cols = [SparseFeat("a", 8, 4), SparseFeat("b", 6, 4), VarLenSparseFeat(SparseFeat("s", 7, 4), maxlen=3, combiner="mean"),
            DenseFeat("x", 1)]
    feed = {"a": rng.randint(0, 8, n).astype(np.int32), "b": rng.randint(0, 6, n).astype(np.int32),
            "s": rng.randint(0, 7, (n, 3)).astype(np.int32), "x": rng.rand(n).astype(np.float32)}
    y = ((feed["a"] % 2) ^ (feed["b"] % 3 == 0)).astype(np.float32)
    torch.manual_seed(0)
    np.random.seed(0)
    model = ONN(cols, cols, dnn_hidden_units=(16, 8), dnn_dropout=0.1, device="cpu")
    model.compile(lambda ps: torch.optim.Adam(ps, lr=0.01), "binary_crossentropy")
    staged = engine.Staged(n)
    model._stage_inputs(feed, staged)
    yt = torch.from_numpy(y)
    w0 = {k: v.copy() for k, v in model.get_weights_by_name().items()}
    m0 = [m.clone() for m in model.masters]
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
    moved = [k for k in w0 if not np.array_equal(w0[k], w1[k])]
    assert {k for k in w0 if k.startswith("sparse_emb_")} <= set(moved)
    assert "batch_normalization/moving_mean" in moved and "batch_normalization/gamma" in moved
    assert all(not torch.equal(a, b) for a, b in zip(m0, model.masters))          # the fused tables followed, in place
    assert all(not t.requires_grad for t in model.weights)
