"""GPU: MLR's forward — the model against the reference's outputs (tests/golden/model_mlr*.npz) through predict, dctr_mlr_fwd
(deepctr_amd/csrc/mlr_kernels.hip) against the float64 oracle of tests/ref_mlr.py over a sweep of shapes, its edge cases, and a seeded
mini-fuzz of whole-model configurations against training._mlr_output in float64.

Bars of the op: z — tests.util.assert_close_terms' defaults (1e-4 of the result plus 2e-6 of the summed magnitude); out —
tests.ref_mlr.out_bar: 1e-4 of it plus the first-order propagation of z's 2e-6 allowance (plus, for regression learners, 2e-6 of the
magnitude the R products were summed at), all from the oracle.

Worst err / bar of out over the sweep on an MI355X: 0.011 .. 0.021 per (F, bias) (printed by the sweep test)."""
import numpy as np
import pytest
import torch

from tests import ref_mlr as RM
from tests.test_gpu_models import check_probs
from tests.test_mlr_cpu import FIXTURES, _binary, _feed, _weights, build_model, kept_rows
from tests.util import assert_close, assert_close_terms, golden_meta, load_golden

pytestmark = pytest.mark.gpu

Z_OFF, Z_PAD = 3, 2


def dev(a, device):
    return torch.tensor(np.asarray(a), device=device)       # (a copy: the cases' arrays are read-only)


def dev_fields(case, device):
    """The case's fields on the device: every owner array uploaded once, the fields' rows views of them."""
    owners = [dev(m, device) for m, _ in case["owners"]]
    fields = []
    for f, own, (_, first) in zip(case["fields"], owners, case["owners"]):
        fields.append(dict(rows=own[:, first:], ids=None if f["ids"] is None else dev(f["ids"], device), col0=f["col0"],
                           width=f["width"]))
    return fields, owners


# ---------------------------------------------------------------------------------------------------
# the model against the fixtures
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_through_predict(device, name):
    g = load_golden(name)
    meta = golden_meta(g)
    model = build_model(meta, device)
    model.set_weights_by_name(_weights(g))
    feed = _feed(g)
    n = g["y"].shape[0]
    rows = kept_rows(meta, feed, n)

    def check(y, what):
        assert y.shape == (n, 1) and y.dtype == np.float32
        if _binary(meta):
            check_probs(y, g["y"], what, rows)
        else:
            assert_close(y[rows], g["y"][rows], rtol=1e-4, atol=2e-5, what=what)

    model.span_rows = 0
    model.span_batches = False
    for bs in (256, 5, 7):
        check(model.predict(feed, batch_size=bs), "%s bs=%d" % (name, bs))
    check(model.predict([feed[k] for k in model.input_names], batch_size=64), name + " list feed")


def test_weights_set_through_the_views_change_the_next_predict(device):
    g = load_golden("model_mlr_bias")
    meta = golden_meta(g)
    model = build_model(meta, device)
    model.set_weights_by_name(_weights(g))
    feed = _feed(g)
    y0 = model.predict(feed)
    w = _weights(g)
    key = "learner_30sparse_emb_sparse_feature_0/embeddings"
    w[key] = w[key] + 1.5
    w["linear_8/linear_kernel"] = w["linear_8/linear_kernel"] * -2.0          # the bias part's dense weights
    model.set_weights_by_name({k: w[k] for k in (key, "linear_8/linear_kernel")}, strict=False)
    y1 = model.predict(feed)
    ref = RM.run_fixture(g, weights=w)
    rows = kept_rows(meta, feed, g["y"].shape[0])
    check_probs(y1, ref.astype(np.float32), "after the writes", rows)
    assert np.abs(y1 - y0)[rows].max() > 1e-2


# ---------------------------------------------------------------------------------------------------
# the op against the oracle
# ---------------------------------------------------------------------------------------------------
def _forward(device, case, R, bias, task, B, want_z=True):
    """One call into NaN-filled buffers wider than the data; returns (out, z or None) as numpy after checking the surroundings."""
    from deepctr_amd import ops
    K = case["K"]
    fields, owners = dev_fields(case, device)
    snap = [o.clone() for o in owners]
    dense = None if case["dense"] is None else dev(case["dense"], device)
    dense_w = None if case["dense_w"] is None else dev(case["dense_w"], device)
    obuf = torch.full((B, 3), float("nan"), device=device)
    zbuf = torch.full((B, Z_OFF + K + Z_PAD), float("nan"), device=device) if want_z else None
    status = ops.new_status(device)
    out, z = ops.mlr(fields, R, bias, task, dense=dense, dense_w=dense_w, out=obuf[:, 1], z=zbuf, z_offset=Z_OFF, status=status, batch=B,
                     device=device)
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    assert all(torch.equal(a, b) for a, b in zip(owners, snap)), "an input changed"
    o = obuf.cpu().numpy()
    assert np.isnan(o[:, 0]).all() and np.isnan(o[:, 2]).all() and np.isfinite(o[:, 1]).all()
    if not want_z:
        assert z is None
        return o[:, 1], None
    zz = zbuf.cpu().numpy()
    assert np.isnan(zz[:, :Z_OFF]).all() and np.isnan(zz[:, Z_OFF + K:]).all()
    return o[:, 1], zz[:, Z_OFF:Z_OFF + K]


def _check_forward(device, F, R, bias, B, n_dense, i64, task, seed):
    case = RM.op_case(F, R, bias, B, n_dense, i64, seed)
    res = RM.mlr_op(case["fields"], B, R, bias, task, case["dense"], case["dense_w"])
    out, z = _forward(device, case, R, bias, task, B)
    what = "F=%d R=%d bias=%d B=%d dense=%d i64=%d %s" % (F, R, bias, B, n_dense, i64, task)
    assert_close_terms(z, res["z"], res["z_terms"], what=what + ": z")
    err = np.abs(out.astype(np.float64) - res["out"])
    bar = RM.out_bar(res, task)
    assert (err <= bar).all(), "%s: out: max err / bar = %.3g" % (what, float((err / bar).max()))
    return float((err / bar).max())


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("F", [1, 2, 5, 26])
def test_op_sweep_against_the_oracle(device, F, bias):
    worst, seed = 0.0, 100 * F + int(bias)
    for R in (2, 3, 4, 7, 16, 31):
        for B in (1, 5, 17, 33, 700):
            for n_dense in (0, 3):
                for i64 in (False, True):
                    seed += 1
                    task = "binary" if (seed % 3) else "regression"
                    worst = max(worst, _check_forward(device, F, R, bias, B, n_dense, i64, task, seed))
    print("[mlr_fwd] F=%d bias=%d: worst err / bar of out %.3g" % (F, bias, worst))


def test_sixty_four_columns(device):
    """K = 64: region_num = 32 without a bias part, every lane of a wave one column of one sample."""
    for task in ("binary", "regression"):
        _check_forward(device, 5, 32, False, 33, 3, False, task, 7)


def test_z_is_optional_and_does_not_change_out(device):
    """Without a z operand the kernel is handed a NULL pointer, so there is no buffer in which a stray write could be seen: what can
    be checked is that asking for z does not change a bit of out."""
    case = RM.op_case(5, 4, True, 33, 3, False, 3)
    a, z = _forward(device, case, 4, True, "binary", 33, want_z=True)
    b, none = _forward(device, case, 4, True, "binary", 33, want_z=False)
    assert none is None and (a.view(np.int32) == b.view(np.int32)).all()


@pytest.mark.parametrize("big", [30.0, 1e4, 1e30])
def test_extreme_region_logit_is_a_finite_exact_one_hot(device, big):
    """|z| of 30, 1e4 and 1e30 in one region column: the row maximum is subtracted, so the softmax is finite and one-hot — with
    regression learners (a = z) and no bias part the output IS the chosen learner's logit, bit for bit."""
    from deepctr_amd import ops
    R, B, V = 4, 9, 6
    rng = np.random.RandomState(1)
    m = rng.standard_normal((V, 8)).astype(np.float32)
    ids = (np.arange(B) % V).astype(np.int32)
    hot = np.arange(V) % R
    m[np.arange(V), hot] = big
    m[0, hot[0]] = -big                    # id 0: a hugely NEGATIVE column: the other three share the softmax
    md, idd = dev(m, device), dev(ids, device)
    out, z = ops.mlr([dict(rows=md, ids=idd, col0=0, width=2 * R)], R, False, "regression", z=True, batch=B)
    out, z = out.cpu().numpy(), z.cpu().numpy()
    assert np.isfinite(out).all() and (z.view(np.int32) == m[ids].view(np.int32)).all()
    res = RM.mlr_op([dict(rows=m, ids=ids, col0=0, width=2 * R)], B, R, False, "regression")
    err, bar = np.abs(out - res["out"]), RM.out_bar(res, "regression")
    rows = ids != 0
    if big >= 1e4:
        assert (out[rows].view(np.int32) == m[ids[rows], R + hot[ids[rows]]].view(np.int32)).all()
        assert (err[~rows] <= 1e-4 * np.abs(res["out"][~rows]) + 2e-6 * res["sum_terms"][~rows]).all()
    else:
        assert (err <= bar).all()
    # and binary learners with a bias part stay finite and inside (0, 1)
    m2 = np.concatenate([m, rng.standard_normal((V, 4)).astype(np.float32)], axis=1)
    out2, _ = ops.mlr([dict(rows=dev(m2, device), ids=idd, col0=0, width=2 * R + 1)], R, True, "binary", batch=B)
    out2 = out2.cpu().numpy()
    assert np.isfinite(out2).all() and (out2 >= 0).all() and (out2 <= 1).all()


def test_out_of_range_id_sets_the_status_bit_and_counts_as_a_zero_row(device):
    from deepctr_amd import ops
    R, B = 3, 33
    case = RM.op_case(5, R, True, B, 3, False, 12)
    fields = [dict(f) for f in case["fields"]]
    bad = fields[0]["ids"].copy()
    bad[17] = fields[0]["rows"].shape[0]               # == the vocabulary size
    bad[4] = -1
    fields[0]["ids"] = bad
    res = RM.mlr_op(fields, B, R, True, "binary", case["dense"], case["dense_w"])
    clean = RM.mlr_op(case["fields"], B, R, True, "binary", case["dense"], case["dense_w"])
    dfields, _ = dev_fields(dict(case, fields=fields), device)
    status = ops.new_status(device)
    out, z = ops.mlr(dfields, R, True, "binary", dense=dev(case["dense"], device), dense_w=dev(case["dense_w"], device), z=True,
                     status=status, batch=B)
    assert int(status.item()) & 1                                     # DCTR_STATUS_INDEX_OOR
    with pytest.raises(IndexError):
        ops.check_status(status)
    assert_close_terms(z.cpu().numpy(), res["z"], res["z_terms"], what="z beside an out-of-range id")
    err = np.abs(out.cpu().numpy() - res["out"])
    assert (err <= RM.out_bar(res, "binary")).all()
    assert np.abs(res["z"][17] - clean["z"][17]).max() > 0 and (np.delete(res["z"], [4, 17], 0) == np.delete(clean["z"], [4, 17], 0)).all()


def test_all_ids_equal(device):
    from deepctr_amd import ops
    R, B = 4, 700
    case = RM.op_case(5, R, False, B, 0, True, 13)
    fields = [dict(f, ids=None if f["ids"] is None else np.full_like(f["ids"], 5)) for f in case["fields"]]
    res = RM.mlr_op(fields, B, R, False, "binary")
    dfields, _ = dev_fields(dict(case, fields=fields), device)
    out, z = ops.mlr(dfields, R, False, "binary", z=True, batch=B)
    assert_close_terms(z.cpu().numpy(), res["z"], res["z_terms"], what="all ids equal: z")
    assert (np.abs(out.cpu().numpy() - res["out"]) <= RM.out_bar(res, "binary")).all()


def test_sixty_five_columns_are_declined_and_the_model_answers_through_the_torch_ops(device):
    from deepctr_amd import _C, ops, training
    from deepctr_amd.feature_column import DenseFeat, SparseFeat
    from deepctr_amd.models.mlr import MLR
    R, B = 32, 5
    assert not ops.mlr_supported(R, True) and ops.mlr_supported(R, False)
    m = torch.randn(9, 68, device=device)
    ids = torch.zeros(B, dtype=torch.int32, device=device)
    out = torch.full((B,), float("nan"), device=device)
    z = torch.full((B, 65), float("nan"), device=device)
    status = ops.new_status(device)
    with pytest.raises(_C.DctrError) as e:
        ops.mlr([dict(rows=m, ids=ids, col0=0, width=65)], R, True, "binary", out=out, z=z, status=status, batch=B)
    assert e.value.rc == _C.E_UNSUPPORTED
    with pytest.raises(_C.DctrError) as e:
        ops.mlr_bwd([dict(rows=m, ids=ids, col0=0, width=65)], R, z, out, bias=True, dz=z.clone(), batch=B)
    assert e.value.rc == _C.E_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(z).all() and int(status.item()) == 0
    rng = np.random.RandomState(3)
    cols = [SparseFeat("a", 9, 4), SparseFeat("b", 5, 4), DenseFeat("x", 2)]
    model = MLR(cols, region_num=R, bias_feature_columns=cols[:1], device=device)
    model.set_weights_by_name({k: rng.standard_normal(v.shape).astype(np.float32) for k, v in model.get_weights_by_name().items()})
    n = 40
    feed = {"a": rng.randint(0, 9, n).astype(np.int32), "b": rng.randint(0, 5, n).astype(np.int32), "x": rng.rand(n, 2).astype(np.float32)}
    y = model.predict(feed, batch_size=16)
    staged = model.stage(feed)
    with torch.no_grad():
        ref = training._mlr_output(model, staged, 0, n, dtype=torch.float64).cpu().numpy()
    assert_close(y.reshape(-1), ref, rtol=1e-4, atol=2e-5, what="65 columns through the torch ops")


def test_feeds_of_different_lengths_on_one_model(device):
    """One model, one batch_size, feeds of different lengths one after the other: the id matrix is [F, N], so the descriptors cached
    for one N must not serve another, even where the allocator hands the next feed's matrix the address of the last one's."""
    from deepctr_amd import training
    from deepctr_amd.feature_column import DenseFeat, SparseFeat, VarLenSparseFeat
    from deepctr_amd.models.mlr import MLR
    rng = np.random.RandomState(17)
    cols = [SparseFeat("a", 9, 4), SparseFeat("b", 50, 4), SparseFeat("c", 7, 4), VarLenSparseFeat(SparseFeat("s", 11, 4), maxlen=3),
            DenseFeat("x", 2)]
    model = MLR(cols, region_num=3, bias_feature_columns=cols[1:3], device=device)
    model.set_weights_by_name({k: rng.standard_normal(v.shape).astype(np.float32) for k, v in model.get_weights_by_name().items()})
    model.span_rows = 0
    model.span_batches = False

    def feed_of(n):
        return {"a": rng.randint(0, 9, n).astype(np.int32), "b": rng.randint(0, 50, n).astype(np.int32),
                "c": rng.randint(0, 7, n).astype(np.int32), "s": rng.randint(1, 11, (n, 3)).astype(np.int32),
                "x": rng.rand(n, 2).astype(np.float32)}

    for n in (40, 24, 40, 32, 16, 48, 24, 8, 40):
        feed = feed_of(n)
        y = model.predict(feed, batch_size=8)             # (its staged tensors are released on return: the next feed may get the address)
        staged = model.stage(feed)
        model._begin()
        with torch.no_grad():
            ref = training._mlr_output(model, staged, 0, n, dtype=torch.float64).cpu().numpy()
        del staged
        assert_close(y.reshape(-1), ref, rtol=1e-4, atol=2e-5, what="feed of %d rows" % n)


def test_dense_only_model_has_no_field_at_all(device):
    """No sparse or sequence feature in any list (the reference allows it): dctr_mlr_fwd with n_fields = 0, the dense part alone."""
    from deepctr_amd import ops, training
    from deepctr_amd.feature_column import DenseFeat
    from deepctr_amd.models.mlr import MLR
    rng = np.random.RandomState(18)
    cols = [DenseFeat("x", 3), DenseFeat("y", 1)]
    model = MLR(cols, region_num=4, bias_feature_columns=cols[1:], device=device)
    assert not model.entries
    model.set_weights_by_name({k: rng.standard_normal(v.shape).astype(np.float32) for k, v in model.get_weights_by_name().items()})
    n = 37
    feed = {"x": rng.standard_normal((n, 3)).astype(np.float32), "y": rng.standard_normal(n).astype(np.float32)}
    y = model.predict(feed, batch_size=16)
    staged = model.stage(feed)
    model._begin()
    with torch.no_grad():
        ref = training._mlr_output(model, staged, 0, n, dtype=torch.float64).cpu().numpy()
    assert_close(y.reshape(-1), ref, rtol=1e-4, atol=2e-5, what="dense-only MLR")
    # the op itself, with an empty field list, against the oracle
    dense, dw = rng.standard_normal((n, 4)).astype(np.float32), rng.standard_normal((4, 9)).astype(np.float32)
    res = RM.mlr_op([], n, 4, True, "binary", dense, dw)
    out, z = ops.mlr([], 4, True, "binary", dense=dev(dense, device), dense_w=dev(dw, device), z=True, batch=n)
    assert_close_terms(z.cpu().numpy(), res["z"], res["z_terms"], what="no fields: z")
    assert (np.abs(out.cpu().numpy() - res["out"]) <= RM.out_bar(res, "binary")).all()
    dz = ops.mlr_bwd([], 4, z, torch.ones(n, device=device), bias=True, batch=n)
    ref_b = RM.mlr_op([], n, 4, True, "binary", dense, dw, d_out=np.ones(n), z=z.cpu().numpy())
    assert_close_terms(dz.cpu().numpy(), ref_b["dz"], ref_b["dz_terms"], what="no fields: dz")


# ---------------------------------------------------------------------------------------------------
# whole-model mini-fuzz
# ---------------------------------------------------------------------------------------------------
def _fuzz_config(seed):
    from deepctr_amd.feature_column import DenseFeat, SparseFeat, VarLenSparseFeat
    rng = np.random.RandomState(1000 + seed)
    n = int(rng.choice([1, 7, 64, 300]))
    pool = [SparseFeat("c%d" % i, int(rng.randint(3, 40)), 4, use_hash=bool(rng.rand() < 0.25)) for i in range(int(rng.randint(1, 6)))]
    pool.append(SparseFeat("shared", 11, 4))
    for i in range(int(rng.randint(0, 4))):
        comb = ["sum", "mean", "max"][int(rng.randint(3))]
        kw = {}
        if rng.rand() < 0.4:
            kw["length_name"] = "len%d" % i
        if rng.rand() < 0.4:
            kw.update(weight_name="w%d" % i, weight_norm=bool(rng.rand() < 0.5))
        sf = SparseFeat("s%d" % i, int(rng.randint(4, 20)), 4, embedding_name="shared" if (i == 0 and rng.rand() < 0.5) else None)
        if sf.embedding_name == "shared":
            sf = sf._replace(vocabulary_size=11)
        pool.append(VarLenSparseFeat(sf, maxlen=int(rng.randint(2, 6)), combiner=comb, **kw))
    for i in range(int(rng.randint(0, 3))):
        pool.append(DenseFeat("d%d" % i, int(rng.randint(1, 4))))

    def subset(p):
        got = [fc for fc in pool if rng.rand() < p]
        return got or pool[:1]

    region = subset(0.8)
    base = None if rng.rand() < 0.4 else subset(0.6)
    bias = None if rng.rand() < 0.4 else subset(0.4)
    kw = dict(region_num=int(rng.choice([2, 3, 4, 5, 9])), task="binary" if rng.rand() < 0.7 else "regression", seed=int(rng.randint(99)))
    used = {fc.name: fc for fc in region + (base or []) + (bias or [])}
    feed = {}
    for fc in used.values():
        if isinstance(fc, DenseFeat):
            feed[fc.name] = rng.rand(n, fc.dimension).astype(np.float32)
        elif isinstance(fc, SparseFeat):
            feed[fc.name] = rng.randint(0, 10 ** 6 if fc.use_hash else fc.vocabulary_size, n).astype(np.int64 if fc.use_hash else np.int32)
        else:
            ids = rng.randint(1, fc.vocabulary_size, (n, fc.maxlen)).astype(np.int32)
            lens = rng.randint(1, fc.maxlen + 1, n)                     # (at least one valid position: a max-pool has something to pool)
            ids[np.arange(fc.maxlen)[None, :] >= lens[:, None]] = 0
            feed[fc.name] = ids
            if fc.length_name:
                feed[fc.length_name] = lens.astype(np.int32)
            if fc.weight_name:
                feed[fc.weight_name] = rng.standard_normal((n, fc.maxlen, 1)).astype(np.float32)
    return region, base, bias, kw, feed, n, rng


@pytest.mark.parametrize("seed", range(12))
def test_whole_model_fuzz_against_the_torch_ops_in_float64(device, seed):
    from deepctr_amd import training
    from deepctr_amd.models.mlr import MLR
    region, base, bias, kw, feed, n, rng = _fuzz_config(seed)
    model = MLR(region, base, bias_feature_columns=bias, device=device, **kw)
    model.set_weights_by_name({k: (0.7 * rng.standard_normal(v.shape)).astype(np.float32) for k, v in model.get_weights_by_name().items()})
    y = model.predict(feed, batch_size=int(rng.choice([3, 32, 256])))
    staged = model.stage(feed)
    model._begin()
    with torch.no_grad():
        ref = training._mlr_output(model, staged, 0, n, dtype=torch.float64).cpu().numpy()
    assert y.shape == (n, 1) and np.isfinite(y).all()
    assert_close(y.reshape(-1), ref, rtol=1e-4, atol=2e-5, what="fuzz %d: %s" % (seed, kw))
