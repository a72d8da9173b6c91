"""GPU: ONN's forward (dctr_embed_pool pre-pass + dctr_ffm_fwd + the DNN kernel) against the reference's own outputs, the field-aware
kernel against the float64 oracle over a sweep of shapes and options on both routes, out-of-range ids, live weights through the
per-name views, fit() on the autograd step, the Criteo defaults and a seeded mini-fuzz of whole models."""
import numpy as np
import pytest
import torch

from tests import ref_onn as RO
from tests.test_autoint_cpu import att_rows
from tests.test_gpu_models import check_probs
from tests.test_onn_cpu import FIXTURES, build_model
from tests.util import assert_close, assert_close_terms, golden_meta, load_golden

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", FIXTURES)
def test_model_matches_reference_code(device, name):
    g = load_golden(name)
    meta = golden_meta(g)
    model = build_model(meta, device)
    model.set_weights_by_name({k[2:]: v for k, v in g.items() if k.startswith("w/")})
    feed = {k[5:]: v for k, v in g.items() if k.startswith("feed/")}
    rows = att_rows(meta, feed, g["y"].shape[0])
    assert rows.sum() * 2 >= rows.size
    if meta["kwargs"].get("task") != "regression":
        assert ((g["y"][rows] > 1e-3) & (g["y"][rows] < 1 - 1e-3)).all()
    for bs in (256, 5):
        check_probs(model.predict(feed, batch_size=bs), g["y"], "%s bs=%d" % (name, bs), rows)
    y = model.predict([feed[n] for n in model.input_names], batch_size=64)
    check_probs(y, g["y"], name + " list feed", rows)
    model.span_rows = 0
    model.span_batches = False
    y1 = model.predict(feed, batch_size=7)
    check_probs(y1, g["y"], name + " bs=7, no spans", rows)
    assert_close(y1[rows], y[rows], rtol=2e-6, atol=2e-7, what=name + ": spans vs per-batch calls")


def _case(device, F, d, B, seed, bn, nd, i64, off, pooled, V=37):
    """Random operands of one op call: (device kwargs of ops.ffm minus reduce_sum / route, oracle kwargs)."""
    rng = np.random.RandomState(seed)
    R = (F - 1) * d
    vocab = [V + 3 * j for j in range(F)]
    masters = [rng.standard_normal((vocab[j], F - 1, d)).astype(np.float32) for j in range(F)]
    ids = np.stack([rng.randint(0, vocab[j], B) for j in range(F)]).astype(np.int64 if i64 else np.int32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)    # noqa: E731
    dev_m = [t(m) for m in masters]
    pool = None
    if pooled:                                      # the last field arrives pre-pooled, in a buffer with a padded row pitch
        buf = rng.standard_normal((B, R + 5)).astype(np.float32)
        pool = {F - 1: buf[:, :R]}
        dev_m[F - 1] = (t(buf),)
    dense = rng.standard_normal((B, nd + 2)).astype(np.float32) if nd else None
    return dict(ids=t(ids), masters=dev_m, dim=d, dense=None if dense is None else t(dense), n_dense=nd or None), \
        dict(ids=ids, masters=masters, pooled=pool, dense=None if dense is None else dense[:, :nd]), rng


SWEEP = [  # F, d, B, BatchNormalization scale / shift, dense columns, int64 ids, column offset, a pre-pooled field
    (2, 1, 5, True, 0, False, 0, False), (2, 3, 17, False, 3, True, 4, False), (3, 5, 33, True, 2, False, 3, True),
    (13, 17, 40, True, 13, True, 8, False), (4, 4, 3, False, 0, False, 0, False), (9, 8, 700, True, 4, False, 1, True),
    (26, 4, 16400, True, 13, False, 0, False),        # the Criteo shape at the reference's default embedding_dim, a ragged last tile
    (26, 16, 1001, True, 13, False, 4, False), (7, 32, 21, False, 1, True, 2, True), (5, 64, 9, True, 0, False, 0, False),
    (60, 16, 6, True, 5, False, 4, False),            # 226 KB of rows per sample: past the LDS, the direct route
    (30, 64, 9, False, 0, True, 0, True), (200, 4, 5, True, 3, False, 2, False),
]


@pytest.mark.parametrize("F,d,B,bn,nd,i64,off,pooled", SWEEP)
def test_ffm_op_vs_float64_oracle(device, F, d, B, bn, nd, i64, off, pooled):
    from deepctr_amd import ops
    dev_kw, ref_kw, rng = _case(device, F, d, B, F * 1000 + d, bn, nd, i64, off, pooled)
    P = F * (F - 1) // 2
    direct_only = F * (F - 1) * d * 4 > 160 * 1024
    assert ops.ffm_route(B, F, d) == ("direct" if direct_only else "lds")
    assert ops.ffm_workspace_bytes(B, F, d) == 0
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)    # noqa: E731
    for reduce_sum in (False, True):
        W = P if reduce_sum else P * d
        scale = shift = None
        if bn:
            scale, shift = (1.0 + 0.2 * rng.standard_normal(W)).astype(np.float32), (0.1 * rng.standard_normal(W)).astype(np.float32)
        ref = RO.ffm_pairs(reduce_sum=reduce_sum, scale=scale, shift=shift, **ref_kw)
        terms = RO.ffm_pairs(reduce_sum=reduce_sum, scale=scale, shift=shift, absolute=True, **ref_kw)
        assert ref.shape == (B, W + nd)
        outs = []
        for route in (None, "direct"):
            stride = (off + W + nd + 7 + 3) // 4 * 4
            outbuf = torch.full((B, stride), float("nan"), device=device)
            status = ops.new_status(device)
            got = ops.ffm(reduce_sum=reduce_sum, scale=None if scale is None else t(scale), shift=None if shift is None else t(shift),
                          out=outbuf, out_offset=off, status=status, route=route, **dev_kw)
            assert got is outbuf and int(status.item()) == 0
            blk = outbuf[:, off:off + W + nd].cpu().numpy()
            assert np.isfinite(blk).all()
            assert torch.isnan(outbuf[:, :off]).all() and torch.isnan(outbuf[:, off + W + nd:]).all()      # nothing else is written
            assert_close_terms(blk, ref, terms, what="ffm F=%d d=%d reduce=%d route=%s" % (F, d, reduce_sum, route))
            if nd:
                assert np.array_equal(blk[:, W:], ref_kw["dense"])
            outs.append(blk)
        if not reduce_sum:          # one fp32 product (and one fma) per output on either route: the same bits
            assert np.array_equal(outs[0], outs[1])
    # a fresh tensor when no `out` is given: row stride padded to a multiple of 4
    y = ops.ffm(dev_kw["ids"], dev_kw["masters"], dim=d)
    assert tuple(y.shape) == (B, (P * d + 3) // 4 * 4)
    assert_close_terms(y[:, :P * d].cpu().numpy(), RO.ffm_pairs(ref_kw["ids"], ref_kw["masters"], pooled=ref_kw["pooled"]),
                       RO.ffm_pairs(ref_kw["ids"], ref_kw["masters"], pooled=ref_kw["pooled"], absolute=True), what="ffm, new tensor")


def test_ffm_criteo_shape_ragged_batch_both_routes(device):
    """26 fields of embedding_dim 16 at 16,400 rows (a ragged last tile on both routes): the routes agree bit for bit on every row,
    and a sample of rows is compared with the float64 oracle."""
    from deepctr_amd import ops
    F, d, B = 26, 16, 16400
    dev_kw, ref_kw, rng = _case(device, F, d, B, 77, True, 13, False, 0, False, V=500)
    W = 325 * d
    scale, shift = (1.0 + 0.2 * rng.standard_normal(W)).astype(np.float32), (0.1 * rng.standard_normal(W)).astype(np.float32)
    st = torch.from_numpy(scale).to(device), torch.from_numpy(shift).to(device)
    assert ops.ffm_route(B, F, d) == "lds"
    a = ops.ffm(scale=st[0], shift=st[1], **dev_kw)
    b = ops.ffm(scale=st[0], shift=st[1], route="direct", **dev_kw)
    assert tuple(a.shape) == (B, 5216) and torch.equal(a[:, :5213], b[:, :5213])
    rows = np.concatenate([np.arange(48), np.arange(B - 48, B), rng.randint(0, B, 160)])
    sub = dict(ids=ref_kw["ids"][:, rows], masters=ref_kw["masters"], dense=ref_kw["dense"][rows])
    assert_close_terms(a[torch.from_numpy(rows).to(device), :5213].cpu().numpy(), RO.ffm_pairs(scale=scale, shift=shift, **sub),
                       RO.ffm_pairs(scale=scale, shift=shift, absolute=True, **sub), what="ffm criteo d=16")


@pytest.mark.parametrize("route", [None, "direct"])
def test_out_of_range_id_sets_the_status_word_and_corrupts_nothing(device, route):
    from deepctr_amd import ops
    F, d, B = 5, 8, 300
    dev_kw, ref_kw, _ = _case(device, F, d, B, 11, False, 2, False, 4, False)
    bad = ref_kw["ids"].copy()
    bad[2, 17] = 37 + 3 * 2             # == vocabulary_size of field 2
    bad[0, 250] = -1
    kw = dict(dev_kw, ids=torch.from_numpy(bad).to(device))
    W = 10 * d
    outbuf = torch.full((B, 4 + W + 2 + 2), float("nan"), device=device)
    status = ops.new_status(device)
    guard = [m.clone() for m in dev_kw["masters"]]
    ops.ffm(out=outbuf, out_offset=4, status=status, route=route, **kw)
    torch.cuda.synchronize()
    assert int(status.item()) & 1                                     # DCTR_STATUS_INDEX_OOR
    ref = RO.ffm_pairs(**ref_kw)
    got = outbuf[:, 4:4 + W + 2].cpu().numpy()
    ok = np.ones(B, dtype=bool)
    ok[[17, 250]] = False
    assert_close_terms(got[ok], ref[ok], RO.ffm_pairs(absolute=True, **ref_kw)[ok], what="rows beside an out-of-range id")
    assert np.isfinite(got).all()                                    # the two rows: a row of zeros entered their products
    pairs = [(i, j) for i in range(F) for j in range(i + 1, F)]
    for row, f in ((17, 2), (250, 0)):
        blk = got[row, :W].reshape(10, d)
        mine = [p for p, ij in enumerate(pairs) if f in ij]
        assert (blk[mine] == 0).all()
        others = [p for p in range(10) if p not in mine]
        assert_close(blk[others], ref[row, :W].reshape(10, d)[others], rtol=1e-5, atol=1e-6, what="pairs without the bad field")
    assert torch.isnan(outbuf[:, :4]).all() and torch.isnan(outbuf[:, 4 + W + 2:]).all()
    assert all(torch.equal(a, b) for a, b in zip(guard, dev_kw["masters"]))
    with pytest.raises(IndexError):
        ops.check_status(status)


def _small(rng, n, d=8):
    from deepctr_amd.feature_column import DenseFeat, SparseFeat, VarLenSparseFeat
    cols = [SparseFeat("C%d" % i, 50, d) for i in range(5)] + [VarLenSparseFeat(SparseFeat("S", 30, d), maxlen=4, combiner="mean"),
                                                                 DenseFeat("I0", 1)]
    feed = {"C%d" % i: rng.randint(0, 50, n).astype(np.int32) for i in range(5)}
    feed["S"] = rng.randint(0, 30, (n, 4)).astype(np.int32)
    feed["S"][:, 0] = np.maximum(feed["S"][:, 0], 1)
    feed["I0"] = rng.rand(n).astype(np.float32)
    return cols, feed


def _hip_vs_torch(model, feed, n, what):
    from deepctr_amd import engine, training
    staged = engine.Staged(n)
    model._stage_inputs(feed, staged)
    model._begin()
    with torch.no_grad():
        t = training.model_logits(model, staged, 0, n).cpu().numpy()
    assert_close(np.asarray(model.predict_logits(feed, batch_size=n)).reshape(-1), t, rtol=1e-4, atol=2e-5, what=what)


def test_in_place_write_to_one_view_changes_exactly_that_pairs_columns(device):
    from deepctr_amd import models
    rng = np.random.RandomState(5)
    n = 257
    cols, feed = _small(rng, n)
    model = models.ONN(cols, cols, dnn_hidden_units=(16,), use_bn=False, device=device)
    w = {k: (rng.standard_normal(v.shape) * 0.3).astype(np.float32) for k, v in model.get_weights_by_name().items()}
    model.set_weights_by_name(w)
    model.predict(feed, batch_size=n)
    x0 = model._buf[n]["dnn_in"].clone()
    dict(model.named_weights())["sparse_emb_C1_C3/embeddings"].mul_(-2.0)          # field 1 towards field 3: pair (1, 3)
    model.predict(feed, batch_size=n)
    x1 = model._buf[n]["dnn_in"]
    d = 8
    p = [(i, j) for i in range(6) for j in range(i + 1, 6)].index((1, 3))
    changed = (x0 != x1).any(dim=0).nonzero().reshape(-1).tolist()
    assert changed == list(range(p * d, (p + 1) * d))
    assert torch.equal(x1[:, p * d:(p + 1) * d], x0[:, p * d:(p + 1) * d] * -2.0)
    _hip_vs_torch(model, feed, n, "predict after an in-place write vs model_logits")


def test_fit_lowers_the_loss_and_predict_reads_the_current_weights(device):
    from deepctr_amd import models
    rng = np.random.RandomState(9)
    n = 4096
    cols, feed = _small(rng, n)
    y = ((feed["C0"] % 2) ^ (feed["C1"] % 3 == 0)).astype(np.float32)          # planted signal
    model = models.ONN(cols, cols, dnn_hidden_units=(32, 16), device=device)
    model.compile("adam", "binary_crossentropy")
    sub = {k: v[:1024] for k, v in feed.items()}
    p0 = model.predict(sub, batch_size=1024)
    before = model.evaluate(feed, y, batch_size=1024, verbose=0)
    hist = model.fit(feed, y, batch_size=256, epochs=2, verbose=0)
    after = model.evaluate(feed, y, batch_size=1024, verbose=0)
    loss = lambda r: r[0] if isinstance(r, (list, tuple)) else r     # noqa: E731
    assert loss(after) < loss(before)
    assert hist.history["loss"][1] < hist.history["loss"][0]
    assert not np.allclose(model.predict(sub, batch_size=1024), p0)
    _hip_vs_torch(model, sub, 1024, "predict after fit vs model_logits")
    w = {k: (rng.standard_normal(v.shape) * (0.2 if k.endswith("embeddings") else 0.3)).astype(np.float32)
         for k, v in model.get_weights_by_name().items()}
    w["batch_normalization/moving_variance"] = np.abs(w["batch_normalization/moving_variance"]) + 0.5
    model.set_weights_by_name(w)
    _hip_vs_torch(model, sub, 1024, "predict after set_weights_by_name vs model_logits")
    kw = dict(dnn_hidden_units=(32, 16), task="regression", dtype=np.float64)
    ref = RO.onn(cols, cols, w, sub, **kw).reshape(-1)
    mag = RO.onn(cols, cols, w, sub, absolute=True, **kw).reshape(-1)
    assert_close_terms(np.asarray(model.predict_logits(sub, batch_size=1024)).reshape(-1), ref, mag, rtol_terms=4e-6,
                       what="predict after set_weights_by_name vs the float64 oracle")


@pytest.mark.parametrize("d,V", [(4, 100000), (16, 20000)])
def test_criteo_defaults(device, d, V):
    from deepctr_amd import models
    from deepctr_amd.feature_column import DenseFeat, SparseFeat
    rng = np.random.RandomState(7)
    n = 4096 + 13
    cols = [SparseFeat("C%d" % i, V, d) for i in range(26)] + [DenseFeat("I%d" % i, 1) for i in range(13)]
    feed = {"C%d" % i: rng.randint(0, V, n).astype(np.int32) for i in range(26)}
    feed.update({"I%d" % i: rng.rand(n).astype(np.float32) for i in range(13)})
    model = models.ONN(cols, cols, device=device)
    assert model.dnn_in_dim == 325 * d + 13
    w = {}
    for m in model.masters:                         # the fused tables whole: 650 per-name host arrays would be the same bytes
        m.copy_(torch.from_numpy((rng.standard_normal(tuple(m.shape)) * 0.3).astype(np.float32)))
    for k, v in model.named_weights():
        if not k.startswith("sparse_emb_"):
            w[k] = (rng.standard_normal(tuple(v.shape)) * 0.1).astype(np.float32)
    w["batch_normalization/moving_variance"] = np.abs(w["batch_normalization/moving_variance"]) + 0.5
    model.set_weights_by_name(w, strict=False)
    lg = np.asarray(model.predict_logits(feed, batch_size=n)).reshape(-1)
    rows = np.concatenate([np.arange(32), np.arange(n - 32, n)])
    fr = {k: v[rows] for k, v in feed.items()}
    names = ["C%d" % i for i in range(26)]
    for j, nj in enumerate(names):                  # the oracle reads per-name tables: only the rows it will look up
        mj = model.masters[j].cpu().numpy()
        k = 0
        for i, ni in enumerate(names):
            if i != j:
                w["sparse_emb_%s_%s/embeddings" % (nj, ni)] = mj[:, k, :]
                k += 1
    ref = RO.onn(cols, cols, w, fr, task="regression", dtype=np.float64).reshape(-1)
    mag = RO.onn(cols, cols, w, fr, task="regression", dtype=np.float64, absolute=True).reshape(-1)
    assert_close_terms(lg[rows], ref, mag, rtol_terms=4e-6, what="criteo logits d=%d" % d)
    assert np.array_equal(model.predict(feed, batch_size=n), model.predict(feed, batch_size=n))


def _fuzz_model(seed):
    """One random ONN: columns, feed, constructor arguments.  Max-pooled sequences are non-empty on three rows of four, so at least
    half of the rows are compared whatever else the seed draws (a model carries at most one max-pooled sequence)."""
    from deepctr_amd.feature_column import DenseFeat, SparseFeat, VarLenSparseFeat
    rng = np.random.RandomState(1000 + seed)
    F, d, n = rng.randint(2, 13), rng.randint(1, 25), 64
    n_seq = rng.randint(0, min(F, 4))
    cols, feed, max_used = [], {}, False
    for i in range(F - n_seq):
        h = bool(rng.rand() < 0.3)
        V = int(rng.randint(3, 40))
        cols.append(SparseFeat("c%d" % i, V, d, use_hash=h))
        feed["c%d" % i] = rng.randint(0, 10 ** 6 if h else V, n).astype(np.int32)
    for i in range(n_seq):
        comb = ["sum", "mean", "max"][rng.randint(0, 3)]
        if comb == "max":
            if max_used:
                comb = "mean"
            max_used = True
        h = bool(rng.rand() < 0.3) and comb != "max"
        V, T = int(rng.randint(4, 30)), int(rng.randint(1, 6))
        cols.append(VarLenSparseFeat(SparseFeat("s%d" % i, V, d, use_hash=h), maxlen=T, combiner=comb))
        ids = rng.randint(1, 10 ** 6 if h else V, (n, T)).astype(np.int32)
        lens = rng.randint(0, T + 1, n)
        lens[np.arange(n) % 4 != 3] = np.maximum(lens[np.arange(n) % 4 != 3], 1)
        ids[np.arange(T)[None, :] >= lens[:, None]] = 0
        feed["s%d" % i] = ids
    for i in range(rng.randint(0, 3)):
        cols.append(DenseFeat("x%d" % i, 1))
        feed["x%d" % i] = rng.rand(n).astype(np.float32)
    order = rng.permutation(len(cols))
    cols = [cols[i] for i in order]
    lin = [c for c in cols if rng.rand() < 0.7]
    kw = dict(dnn_hidden_units=tuple(int(rng.randint(3, 40)) for _ in range(rng.randint(0, 4))), use_bn=bool(rng.rand() < 0.6),
              reduce_sum=bool(rng.rand() < 0.4))
    return rng, cols, lin, feed, kw, n


@pytest.mark.parametrize("seed", range(40))
def test_mini_fuzz_vs_float64_oracle(device, seed):
    from deepctr_amd import models
    rng, cols, lin, feed, kw, n = _fuzz_model(seed)
    model = models.ONN(lin, cols, device=device, **kw)
    w = {k: (rng.standard_normal(v.shape) * (0.4 if k.endswith("embeddings") else 0.3)).astype(np.float32)
         for k, v in model.get_weights_by_name().items()}
    if kw["use_bn"]:
        w["batch_normalization/moving_variance"] = np.abs(w["batch_normalization/moving_variance"]) + 0.5
    model.set_weights_by_name(w)
    rows = np.ones(n, dtype=bool)
    for fc in cols:
        if getattr(fc, "combiner", None) == "max":
            rows &= (feed[fc.name] != 0).any(axis=1)
    assert rows.sum() * 2 >= n
    lg = np.asarray(model.predict_logits(feed, batch_size=24)).reshape(-1)
    okw = dict(task="regression", dtype=np.float64, **kw)
    ref = RO.onn(lin, cols, w, feed, **okw).reshape(-1)
    mag = RO.onn(lin, cols, w, feed, absolute=True, **okw).reshape(-1)
    assert_close_terms(lg[rows], ref[rows], mag[rows], rtol_terms=4e-6, what="fuzz seed %d" % seed)
