"""GPU: the forwards of IFM (stage + DNN kernel + dctr_ifm_fwd) and DIFM (+ dctr_interacting_fwd) against the reference's own outputs,
dctr_ifm_fwd against the float64 oracle over a sweep of shapes and options on both routes with bit equality between them, out-of-range
ids, factor_out, live weights, fit() on the autograd step and a seeded mini-fuzz of whole models."""
import numpy as np
import pytest
import torch

from tests import ref_ifm as RI
from tests.test_autoint_cpu import att_rows
from tests.test_gpu_models import check_probs
from tests.test_ifm_cpu import FIXTURES, build_model
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


def _t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _case(device, F, d, B, Ks, mprime, n_lin, i64, pooled, pad, n_add, seed, V=37):
    """Random operands of one op call: (device kwargs of ops.ifm, oracle kwargs).  ``pad``: extra columns behind every matrix, so the
    row strides differ from the widths.  ``pooled``: the positions that arrive as [B] vectors (read at a stride of 1 or 2 floats)."""
    rng = np.random.RandomState(seed)
    x = (rng.standard_normal((B, F * d + pad)) * 0.5).astype(np.float32)
    dev, ref = dict(x=_t(x, device)[:, :F * d + (pad and 1)], fields=F, dim=d), dict(x=x, fields=F, dim=d)
    srcs_d, srcs_r = [], []
    for K in Ks:
        act = rng.standard_normal((B, K + pad)).astype(np.float32)
        w = (rng.standard_normal((K, F)) / np.sqrt(K)).astype(np.float32)
        srcs_d.append((_t(act, device)[:, :K], _t(w, device)))
        srcs_r.append((act[:, :K], w))
    dev["sources"], ref["sources"] = srcs_d, srcs_r
    if mprime:
        mp = rng.standard_normal((B, F + pad)).astype(np.float32)
        dev["mprime"], ref["mprime"] = _t(mp, device)[:, :F + (pad and 2)], mp[:, :F]
    if n_lin:
        terms, lin = [], np.zeros((B, F), dtype=np.float32)
        ids = np.stack([rng.randint(0, V + 3 * k, B) for k in range(F)], axis=1).astype(np.int64 if i64 else np.int32)      # [B, F]
        ids_d = _t(ids, device)
        for k in range(F):
            if k in pooled:
                v = rng.standard_normal((B, 2)).astype(np.float32)
                lin[:, k] = v[:, 0]
                terms.append(_t(v, device)[:, :1] if k % 2 else _t(v[:, 0], device))
            else:
                table = (rng.standard_normal((V + 3 * k, 1)) * 0.3).astype(np.float32)
                lin[:, k] = table[ids[:, k], 0]
                terms.append((_t(table, device), ids_d[:, k]))
        dev["lin"], ref["lin"] = terms, lin
        ref["_ids"], ref["_ids_dev"] = ids, ids_d
    adds = [rng.standard_normal(B).astype(np.float32) for _ in range(n_add)]
    dev["add"], ref["add"] = [_t(a, device) for a in adds], adds
    bias = np.float32(rng.standard_normal() * 0.1)
    dev["global_bias"], ref["bias"] = _t(np.array([bias]), device), float(bias)
    return dev, ref


SWEEP = [  # F, d, B, K per source, m' handed over, first-order terms, int64 ids, pre-pooled positions, padded strides, add vectors
    (1, 1, 5, (3,), False, True, False, (), 0, 0), (2, 3, 17, (), True, True, True, (1,), 3, 1), (3, 5, 33, (7, 21), False, False, False, (), 5, 2),
    (5, 2, 64, (64,), True, True, False, (0, 4), 0, 4), (9, 4, 700, (8,), False, True, False, (3, 4, 5, 6, 7, 8), 1, 1),
    (13, 17, 40, (65, 130), False, True, True, (), 7, 1), (16, 16, 129, (16,), False, True, False, (), 0, 0),
    (17, 8, 63, (1, 2), True, True, False, (16,), 2, 3), (26, 16, 1001, (64,), False, True, False, (), 4, 1),
    (39, 4, 4099, (64,), False, True, False, (), 0, 1),             # Criteo defaults, IFM: 26 sparse + 13 bucketised; a ragged last tile
    (39, 4, 257, (2496, 64), False, True, False, (), 0, 1),         # Criteo defaults, DIFM: the flattened attention output + the DNN
    (26, 4, 16400, (64,), False, True, True, (), 0, 1),
    (7, 64, 21, (100,), False, True, True, (2,), 1, 0), (5, 33, 9, (19,), False, True, False, (), 3, 0), (64, 1, 70, (5,), False, True, False, (), 0, 0),
    (65, 3, 66, (33, 31), False, False, False, (), 1, 2), (200, 4, 35, (77,), False, True, False, (199,), 2, 1),
    (600, 2, 19, (40,), False, True, False, (), 1, 1),               # 4 x [16, 612] floats of m' beside the source chunks: past the LDS
    (577, 1, 130, (9, 70), True, False, False, (), 0, 0),
]


@pytest.mark.parametrize("F,d,B,Ks,mprime,n_lin,i64,pooled,pad,n_add", SWEEP)
def test_ifm_op_vs_float64_oracle(device, F, d, B, Ks, mprime, n_lin, i64, pooled, pad, n_add):
    from deepctr_amd import ops
    dev_kw, ref_kw = _case(device, F, d, B, Ks, mprime, n_lin, i64, pooled, pad, n_add, F * 1000 + d)
    ref_kw = {k: v for k, v in ref_kw.items() if not k.startswith("_")}
    past_lds = F > 560
    n_src = len(Ks)
    if n_src:
        assert ops.ifm_route(B, F, d, n_src) == ("workspace" if past_lds else "lds")
        assert (ops.ifm_workspace_bytes(B, F, d, n_src) > 0) == past_lds
    for softmax in (False, True):
        ref, m = RI.ifm_op(softmax=softmax, **ref_kw)
        terms, _ = RI.ifm_op(softmax=softmax, absolute=True, **ref_kw)
        m_terms = m if softmax else RI.ifm_op(absolute=True, **ref_kw)[1]
        if softmax:
            # (the bound of ifm_op's docstring for m itself: relative e A, A the summed magnitude of m')
            m_terms = m * (1 + 4 * RI.ifm_op(absolute=True, **ref_kw)[1].max(axis=1, keepdims=True))
        outs, facs = [], []
        for route in (None, "workspace"):
            status = ops.new_status(device)
            fac = torch.full((B, F + pad), float("nan"), device=device)
            got = ops.ifm(softmax=softmax, factor_out=fac[:, :F + (pad and 1)], status=status, route=route, **dev_kw)
            assert tuple(got.shape) == (B,) and int(status.item()) == 0
            what = "ifm F=%d d=%d K=%s softmax=%d route=%s" % (F, d, Ks, softmax, route)
            assert_close_terms(got.cpu().numpy(), ref, terms, what=what)
            assert_close_terms(fac[:, :F].cpu().numpy(), m, m_terms, what=what + " factor_out")
            assert torch.isnan(fac[:, F:]).all()                          # nothing behind the F columns is written
            outs.append(got.cpu().numpy())
            facs.append(fac[:, :F].cpu().numpy())
        assert np.array_equal(outs[0], outs[1]) and np.array_equal(facs[0], facs[1])          # the routes give the same bits
    # the probability: sigmoid of the same logit (its slope is <= 1/4, its own value <= 1)
    ref, _ = RI.ifm_op(sigmoid=True, **ref_kw)
    terms, _ = RI.ifm_op(absolute=True, **ref_kw)
    p = [ops.ifm(sigmoid_out=True, route=route, **dev_kw).cpu().numpy() for route in (None, "workspace")]
    assert_close_terms(p[0], ref, 0.25 * terms + 1.0, what="ifm F=%d d=%d sigmoid" % (F, d))
    assert np.array_equal(p[0], p[1])
    if n_src:
        # m' handed over instead of projected in the launch: the same function of it
        mp = sum(a.astype(np.float64) @ w for a, w in ref_kw["sources"]) + (ref_kw["mprime"] if mprime else 0)
        kw = dict(dev_kw, sources=(), mprime=_t(mp.astype(np.float32), device))
        rk = dict(ref_kw, sources=(), mprime=mp.astype(np.float32))
        got = ops.ifm(softmax=True, **kw)
        assert_close_terms(got.cpu().numpy(), RI.ifm_op(softmax=True, **rk)[0], RI.ifm_op(softmax=True, absolute=True, **rk)[0],
                           what="ifm F=%d d=%d, m' handed over" % (F, d))


def test_argument_checks_raise_before_any_launch(device):
    from deepctr_amd import ops
    dev_kw, _ = _case(device, 4, 3, 6, (5,), False, True, False, (), 0, 1, 1)
    bad = [dict(x=dev_kw["x"][:, :11]), dict(x=dev_kw["x"].double()), dict(x=dev_kw["x"].t().contiguous().t()),
           dict(sources=[(dev_kw["sources"][0][0], dev_kw["sources"][0][1][:, :3])]), dict(sources=[(dev_kw["sources"][0][0][:5], dev_kw["sources"][0][1])]),
           dict(sources=dev_kw["sources"] * 3), dict(sources=(), mprime=None), dict(mprime=torch.zeros(6, 3, device=device)),
           dict(lin=dev_kw["lin"][:3]), dict(lin=[torch.zeros(5, device=device)] * 4), dict(add=[torch.zeros(5, device=device)]),
           dict(add=[torch.zeros(6, device=device)] * 5), dict(global_bias=torch.zeros(2, device=device)), dict(out=torch.zeros(5, device=device)),
           dict(factor_out=torch.zeros(6, 3, device=device)), dict(route="lds"), dict(status=torch.zeros(1, device=device)),
           dict(route="workspace", workspace=torch.zeros(4, device=device))]
    for kw in bad:
        with pytest.raises((ValueError, TypeError)):
            ops.ifm(**dict(dev_kw, **kw))
    from deepctr_amd import _C
    with pytest.raises(_C.DctrExtensionError):
        ops.ifm(**dict(dev_kw, add=[torch.zeros(6)]))


@pytest.mark.parametrize("route", [None, "workspace"])
def test_out_of_range_id_sets_the_status_word_and_contributes_zero(device, route):
    from deepctr_amd import ops
    F, d, B = 5, 8, 300
    dev_kw, ref_kw = _case(device, F, d, B, (12,), False, True, False, (), 2, 1, 11)
    bad = ref_kw["_ids"].copy()
    bad[17, 2] = 37 + 3 * 2             # == vocabulary of position 2
    bad[250, 0] = -1
    bad_d = _t(bad, device)
    lin = [(t[0], bad_d[:, k]) for k, t in enumerate(dev_kw["lin"])]
    guard = [t[0].clone() for t in dev_kw["lin"]]
    status = ops.new_status(device)
    got = ops.ifm(status=status, route=route, **dict(dev_kw, lin=lin)).cpu().numpy()
    assert int(status.item()) & 1                                     # DCTR_STATUS_INDEX_OOR
    zeroed = ref_kw["lin"].copy()
    zeroed[17, 2] = 0
    zeroed[250, 0] = 0
    rk = {k: v for k, v in ref_kw.items() if not k.startswith("_")}
    rk["lin"] = zeroed
    assert_close_terms(got, RI.ifm_op(**rk)[0], RI.ifm_op(absolute=True, **rk)[0], what="out-of-range ids enter as zero")
    assert all(torch.equal(a, t[0]) for a, t in zip(guard, dev_kw["lin"]))
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


def _ctor(kind):
    from deepctr_amd import models
    return getattr(models, kind), (dict(att_embedding_size=4, att_head_num=2) if kind == "DIFM" else {})


def _hip_vs_torch(model, feed, n, what):
    from deepctr_amd import engine, training
    staged = engine.Staged(n)
    model._stage_inputs(feed, staged)
    model._begin()
    with torch.no_grad():
        t = training.model_logits(model, staged, 0, n).cpu().numpy()
    assert_close(np.asarray(model.predict_logits(feed, batch_size=n)).reshape(-1), t, rtol=1e-4, atol=2e-5, what=what)


@pytest.mark.parametrize("kind", ["IFM", "DIFM"])
def test_in_place_weight_updates_are_seen_by_the_next_predict(device, kind):
    rng = np.random.RandomState(5)
    n = 257
    cols, feed = _small(rng, n)
    ctor, kw = _ctor(kind)
    model = ctor(cols[::-1], cols, dnn_hidden_units=(16,), device=device, **kw)
    model.set_weights_by_name({k: (rng.standard_normal(v.shape) * 0.3).astype(np.float32) for k, v in model.get_weights_by_name().items()})
    p0 = model.predict(feed, batch_size=n)
    w = dict(model.named_weights())
    for name in ["dense/kernel", "linear0sparse_emb_C1/embeddings", "sparse_emb_C3/embeddings", "linear/linear_kernel",
                 "prediction_layer/global_bias"] + (["dense_1/kernel", "interacting_layer/value"] if kind == "DIFM" else []):
        w[name].mul_(-1.5).add_(0.05)
        p1 = model.predict(feed, batch_size=n)
        assert not np.array_equal(p0, p1), name
        p0 = p1
    _hip_vs_torch(model, feed, n, kind + ": predict after in-place writes vs model_logits")


@pytest.mark.parametrize("kind", ["IFM", "DIFM"])
def test_fit_lowers_the_loss_and_predict_reads_the_current_weights(device, kind):
    rng = np.random.RandomState(9)
    n = 4096
    cols, feed = _small(rng, n)
    y = ((feed["C0"] % 2) ^ (feed["C1"] % 3 == 0)).astype(np.float32)          # planted signal
    ctor, kw = _ctor(kind)
    model = ctor(cols, cols, dnn_hidden_units=(32, 16), device=device, **kw)
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
    _hip_vs_torch(model, sub, 1024, kind + ": predict after fit vs model_logits")
    w = {k: (rng.standard_normal(v.shape) * 0.3).astype(np.float32) for k, v in model.get_weights_by_name().items()}
    model.set_weights_by_name(w)
    okw = dict(dnn_hidden_units=(32, 16), task="regression", dtype=np.float64, **kw)
    ref = RI.input_aware(kind, cols, cols, w, sub, **okw).reshape(-1)
    mag = RI.input_aware(kind, cols, cols, w, sub, absolute=True, **okw).reshape(-1)
    assert_close_terms(np.asarray(model.predict_logits(sub, batch_size=1024)).reshape(-1), ref, mag, rtol_terms=4e-6,
                       what=kind + ": predict after set_weights_by_name vs the float64 oracle")


def test_difm_vector_part_in_the_launch_or_on_the_gemm_in_front(device):
    """DIFM's default projects the attention output inside dctr_ifm_fwd (its second factor source); with vector_part_in_kernel = False
    dctr_sgemm computes m_vec in front and hands it over as m': the same model."""
    g = load_golden("model_difm_h3")
    meta = golden_meta(g)
    model = build_model(meta, device)
    model.set_weights_by_name({k[2:]: v for k, v in g.items() if k.startswith("w/")})
    feed = {k[5:]: v for k, v in g.items() if k.startswith("feed/")}
    rows = att_rows(meta, feed, g["y"].shape[0])
    assert model.vector_part_in_kernel is True
    y0 = model.predict(feed, batch_size=32)
    model.vector_part_in_kernel = False
    y1 = model.predict(feed, batch_size=32)
    check_probs(y0, g["y"], "m_vec in the launch", rows)
    check_probs(y1, g["y"], "m_vec on the GEMM", rows)
    assert_close(y1[rows], y0[rows], rtol=1e-5, atol=1e-6, what="the two forms")


@pytest.mark.parametrize("kind", ["IFM", "DIFM"])
def test_criteo_defaults(device, kind):
    """26 SparseFeat + 13 bucketised SparseFeat of embedding_dim 4 behind the default DNN (and the default 8 heads of 8)."""
    from deepctr_amd import models
    from deepctr_amd.feature_column import SparseFeat
    rng = np.random.RandomState(7)
    n = 4096 + 13
    cols = [SparseFeat("C%d" % i, 2000, 4) for i in range(26)] + [SparseFeat("I%d" % i, 40, 4) for i in range(13)]
    feed = {fc.name: rng.randint(0, fc.vocabulary_size, n).astype(np.int32) for fc in cols}
    model = getattr(models, kind)(cols, cols, device=device)
    assert model.n_fields == 39 and model.stage_plan.in_dim == 156
    w = {k: (rng.standard_normal(v.shape) * (0.3 if k.endswith("embeddings") else 0.1)).astype(np.float32)
         for k, v in model.get_weights_by_name().items()}
    model.set_weights_by_name(w)
    lg = np.asarray(model.predict_logits(feed, batch_size=n)).reshape(-1)
    rows = np.concatenate([np.arange(32), np.arange(n - 32, n)])
    fr = {k: v[rows] for k, v in feed.items()}
    ref = RI.input_aware(kind, cols, cols, w, fr, task="regression", dtype=np.float64).reshape(-1)
    mag = RI.input_aware(kind, cols, cols, w, fr, task="regression", dtype=np.float64, absolute=True).reshape(-1)
    assert_close_terms(lg[rows], ref, mag, rtol_terms=4e-6, what=kind + " criteo logits")
    assert np.array_equal(model.predict(feed, batch_size=n), model.predict(feed, batch_size=n))


def _fuzz_model(seed):
    """One random IFM or DIFM: columns, linear list, feed, constructor arguments.  Max-pooled sequences are non-empty on three rows of
    four, so at least half of the rows are compared whatever else the seed draws (a model carries at most one max-pooled sequence)."""
    from deepctr_amd.feature_column import DenseFeat, SparseFeat, VarLenSparseFeat
    rng = np.random.RandomState(2000 + seed)
    kind = "IFM" if seed % 2 == 0 else "DIFM"
    F, d, n = rng.randint(1, 13), rng.randint(1, 25), 64
    n_seq = rng.randint(0, min(F, 4))
    cols, feed, max_used = [], {}, False
    for i in range(F - n_seq):
        h = bool(rng.rand() < 0.3)
        V = int(rng.randint(3, 40))
        cols.append(SparseFeat("c%d" % i, V, d, use_hash=h, group_name="g1" if rng.rand() < 0.2 else "default_group"))
        feed["c%d" % i] = rng.randint(0, 10 ** 6 if h else V, n).astype(np.int32)
    for i in range(n_seq):
        comb = ["sum", "mean", "max"][rng.randint(0, 3)]
        if comb == "max":
            if max_used:
                comb = "mean"
            max_used = True
        h = bool(rng.rand() < 0.3) and comb != "max"
        V, T = int(rng.randint(4, 30)), int(rng.randint(1, 6))
        use_len = bool(rng.rand() < 0.4)
        cols.append(VarLenSparseFeat(SparseFeat("s%d" % i, V, d, use_hash=h), maxlen=T, combiner=comb,
                                     length_name="s%d_len" % i if use_len else None))
        ids = rng.randint(1, 10 ** 6 if h else V, (n, T)).astype(np.int32)
        lens = rng.randint(0, T + 1, n)
        lens[np.arange(n) % 4 != 3] = np.maximum(lens[np.arange(n) % 4 != 3], 1)
        ids[np.arange(T)[None, :] >= lens[:, None]] = 0
        feed["s%d" % i] = ids
        if use_len:
            feed["s%d_len" % i] = lens.astype(np.int32)
    for i in range(rng.randint(0, 3)):
        cols.append(DenseFeat("x%d" % i, int(rng.randint(1, 4))))
        feed["x%d" % i] = rng.rand(n, cols[-1].dimension).astype(np.float32)
    cols = [cols[i] for i in rng.permutation(len(cols))]
    # the linear list: every sparse / sequence feature in a permuted order, or none of them; any subset of the dense ones
    mode = rng.randint(0, 3)
    lin = [c for c in cols if isinstance(c, DenseFeat) and rng.rand() < 0.7]
    if mode < 2:
        lin += [c for c in cols if not isinstance(c, DenseFeat)]
        lin = [lin[i] for i in rng.permutation(len(lin))]
    kw = dict(dnn_hidden_units=tuple(int(rng.randint(3, 40)) for _ in range(rng.randint(1, 4))))
    if kind == "DIFM":
        kw.update(att_embedding_size=int(rng.randint(1, 9)), att_head_num=int(rng.randint(1, 5)), att_res=bool(rng.rand() < 0.7))
    return rng, kind, cols, lin, feed, kw, n


@pytest.mark.parametrize("seed", range(40))
def test_mini_fuzz_vs_float64_oracle(device, seed):
    from deepctr_amd import models
    rng, kind, cols, lin, feed, kw, n = _fuzz_model(seed)
    model = getattr(models, kind)(lin, cols, device=device, **kw)
    w = {k: (rng.standard_normal(v.shape) * (0.4 if k.endswith("embeddings") else 0.3)).astype(np.float32)
         for k, v in model.get_weights_by_name().items()}
    model.set_weights_by_name(w)
    rows = np.ones(n, dtype=bool)
    for fc in cols:
        if getattr(fc, "combiner", None) == "max":
            rows &= (feed[fc.name] != 0).any(axis=1)
    assert rows.sum() * 2 >= n
    lg = np.asarray(model.predict_logits(feed, batch_size=24)).reshape(-1)
    okw = dict(task="regression", dtype=np.float64, **kw)
    ref = RI.input_aware(kind, lin, cols, w, feed, **okw).reshape(-1)
    mag = RI.input_aware(kind, lin, cols, w, feed, absolute=True, **okw).reshape(-1)
    assert_close_terms(lg[rows], ref[rows], mag[rows], rtol_terms=4e-6, what="fuzz seed %d (%s)" % (seed, kind))
