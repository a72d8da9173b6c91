"""GPU: FiBiNET's forward (dctr_bilinear_fwd + the DNN kernel) against the reference's own outputs, the SENET / bilinear kernel against
the float64 oracle over a seeded sweep of shapes (every mode, both routes), and fit() on the autograd step, after which (and after
set_weights_by_name) the HIP forward reads the current weights."""
import numpy as np
import pytest
import torch

from tests import ref_fibinet as RF
from tests.test_autoint_cpu import att_rows
from tests.test_fibinet_cpu import FIBINET_FIXTURES, build_fibinet
from tests.test_gpu_models import check_probs
from tests.util import assert_close, assert_close_terms, golden_meta, load_golden

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", FIBINET_FIXTURES)
def test_fibinet_matches_reference_code(device, name):
    g = load_golden(name)
    meta = golden_meta(g)
    model = build_fibinet(meta, device)
    model.set_weights_by_name({k[2:]: v for k, v in g.items() if k.startswith("w/")})
    feed = {k[5:]: v for k, v in g.items() if k.startswith("feed/")}
    rows = att_rows(meta, feed, g["y"].shape[0])
    assert rows.sum() >= 0.5 * rows.size
    for bs in (256, 5):
        check_probs(model.predict(feed, batch_size=bs), g["y"], "%s bs=%d" % (name, bs), rows)
    y = model.predict([feed[n] for n in model.input_names], batch_size=64)
    check_probs(y, g["y"], name + " list feed", rows)
    model.span_rows = 0
    model.span_batches = False
    y1 = model.predict(feed, batch_size=7)
    check_probs(y1, g["y"], name + " bs=7, no spans", rows)
    assert_close(y1, y, rtol=2e-6, atol=2e-7, what=name + ": spans vs per-batch calls")


def _case(F, E, btype, seed):
    rng = np.random.RandomState(seed)
    r = max(1, F // 3)
    w1 = rng.standard_normal((F, r)) / np.sqrt(F)
    w2 = np.abs(rng.standard_normal((r, F))) / np.sqrt(r) + 0.1
    n = {"all": 1, "each": F - 1, "interaction": F * (F - 1) // 2}[btype]
    ws = [[rng.standard_normal((E, E)) / np.sqrt(E) for _ in range(n)] for _ in range(2)]
    return rng, w1, w2, ws


def _senet_scale_bound(x, w1, w2):
    """an upper bound of A2 from |x| and |weights| (the magnitude the SENET scalars are summed at)"""
    return (np.abs(x).mean(-1) @ np.abs(w1)) @ np.abs(w2)


SWEEP = [  # F, E, bilinear_type, batch
    (2, 1, "all", 5), (2, 3, "interaction", 17), (3, 4, "each", 33), (26, 16, "interaction", 1001), (26, 16, "all", 70),
    (26, 16, "each", 70), (13, 17, "interaction", 40), (39, 8, "each", 19), (7, 32, "interaction", 21), (5, 64, "all", 9),
    (4, 256, "each", 4), (60, 16, "interaction", 6), (200, 4, "interaction", 5), (200, 4, "each", 18),
    (200, 256, "all", 3),       # the last three: one tile exceeds the LDS -> general route
]


@pytest.mark.parametrize("F,E,btype,B", SWEEP)
def test_senet_bilinear_op_vs_float64_oracle(device, F, E, btype, B):
    from deepctr_amd import ops
    rng, w1, w2, ws = _case(F, E, btype, F * 1000 + E)
    D, pad = 5, 3
    xbuf = rng.standard_normal((B, F * E + D + pad)).astype(np.float32)     # a strided buffer read in place, like dnn_in
    x = xbuf[:, :F * E].reshape(B, F, E).astype(np.float64)
    v = RF.senet(x, w1, w2)
    bs, bx = RF.bilinear(v, ws[0], btype), RF.bilinear(x, ws[1], btype)
    a2m = _senet_scale_bound(x, w1, w2)
    ii, jj = np.triu_indices(F, 1)
    ts = RF.bilinear(np.abs(x), [np.abs(w) for w in ws[0]], btype) * (a2m[:, ii] * a2m[:, jj])[:, :, None]
    tx = RF.bilinear(np.abs(x), [np.abs(w) for w in ws[1]], btype)
    P = F * (F - 1) // 2
    width = 2 * P * E + D
    ref = np.concatenate([np.concatenate([bs, bx], axis=-1).reshape(B, -1), xbuf[:, F * E:F * E + D]], axis=1)
    terms = np.concatenate([np.concatenate([ts, tx], axis=-1).reshape(B, -1), np.abs(xbuf[:, F * E:F * E + D])], axis=1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)    # noqa: E731
    xt, sw = t(xbuf), (t(w1), t(w2))
    tw = [[t(w) for w in layer] for layer in ws]
    if F == 200:
        assert ops.senet_bilinear_workspace_bytes(B, F, E, btype, 0, w1.shape[1]) > 0
    # the model form: strided input with the dense tail, strided output; NaN beyond the width stays untouched
    outbuf = torch.full((B, width + 7), float("nan"), device=device)
    out = outbuf[:, :width]
    ops.senet_bilinear(xt, senet_w=sw, senet_bilinear_w=tw[0], bilinear_w=tw[1], bilinear_type=btype, fields=F, dim=E, dense_cols=D,
                       out=out)
    got = out.cpu().numpy()
    assert np.isfinite(got).all() and torch.isnan(outbuf[:, width:]).all()
    assert_close_terms(got, ref, terms, rtol_terms=8e-6, what="model form F=%d E=%d %s" % (F, E, btype))
    # SENET alone (3-D input) and one bilinear layer alone, each into a strided output
    x3 = t(x)
    so = torch.full((B, F * E + 2), float("nan"), device=device)[:, :F * E]
    ops.senet_bilinear(x3, senet_w=sw, out=so)
    sterm = np.abs(x) * a2m[:, :, None]
    assert_close_terms(so.cpu().numpy(), v.reshape(B, -1), sterm.reshape(B, -1), rtol_terms=8e-6, what="SENET only")
    lo = ops.senet_bilinear(x3, bilinear_w=tw[1], bilinear_type=btype)
    assert tuple(lo.shape) == (B, P * E)
    assert_close_terms(lo.cpu().numpy(), bx.reshape(B, -1), tx.reshape(B, -1), rtol_terms=8e-6, what="bilinear only")
    # the layer API on the list-of-[B,1,E] form, on the small shapes
    if F * E <= 1024 and P <= 400:
        from deepctr_amd.layers import BilinearInteraction, SENETLayer
        inputs = [x3[:, f:f + 1] for f in range(F)]
        sl = SENETLayer(3, device=device)
        sl.build([(None, 1, E)] * F)
        sl.set_weights([w1.astype(np.float32), w2.astype(np.float32)])
        ys = sl(inputs)
        assert len(ys) == F and tuple(ys[0].shape) == (B, 1, E)
        assert torch.equal(torch.cat(ys, dim=1).reshape(B, -1), so)
        bl = BilinearInteraction(btype, device=device)
        bl.build([(None, 1, E)] * F)
        bl.set_weights([w.astype(np.float32) for w in ws[1]])
        yb = bl(inputs)
        assert tuple(yb.shape) == (B, P, E) and torch.equal(yb.reshape(B, -1), lo)


def _small(rng, n):
    from deepctr_amd.feature_column import DenseFeat, SparseFeat
    cols = [SparseFeat("C%d" % i, 50, 8) for i in range(6)] + [DenseFeat("I0", 1)]
    feed = {"C%d" % i: rng.randint(0, 50, n).astype(np.int32) for i in range(6)}
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


@pytest.mark.parametrize("btype", ["interaction", "each"])
def test_fit_lowers_the_loss_and_predict_reads_the_current_weights(device, btype):
    from deepctr_amd.models import FiBiNET
    rng = np.random.RandomState(9)
    n = 8192
    cols, feed = _small(rng, n)
    y = ((feed["C0"] % 2) ^ (feed["C1"] % 3 == 0)).astype(np.float32)          # planted signal
    model = FiBiNET(cols, cols, bilinear_type=btype, dnn_hidden_units=(32, 16), device=device)
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
    # new weights by name: the bilinear tables follow the tensors (rewritten in place)
    w = {k: (rng.standard_normal(v.shape) * (0.1 if k.endswith("embeddings") else 0.3)).astype(np.float32)
         for k, v in model.get_weights_by_name().items()}
    model.set_weights_by_name(w)
    _hip_vs_torch(model, sub, 1024, "predict after set_weights_by_name vs model_logits")
    ref = RF.fibinet(cols, cols, w, sub, bilinear_type=btype, dnn_hidden_units=(32, 16), task="regression",
                     dtype=np.float64).reshape(-1)
    mag = RF.fibinet(cols, cols, {k: np.abs(v) for k, v in w.items()}, sub, bilinear_type=btype, dnn_hidden_units=(32, 16),
                     task="regression", dtype=np.float64).reshape(-1)
    assert_close_terms(np.asarray(model.predict_logits(sub, batch_size=1024)).reshape(-1), ref, mag, rtol_terms=4e-6,
                       what="predict after set_weights_by_name vs the float64 oracle")


def test_fibinet_criteo_defaults(device):
    from deepctr_amd.feature_column import DenseFeat, SparseFeat
    from deepctr_amd.models import FiBiNET
    rng = np.random.RandomState(7)
    V, n = 100000, 4096
    cols = [SparseFeat("C%d" % i, V, 16) for i in range(26)] + [DenseFeat("I%d" % i, 1) for i in range(13)]
    feed = {"C%d" % i: rng.randint(0, V, n).astype(np.int32) for i in range(26)}
    feed.update({"I%d" % i: rng.rand(n).astype(np.float32) for i in range(13)})
    model = FiBiNET(cols, cols, device=device)
    assert model.dnn_in_dim == 10413
    w = {k: (rng.standard_normal(v.shape) * (0.05 if k.endswith("embeddings") else 0.1)).astype(np.float32)
         for k, v in model.get_weights_by_name().items()}
    model.set_weights_by_name(w)
    lg = np.asarray(model.predict_logits(feed, batch_size=n)).reshape(-1)
    rows = np.concatenate([np.arange(32), np.arange(n - 32, n)])
    fr = {k: v[rows] for k, v in feed.items()}
    ref = RF.fibinet(cols, cols, w, fr, task="regression", dtype=np.float64).reshape(-1)
    mag = RF.fibinet(cols, cols, {k: np.abs(v) for k, v in w.items()}, fr, task="regression", dtype=np.float64).reshape(-1)
    assert_close_terms(lg[rows], ref, mag, rtol_terms=4e-6, what="criteo logits")
    assert np.array_equal(model.predict(feed, batch_size=n), model.predict(feed, batch_size=n))
    _hip_vs_torch(model, feed, n, "criteo HIP forward vs model_logits")
