"""GPU: FwFM's and DeepFEFM's forward (dctr_fieldpair_fwd + the DNN kernel) against the reference's own outputs, the field-pair kernel
against the float64 oracle over a seeded sweep of shapes (both kinds, every output combination, both routes), the two layers against
the layer fixture, and fit() on the autograd step, after which (and after set_weights_by_name or an in-place write) the HIP forward
reads the current weights."""
import numpy as np
import pytest
import torch

from tests import ref_fefm as RF
from tests.test_autoint_cpu import att_rows
from tests.test_fefm_cpu import FIXTURES, LAYER_TAGS, build_model
from tests.test_gpu_models import check_probs
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
    assert rows.sum() >= 0.5 * rows.size
    for bs in (256, 5):
        check_probs(model.predict(feed, batch_size=bs), g["y"], "%s bs=%d" % (name, bs), rows)
    y = model.predict([feed[n] for n in model.input_names], batch_size=64)
    check_probs(y, g["y"], name + " list feed", rows)
    model.span_rows = 0
    model.span_batches = False
    y1 = model.predict(feed, batch_size=7)
    check_probs(y1, g["y"], name + " bs=7, no spans", rows)
    assert_close(y1[rows], y[rows], rtol=2e-6, atol=2e-7, what=name + ": spans vs per-batch calls")


SWEEP = [  # F, E, batch
    (2, 1, 5), (2, 3, 17), (3, 4, 33), (26, 16, 1001), (26, 16, 70), (13, 17, 40), (39, 8, 19), (7, 32, 21), (5, 64, 9), (4, 5, 100),
    (6, 12, 8200),              # two sub-tiles of 16 samples per workgroup, a ragged last tile
    (26, 16, 16400),            # the same at the Criteo shape
    (60, 16, 6),                # 1,770 pairs: several chunks of the pair table
    (200, 16, 5), (200, 32, 18), (300, 20, 3),      # the last three: one tile exceeds the LDS -> general route
]


@pytest.mark.parametrize("F,E,B", SWEEP)
def test_fieldpair_op_vs_float64_oracle(device, F, E, B):
    from deepctr_amd import ops
    rng = np.random.RandomState(F * 1000 + E)
    P = F * (F - 1) // 2
    off, D = 3, 5                                  # the group's slice starts at column 3 of a strided buffer, like a group of dnn_in
    xbuf = rng.standard_normal((B, off + F * E + D)).astype(np.float32)
    x = xbuf[:, off:off + F * E].reshape(B, F, E).astype(np.float64)
    ws = [(rng.standard_normal((E, E)) / np.sqrt(E)).astype(np.float32) for _ in range(P)]
    r = rng.standard_normal((F, F)).astype(np.float32)
    add = rng.standard_normal(B).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)    # noqa: E731
    xt, wt, rt, addt = t(xbuf), [t(w) for w in ws], t(r), t(add)
    general = F >= 200
    assert (ops.fieldpair_workspace_bytes(B, F, E, "fefm") > 0) == general

    ref = RF.fefm_layer(x, ws)
    terms = RF.fefm_layer(np.abs(x), [np.abs(w) for w in ws])
    # FEFM, both outputs: the scalars into a strided row behind `off + D` untouched columns, the row sum plus `add`
    outbuf = torch.full((B, off + D + P + 7), float("nan"), device=device)
    pairs, logit = ops.fieldpair(xt, wt, kind="fefm", fields=F, dim=E, x_offset=off, pairs=outbuf, pairs_offset=off + D, logit=True,
                                 add=addt)
    assert pairs is outbuf and tuple(logit.shape) == (B,)
    got = outbuf[:, off + D:off + D + P].cpu().numpy()
    assert np.isfinite(got).all() and torch.isnan(outbuf[:, :off + D]).all() and torch.isnan(outbuf[:, off + D + P:]).all()
    assert_close_terms(got, ref, terms, what="FEFM pairs F=%d E=%d" % (F, E))
    assert_close_terms(logit.cpu().numpy(), ref.sum(-1) + add, terms.sum(-1) + np.abs(add), what="FEFM logit + add F=%d E=%d" % (F, E))
    # pairs alone (3-D input, a new tensor), logit alone without add
    x3 = t(x)
    p2, l2 = ops.fieldpair(x3, wt, kind="fefm", pairs=True)
    assert l2 is None and tuple(p2.shape) == (B, P)
    assert_close_terms(p2.cpu().numpy(), ref, terms, what="FEFM pairs only")
    p3, l3 = ops.fieldpair(x3, wt, kind="fefm", logit=True)
    assert p3 is None
    assert_close_terms(l3.cpu().numpy(), ref.sum(-1), terms.sum(-1), what="FEFM logit only")
    # FwFM: the strided slice with add, the 3-D input without; the lower triangle and the diagonal never enter
    fref = RF.fwfm_layer(x, r).reshape(-1)
    fterms = RF.fwfm_layer(np.abs(x), np.abs(r)).reshape(-1)
    _, fl = ops.fieldpair(xt, rt, kind="fwfm", fields=F, dim=E, x_offset=off, add=addt)
    assert_close_terms(fl.cpu().numpy(), fref + add, fterms + np.abs(add), what="FwFM logit + add F=%d E=%d" % (F, E))
    r2 = r.copy()
    r2[np.tril_indices(F)] = np.nan
    _, fl2 = ops.fieldpair(x3, t(r2), kind="fwfm")
    assert_close_terms(fl2.cpu().numpy(), fref, fterms, what="FwFM logit, NaN below the diagonal")


def test_fieldpair_reads_the_live_weights(device):
    """The kernel forms W + W^T from the per-name tensors themselves: an in-place write is seen by the next call."""
    from deepctr_amd import ops
    rng = np.random.RandomState(3)
    B, F, E = 37, 5, 8
    x = rng.standard_normal((B, F, E))
    ws = [rng.standard_normal((E, E)).astype(np.float32) for _ in range(F * (F - 1) // 2)]
    wt = [torch.from_numpy(w).to(device) for w in ws]
    xt = torch.from_numpy(x.astype(np.float32)).to(device)
    p0, _ = ops.fieldpair(xt, wt, kind="fefm", pairs=True)
    ws[3] = ws[3] * 0.5 + 1.0
    wt[3].mul_(0.5).add_(1.0)
    p1, _ = ops.fieldpair(xt, wt, kind="fefm", pairs=True)
    assert not torch.equal(p0[:, 3], p1[:, 3]) and torch.equal(p0[:, :3], p1[:, :3]) and torch.equal(p0[:, 4:], p1[:, 4:])
    assert_close_terms(p1.cpu().numpy(), RF.fefm_layer(x.astype(np.float32), ws), RF.fefm_layer(np.abs(x), [np.abs(w) for w in ws]),
                       what="after an in-place write")


@pytest.mark.parametrize("tag", LAYER_TAGS)
def test_layers_match_the_layer_fixture(device, tag):
    from deepctr_amd.layers import FEFMLayer, FwFMLayer
    g = load_golden("fwfm_fefm_layer")
    x, r, w = g["fwfm_%s_x" % tag], g["fwfm_%s_r" % tag], g["fefm_%s_w" % tag]
    B, F, E = x.shape
    xt = torch.from_numpy(x).to(device)
    layer = FwFMLayer(num_fields=F, device=device)
    layer.build((None, F, E))
    layer.set_weights([r])
    y = layer(xt)
    assert tuple(y.shape) == (B, 1)
    assert_close_terms(y.cpu().numpy(), g["fwfm_%s_y" % tag], RF.fwfm_layer(np.abs(x), np.abs(r)), what="FwFMLayer " + tag)
    x2 = g["fefm_%s_x" % tag]
    fl = FEFMLayer(1e-5, device=device)
    fl.build((None, F, E))
    fl.set_weights(list(w))
    y = fl(torch.from_numpy(x2).to(device))
    assert tuple(y.shape) == (B, F * (F - 1) // 2)
    assert_close_terms(y.cpu().numpy(), g["fefm_%s_y" % tag], RF.fefm_layer(np.abs(x2), np.abs(w)), what="FEFMLayer " + tag)


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


@pytest.mark.parametrize("which", ["FwFM", "DeepFEFM"])
def test_fit_lowers_the_loss_and_predict_reads_the_current_weights(device, which):
    from deepctr_amd import models
    rng = np.random.RandomState(9)
    n = 8192
    cols, feed = _small(rng, n)
    y = ((feed["C0"] % 2) ^ (feed["C1"] % 3 == 0)).astype(np.float32)          # planted signal
    model = getattr(models, which)(cols, cols, dnn_hidden_units=(32, 16), device=device)
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
    # new weights by name: the pair-matrix table follows the tensors (rewritten in place)
    w = {k: (rng.standard_normal(v.shape) * (0.1 if k.endswith("embeddings") else 0.3)).astype(np.float32)
         for k, v in model.get_weights_by_name().items()}
    model.set_weights_by_name(w)
    _hip_vs_torch(model, sub, 1024, "predict after set_weights_by_name vs model_logits")
    fn = RF.fwfm if which == "FwFM" else RF.deepfefm
    ref = fn(cols, cols, w, sub, dnn_hidden_units=(32, 16), task="regression", dtype=np.float64).reshape(-1)
    mag = fn(cols, cols, {k: np.abs(v) for k, v in w.items()}, sub, dnn_hidden_units=(32, 16), task="regression",
             dtype=np.float64).reshape(-1)
    assert_close_terms(np.asarray(model.predict_logits(sub, batch_size=1024)).reshape(-1), ref, mag, rtol_terms=4e-6,
                       what="predict after set_weights_by_name vs the float64 oracle")
    # one weight changed in place
    lg0 = np.asarray(model.predict_logits(sub, batch_size=1024)).reshape(-1)
    t = model.fwfm_layers[0].field_strengths if which == "FwFM" else model.fefm.matrices[2]
    t.mul_(-1.5)
    lg1 = np.asarray(model.predict_logits(sub, batch_size=1024)).reshape(-1)
    assert not np.allclose(lg0, lg1)
    _hip_vs_torch(model, sub, 1024, "predict after an in-place write vs model_logits")


@pytest.mark.parametrize("which", ["FwFM", "DeepFEFM"])
def test_criteo_defaults(device, which):
    from deepctr_amd import models
    from deepctr_amd.feature_column import DenseFeat, SparseFeat
    rng = np.random.RandomState(7)
    V, n = 100000, 4096 + 13
    cols = [SparseFeat("C%d" % i, V, 16) for i in range(26)] + [DenseFeat("I%d" % i, 1) for i in range(13)]
    feed = {"C%d" % i: rng.randint(0, V, n).astype(np.int32) for i in range(26)}
    feed.update({"I%d" % i: rng.rand(n).astype(np.float32) for i in range(13)})
    model = getattr(models, which)(cols, cols, device=device)
    if which == "DeepFEFM":
        assert model.dnn_in_dim == 26 * 16 + 13 + 325
    w = {k: (rng.standard_normal(v.shape) * (0.05 if k.endswith("embeddings") else 0.1)).astype(np.float32)
         for k, v in model.get_weights_by_name().items()}
    model.set_weights_by_name(w)
    lg = np.asarray(model.predict_logits(feed, batch_size=n)).reshape(-1)
    rows = np.concatenate([np.arange(32), np.arange(n - 32, n)])
    fr = {k: v[rows] for k, v in feed.items()}
    fn = RF.fwfm if which == "FwFM" else RF.deepfefm
    ref = fn(cols, cols, w, fr, task="regression", dtype=np.float64).reshape(-1)
    mag = fn(cols, cols, {k: np.abs(v) for k, v in w.items()}, fr, task="regression", dtype=np.float64).reshape(-1)
    assert_close_terms(lg[rows], ref, mag, rtol_terms=4e-6, what="criteo logits")
    assert np.array_equal(model.predict(feed, batch_size=n), model.predict(feed, batch_size=n))
    _hip_vs_torch(model, feed, n, "criteo HIP forward vs model_logits")
