"""GPU: AutoInt's forward (dctr_interacting_fwd + the DNN kernel) against the reference's own outputs and the float64 oracle, the
interacting kernel against the oracle over a seeded sweep of shapes (both routes), and fit() on the autograd step."""
import numpy as np
import pytest
import torch

from tests import ref_autoint as RA
from tests.test_autoint_cpu import AUTOINT_FIXTURES, att_rows, build_autoint
from tests.test_gpu_models import check_probs
from tests.util import assert_close, assert_close_terms, golden_meta, load_golden

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", AUTOINT_FIXTURES)
def test_autoint_matches_reference_code(device, name):
    g = load_golden(name)
    meta = golden_meta(g)
    model = build_autoint(meta, device)
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
    y1 = model.predict(feed, batch_size=37)
    check_probs(y1, g["y"], name + " bs=37, no spans", rows)
    assert_close(y1, y, rtol=2e-6, atol=2e-7, what=name + ": spans vs per-batch calls")


def _weights(rng, E, d, H, L, use_res):
    out, e = [], E
    for _ in range(L):
        out.append([rng.standard_normal((e, d * H)) * (0.6 / np.sqrt(e)) for _ in range(4 if use_res else 3)])
        e = d * H
    return out


SWEEP = [  # F, E, d, H, layers, use_res, scaling, batch
    (1, 3, 8, 2, 1, True, False, 5), (2, 4, 1, 1, 2, False, True, 33), (4, 3, 8, 2, 3, True, True, 5),
    (26, 16, 8, 2, 3, True, False, 1001), (39, 32, 16, 4, 2, False, False, 67), (26, 4, 16, 1, 4, True, True, 130),
    (39, 16, 1, 4, 1, True, False, 17), (100, 16, 8, 2, 2, True, True, 9), (128, 32, 16, 2, 1, False, True, 6),
    (7, 16, 17, 3, 2, True, False, 40), (200, 32, 16, 4, 2, True, False, 11),    # the last: one sample exceeds the LDS -> general route
]


@pytest.mark.parametrize("F,E,d,H,L,use_res,scaling,B", SWEEP)
def test_interacting_op_vs_float64_oracle(device, F, E, d, H, L, use_res, scaling, B):
    from deepctr_amd import ops
    rng = np.random.RandomState(F * 1000 + E * 10 + L)
    ws = _weights(rng, E, d, H, L, use_res)
    pad = 5
    xbuf = rng.standard_normal((B, F * E + pad)).astype(np.float32)       # a strided buffer read in place, like dnn_in
    x = xbuf[:, :F * E].reshape(B, F, E)
    ref = x.astype(np.float64)
    for w in ws:
        ref = RA.interacting_layer(ref, w[0], w[1], w[2], w[3] if use_res else None, d, H, use_res, scaling)
    ref = ref.reshape(B, -1)
    head = rng.standard_normal(F * d * H) * 0.1
    # magnitude bound of the flattened output's terms: the same stack over |x| with |weights| would overflow the softmax's meaning;
    # the bar is 1e-4 relative plus a few ulp of the largest activation of the row
    tw = [[torch.from_numpy(a.astype(np.float32)).to(device) for a in w] for w in ws]
    xt = torch.from_numpy(xbuf).to(device)
    out = torch.full((B, F * d * H + 3), float("nan"), device=device)[:, :F * d * H]
    ops.interacting(xt, tw, d, H, use_res, scaling, fields=F, dim=E, out=out)
    got = out.cpu().numpy().astype(np.float64)
    scale = np.abs(ref).max(axis=1, keepdims=True) + 1e-30
    err = np.abs(got - ref) / (1e-4 * np.abs(ref) + 2e-6 * scale)
    assert np.isfinite(got).all() and err.max() <= 1.0, "max err / bar %.3g" % err.max()
    # the fused head agrees with out . head_w, and both forms together
    ht = torch.from_numpy(head.astype(np.float32)).to(device)
    logit = ops.interacting(xt, tw, d, H, use_res, scaling, fields=F, dim=E, head_w=ht)
    lref = ref @ head
    assert_close_terms(logit.cpu().numpy(), lref, np.abs(ref) @ np.abs(head), rtol_terms=4e-6, what="fused head")
    out2 = torch.empty(B, F * d * H, device=device)
    logit2 = torch.empty(B, device=device)
    ops.interacting(xt, tw, d, H, use_res, scaling, fields=F, dim=E, out=out2, head_w=ht, logit=logit2)
    assert torch.equal(out2, out) and torch.equal(logit2, logit)
    # the 3-D form of the layer API
    if L == 1:
        from deepctr_amd.layers import InteractingLayer
        layer = InteractingLayer(d, H, use_res, scaling, device=device)
        layer.build((None, F, E))
        layer.set_weights([a.astype(np.float32) for a in ws[0]])
        y = layer.call(torch.from_numpy(np.ascontiguousarray(x)).to(device))
        assert tuple(y.shape) == (B, F, d * H) and torch.equal(y.reshape(B, -1), out)


def test_general_route_is_taken_and_layers_chain(device):
    from deepctr_amd import ops
    assert ops.interacting_workspace_bytes(11, 200, 32, 2, 16, 4) > 0         # SWEEP's last shape runs without the LDS tile
    # more than 32 layers: launches chained through out, and through the workspace with the head only
    rng = np.random.RandomState(3)
    F, E, d, H, L, B = 5, 4, 2, 2, 34, 9
    ws = _weights(rng, E, d, H, L, True)
    x = rng.standard_normal((B, F, E))
    ref = x
    for w in ws:
        ref = RA.interacting_layer(ref, *w, d, H, True, False)
    ref = ref.reshape(B, -1)
    tw = [[torch.from_numpy(a.astype(np.float32)).to(device) for a in w] for w in ws]
    xt = torch.from_numpy(x.astype(np.float32)).to(device)
    got = ops.interacting(xt, tw, d, H, True, False).cpu().numpy()
    scale = np.abs(ref).max(axis=1, keepdims=True) + 1e-30
    assert (np.abs(got - ref) <= 1e-4 * np.abs(ref) + 1e-5 * scale).all()
    head = torch.from_numpy(rng.standard_normal(F * d * H).astype(np.float32)).to(device)
    logit = ops.interacting(xt, tw, d, H, True, False, head_w=head).cpu().numpy()
    assert_close(logit, got @ head.cpu().numpy(), rtol=1e-5, atol=1e-6, what="chained head")


def _criteo(rng, n, V=100000):
    from deepctr_amd.feature_column import DenseFeat, SparseFeat
    cols = [SparseFeat("C%d" % i, V, 16) for i in range(26)] + [DenseFeat("I%d" % i, 1) for i in range(13)]
    feed = {"C%d" % i: rng.randint(0, V, n).astype(np.int32) for i in range(26)}
    feed.update({"I%d" % i: rng.rand(n).astype(np.float32) for i in range(13)})
    return cols, feed


def test_autoint_criteo_defaults(device):
    from deepctr_amd import engine, training
    from deepctr_amd.models import AutoInt
    rng = np.random.RandomState(7)
    cols, feed = _criteo(rng, 65536)
    model = AutoInt(cols, cols, device=device)
    w = {k: (rng.standard_normal(v.shape) * (0.05 if k.endswith("embeddings") else 0.1)).astype(np.float32)
         for k, v in model.get_weights_by_name().items()}
    model.set_weights_by_name(w)
    for n in (4096, 65536):
        sub = {k: v[:n] for k, v in feed.items()}
        lg = model.predict_logits(sub, batch_size=n)
        rows = np.concatenate([np.arange(64), np.arange(n - 64, n)])
        fr = {k: v[rows] for k, v in sub.items()}
        ref = RA.autoint(cols, cols, w, fr, task="regression", dtype=np.float64).reshape(-1)
        # the magnitude the head's sum is taken at: |DNN input to the Dense| . |kernel| bounded by the same oracle over |weights|
        mag = RA.autoint(cols, cols, {k: np.abs(v) for k, v in w.items()}, fr, task="regression", dtype=np.float64).reshape(-1)
        assert_close_terms(np.asarray(lg).reshape(-1)[rows], ref, mag, rtol_terms=4e-6, what="criteo %d logits" % n)
        y1 = model.predict(sub, batch_size=n)
        y2 = model.predict(sub, batch_size=n)
        assert np.array_equal(y1, y2)
    # the torch-ops forward (model_logits) agrees on the same rows
    staged = engine.Staged(4096)
    model._stage_inputs({k: v[:4096] for k, v in feed.items()}, staged)
    model._begin()
    with torch.no_grad():
        t = training.model_logits(model, staged, 0, 4096).cpu().numpy()
    assert_close(np.asarray(model.predict_logits({k: v[:4096] for k, v in feed.items()}, batch_size=4096)).reshape(-1), t,
                 rtol=1e-4, atol=2e-5, what="HIP forward vs model_logits")


def test_fit_lowers_the_loss_and_predict_follows(device):
    from deepctr_amd import engine, training
    from deepctr_amd.feature_column import DenseFeat, SparseFeat
    from deepctr_amd.models import AutoInt
    rng = np.random.RandomState(9)
    n = 8192
    cols = [SparseFeat("C%d" % i, 50, 8) for i in range(6)] + [DenseFeat("I0", 1)]
    feed = {"C%d" % i: rng.randint(0, 50, n).astype(np.int32) for i in range(6)}
    feed["I0"] = rng.rand(n).astype(np.float32)
    y = ((feed["C0"] % 2) ^ (feed["C1"] % 3 == 0)).astype(np.float32)          # planted signal
    model = AutoInt(cols, cols, att_layer_num=2, dnn_hidden_units=(32, 16), device=device)
    model.compile("adam", "binary_crossentropy")
    before = model.evaluate(feed, y, batch_size=1024, verbose=0)
    hist = model.fit(feed, y, batch_size=256, epochs=2, verbose=0)
    after = model.evaluate(feed, y, batch_size=1024, verbose=0)
    loss = lambda r: r[0] if isinstance(r, (list, tuple)) else r     # noqa: E731
    assert loss(after) < loss(before)
    assert hist.history["loss"][1] < hist.history["loss"][0]
    staged = engine.Staged(1024)
    sub = {k: v[:1024] for k, v in feed.items()}
    model._stage_inputs(sub, staged)
    model._begin()
    with torch.no_grad():
        t = training.model_logits(model, staged, 0, 1024).cpu().numpy()
    assert_close(np.asarray(model.predict_logits(sub, batch_size=1024)).reshape(-1), t, rtol=1e-4, atol=2e-5,
                 what="predict after fit vs model_logits")
