"""GPU: dctr_interacting_bwd (deepctr_amd/csrc/interacting_bwd_kernels.hip) against the float64 oracle of tests/ref_interacting_bwd.py on
every case of the table there, the differentiable InteractingLayer, and AutoInt / DIFM on the autograd step with the attention stack on
HIP.  The oracle, the cases' ReLU margin, the plan and the room the bar leaves are pinned without a GPU by
tests/test_interacting_bwd_oracle_cpu.py.

Bar of the op: tests.util.assert_close_terms' defaults — 1e-4 of the result plus 2e-6 of the summed magnitude — for every case and
output; none has a bar of its own.  Weight gradients ACCUMULATE, so each starts at a random non-zero g0 of the result's magnitude and
``g - g0`` is compared, |g0| added to ``terms``.  dx is exercised written onto NaN and accumulated onto a sentinel; x, dy and dx sit on row
strides 3, 1 and 2 wider than the row: the padding of dx comes back bit-identical, x, dy and the weights unchanged.  The workspace is
the caller's, filled with NaN, with a guard tail that must come back untouched.

Worst err / bar per case, largest over the outputs (for judging a later change of the bar):
  float32 torch autograd on the CPU (test_interacting_bwd_oracle_cpu.py -s):
      one_field 0.003, d1_h1 0, three_layers 0.11, d17 0.16, criteo 0.68, criteo_walk 0.97, no_res 0.16, past_lds 0.036
  these tests on an MI355X (MEASURED_GPU below; weight gradients vary in the last bits with the order of the workgroups' atomics):
      one_field 0.006, d1_h1 0, three_layers 0.043, d17 0.20, criteo 0.082, criteo_walk 0.044, no_res 0.11, past_lds 0.050
  The worst output is a last-layer weight gradient everywhere but past_lds (dx); every other dx stays below 0.005."""
import functools

import numpy as np
import pytest
import torch

from tests import ref_interacting_bwd as RB
from tests.util import TERMS_REPORT, assert_close, assert_close_terms

pytestmark = pytest.mark.gpu

MEASURED_GPU = {"one_field": 0.0064, "d1_h1": 0.0, "three_layers": 0.043, "d17": 0.20, "criteo": 0.082, "criteo_walk": 0.044,
                "no_res": 0.11, "past_lds": 0.050}        # case -> worst err / bar over its outputs, on an MI355X

GUARD = 4096
SENTINEL = 0.75
PAD_X, PAD_DY, PAD_DX = 3, 1, 2
E_UNSUPPORTED = -5
NAMES = ("query", "key", "value", "res")


def dev(a, device):
    return torch.tensor(np.asarray(a), device=device)       # (a copy: the cases' arrays are read-only)


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def padded(a, pad, device, fill=-3.5):
    a = np.asarray(a, dtype=np.float32).reshape(a.shape[0], -1)
    buf = np.full((a.shape[0], a.shape[1] + pad), fill, dtype=np.float32)
    buf[:, :a.shape[1]] = a
    return dev(buf, device)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """Case, inputs, oracle and g0 of a case: computed once, never modified."""
    case = RB.CASE_BY_NAME[name]
    F, E, d, H, L, use_res, scaling, B = case.shape
    x, weights, dy = RB.case_inputs(case)
    G, T = RB.interacting_bwd(x, weights, d, H, use_res, scaling, dy)
    rng = np.random.RandomState(11 + len(name))
    g0 = {k: (rng.standard_normal(G[k].shape) * max(float(np.sqrt(np.mean(np.square(G[k])))), 1e-3)).astype(np.float32)
          for k in G if k != "dx"}
    return case, x, weights, dy, G, T, g0


def _call(device, name, dx_mode, calls=1):
    """``calls`` identical calls from g0; returns (dx of each call [B, F*E] as numpy, weight gradients of the first, worst err / bar)."""
    from deepctr_amd import ops
    case, x, weights, dy, G, T, g0 = _reference(name)
    F, E, d, H, L, use_res, scaling, B = case.shape
    n, ndy = F * E, F * d * H
    xd, dyd = padded(x, PAD_X, device), padded(dy, PAD_DY, device)
    wd = [[dev(w, device) for w in layer] for layer in weights]
    need = RB.plan(F, E, d, H, L, use_res).workspace_bytes
    assert ops.interacting_bwd_workspace_bytes(B, F, E, L, d, H, use_res) == need
    snap = [bits(t) for t in [xd, dyd] + [w for layer in wd for w in layer]]
    dxs, grads = [], None
    for _ in range(calls):
        dx = torch.full((B, n + PAD_DX), float("nan") if dx_mode == "write" else SENTINEL, device=device)
        if dx_mode == "write":
            dx[:, n:] = SENTINEL
        ws = torch.full((need // 4 + GUARD,), float("nan"), device=device) if need else None
        gd = [[dev(g0["d%s%d" % (NAMES[m], l)], device) for m in range(len(layer))] for l, layer in enumerate(weights)]
        ops.interacting_bwd(xd, wd, d, H, use_res, scaling, dyd[:, :ndy], fields=F, dim=E, dx=dx, accumulate=dx_mode == "add",
                            d_weights=gd, max_blocks=case.max_blocks, workspace=None if ws is None else ws[:need // 4])
        torch.cuda.synchronize()
        if ws is not None:
            assert torch.isnan(ws[need // 4:]).all(), "%s: the guard behind the workspace was written" % name
        assert (bits(dx[:, n:]) == bits(torch.full((B, PAD_DX), SENTINEL))).all(), "%s: dx's padding changed" % name
        dxs.append(dx[:, :n].cpu().numpy())
        grads = grads or gd
    for t, s in zip([xd, dyd] + [w for layer in wd for w in layer], snap):
        assert (bits(t) == s).all(), "%s: an input changed" % name
    worst = {}
    n0 = len(TERMS_REPORT)
    base = SENTINEL if dx_mode == "add" else 0.0
    assert np.isfinite(dxs[0]).all(), "%s: dx holds what it held before (NaN) or a NaN was read" % name
    assert_close_terms(dxs[0].astype(np.float64) - base, G["dx"].reshape(B, n), T["dx"].reshape(B, n) + abs(base), what="%s dx (%s)" % (name, dx_mode))
    worst["dx"] = TERMS_REPORT[n0][4]
    for l, layer in enumerate(grads):
        for m, g in enumerate(layer):
            k = "d%s%d" % (NAMES[m], l)
            n0 = len(TERMS_REPORT)
            got = g.cpu().numpy().astype(np.float64) - g0[k]
            print("[interacting_bwd] %s %s %s" % (name, dx_mode, k), end=" ")
            assert_close_terms(got, G[k], T[k] + np.abs(g0[k]), what="%s %s" % (name, k))
            worst[k] = TERMS_REPORT[n0][4]
            print("%.3g" % worst[k])
    print("[interacting_bwd] %s %s: worst err / bar %.3g (dx %.3g)" % (name, dx_mode, max(worst.values()), worst["dx"]))
    return dxs, grads, worst


@pytest.mark.parametrize("dx_mode", ["write", "add"])
@pytest.mark.parametrize("name", [c.name for c in RB.CASES])
def test_op_against_the_oracle(device, name, dx_mode):
    _call(device, name, dx_mode)


@pytest.mark.parametrize("name", ["criteo_walk", "d17", "past_lds"])
def test_dx_is_bit_identical_from_call_to_call(device, name):
    dxs, _, _ = _call(device, name, "write", calls=2)
    assert (dxs[0].view(np.int32) == dxs[1].view(np.int32)).all()


def test_optional_outputs(device):
    """No dx, no weight gradients, single weight gradients: what is asked for equals the full call's, bit for bit in dx."""
    from deepctr_amd import ops
    case, x, weights, dy, G, T, g0 = _reference("three_layers")
    F, E, d, H, L, use_res, scaling, B = case.shape
    xd, dyd = dev(x, device), dev(dy, device)
    wd = [[dev(w, device) for w in layer] for layer in weights]
    full = torch.zeros(B, F * E, device=device)
    ops.interacting_bwd(xd, wd, d, H, use_res, scaling, dyd, dx=full, d_weights=[[torch.zeros_like(w) for w in layer] for layer in wd])
    only = torch.zeros(B, F * E, device=device)
    ops.interacting_bwd(xd, wd, d, H, use_res, scaling, dyd, dx=only)
    assert (bits(only) == bits(full)).all()
    one = torch.zeros_like(wd[1][2])
    ops.interacting_bwd(xd, wd, d, H, use_res, scaling, dyd, d_weights=[[None] * 4, [None, None, one, None], [None] * 4])
    assert_close_terms(one.cpu().numpy(), G["dvalue1"], T["dvalue1"], what="a single weight gradient")


def test_a_refused_shape_raises_and_writes_nothing(device, monkeypatch):
    from deepctr_amd import _C, ops, training
    F, E, d, H, L, B = 3, 4, 2, 2, 33, 4
    rng = np.random.RandomState(3)
    x = dev(rng.randn(B, F, E).astype(np.float32), device)
    wd = [[dev((rng.randn(E if l == 0 else d * H, d * H) * 0.5).astype(np.float32), device) for _ in range(4)] for l in range(L)]
    dy = dev(rng.randn(B, F * d * H).astype(np.float32), device)
    dx = torch.full((B, F * E), SENTINEL, device=device)
    gd = [[torch.full_like(w, SENTINEL) for w in layer] for layer in wd]
    assert not ops.interacting_bwd_supported(F, E, L, d, H, True)
    with pytest.raises(_C.DctrError) as err:
        ops.interacting_bwd(x, wd, d, H, True, False, dy, dx=dx, d_weights=gd)
    assert err.value.rc == E_UNSUPPORTED
    torch.cuda.synchronize()
    for t in [dx] + [g for layer in gd for g in layer]:
        assert (bits(t) == bits(torch.full_like(t, SENTINEL))).all()
    # the autograd step then takes the torch loop
    calls = []
    monkeypatch.setattr(ops, "interacting_bwd", lambda *a, **k: calls.append(1))
    layers = [RB.Layer([w.clone().requires_grad_(True) for w in layer], d, H, True, False) for layer in wd]
    xg = x.clone().requires_grad_(True)
    y = training.interacting_stack(layers, xg)
    want = xg
    for layer in layers:
        want = training._interacting(layer, want)
    assert torch.equal(y, want)
    y.backward(dy.reshape(B, F, d * H))
    assert not calls and xg.grad is not None


# ---------------------------------------------------------------------------------------------------
# the layer
# ---------------------------------------------------------------------------------------------------
def _normalised(got, ref, gmax, what, rtol=5e-4, atol=1e-5):
    """The bar of tests/test_gpu_flen.py:_normalised: relative to the tensor's largest gradient, at least 1e-2 of the step's."""
    scale = max(float(np.abs(ref).max()), 1e-2 * gmax)
    assert_close(np.asarray(got) / scale, np.asarray(ref) / scale, rtol=rtol, atol=atol, what=what)


@pytest.mark.parametrize("use_res,scaling", [(True, False), (False, True)])
def test_layer_is_differentiable(device, use_res, scaling):
    from deepctr_amd import training
    from deepctr_amd.layers import InteractingLayer
    rng = np.random.RandomState(4)
    B, F, E = 37, 6, 8
    layer = InteractingLayer(4, 2, use_res=use_res, scaling=scaling, device=device).build_for(E)
    x = dev(rng.randn(B, F, E).astype(np.float32), device)
    dy = dev(rng.randn(B, F, 8).astype(np.float32), device)
    plain = layer(x)
    assert plain.grad_fn is None and plain.shape == (B, F, 8)
    ws = [w for w in layer.weights_qkvr if w is not None]
    xg = x.clone().requires_grad_(True)
    try:
        for w in ws:
            w.requires_grad_(True)
        with torch.no_grad():
            y0 = layer(xg)
        assert y0.grad_fn is None and torch.equal(y0, plain)
        y = layer(xg)
        assert y.grad_fn is not None and torch.equal(y.detach(), plain)
        y.backward(dy)
        got = [xg.grad] + [w.grad for w in ws]
        assert all(g is not None for g in got)
        got = [g.cpu().numpy() for g in got]
        for w in ws:
            w.grad = None
        xr = x.clone().requires_grad_(True)
        training._interacting(layer, xr).backward(dy)
        ref = [xr.grad.cpu().numpy()] + [w.grad.cpu().numpy() for w in ws]
    finally:
        for w in ws:
            w.requires_grad_(False)
            w.grad = None
    gmax = max(float(np.abs(r).max()) for r in ref)
    for k, (g, r) in enumerate(zip(got, ref)):
        _normalised(g, r, gmax, "layer gradient %d" % k)
    # weights only: x needs no gradient and gets none
    try:
        ws[0].requires_grad_(True)
        y = layer(x)
        assert y.grad_fn is not None
        y.backward(dy)
        _normalised(ws[0].grad.cpu().numpy(), ref[1], gmax, "d query alone")
    finally:
        ws[0].requires_grad_(False)
        ws[0].grad = None


# ---------------------------------------------------------------------------------------------------
# the models
# ---------------------------------------------------------------------------------------------------
def _model(kind, device):
    from deepctr_amd import models
    from deepctr_amd.feature_column import DenseFeat, SparseFeat
    if kind == "difm":
        cols = [SparseFeat("s%d" % i, 9 + i, embedding_dim=8) for i in range(5)]
        return cols, models.DIFM(cols, cols, att_head_num=2, dnn_hidden_units=(32, 16), seed=5, device=device)
    cols = [SparseFeat("s%d" % i, 9 + i, embedding_dim=8) for i in range(6)] + [DenseFeat("v", 1)]
    hidden = () if kind == "autoint_nodnn" else (32, 16)
    return cols, models.AutoInt(cols, cols, att_layer_num=2, dnn_hidden_units=hidden, seed=5, device=device)


def _feed(cols, n, rng):
    feed = {}
    for c in cols:
        if hasattr(c, "vocabulary_size"):
            feed[c.name] = rng.randint(0, c.vocabulary_size, n).astype(np.int32)
        else:
            feed[c.name] = rng.rand(n).astype(np.float32)
    return feed


def _loss_and_grads(model, staged, n, y, params):
    from deepctr_amd import training
    model._begin()
    logit = training.model_logits(model, staged, 0, n, training=True)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(logit, y)
    grads = torch.autograd.grad(loss, params, allow_unused=True)
    return float(loss.detach()), [None if g is None else g.cpu().numpy() for g in grads]


@pytest.mark.parametrize("kind", ["autoint", "autoint_nodnn", "difm"])
def test_model_gradients_with_the_switch_on_and_off(device, kind, monkeypatch):
    from deepctr_amd import engine, ops, training
    rng = np.random.RandomState(8)
    n = 211
    cols, model = _model(kind, device)
    feed = _feed(cols, n, rng)
    y = dev(rng.randint(0, 2, n).astype(np.float32), device)
    staged = engine.Staged(n)
    model._stage_inputs(feed, staged)
    frozen = training.frozen_weights(model)
    named = [(k, t) for k, t in model.named_weights() if "moving_" not in k and t.data_ptr() not in frozen]
    params = [t for _, t in named]
    seen = []
    real = ops.interacting_bwd
    monkeypatch.setattr(ops, "interacting_bwd", lambda *a, **k: (seen.append(1), real(*a, **k))[1])
    try:
        for t in params:
            t.requires_grad_(True)
        monkeypatch.setattr(training, "HIP_AUTOGRAD_OPS", False)
        loss_off, g_off = _loss_and_grads(model, staged, n, y, params)
        assert not seen
        monkeypatch.setattr(training, "HIP_AUTOGRAD_OPS", True)
        loss_on, g_on = _loss_and_grads(model, staged, n, y, params)
        assert len(seen) == 1
    finally:
        for t in params:
            t.requires_grad_(False)
    assert abs(loss_on - loss_off) <= 1e-5 * abs(loss_off)
    gmax = max(float(np.abs(g).max()) for g in g_off if g is not None)
    att = 0
    for (k, _), a, b in zip(named, g_on, g_off):
        assert (a is None) == (b is None), k
        if a is not None:
            _normalised(a, b, gmax, "%s: d %s" % (kind, k))
            att += "interacting" in k and float(np.abs(a).max()) > 0
    assert att >= 3


@pytest.mark.parametrize("kind", ["autoint", "difm"])
def test_fit_runs_the_attention_backward_on_hip(device, kind, monkeypatch):
    from deepctr_amd import engine, ops, training, training_hip
    rng = np.random.RandomState(9)
    n = 4096
    cols, model = _model(kind, device)
    feed = _feed(cols, n, rng)
    y = ((feed["s0"] % 2) ^ (feed["s1"] % 3 == 0)).astype(np.float32)          # a planted interaction of two fields
    layers = model.att_layers if kind != "difm" else [model.att]
    before = [w.clone() for layer in layers for w in layer.weights_qkvr if w is not None]
    seen = []
    real = ops.interacting_bwd
    monkeypatch.setattr(ops, "interacting_bwd", lambda *a, **k: (seen.append(1), real(*a, **k))[1])
    assert not training_hip.supported(model)
    model.compile("adam", "binary_crossentropy")
    hist = model.fit(feed, y, batch_size=256, epochs=2, verbose=0)
    assert getattr(model, "_hip_trainer", None) is None and not training_hip.supported(model)
    loss = hist.history["loss"]
    assert np.isfinite(loss).all() and loss[-1] < loss[0]
    assert len(seen) == 2 * (n // 256)
    after = [w for layer in layers for w in layer.weights_qkvr if w is not None]
    assert all(not torch.equal(a, b) for a, b in zip(after, before))
    got = model.predict_logits(feed, batch_size=1024).reshape(-1)
    staged = engine.Staged(n)
    model._stage_inputs(feed, staged)
    model._begin()
    with torch.no_grad():
        logit = training.model_logits(model, staged, 0, n)
    assert logit.grad_fn is None and not seen[2 * (n // 256):]
    assert_close(got, logit.double().cpu().numpy().reshape(-1), rtol=1e-4, atol=2e-5, what="%s: predict_logits vs model_logits" % kind)
