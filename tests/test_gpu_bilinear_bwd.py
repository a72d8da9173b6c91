"""GPU: dctr_bilinear_bwd (deepctr_amd/csrc/bilinear_bwd_kernels.hip) against the float64 oracle of tests/ref_bilinear_bwd.py on every
case of the table there; the differentiable SENETLayer / BilinearInteraction; FiBiNET on the autograd step with its DNN input on HIP.
The oracle and the room the bar leaves are pinned without a GPU by tests/test_bilinear_bwd_oracle_cpu.py.  FiBiNET's autograd step has a
measured row threshold (training.FIBINET_HIP_MIN_ROWS = 8192, profiles/fibinet_bilinear_bwd.txt); the model and fit() tests run a few
hundred rows, so they lift it: what they check is the HIP route.  One test pins the default.

Bar of the op: tests.util.assert_close_terms' defaults — 1e-4 of the result plus 2e-6 of the summed magnitude — for every case and
output; none has a bar of its own.  Weight gradients ACCUMULATE, so each starts at a random non-zero g0 of the result's magnitude and
``g - g0`` is compared, |g0| added to ``terms``.  dx is exercised written onto NaN and accumulated onto a sentinel; x, d_out and dx sit
at offsets 5, 2 (4 when dx accumulates: its rows are then 16-B aligned, which the 16-B loads of the staging need) and 4 inside rows
wider than their data: the padding of dx comes back bit-identical, x, d_out and the weights unchanged.  The workspace is the caller's, filled with NaN, with a guard tail that must come back untouched.

Worst err / bar per case, largest over types, modes and outputs, on an MI355X (MEASURED_GPU below; weight gradients vary in the last
bits with the order of the workgroups' atomics):
      smallest 0.0035, ragged 0.019, e17 0.076, criteo 0.041, e32 0.049, f60 0.039, many_tiles 0.048, general 0.029, walk 0.062
  float32 torch autograd on the CPU (test_bilinear_bwd_oracle_cpu.py -s; MEASURED_CPU_FLOAT32):
      smallest 0.0015, ragged 0.016, e17 0.047, criteo 0.052, e32 0.043, f60 0.039, many_tiles 0.041, general 0.038, walk 0.049"""
import functools

import numpy as np
import pytest
import torch

from tests import ref_bilinear_bwd as RB
from tests.util import TERMS_REPORT, assert_close, assert_close_terms

pytestmark = pytest.mark.gpu

# case -> worst err / bar over its types, modes and outputs
MEASURED_GPU = {"smallest": 0.0035, "ragged": 0.019, "e17": 0.076, "criteo": 0.041, "e32": 0.049, "f60": 0.039, "many_tiles": 0.048,
                "general": 0.029, "walk": 0.062}
MEASURED_CPU_FLOAT32 = {"smallest": 0.0015, "ragged": 0.016, "e17": 0.047, "criteo": 0.052, "e32": 0.043, "f60": 0.039,
                        "many_tiles": 0.041, "general": 0.038, "walk": 0.049}

GUARD = 4096
SENTINEL = 0.75
X_OFF, X_PAD, DX_OFF, DX_PAD = 5, 3, 4, 4
DO_OFF = {"write": 2, "add": 4}         # "add": d_out rows 16-B aligned (the 16-B loads of its staging), "write": off 16 B
SIDE_CASES = ("smallest", "ragged", "criteo", "general")       # the cases modes LAYER and SENET run
RUNS = [(c.name, t, "model", 0) for c in RB.CASES for t in RB.TYPES]
RUNS += [(n, t, "layer", 0) for n in SIDE_CASES for t in RB.TYPES] + [(n, "interaction", "senet", 0) for n in SIDE_CASES]
RUNS += [(n, "interaction", "model", RB.DENSE) for n in ("ragged", "criteo")]
RUN_IDS = ["%s-%s-%s-d%d" % r for r in RUNS]
KEYS = ("dw1", "dw2", "dws", "dwr")


def dev(a, device):
    return torch.tensor(np.asarray(a), device=device)       # (a copy: the cases' arrays are read-only)


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def placed(a, off, pad, device, fill=-3.5):
    """``a`` flattened to rows, at column ``off`` of rows ``pad`` wider than off + its data."""
    a = np.asarray(a, dtype=np.float32).reshape(a.shape[0], -1)
    buf = np.full((a.shape[0], off + a.shape[1] + pad), fill, dtype=np.float32)
    buf[:, off:off + a.shape[1]] = a
    return dev(buf, device)


@functools.lru_cache(maxsize=None)
def _reference(name, bilinear_type, mode, dense, r=None):
    """Case, operands, oracle and g0 of a run: computed once, never modified."""
    case = RB.CASE_BY_NAME[name]
    ops_ = RB.run_operands(case, bilinear_type, mode, dense, r)
    G, T = RB.oracle(case, bilinear_type, mode, dense, r)
    rng = np.random.RandomState(11 + len(name))
    g0 = {}
    for k in KEYS:
        if k in G:
            g0[k] = (rng.standard_normal(G[k].shape) * max(float(np.sqrt(np.mean(np.square(G[k])))), 1e-3)).astype(np.float32)
            g0[k].setflags(write=False)
    return case, ops_, G, T, g0


def _stack(W, device):
    """A layer's matrices as views of one device tensor (E*E floats apart: off 16 B whenever E is odd)."""
    return None if W is None else list(torch.unbind(dev(np.stack(W), device)))


def _call(device, name, bilinear_type, mode, dense, dx_mode, calls=1, want=("dx",) + KEYS, r=None):
    """``calls`` identical calls from g0; returns (dx of each call as numpy, the weight gradients of the first, worst err / bar)."""
    from deepctr_amd import ops
    case, (x, d_out, w1, w2, Ws, Wr), G, T, g0 = _reference(name, bilinear_type, mode, dense, r)
    F, E, B = case.shape
    n = F * E + dense
    xn = np.asarray(x, dtype=np.float32).reshape(B, F * E)
    if dense:
        xn = np.concatenate([xn, np.full((B, dense), 0.25, dtype=np.float32)], axis=1)
    xd = placed(xn, X_OFF, X_PAD, device)
    do_off = DO_OFF[dx_mode]
    dod = placed(d_out, do_off, 8 - d_out.shape[1] % 4 if dx_mode == "add" else 1, device)
    w1d, w2d = (None if w is None else dev(w, device) for w in (w1, w2))
    Wsd, Wrd = _stack(Ws, device), _stack(Wr, device)
    rr = 1 if w1 is None else w1.shape[1]
    need = ops.senet_bilinear_bwd_workspace_bytes(B, F, E, bilinear_type, mode, rr)
    if mode == "model":
        assert (need > 0) == (case.route == "workspace"), (name, need)
    ins = [t for t in [xd, dod, w1d, w2d] + (Wsd or []) + (Wrd or []) if t is not None]
    snap = [bits(t) for t in ins]
    dxs, grads = [], None
    for _ in range(calls):
        dx = None
        if "dx" in want:
            dx = torch.full((B, DX_OFF + n + DX_PAD), float("nan") if dx_mode == "write" else SENTINEL, device=device)
            if dx_mode == "write":
                dx[:, :DX_OFF] = SENTINEL
                dx[:, DX_OFF + n:] = SENTINEL
        ws = torch.full((need // 4 + GUARD,), float("nan"), device=device) if need else None
        gd = {k: dev(g0[k], device) for k in g0}
        gw = {k: (gd[k] if k in want else None) for k in KEYS if k in gd}
        ops.senet_bilinear_bwd(xd[:, X_OFF:], dod, senet_w=None if w1d is None else (w1d, w2d), senet_bilinear_w=Wsd, bilinear_w=Wrd,
                               bilinear_type=bilinear_type, fields=F, dim=E, dense_cols=dense, d_out_offset=do_off, dx=dx,
                               dx_offset=DX_OFF, accumulate=dx_mode == "add",
                               d_senet_w=(gw.get("dw1"), gw.get("dw2")) if w1d is not None else None,
                               d_senet_bilinear_w=gw.get("dws"), d_bilinear_w=gw.get("dwr"), max_blocks=case.max_blocks,
                               workspace=None if ws is None else ws[:need // 4])
        torch.cuda.synchronize()
        if ws is not None:
            assert torch.isnan(ws[need // 4:]).all(), "%s: the guard behind the workspace was written" % name
        if dx is not None:
            pad = torch.cat([dx[:, :DX_OFF], dx[:, DX_OFF + n:]], dim=1)
            assert (bits(pad) == bits(torch.full_like(pad, SENTINEL))).all(), "%s: dx's padding changed" % name
            dxs.append(dx[:, DX_OFF:DX_OFF + n].cpu().numpy())
        grads = gd if grads is None else grads
    for t, s in zip(ins, snap):
        assert (bits(t) == s).all(), "%s: an input changed" % name
    worst = {}
    print("[bilinear_bwd] %s %s %s d%d %s" % (name, bilinear_type, mode, dense, dx_mode), end=" ")

    def check(key, got, ref, terms):
        n0 = len(TERMS_REPORT)
        try:
            assert_close_terms(got, ref, terms, what="%s %s %s %s (%s)" % (name, bilinear_type, mode, key, dx_mode))
        finally:
            worst[key] = TERMS_REPORT[n0][4]
            print("%s %.3g" % (key, worst[key]), end=" ")
    try:
        if dxs:
            base = SENTINEL if dx_mode == "add" else 0.0
            assert np.isfinite(dxs[0]).all(), "%s: dx holds what it held before (NaN) or a NaN was read" % name
            check("dx", dxs[0][:, :F * E].astype(np.float64) - base, G["dx"].reshape(B, F * E), T["dx"].reshape(B, F * E) + abs(base))
            if dense:
                tail, ref = dxs[0][:, F * E:], np.asarray(G["d_dense"], dtype=np.float32)
                if dx_mode == "write":      # the transpose of the forward's copy: bit for bit
                    assert (tail.view(np.int32) == ref.view(np.int32)).all(), "%s: the dense tail of dx" % name
                else:
                    assert (tail == (np.float32(SENTINEL) + ref)).all(), "%s: the dense tail of dx (added)" % name
        for k in g0:
            got = grads[k].cpu().numpy()
            if k in want:
                check(k, got.astype(np.float64) - g0[k], G[k], T[k] + np.abs(g0[k]))
            else:
                assert (got.view(np.int32) == g0[k].view(np.int32)).all(), "%s: %s was not asked for and changed" % (name, k)
    finally:
        print()
    return dxs, grads, worst


@pytest.mark.parametrize("dx_mode", ["write", "add"])
@pytest.mark.parametrize("name,bilinear_type,mode,dense", RUNS, ids=RUN_IDS)
def test_op_against_the_oracle(device, name, bilinear_type, mode, dense, dx_mode):
    _call(device, name, bilinear_type, mode, dense, dx_mode)


def test_reduction_wider_than_the_fields(device):
    _call(device, "ragged", "interaction", "model", 0, "write", r=5)


@pytest.mark.parametrize("want", [("dx",), KEYS, ("dw1",), ("dw2",), ("dws",), ("dwr",)], ids=lambda w: "+".join(w))
@pytest.mark.parametrize("name", ["ragged", "criteo"])
def test_gradient_combinations(device, name, want):
    """dx only, the weights only, each weight gradient alone: what is asked for meets the oracle, what is not keeps its bits."""
    _call(device, name, "interaction", "model", 0, "write", want=want)


@pytest.mark.parametrize("name", ["criteo", "many_tiles", "walk"])
def test_dx_is_bit_identical_from_call_to_call(device, name):
    dxs, _, _ = _call(device, name, "interaction", "model", 0, "write", calls=2)
    assert (dxs[0].view(np.int32) == dxs[1].view(np.int32)).all()


def test_a_missing_required_workspace_raises_and_writes_nothing(device):
    import ctypes
    from deepctr_amd import _C, ops
    case, (x, d_out, w1, w2, Ws, Wr), G, T, g0 = _reference("general", "interaction", "model", 0)
    F, E, B = case.shape
    P = F * (F - 1) // 2
    xd, dod, w1d, w2d = dev(x, device), dev(d_out, device), dev(w1, device), dev(w2, device)
    Wsd, Wrd = _stack(Ws, device), _stack(Wr, device)
    dx = torch.full((B, F * E), SENTINEL, device=device)
    gd = torch.full((P, E, E), SENTINEL, device=device)
    b = _C.bilinear.BwdArgs(d_out=dod.data_ptr(), d_out_stride=2 * P * E, dx=dx.data_ptr(), dx_stride=F * E, d_bilinear_w=gd.data_ptr())
    b.fwd = _C.bilinear.Args(x=xd.data_ptr(), batch=B, x_stride=F * E, fields=F, dim=E, bilinear_type=2, mode=0,
                             reduction_size=w1.shape[1], senet_w1=w1d.data_ptr(), senet_w2=w2d.data_ptr(),
                             senet_bilinear_w=ops.bilinear_table(Wsd).data_ptr(), bilinear_w=ops.bilinear_table(Wrd).data_ptr())
    assert _C.lib().dctr_bilinear_bwd_workspace_bytes(ctypes.byref(b)) > 0
    with torch.cuda.device(xd.device):
        rc = _C.lib().dctr_bilinear_bwd(ctypes.byref(b), _C.stream_ptr())
    assert rc == -1 and b"workspace" in _C.lib().dctr_last_error()
    torch.cuda.synchronize()
    for t in (dx, gd):
        assert (bits(t) == bits(torch.full_like(t, SENTINEL))).all()


# ---------------------------------------------------------------------------------------------------
# the layers
# ---------------------------------------------------------------------------------------------------
def _normalised(got, ref, gmax, what, rtol=5e-4, atol=1e-5):
    """The bar of tests/test_gpu_fieldpair_bwd.py:_normalised: relative to the tensor's largest gradient, at least 1e-2 of the step's."""
    scale = max(float(np.abs(ref).max()), 1e-2 * gmax)
    assert_close(np.asarray(got) / scale, np.asarray(ref) / scale, rtol=rtol, atol=atol, what=what)


@pytest.mark.parametrize("kind", ["senet", "all", "each", "interaction"])
def test_layer_is_differentiable(device, kind):
    """SENETLayer(x) / BilinearInteraction(x) with requires_grad run .backward(): the gradients meet the oracle within the op's bar;
    under no_grad, and with nothing requiring grad, the output is today's plain launch, bit for bit."""
    from deepctr_amd import ops
    from deepctr_amd.layers import BilinearInteraction, SENETLayer
    case = RB.CASE_BY_NAME["ragged"]
    F, E, B = case.shape
    mode = "senet" if kind == "senet" else "layer"
    btype = "interaction" if kind == "senet" else kind
    x, d_out, w1, w2, _, Wr = RB.run_operands(case, btype, mode)
    G, T = RB.oracle(case, btype, mode)
    if kind == "senet":
        layer = SENETLayer(3, device=device).build_for(F, E)
        ws = list(layer.weights_w12)
        vals, keys = [w1, w2], ["dw1", "dw2"]
    else:
        layer = BilinearInteraction(kind, device=device).build_for(F, E)
        ws = layer.matrices
        vals, keys = list(Wr), None
    with torch.no_grad():
        for w, v in zip(ws, vals):
            w.copy_(dev(v, device))
    xt = dev(x, device)
    parts = lambda t: list(torch.split(t, 1, dim=1))     # noqa: E731
    flat = lambda y: (torch.cat(y, dim=1) if isinstance(y, list) else y).reshape(B, -1)      # noqa: E731
    plain = flat(layer(parts(xt)))
    assert plain.grad_fn is None
    if kind == "senet":
        assert torch.equal(plain, ops.senet_bilinear(xt, senet_w=tuple(ws)))
    else:
        assert torch.equal(plain, ops.senet_bilinear(xt, bilinear_w=ws, bilinear_type=kind))
    dy = dev(d_out, device)
    xg = xt.clone().requires_grad_(True)
    try:
        for w in ws:
            w.requires_grad_(True)
        with torch.no_grad():
            y0 = flat(layer(parts(xg)))
        assert y0.grad_fn is None and torch.equal(y0, plain)
        y = flat(layer(parts(xg)))
        assert y.grad_fn is not None and torch.equal(y.detach(), plain)
        y.backward(dy)
        assert xg.grad is not None and all(w.grad is not None for w in ws)
        assert_close_terms(xg.grad.cpu().numpy(), G["dx"], T["dx"], what="%s layer dx" % kind)
        if kind == "senet":
            for w, k in zip(ws, keys):
                assert_close_terms(w.grad.cpu().numpy(), G[k], T[k], what="%s layer %s" % (kind, k))
        else:
            assert_close_terms(torch.stack([w.grad for w in ws]).cpu().numpy(), G["dwr"], T["dwr"], what="%s layer dW" % kind)
        # a weight only: x needs no gradient and gets none
        for w in ws:
            w.grad = None
            w.requires_grad_(False)
        ws[-1].requires_grad_(True)
        y = flat(layer(parts(xt)))
        assert y.grad_fn is not None
        y.backward(dy)
        ref, terms = (G["dw2"], T["dw2"]) if kind == "senet" else (G["dwr"][-1], T["dwr"][-1])
        assert_close_terms(ws[-1].grad.cpu().numpy(), ref, terms, what="%s: one weight alone" % kind)
    finally:
        for w in ws:
            w.requires_grad_(False)
            w.grad = None
    # nothing requires grad: today's plain launch
    y = flat(layer(parts(xt)))
    assert y.grad_fn is None and torch.equal(y, plain)


# ---------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------
def _model(device, bilinear_type, hidden, trainable=True):
    from deepctr_amd import models
    from deepctr_amd.feature_column import DenseFeat, SparseFeat, VarLenSparseFeat
    kw = {} if trainable else {"trainable": False}
    cols = [SparseFeat("s%d" % i, 9 + i, embedding_dim=8, **kw) for i in range(4)]
    cols += [VarLenSparseFeat(SparseFeat("q", 12, embedding_dim=8, **kw), maxlen=5, combiner="mean")]
    cols += [DenseFeat("v", 1), DenseFeat("u", 1)]
    return cols, models.FiBiNET(cols, cols, bilinear_type=bilinear_type, dnn_hidden_units=hidden, seed=5, device=device)


def _feed(cols, n, rng):
    feed = {}
    for c in cols:
        if hasattr(c, "maxlen"):
            seq = rng.randint(1, c.vocabulary_size, (n, c.maxlen)).astype(np.int32)
            seq[rng.rand(n, c.maxlen) < 0.3] = 0
            seq[:, 0] = np.maximum(seq[:, 0], 1)
            feed[c.name] = seq
        elif hasattr(c, "vocabulary_size"):
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


def _counted(monkeypatch):
    """A counter around ops.senet_bilinear_bwd; the measured row threshold is lifted (these tests run a few hundred rows: what they
    check is the HIP route)."""
    from deepctr_amd import ops, training
    monkeypatch.setattr(training, "FIBINET_HIP_MIN_ROWS", 0)
    seen = []
    real = ops.senet_bilinear_bwd
    monkeypatch.setattr(ops, "senet_bilinear_bwd", lambda *a, **k: (seen.append(1), real(*a, **k))[1])
    return seen


@pytest.mark.parametrize("hidden", [(32, 16), ()], ids=["dnn", "nodnn"])
@pytest.mark.parametrize("bilinear_type", RB.TYPES)
def test_model_gradients_with_the_switch_on_and_off(device, bilinear_type, hidden, monkeypatch):
    """One autograd step's gradients of EVERY parameter with training.HIP_AUTOGRAD_OPS on meet those with it off; the HIP backward ran
    with the switch on and did not with it off."""
    from deepctr_amd import engine, training, training_hip
    rng = np.random.RandomState(8)
    n = 211
    cols, model = _model(device, bilinear_type, hidden)
    assert not training_hip.supported(model)
    feed = _feed(cols, n, rng)
    y = dev(rng.randint(0, 2, n).astype(np.float32), device)
    staged = engine.Staged(n)
    model._stage_inputs(feed, staged)
    frozen = training.frozen_weights(model)
    named = [(k, t) for k, t in model.named_weights() if "moving_" not in k and t.data_ptr() not in frozen]
    params = [t for _, t in named]
    seen = _counted(monkeypatch)
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
    live = 0
    for (k, _), a, b in zip(named, g_on, g_off):
        assert (a is None) == (b is None), k
        if a is not None:
            _normalised(a, b, gmax, "%s: d %s" % (bilinear_type, k))
            live += ("bilinear_weight" in k or "W_1" in k or "W_2" in k) and float(np.abs(a).max()) > 0
    assert live >= 3


def test_fit_agrees_with_the_switch_on_and_off(device, monkeypatch):
    """fit() runs two epochs at batch 256 from the same weights with the switch on and off: the HIP backward runs once per step with it
    on, never with it off, and the losses agree."""
    from deepctr_amd import training, training_hip
    rng = np.random.RandomState(9)
    n = 2048
    seen = _counted(monkeypatch)
    losses = {}
    for on in (True, False):
        monkeypatch.setattr(training, "HIP_AUTOGRAD_OPS", on)
        cols, model = _model(device, "interaction", (32, 16))
        if not losses:
            feed = _feed(cols, n, rng)
            y = ((feed["s0"] % 2) ^ (feed["s1"] % 3 == 0)).astype(np.float32)          # a planted interaction of two fields
        del seen[:]
        model.compile("adam", "binary_crossentropy")
        hist = model.fit(feed, y, batch_size=256, epochs=2, verbose=0)
        assert getattr(model, "_hip_trainer", None) is None and not training_hip.supported(model)
        assert len(seen) == (2 * (n // 256) if on else 0)
        losses[on] = np.asarray(hist.history["loss"])
    assert np.isfinite(losses[True]).all() and losses[True][-1] < losses[True][0]
    assert_close(losses[True], losses[False], rtol=1e-3, atol=1e-5, what="fit() losses, HIP route vs torch ops")


def test_frozen_embeddings_keep_their_bits(device, monkeypatch):
    from deepctr_amd import training
    rng = np.random.RandomState(10)
    n = 512
    cols, model = _model(device, "interaction", (16,), trainable=False)
    feed = _feed(cols, n, rng)
    y = rng.randint(0, 2, n).astype(np.float32)
    frozen = training.frozen_weights(model)
    tables = [(k, t, t.clone()) for k, t in model.named_weights() if t.data_ptr() in frozen]
    others = [(k, t, t.clone()) for k, t in model.named_weights() if "bilinear_weight" in k]
    assert tables and others
    seen = _counted(monkeypatch)
    model.compile("adam", "binary_crossentropy")
    hist = model.fit(feed, y, batch_size=256, epochs=1, verbose=0)
    assert len(seen) == 2 and np.isfinite(hist.history["loss"]).all()
    for k, t, before in tables:
        assert torch.equal(t, before), k
    assert any(not torch.equal(t, before) for _, t, before in others)


def test_a_refused_shape_falls_back_to_the_torch_ops(device, monkeypatch):
    from deepctr_amd import engine, ops, training
    rng = np.random.RandomState(5)
    n = 19
    cols, model = _model(device, "each", (8,))
    feed = _feed(cols, n, rng)
    staged = engine.Staged(n)
    model._stage_inputs(feed, staged)
    calls = []
    monkeypatch.setattr(ops, "senet_bilinear_bwd", lambda *a, **k: calls.append(1))
    monkeypatch.setattr(ops, "senet_bilinear_bwd_supported", lambda *a, **k: False)
    monkeypatch.setattr(training, "FIBINET_HIP_MIN_ROWS", 0)
    params = [t for k, t in model.named_weights() if "bilinear_weight" in k]
    try:
        for t in params:
            t.requires_grad_(True)
        model._begin()
        logit = training.model_logits(model, staged, 0, n, training=True)
        grads = torch.autograd.grad(logit.sum(), params)
    finally:
        for t in params:
            t.requires_grad_(False)
    assert not calls and all(g is not None for g in grads)


def test_below_the_row_threshold_the_step_stays_on_the_torch_ops(device, monkeypatch):
    """The measured threshold (profiles/fibinet_bilinear_bwd.txt): under FIBINET_HIP_MIN_ROWS rows training.senet_bilinear takes the
    torch ops, from it on the HIP op."""
    from deepctr_amd import engine, ops, training
    assert training.FIBINET_HIP_MIN_ROWS == 8192
    monkeypatch.setattr(training, "FIBINET_HIP_MIN_ROWS", 32)
    rng = np.random.RandomState(6)
    cols, model = _model(device, "interaction", (8,))
    seen = []
    real = ops.senet_bilinear_bwd
    monkeypatch.setattr(ops, "senet_bilinear_bwd", lambda *a, **k: (seen.append(1), real(*a, **k))[1])
    params = [t for k, t in model.named_weights() if "bilinear_weight" in k]
    try:
        for t in params:
            t.requires_grad_(True)
        for n, want in ((31, 0), (32, 1)):
            del seen[:]
            staged = engine.Staged(n)
            model._stage_inputs(_feed(cols, n, rng), staged)
            model._begin()
            logit = training.model_logits(model, staged, 0, n, training=True)
            grads = torch.autograd.grad(logit.sum(), params)
            assert len(seen) == want and all(g is not None for g in grads), (n, seen)
    finally:
        for t in params:
            t.requires_grad_(False)
