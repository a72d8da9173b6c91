"""GPU: dctr_fieldpair_bwd (deepctr_amd/csrc/fieldpair_bwd_kernels.hip) against the float64 oracle of tests/ref_fieldpair_bwd.py on every
case of the table there, both kinds and every gradient combination; the differentiable FwFMLayer / FEFMLayer; FwFM and DeepFEFM on the
autograd step with the field-pair layer on HIP.  The oracle and the room the bar leaves are pinned without a GPU by
tests/test_fieldpair_bwd_oracle_cpu.py.

Bar of the op: tests.util.assert_close_terms' defaults — 1e-4 of the result plus 2e-6 of the summed magnitude — for every case and
output; none has a bar of its own.  Weight gradients ACCUMULATE, so each starts at a random non-zero g0 of the result's magnitude and
``g - g0`` is compared, |g0| added to ``terms``.  dx is exercised written onto NaN and accumulated onto a sentinel; x, d_pairs and dx sit
at offsets 5, 2 and 4 inside rows wider than their data: the padding of dx comes back bit-identical, x, d_pairs, d_logit and the weights
unchanged.  The workspace is the caller's, filled with NaN, with a guard tail that must come back untouched.

Worst err / bar per case, largest over kinds, combinations and outputs, on an MI355X (MEASURED_GPU below; weight gradients vary in the
last bits with the order of the workgroups' atomics):
      smallest 0.005, ragged 0.019, e17 0.041, criteo 0.038, e32 0.037, f60 0.043, two_subtiles 0.041, general 0.048, walk 0.052
  float32 torch autograd on the CPU (test_fieldpair_bwd_oracle_cpu.py -s):
      smallest 0.006, ragged 0.018, e17 0.038, criteo 0.066, e32 0.035, f60 0.050, two_subtiles 0.035, general 0.058, walk 0.048

FEFMLayer's autograd step has a measured row threshold (training.FEFM_HIP_MIN_ROWS = 8192, profiles/fefm_fieldpair_bwd.txt); the model
and fit() tests run a few hundred rows, so they lift it: what they check is the HIP route.  One test pins the default."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import ref_fieldpair_bwd as RF
from tests.util import TERMS_REPORT, assert_close, assert_close_terms

pytestmark = pytest.mark.gpu

MEASURED_GPU = {"smallest": 0.0050, "ragged": 0.019, "e17": 0.041, "criteo": 0.038, "e32": 0.037, "f60": 0.043, "two_subtiles": 0.041,
                "general": 0.048, "walk": 0.052}        # case -> worst err / bar over its kinds, combinations and outputs, on an MI355X

GUARD = 4096
SENTINEL = 0.75
X_OFF, X_PAD, DP_OFF, DP_PAD, DX_OFF, DX_PAD = 5, 3, 2, 1, 4, 4
RUNS = [(c.name, kind, combo) for c in RF.CASES for kind in RF.KINDS for combo in RF.COMBOS[kind]]
RUN_IDS = ["%s-%s-%s" % r for r in RUNS]


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
def _reference(name, kind, combo):
    """Case, inputs, oracle and g0 of a run: computed once, never modified."""
    case = RF.CASE_BY_NAME[name]
    x, weights, d_pairs, d_logit = RF.case_inputs(case, kind)
    dp, dl = RF.combo_grads(combo, d_pairs, d_logit)
    G, T = RF.oracle(case, kind, combo)
    rng = np.random.RandomState(11 + len(name))
    g0 = (rng.standard_normal(G["dw"].shape) * max(float(np.sqrt(np.mean(np.square(G["dw"])))), 1e-3)).astype(np.float32)
    g0.setflags(write=False)
    return case, x, weights, dp, dl, G, T, g0


def _device_weights(weights, kind, device):
    """FEFM: the P matrices as views of one device tensor (E*E floats apart: off 16 B whenever E is odd); FwFM: [F,F]."""
    if kind == "fefm":
        return list(torch.unbind(dev(np.stack(weights), device)))
    return dev(weights, device)


def _call(device, name, kind, combo, dx_mode, calls=1):
    """``calls`` identical calls from g0; returns (dx of each call [B, F*E] as numpy, the weight gradient of the first, worst err / bar)."""
    from deepctr_amd import ops
    case, x, weights, dp, dl, G, T, g0 = _reference(name, kind, combo)
    F, E, B = case.shape
    n, P = F * E, F * (F - 1) // 2
    xd = placed(x, X_OFF, X_PAD, device)
    dpd = None if dp is None else placed(dp, DP_OFF, DP_PAD, device)
    dld = None if dl is None else dev(dl, device)
    wd = _device_weights(weights, kind, device)
    need = ops.fieldpair_bwd_workspace_bytes(B, F, E, kind)
    assert (need > 0) == (case.route == "workspace")
    ins = [t for t in [xd, dpd, dld] + (wd if kind == "fefm" else [wd]) if t is not None]
    snap = [bits(t) for t in ins]
    dxs, grad = [], None
    for _ in range(calls):
        dx = torch.full((B, DX_OFF + n + DX_PAD), float("nan") if dx_mode == "write" else SENTINEL, device=device)
        if dx_mode == "write":
            dx[:, :DX_OFF] = SENTINEL
            dx[:, DX_OFF + n:] = SENTINEL
        ws = torch.full((need // 4 + GUARD,), float("nan"), device=device) if need else None
        gd = dev(g0, device)
        ops.fieldpair_bwd(xd, wd, kind, d_pairs=dpd, d_pairs_offset=DP_OFF, d_logit=dld, fields=F, dim=E, x_offset=X_OFF, dx=dx,
                          dx_offset=DX_OFF, accumulate=dx_mode == "add", d_weights=gd, max_blocks=case.max_blocks,
                          workspace=None if ws is None else ws[:need // 4])
        torch.cuda.synchronize()
        if ws is not None:
            assert torch.isnan(ws[need // 4:]).all(), "%s: the guard behind the workspace was written" % name
        pad = torch.cat([dx[:, :DX_OFF], dx[:, DX_OFF + n:]], dim=1)
        assert (bits(pad) == bits(torch.full_like(pad, SENTINEL))).all(), "%s: dx's padding changed" % name
        dxs.append(dx[:, DX_OFF:DX_OFF + n].cpu().numpy())
        grad = gd if grad is None else grad
    for t, s in zip(ins, snap):
        assert (bits(t) == s).all(), "%s: an input changed" % name
    worst = {}
    base = SENTINEL if dx_mode == "add" else 0.0
    assert np.isfinite(dxs[0]).all(), "%s: dx holds what it held before (NaN) or a NaN was read" % name
    n0 = len(TERMS_REPORT)
    print("[fieldpair_bwd] %s %s %s %s" % (name, kind, combo, dx_mode), end=" ")
    try:
        assert_close_terms(dxs[0].astype(np.float64) - base, G["dx"].reshape(B, n), T["dx"].reshape(B, n) + abs(base),
                           what="%s %s %s dx (%s)" % (name, kind, combo, dx_mode))
    finally:
        worst["dx"] = TERMS_REPORT[n0][4]
        print("dx %.3g" % worst["dx"], end=" ")
    got = grad.cpu().numpy()
    if kind == "fwfm":
        low = np.tril_indices(F)
        assert (got[low].view(np.int32) == g0[low].view(np.int32)).all(), "%s: d_weights' diagonal or lower triangle changed" % name
    n0 = len(TERMS_REPORT)
    try:
        assert_close_terms(got.astype(np.float64) - g0, G["dw"], T["dw"] + np.abs(g0), what="%s %s %s dw" % (name, kind, combo))
    finally:
        worst["dw"] = TERMS_REPORT[n0][4]
        print("dw %.3g" % worst["dw"])
    return dxs, grad, worst


@pytest.mark.parametrize("dx_mode", ["write", "add"])
@pytest.mark.parametrize("name,kind,combo", RUNS, ids=RUN_IDS)
def test_op_against_the_oracle(device, name, kind, combo, dx_mode):
    _call(device, name, kind, combo, dx_mode)


@pytest.mark.parametrize("kind", RF.KINDS)
@pytest.mark.parametrize("name", ["criteo", "walk", "general"])
def test_dx_is_bit_identical_from_call_to_call(device, name, kind):
    dxs, _, _ = _call(device, name, kind, RF.COMBOS[kind][-1], "write", calls=2)
    assert (dxs[0].view(np.int32) == dxs[1].view(np.int32)).all()


@pytest.mark.parametrize("kind", RF.KINDS)
def test_optional_outputs(device, kind):
    """No dx, no weight gradient, neither: what is asked for equals the full call's, dx bit for bit."""
    from deepctr_amd import ops
    combo = RF.COMBOS[kind][-1]
    case, x, weights, dp, dl, G, T, g0 = _reference("criteo", kind, combo)
    F, E, B = case.shape
    xd, wd = dev(x, device), _device_weights(weights, kind, device)
    kw = dict(d_pairs=None if dp is None else dev(dp, device), d_logit=dev(dl, device))
    full, gfull = torch.zeros(B, F, E, device=device), torch.zeros(G["dw"].shape, device=device)
    ops.fieldpair_bwd(xd, wd, kind, dx=full, d_weights=gfull, **kw)
    only = torch.full((B, F, E), float("nan"), device=device)
    ops.fieldpair_bwd(xd, wd, kind, dx=only, **kw)
    assert (bits(only) == bits(full)).all()
    assert_close_terms(full.cpu().numpy(), G["dx"], T["dx"], what="dx of the full call")
    alone = torch.zeros(G["dw"].shape, device=device)
    ops.fieldpair_bwd(xd, wd, kind, d_weights=alone, **kw)
    assert_close_terms(alone.cpu().numpy(), G["dw"], T["dw"], what="the weight gradient alone")
    assert_close_terms(gfull.cpu().numpy(), G["dw"], T["dw"], what="the weight gradient of the full call")
    ops.fieldpair_bwd(xd, wd, kind, **kw)                     # neither: nothing to do, nothing raised


@pytest.mark.parametrize("kind", RF.KINDS)
def test_a_missing_required_workspace_raises_and_writes_nothing(device, kind):
    from deepctr_amd import _C, ops
    combo = RF.COMBOS[kind][-1]
    case, x, weights, dp, dl, G, T, g0 = _reference("general", kind, combo)
    F, E, B = case.shape
    P = F * (F - 1) // 2
    xd, wd = dev(x, device), _device_weights(weights, kind, device)
    dpd, dld = None if dp is None else dev(dp, device), dev(dl, device)
    dx = torch.full((B, F * E), SENTINEL, device=device)
    gd = torch.full(G["dw"].shape, SENTINEL, device=device)
    table = ops.bilinear_table(wd) if kind == "fefm" else wd
    b = _C.fieldpair.BwdArgs(d_pairs=None if dpd is None else dpd.data_ptr(), d_pairs_stride=P if dpd is not None else 0,
                             d_logit=dld.data_ptr(), dx=dx.data_ptr(), dx_stride=F * E, d_weights=gd.data_ptr())
    b.fwd = _C.fieldpair.Args(x=xd.data_ptr(), batch=B, x_stride=F * E, fields=F, dim=E, kind=ops._FIELDPAIR_KINDS[kind],
                              weights=table.data_ptr())
    assert _C.lib().dctr_fieldpair_bwd_workspace_bytes(ctypes.byref(b)) > 0
    with torch.cuda.device(xd.device):
        rc = _C.lib().dctr_fieldpair_bwd(ctypes.byref(b), _C.stream_ptr())
    assert rc == -1 and b"workspace" in _C.lib().dctr_last_error()
    torch.cuda.synchronize()
    for t in (dx, gd):
        assert (bits(t) == bits(torch.full_like(t, SENTINEL))).all()


# ---------------------------------------------------------------------------------------------------
# the layers
# ---------------------------------------------------------------------------------------------------
def _normalised(got, ref, gmax, what, rtol=5e-4, atol=1e-5):
    """The bar of tests/test_gpu_flen.py:_normalised: relative to the tensor's largest gradient, at least 1e-2 of the step's."""
    scale = max(float(np.abs(ref).max()), 1e-2 * gmax)
    assert_close(np.asarray(got) / scale, np.asarray(ref) / scale, rtol=rtol, atol=atol, what=what)


def _layer(kind, F, E, device):
    from deepctr_amd.layers import FEFMLayer, FwFMLayer
    if kind == "fefm":
        layer = FEFMLayer(1e-5, device=device).build_for(F, E)
        return layer, layer.matrices
    layer = FwFMLayer(num_fields=F, device=device).build_for()
    return layer, [layer.field_strengths]


def _torch_layer(kind, layer, x):
    from deepctr_amd import training
    if kind == "fefm":
        return training._fefm(layer, x)
    gram = torch.einsum("bie,bje->bij", x, x)
    return (gram * torch.triu(layer.field_strengths, diagonal=1)).sum((1, 2)).reshape(-1, 1)


@pytest.mark.parametrize("kind", RF.KINDS)
def test_layer_is_differentiable(device, kind):
    rng = np.random.RandomState(4)
    B, F, E = 37, 6, 8
    layer, ws = _layer(kind, F, E, device)
    x = dev(rng.randn(B, F, E).astype(np.float32), device)
    plain = layer(x)
    assert plain.grad_fn is None and plain.shape == ((B, F * (F - 1) // 2) if kind == "fefm" else (B, 1))
    dy = dev(rng.randn(*plain.shape).astype(np.float32), device)
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
        _torch_layer(kind, layer, xr).backward(dy)
        ref = [xr.grad.cpu().numpy()] + [w.grad.cpu().numpy() for w in ws]
    finally:
        for w in ws:
            w.requires_grad_(False)
            w.grad = None
    gmax = max(float(np.abs(r).max()) for r in ref)
    for k, (g, r) in enumerate(zip(got, ref)):
        _normalised(g, r, gmax, "%s layer gradient %d" % (kind, k))
    # nothing requires grad: today's plain launch
    y = layer(x)
    assert y.grad_fn is None and torch.equal(y, plain)
    # a weight only: x needs no gradient and gets none
    try:
        ws[-1].requires_grad_(True)
        y = layer(x)
        assert y.grad_fn is not None
        y.backward(dy)
        _normalised(ws[-1].grad.cpu().numpy(), ref[-1], gmax, "%s: one weight alone" % kind)
    finally:
        ws[-1].requires_grad_(False)
        ws[-1].grad = None


# ---------------------------------------------------------------------------------------------------
# the models
# ---------------------------------------------------------------------------------------------------
MODELS = {
    "fwfm": dict(),
    "fwfm_two_groups": dict(fm_group=("default_group", "g1")),
    "fwfm_nodnn": dict(dnn_hidden_units=()),
    "deepfefm": dict(),
    "deepfefm_exclude_embed": dict(exclude_feature_embed_in_dnn=True),
    "deepfefm_pairs_out_of_dnn": dict(use_fefm_embed_in_dnn=False),
    "deepfefm_nodnn": dict(dnn_hidden_units=()),
}


def _model(kind, device):
    from deepctr_amd import models
    from deepctr_amd.feature_column import DenseFeat, SparseFeat
    kw = dict(dnn_hidden_units=(32, 16), seed=5, device=device)
    kw.update(MODELS[kind])
    if kind == "fwfm_two_groups":
        cols = [SparseFeat("s%d" % i, 9 + i, embedding_dim=8, group_name="g1" if i >= 4 else "default_group") for i in range(7)]
    else:
        cols = [SparseFeat("s%d" % i, 9 + i, embedding_dim=8) for i in range(6)]
    cols = cols + [DenseFeat("v", 1)]
    ctor = models.FwFM if kind.startswith("fwfm") else models.DeepFEFM
    model = ctor(cols, cols, **kw)
    return cols, model, (len(model.groups) if kind.startswith("fwfm") else 1)


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


def _is_pair_weight(name):
    return "field_embeddings" in name or "field_pair_strengths" in name


@pytest.mark.parametrize("kind", sorted(MODELS))
def test_model_gradients_with_the_switch_on_and_off(device, kind, monkeypatch):
    from deepctr_amd import engine, ops, training, training_hip
    rng = np.random.RandomState(8)
    n = 211
    cols, model, groups = _model(kind, device)
    assert not training_hip.supported(model)
    feed = _feed(cols, n, rng)
    y = dev(rng.randint(0, 2, n).astype(np.float32), device)
    staged = engine.Staged(n)
    model._stage_inputs(feed, staged)
    frozen = training.frozen_weights(model)
    named = [(k, t) for k, t in model.named_weights() if "moving_" not in k and t.data_ptr() not in frozen]
    params = [t for _, t in named]
    seen = []
    real = ops.fieldpair_bwd
    monkeypatch.setattr(ops, "fieldpair_bwd", lambda *a, **k: (seen.append(1), real(*a, **k))[1])
    monkeypatch.setattr(training, "FEFM_HIP_MIN_ROWS", 0)        # (the measured row threshold would keep 211 rows on the torch ops)
    try:
        for t in params:
            t.requires_grad_(True)
        monkeypatch.setattr(training, "HIP_AUTOGRAD_OPS", False)
        loss_off, g_off = _loss_and_grads(model, staged, n, y, params)
        assert not seen
        monkeypatch.setattr(training, "HIP_AUTOGRAD_OPS", True)
        loss_on, g_on = _loss_and_grads(model, staged, n, y, params)
        assert len(seen) == groups
    finally:
        for t in params:
            t.requires_grad_(False)
    assert abs(loss_on - loss_off) <= 1e-5 * abs(loss_off)
    gmax = max(float(np.abs(g).max()) for g in g_off if g is not None)
    live = 0
    for (k, _), a, b in zip(named, g_on, g_off):
        assert (a is None) == (b is None), k
        if a is not None:
            _normalised(a, b, gmax, "%s: d %s" % (kind, k))
            live += _is_pair_weight(k) and float(np.abs(a).max()) > 0
    assert live >= 1


@pytest.mark.parametrize("kind", ["fwfm", "deepfefm"])
def test_fit_runs_the_field_pair_backward_on_hip(device, kind, monkeypatch):
    from deepctr_amd import engine, ops, training, training_hip
    rng = np.random.RandomState(9)
    n = 4096
    cols, model, groups = _model(kind, device)
    feed = _feed(cols, n, rng)
    y = ((feed["s0"] % 2) ^ (feed["s1"] % 3 == 0)).astype(np.float32)          # a planted interaction of two fields
    pair_weights = [t for k, t in model.named_weights() if _is_pair_weight(k)]
    before = [w.clone() for w in pair_weights]
    assert before
    seen = []
    real = ops.fieldpair_bwd
    monkeypatch.setattr(ops, "fieldpair_bwd", lambda *a, **k: (seen.append(1), real(*a, **k))[1])
    assert not training_hip.supported(model)
    monkeypatch.setattr(training, "FEFM_HIP_MIN_ROWS", 0)        # (batches of 256 lie below the measured row threshold)
    model.compile("adam", "binary_crossentropy")
    hist = model.fit(feed, y, batch_size=256, epochs=2, verbose=0)
    assert getattr(model, "_hip_trainer", None) is None and not training_hip.supported(model)
    loss = hist.history["loss"]
    assert np.isfinite(loss).all() and loss[-1] < loss[0]
    assert len(seen) == 2 * (n // 256) * groups
    after = [t for k, t in model.named_weights() if _is_pair_weight(k)]
    assert any(not torch.equal(a, b) for a, b in zip(after, before))
    got = model.predict_logits(feed, batch_size=1024).reshape(-1)
    staged = engine.Staged(n)
    model._stage_inputs(feed, staged)
    model._begin()
    with torch.no_grad():
        logit = training.model_logits(model, staged, 0, n)
    assert logit.grad_fn is None and not seen[2 * (n // 256) * groups:]
    assert_close(got, logit.double().cpu().numpy().reshape(-1), rtol=1e-4, atol=2e-5, what="%s: predict_logits vs model_logits" % kind)


@pytest.mark.parametrize("kind", RF.KINDS)
def test_a_refused_shape_falls_back_to_the_torch_ops(device, kind, monkeypatch):
    from deepctr_amd import ops, training
    rng = np.random.RandomState(5)
    B, F, E = 19, 5, 4
    layer, ws = _layer(kind, F, E, device)
    x = dev(rng.randn(B, F, E).astype(np.float32), device)
    calls = []
    monkeypatch.setattr(ops, "fieldpair_bwd", lambda *a, **k: calls.append(1))
    monkeypatch.setattr(ops, "fieldpair_bwd_supported", lambda *a, **k: False)
    try:
        for w in ws:
            w.requires_grad_(True)
        xg = x.clone().requires_grad_(True)
        if kind == "fefm":
            pairs, logit = training.fefm_pairs(layer, xg, True, True)
            want = training._fefm(layer, xg)
            assert torch.equal(pairs, want) and torch.equal(logit, want.sum(-1))
            (pairs.sum() + logit.sum()).backward()
        else:
            logit = training.fwfm_logit(layer, xg)
            assert torch.equal(logit.reshape(-1, 1), _torch_layer(kind, layer, xg))
            logit.sum().backward()
        assert not calls and xg.grad is not None and all(w.grad is not None for w in ws)
    finally:
        for w in ws:
            w.requires_grad_(False)
            w.grad = None


def test_fefm_below_the_row_threshold_stays_on_the_torch_ops(device, monkeypatch):
    """The measured threshold (profiles/fefm_fieldpair_bwd.txt): FEFM under FEFM_HIP_MIN_ROWS rows takes the torch ops, from it on the
    HIP op; FwFM has no threshold."""
    from deepctr_amd import ops, training
    assert training.FEFM_HIP_MIN_ROWS == 8192
    monkeypatch.setattr(training, "FEFM_HIP_MIN_ROWS", 32)
    rng = np.random.RandomState(6)
    F, E = 4, 4
    layer, ws = _layer("fefm", F, E, device)
    flayer, fws = _layer("fwfm", F, E, device)
    seen = []
    real = ops.fieldpair_bwd
    monkeypatch.setattr(ops, "fieldpair_bwd", lambda *a, **k: (seen.append(a[2]), real(*a, **k))[1])
    for B, want in ((31, ["fwfm"]), (32, ["fefm", "fwfm"])):
        del seen[:]
        xg = dev(rng.randn(B, F, E).astype(np.float32), device).requires_grad_(True)
        pairs, _ = training.fefm_pairs(layer, xg)
        (pairs.sum() + training.fwfm_logit(flayer, xg).sum()).backward()
        assert sorted(seen) == want, (B, seen)
        if B < 32:
            assert torch.equal(pairs, training._fefm(layer, xg))
