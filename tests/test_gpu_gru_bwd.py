"""GPU: dctr_gru_bwd (deepctr_amd/csrc/gru_bwd_kernels.hip) against the float64 oracle of tests/ref_gru_bwd.py on every case of the
table there, the differentiable DynamicGRU layer (ops.DynamicGRUFunction, training.dynamic_gru), and DIEN on the autograd step with its
GRUs on HIP.  The oracle, the table and the room the bar leaves are pinned without a GPU by tests/test_gru_bwd_oracle_cpu.py.

Bar of the op: tests.util.assert_close_terms' defaults — 1e-4 of the result plus 2e-6 of the summed magnitude — for every case and
output; none has a bar of its own.  h_seq is the kernel's own forward (ops.dynamic_gru).  Weight gradients ACCUMULATE, so each starts
at a random non-zero g0 of the result's magnitude and ``g - g0`` is compared, |g0| added to ``terms``.  dx is exercised written onto NaN
and accumulated onto a sentinel; x, h_seq, d_out and dx sit on padded sample and step strides: the padding of dx comes back
bit-identical, the inputs unchanged.  The caller's workspace (no shape needs one) is NaN with a guard tail and comes back untouched.

Worst err / bar per case, largest over the outputs (for judging a later change of the bar):
  float32 torch autograd on the CPU (test_gru_bwd_oracle_cpu.py -s): at most 0.35 (E49_AGRU_final_T2_B33, d candidate kernel)
  these tests on an MI355X (MEASURED_GPU below; weight gradients vary in the last bits with the order of the workgroups' atomics):
      at most 0.057 (E64_GRU_seq_T1_B17, d gate kernel); 0.035 and below on every other case; every dx and d_att below 0.02."""
import functools

import numpy as np
import pytest
import torch

from tests import ref_gru_bwd as RG
from tests.util import TERMS_REPORT, assert_close, assert_close_terms

pytestmark = pytest.mark.gpu

# case -> worst err / bar over its outputs and both dx modes, on an MI355X
MEASURED_GPU = {
    "E1_GRU_seq_T1_B1": 0.00098, "E1_GRU_final_T2_B1": 0.016, "E1_AIGRU_seq_T2_B17": 0.013, "E1_AIGRU_final_T6_B17": 0.017,
    "E1_AGRU_seq_T6_B33": 0.0071, "E1_AGRU_final_T1_B33": 0.0073, "E1_AUGRU_seq_T1_B1": 0.0022, "E1_AUGRU_final_T2_B1": 0.0034,
    "E4_GRU_seq_T2_B17": 0.019, "E4_GRU_final_T6_B17": 0.0051, "E4_AIGRU_seq_T6_B33": 0.012, "E4_AIGRU_final_T1_B33": 0.011,
    "E4_AGRU_seq_T1_B1": 0.01, "E4_AGRU_final_T2_B1": 0.015, "E4_AUGRU_seq_T2_B17": 0.0065, "E4_AUGRU_final_T6_B17": 0.004,
    "E12_GRU_seq_T6_B33": 0.0051, "E12_GRU_final_T1_B33": 0.01, "E12_AIGRU_seq_T1_B1": 0.018, "E12_AIGRU_final_T2_B1": 0.022,
    "E12_AGRU_seq_T2_B17": 0.029, "E12_AGRU_final_T6_B17": 0.011, "E12_AUGRU_seq_T6_B33": 0.014,
    "E12_AUGRU_final_T1_B33": 0.0095, "E16_GRU_seq_T1_B1": 0.013, "E16_GRU_final_T2_B1": 0.025, "E16_AIGRU_seq_T2_B17": 0.018,
    "E16_AIGRU_final_T6_B17": 0.0077, "E16_AGRU_seq_T6_B33": 0.018, "E16_AGRU_final_T1_B33": 0.011,
    "E16_AUGRU_seq_T1_B1": 0.021, "E16_AUGRU_final_T2_B1": 0.024, "E17_GRU_seq_T2_B17": 0.018, "E17_GRU_final_T6_B17": 0.0043,
    "E17_AIGRU_seq_T6_B33": 0.0083, "E17_AIGRU_final_T1_B33": 0.016, "E17_AGRU_seq_T1_B1": 0.022, "E17_AGRU_final_T2_B1": 0.022,
    "E17_AUGRU_seq_T2_B17": 0.012, "E17_AUGRU_final_T6_B17": 0.011, "E40_GRU_seq_T6_B33": 0.0042, "E40_GRU_final_T1_B33": 0.013,
    "E40_AIGRU_seq_T1_B17": 0.029, "E40_AIGRU_final_T2_B17": 0.024, "E40_AGRU_seq_T2_B33": 0.033,
    "E40_AGRU_final_T6_B33": 0.012, "E40_AUGRU_seq_T6_B17": 0.0054, "E40_AUGRU_final_T1_B17": 0.015,
    "E64_GRU_seq_T1_B17": 0.057, "E64_GRU_final_T2_B17": 0.035, "E64_AIGRU_seq_T2_B33": 0.024, "E64_AIGRU_final_T6_B33": 0.0054,
    "E64_AGRU_seq_T6_B17": 0.015, "E64_AGRU_final_T1_B17": 0.021, "E64_AUGRU_seq_T1_B33": 0.0093,
    "E64_AUGRU_final_T2_B33": 0.02, "E49_GRU_seq_T2_B33": 0.022, "E49_GRU_final_T6_B33": 0.0039, "E49_AIGRU_seq_T6_B17": 0.0071,
    "E49_AIGRU_final_T1_B17": 0.017, "E49_AGRU_seq_T1_B33": 0.025, "E49_AGRU_final_T2_B33": 0.032,
    "E49_AUGRU_seq_T2_B17": 0.026, "E49_AUGRU_final_T6_B17": 0.013, "E65_GRU_seq_T6_B17": 0.0032, "E65_GRU_final_T1_B17": 0.016,
    "E65_AIGRU_seq_T1_B33": 0.021, "E65_AIGRU_final_T2_B33": 0.022, "E65_AGRU_seq_T2_B17": 0.034,
    "E65_AGRU_final_T6_B17": 0.015, "E65_AUGRU_seq_T6_B33": 0.011, "E65_AUGRU_final_T1_B33": 0.02,
    "E17_GRU_seq_T6_B33_wide": 0.0038, "E17_AUGRU_final_T6_B33_wide": 0.0055, "E12_AIGRU_seq_T6_B33_streamed": 0.0097,
    "E12_AGRU_final_T6_B33_streamed": 0.012}

GUARD = 1024
SENTINEL = 0.75
PAD_ROW, PAD_SAMPLE = 3, 5          # floats behind every step's row and behind every sample's block
E_UNSUPPORTED = -5
WKEYS = RG.KEYS[2:]


def dev(a, device):
    return torch.tensor(np.asarray(a), device=device)       # (a copy: the cases' arrays are shared)


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def padded3(a, device, fill=-3.5):
    """[B, T, E] inside a buffer with PAD_ROW floats behind every row and PAD_SAMPLE behind every sample; (buffer, view)."""
    B, T, E = a.shape
    buf = torch.full((B, T * (E + PAD_ROW) + PAD_SAMPLE), fill, device=device)
    view = buf[:, :T * (E + PAD_ROW)].view(B, T, E + PAD_ROW)[:, :, :E]
    if isinstance(a, np.ndarray):
        view.copy_(dev(a.astype(np.float32), device))
    return buf, view


def pad_mask(B, T, E, device):
    m = torch.ones(B, T * (E + PAD_ROW) + PAD_SAMPLE, dtype=torch.bool, device=device)
    m[:, :T * (E + PAD_ROW)].view(B, T, E + PAD_ROW)[:, :, :E] = False
    return m


@functools.lru_cache(maxsize=None)
def _reference(name):
    """Case, inputs, oracle and g0 of a case: computed once, never modified."""
    case = RG.CASE_BY_NAME[name]
    x, lens, layer, att, d_out = RG.case_inputs(case)
    G, T = RG.case_oracle(case)
    rng = np.random.RandomState(11 + case.seed)
    g0 = {k: (rng.standard_normal(G[k].shape) * max(float(np.sqrt(np.mean(np.square(G[k])))), 1e-3)).astype(np.float32) for k in WKEYS}
    return case, x, lens, layer, att, d_out, G, T, g0


def _call(device, name, dx_mode, calls=1, outputs="all"):
    """``calls`` identical calls from g0; returns (dx of each call, d_att of each call, weight gradients of the first call)."""
    from deepctr_amd import ops
    case, x, lens, layer, att, d_out, G, T, g0 = _reference(name)
    cell, scale = RG.case_options(case)
    B, Tn, E = x.shape
    need_att = G["d_att"] is not None
    xbuf, xd = padded3(x, device)
    ld, ad = dev(lens, device), dev(att, device)
    wd = [dev(w, device) for w in layer]
    hbuf, hd = padded3(np.zeros_like(x), device)
    ops.dynamic_gru(xd, ld, [wd], cell=cell, att_scores=ad if need_att else None, scale_input=scale, return_sequence=True, out=hd)
    if case.return_sequence:
        dbuf, dd = padded3(d_out, device)
    else:
        dbuf = torch.full((B, E + PAD_ROW), -3.5, device=device)
        dd = dbuf[:, :E]
        dd.copy_(dev(d_out, device))
    assert ops.gru_bwd_workspace_bytes(B, Tn, E, cell, scale, case.return_sequence, case.route) == 0
    inputs = [xbuf, hbuf, dbuf, ld, ad] + wd
    snap = [bits(t) for t in inputs]
    mask = pad_mask(B, Tn, E, device)
    dxs, das, grads = [], [], None
    for _ in range(calls):
        dxbuf, dx = padded3(np.zeros_like(x), device, fill=SENTINEL)
        dx.fill_(float("nan") if dx_mode == "write" else SENTINEL)
        datt = torch.full((B, Tn + 2), float("nan"), device=device)
        datt[:, Tn:] = SENTINEL
        ws = torch.full((GUARD,), float("nan"), device=device)
        gd = [dev(g0[k], device) for k in WKEYS]
        ops.gru_bwd(xd, ld, wd, hd, dd, cell=cell, att_scores=ad if need_att else None, scale_input=scale,
                    return_sequence=case.return_sequence, dx=dx if outputs != "weights" else None, accumulate=dx_mode == "add",
                    d_att=datt[:, :Tn] if need_att and outputs == "all" else None, d_weights=gd if outputs != "dx" else None,
                    max_blocks=case.max_blocks, route=case.route, workspace=ws)
        torch.cuda.synchronize()
        assert torch.isnan(ws).all(), "%s: the workspace was written" % name
        assert (bits(dxbuf[mask]) == bits(torch.full_like(dxbuf[mask], SENTINEL))).all(), "%s: dx's padding changed" % name
        assert (bits(datt[:, Tn:]) == bits(torch.full((B, 2), SENTINEL))).all(), "%s: d_att's padding changed" % name
        dxs.append(dx.cpu().numpy())
        das.append(datt[:, :Tn].cpu().numpy())
        grads = grads or gd
    for t, s in zip(inputs, snap):
        assert (bits(t) == s).all(), "%s: an input changed" % name
    return dxs, das, [g.cpu().numpy() for g in grads]


def _compare(name, dx_mode, dxs, das, grads):
    case, x, lens, layer, att, d_out, G, T, g0 = _reference(name)
    B, Tn, E = x.shape
    worst = {}
    base = SENTINEL if dx_mode == "add" else 0.0
    dead = np.arange(Tn)[None, :] >= np.clip(lens, 0, Tn)[:, None]
    assert np.isfinite(dxs[0]).all(), "%s: dx holds what it held before (NaN) or a NaN was read" % name
    assert (dxs[0][dead] == np.float32(base)).all(), "%s: dx at t >= length" % name
    n0 = len(TERMS_REPORT)
    assert_close_terms(dxs[0].astype(np.float64) - base, G["dx"], T["dx"] + abs(base), what="%s dx (%s)" % (name, dx_mode))
    worst["dx"] = TERMS_REPORT[n0][4]
    if G["d_att"] is not None:
        assert np.isfinite(das[0]).all() and (das[0][dead] == 0).all(), "%s: d_att at t >= length" % name
        n0 = len(TERMS_REPORT)
        assert_close_terms(das[0], G["d_att"], T["d_att"], what="%s d_att" % name)
        worst["d_att"] = TERMS_REPORT[n0][4]
    else:
        assert np.isnan(das[0]).all(), "%s: d_att written by a cell without scores" % name
    for k, g in zip(WKEYS, grads):
        n0 = len(TERMS_REPORT)
        assert_close_terms(g.astype(np.float64).reshape(G[k].shape) - g0[k], G[k], T[k] + np.abs(g0[k]), what="%s %s" % (name, k))
        worst[k] = TERMS_REPORT[n0][4]
    print("[gru_bwd] %s %s: worst err / bar %.3g (%s)" % (name, dx_mode, max(worst.values()),
                                                         ", ".join("%s %.2g" % kv for kv in sorted(worst.items()))))
    return worst


@pytest.mark.parametrize("name", [c.name for c in RG.CASES])
def test_op_against_the_oracle(device, name):
    """Both dx modes; the second of two identical calls repeats dx and d_att bit for bit."""
    dxs, das, grads = _call(device, name, "write", calls=2)
    _compare(name, "write", dxs, das, grads)
    assert (dxs[0].view(np.int32) == dxs[1].view(np.int32)).all() and (das[0].view(np.int32) == das[1].view(np.int32)).all()
    _compare(name, "add", *_call(device, name, "add"))


@pytest.mark.parametrize("name", ["E17_AUGRU_seq_T2_B17", "E12_AIGRU_seq_T6_B33_streamed", "E64_GRU_final_T2_B17"])
def test_optional_outputs(device, name):
    """dx alone and the weight gradients alone: what is asked for equals the full call's, bit for bit in dx."""
    full = _call(device, name, "write")
    only_dx = _call(device, name, "write", outputs="dx")
    assert (full[0][0].view(np.int32) == only_dx[0][0].view(np.int32)).all()
    case, x, lens, layer, att, d_out, G, T, g0 = _reference(name)
    assert all((g == g0[k].reshape(g.shape)).all() for k, g in zip(WKEYS, only_dx[2]))       # not asked for: not touched
    only_w = _call(device, name, "write", outputs="weights")
    assert np.isnan(only_w[0][0]).all()
    for k, g in zip(WKEYS, only_w[2]):
        assert_close_terms(g.astype(np.float64).reshape(G[k].shape) - g0[k], G[k], T[k] + np.abs(g0[k]), what="%s %s alone" % (name, k))


@pytest.mark.parametrize("variant", [v for v, _ in RG.VARIANTS])
def test_saturated_gates(device, variant):
    """Zero kernels and biases of +-30 mixed over the units: every gate and candidate saturates.  All outputs finite and within the bar
    with the terms floored at the tensor's max |ref| (float64 leaves 1e-13 residues where float32 leaves 0)."""
    from deepctr_amd import ops
    rng = np.random.RandomState(17)
    B, Tn, E = 19, 4, 10
    cell, scale = RG.cell_of(variant), dict(RG.VARIANTS)[variant]
    x = rng.randn(B, Tn, E).astype(np.float32)
    lens = RG.case_lengths(Tn, B)
    sign = lambda n: np.where(rng.rand(n) < 0.5, -30.0, 30.0).astype(np.float32)       # noqa: E731
    layer = [np.zeros((2 * E, 2 * E), np.float32), sign(2 * E), np.zeros((2 * E, E), np.float32), sign(E)]
    att = rng.rand(B, Tn).astype(np.float32)
    for seq in (True, False):
        d_out = rng.randn(*((B, Tn, E) if seq else (B, E))).astype(np.float32)
        G, T = RG.gru_bwd(x, lens, layer, cell, att, scale, seq, d_out)
        xd, ld, ad, dd = dev(x, device), dev(lens, device), dev(att, device), dev(d_out, device)
        wd = [dev(w, device) for w in layer]
        need_att = G["d_att"] is not None
        h = ops.dynamic_gru(xd, ld, [wd], cell=cell, att_scores=ad if need_att else None, scale_input=scale)
        dx, datt = torch.full_like(xd, float("nan")), torch.full_like(ad, float("nan"))
        gd = [torch.zeros_like(w) for w in wd]
        ops.gru_bwd(xd, ld, wd, h, dd, cell=cell, att_scores=ad if need_att else None, scale_input=scale, return_sequence=seq, dx=dx,
                    d_att=datt if need_att else None, d_weights=gd)
        got = dict(zip(RG.KEYS, [dx, datt if need_att else None] + gd))
        for k in RG.KEYS:
            if G[k] is None:
                continue
            g = got[k].cpu().numpy().reshape(G[k].shape)
            assert np.isfinite(g).all(), (variant, seq, k)
            assert_close_terms(g, G[k], np.maximum(T[k], np.abs(G[k]).max()), what="saturated %s %s" % (variant, k))


def test_a_refused_shape_raises_and_writes_nothing(device, monkeypatch):
    from deepctr_amd import _C, ops, training
    B, Tn, E = 5, 3, RG.SUPPORT_MAX_E + 1
    rng = np.random.RandomState(3)
    x = dev(rng.randn(B, Tn, E).astype(np.float32), device)
    lens = dev(np.array([3, 0, 1, 6, 2], np.int32), device)
    wd = [dev((rng.randn(*s) * 0.1).astype(np.float32), device) for s in ((2 * E, 2 * E), (2 * E,), (2 * E, E), (E,))]
    h = ops.dynamic_gru(x, lens, [wd])
    dy = dev(rng.randn(B, Tn, E).astype(np.float32), device)
    dx = torch.full_like(x, SENTINEL)
    gd = [torch.full_like(w, SENTINEL) for w in wd]
    assert not ops.gru_bwd_supported(Tn, E) and ops.gru_bwd_supported(Tn, E - 1)
    with pytest.raises(_C.DctrError) as err:
        ops.gru_bwd(x, lens, wd, h, dy, dx=dx, d_weights=gd)
    assert err.value.rc == E_UNSUPPORTED
    torch.cuda.synchronize()
    for t in [dx] + gd:
        assert (bits(t) == bits(torch.full_like(t, SENTINEL))).all()
    # the autograd step then takes the torch loop
    calls = []
    monkeypatch.setattr(ops, "gru_bwd", lambda *a, **k: calls.append(1))
    ws = [w.clone().requires_grad_(True) for w in wd]
    xg = x.clone().requires_grad_(True)
    y = training.dynamic_gru(xg, lens, [ws])
    assert torch.equal(y, training._gru(xg, lens, [ws]))
    y.backward(dy)
    assert not calls and xg.grad is not None and all(w.grad is not None for w in ws)


# ---------------------------------------------------------------------------------------------------
# the function
# ---------------------------------------------------------------------------------------------------
def _normalised(got, ref, gmax, what, rtol=5e-4, atol=1e-5):
    """The bar of tests/test_gpu_interacting_bwd.py:_normalised: relative to the tensor's largest gradient, at least 1e-2 of the step's."""
    scale = max(float(np.abs(ref).max()), 1e-2 * gmax)
    assert_close(np.asarray(got) / scale, np.asarray(ref) / scale, rtol=rtol, atol=atol, what=what)


@pytest.mark.parametrize("seq", [True, False])
@pytest.mark.parametrize("variant", [v for v, _ in RG.VARIANTS])
def test_function_is_differentiable(device, variant, seq, monkeypatch):
    from deepctr_amd import ops, training
    rng = np.random.RandomState(4)
    B, Tn, E = 37, 5, 12
    cell, scale = RG.cell_of(variant), dict(RG.VARIANTS)[variant]
    need_att = cell != "GRU" or scale
    case = RG.Case("fn", E, Tn, B, variant, seq, 0, None, 90)
    x, lens, layer, att, d_out = RG.case_inputs(case)
    ld = dev(lens, device)
    dy = dev(d_out, device)
    kw = dict(cell=cell, scale_input=scale, return_sequence=seq)

    def run(fn):
        xg = dev(x, device).requires_grad_(True)
        ag = dev(att, device).requires_grad_(need_att)
        ws = [dev(w, device).requires_grad_(True) for w in layer]
        y = fn(xg, ld, [ws], att_scores=ag if need_att else None, **kw)
        y.backward(dy)
        return y.detach(), [t.grad.cpu().numpy() for t in [xg] + ([ag] if need_att else []) + ws]

    seen = []
    real = ops.gru_bwd
    monkeypatch.setattr(ops, "gru_bwd", lambda *a, **k: (seen.append(1), real(*a, **k))[1])
    y_hip, got = run(training.dynamic_gru)
    assert len(seen) == 1
    plain = ops.dynamic_gru(dev(x, device), ld, [[dev(w, device) for w in layer]], cell=cell, att_scores=dev(att, device) if need_att else None,
                            scale_input=scale, return_sequence=seq)
    assert torch.equal(y_hip, plain)                # the forward's value is dctr_gru_fwd's
    y_ref, ref = run(training._gru)
    assert len(seen) == 1
    gmax = max(float(np.abs(r).max()) for r in ref)
    for k, (g, r) in enumerate(zip(got, ref)):
        _normalised(g, r, gmax, "%s %s: gradient %d" % (variant, "seq" if seq else "final", k))
    # a stack is one application per layer
    if variant == "GRU":
        def two(fn):
            xg = dev(x, device).requires_grad_(True)
            w1 = [dev(w, device).requires_grad_(True) for w in layer]
            w2 = [dev(w * 0.7, device).requires_grad_(True) for w in layer]
            fn(xg, ld, [w1, w2], return_sequence=seq).backward(dy)
            return [t.grad.cpu().numpy() for t in [xg] + w1 + w2]
        got2 = two(training.dynamic_gru)
        assert len(seen) == 3
        ref2 = two(training._gru)
        gmax = max(float(np.abs(r).max()) for r in ref2)
        for k, (g, r) in enumerate(zip(got2, ref2)):
            _normalised(g, r, gmax, "two layers: gradient %d" % k)
    # under no_grad, and with nothing requiring grad: the torch loop
    with torch.no_grad():
        xg = dev(x, device).requires_grad_(True)
        training.dynamic_gru(xg, ld, [[dev(w, device) for w in layer]], att_scores=dev(att, device) if need_att else None, **kw)
    training.dynamic_gru(dev(x, device), ld, [[dev(w, device) for w in layer]], att_scores=dev(att, device) if need_att else None, **kw)
    assert len(seen) == (3 if variant == "GRU" else 1)


# ---------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------
MODELS = [("GRU", False), ("AIGRU", False), ("AGRU", False), ("AUGRU", False), ("AUGRU", True)]


def _dien(device, gru_type, neg, n, seed):
    from deepctr_amd.models import DIEN
    from tests.test_gpu_dien import dien_problem, randomise
    rng = np.random.RandomState(seed)
    cols, names, feed = dien_problem(rng, n, n_hist=2, T=6, widths=(8, 4), neg=neg)
    model = DIEN(cols, names, gru_type=gru_type, use_negsampling=neg, dnn_hidden_units=(16, 8), att_hidden_units=(16, 8), device=device)
    randomise(model, rng)
    return model, feed, rng


def _loss_and_grads(model, staged, n, y, params):
    from deepctr_amd import training
    model._begin()
    logit = training.model_logits(model, staged, 0, n, training=True)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(logit, y)
    added = model._autograd_added_loss()
    if added is not None:
        loss = loss + added
    grads = torch.autograd.grad(loss, params, allow_unused=True)
    return float(loss.detach()), [None if g is None else g.cpu().numpy() for g in grads]


@pytest.mark.parametrize("gru_type,neg", MODELS)
def test_model_gradients_with_the_switch_on_and_off(device, gru_type, neg, monkeypatch):
    from deepctr_amd import engine, ops, training
    n = 203
    model, feed, rng = _dien(device, gru_type, neg, n, 8)
    y = dev(rng.randint(0, 2, n).astype(np.float32), device)
    staged = engine.Staged(n)
    model._stage_inputs(feed, staged)
    frozen = training.frozen_weights(model)
    named = [(k, t) for k, t in model.named_weights() if "moving_" not in k and t.data_ptr() not in frozen]
    params = [t for _, t in named]
    seen = []
    real = ops.gru_bwd
    monkeypatch.setattr(ops, "gru_bwd", lambda *a, **k: (seen.append(1), real(*a, **k))[1])
    try:
        for t in params:
            t.requires_grad_(True)
        monkeypatch.setattr(training, "HIP_AUTOGRAD_OPS", False)
        loss_off, g_off = _loss_and_grads(model, staged, n, y, params)
        assert not seen
        monkeypatch.setattr(training, "HIP_AUTOGRAD_OPS", True)
        loss_on, g_on = _loss_and_grads(model, staged, n, y, params)
        assert len(seen) == 2                       # gru1 and gru2
    finally:
        for t in params:
            t.requires_grad_(False)
    assert abs(loss_on - loss_off) <= 1e-5 * abs(loss_off)
    gmax = max(float(np.abs(g).max()) for g in g_off if g is not None)
    gru = 0
    for (k, _), a, b in zip(named, g_on, g_off):
        assert (a is None) == (b is None), k
        if a is not None:
            _normalised(a, b, gmax, "%s neg=%d: d %s" % (gru_type, neg, k))
            gru += "gru" in k and float(np.abs(a).max()) > 0
    assert gru == 8


@pytest.mark.parametrize("gru_type,neg", [("GRU", False), ("AUGRU", True)])
def test_fit_runs_the_gru_backward_on_hip(device, gru_type, neg, monkeypatch):
    from deepctr_amd import engine, ops, training, training_hip
    n = 192
    model, feed, rng = _dien(device, gru_type, neg, n, 9)
    y = (feed["item_id"] % 2).astype(np.float32)
    before = [w.clone() for layer in (model.gru1, model.gru2) for w in layer.operands()]
    seen = []
    real = ops.gru_bwd
    monkeypatch.setattr(ops, "gru_bwd", lambda *a, **k: (seen.append(1), real(*a, **k))[1])
    assert not training_hip.supported(model)
    model.compile("adam", "binary_crossentropy")
    hist = model.fit(feed, y, batch_size=64, epochs=1, verbose=0)
    assert np.isfinite(hist.history["loss"]).all()
    assert len(seen) == 2 * (n // 64)
    after = [w for layer in (model.gru1, model.gru2) for w in layer.operands()]
    assert len(after) == 8 and all(not torch.equal(a, b) for a, b in zip(after, before))
    slim = {k: v for k, v in feed.items() if not k.startswith("neg_")}
    got = np.asarray(model.predict_logits(slim, batch_size=64)).reshape(-1)
    staged = engine.Staged(n)
    model._stage_inputs(feed, staged)
    model._begin()
    with torch.no_grad():
        logit = training.model_logits(model, staged, 0, n)
    assert logit.grad_fn is None and len(seen) == 2 * (n // 64)
    assert_close(got, logit.double().cpu().numpy().reshape(-1), rtol=1e-4, atol=2e-5, what="%s: predict_logits vs model_logits" % gru_type)
