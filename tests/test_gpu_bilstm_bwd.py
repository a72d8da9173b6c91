"""GPU: dctr_bilstm_train_fwd / dctr_bilstm_bwd (deepctr_amd/csrc/lstm_kernels.hip, lstm_bwd_kernels.hip) against the float64 oracle of
tests/ref_bilstm_bwd.py on every case of the table there, the differentiable BiLSTM (ops.BiLSTMFunction, training.bilstm), and DSIN
on the autograd step with its BiLSTM on HIP.  The oracle, the table and the room the bar leaves are pinned without a GPU by
tests/test_bilstm_bwd_oracle_cpu.py.

Bar of the op: tests.util.assert_close_terms' defaults — 1e-4 of the result plus 2e-6 of the summed magnitude — for every case and
output; none has a bar of its own.  The tape is the kernel's own forward (ops.bilstm_train).  Weight gradients ACCUMULATE, so each
starts at a random non-zero g0 of the result's magnitude and ``g - g0`` is compared, |g0| added to ``terms``.  dx is exercised
written onto NaN and accumulated onto a sentinel; x, d_out and dx sit on padded sample and step strides: the padding of dx comes back
bit-identical, the inputs unchanged.  The caller's workspace has a guard tail that comes back untouched.

Worst err / bar per case, largest over the outputs (for judging a later change of the bar):
  float32 torch autograd on the CPU (test_bilstm_bwd_oracle_cpu.py -s): see that file's docstring
  these tests on an MI355X (MEASURED_GPU below; nothing varies from call to call): at most 0.26 (u16_D16_T1_B1_L1_r1_fw_none)."""
import functools

import numpy as np
import pytest
import torch

from tests import ref_bilstm_bwd as RB
from tests.util import TERMS_REPORT, assert_close, assert_close_terms

pytestmark = pytest.mark.gpu

# case -> worst err / bar over its outputs and both dx modes, on an MI355X
MEASURED_GPU = {
    "u4_D7_T1_B1_L1_r0_fw_all": 0.018, "u4_D4_T2_B17_L2_r2_bw_none": 0.015, "u4_D7_T5_B33_L3_r1_sum_partial": 0.016,
    "u12_D9_T2_B17_L2_r1_mul_all": 0.052, "u12_D15_T5_B33_L3_r0_ave_none": 0.013, "u12_D12_T1_B1_L1_r1_concat_partial": 0.017,
    "u16_D16_T5_B33_L3_r3_None_all": 0.0028, "u16_D16_T1_B1_L1_r1_fw_none": 0.26, "u16_D19_T2_B17_L2_r0_bw_partial": 0.035,
    "u17_D14_T1_B1_L1_r0_sum_all": 0.023, "u17_D17_T2_B17_L2_r2_mul_none": 0.031, "u17_D14_T5_B33_L3_r1_ave_partial": 0.018,
    "u40_D43_T2_B17_L2_r1_concat_all": 0.064, "u40_D37_T5_B33_L3_r0_None_none": 0.015, "u40_D40_T1_B17_L1_r1_fw_partial": 0.028,
    "u52_D52_T5_B33_L3_r3_bw_all": 0.013, "u52_D52_T1_B17_L1_r1_sum_none": 0.033, "u52_D49_T2_B33_L2_r0_mul_partial": 0.077,
    "u12_D12_T5_B17_L2_r0_fw_all_dsin": 0.012, "u12_D12_T5_B17_L2_r0_bw_all_dsin": 0.0095,
    "u12_D12_T5_B17_L2_r0_sum_all_dsin": 0.0097, "u12_D12_T5_B17_L2_r0_mul_all_dsin": 0.014,
    "u12_D12_T5_B17_L2_r0_ave_all_dsin": 0.0078, "u12_D12_T5_B17_L2_r0_concat_all_dsin": 0.0083,
    "u12_D12_T5_B17_L2_r0_None_all_dsin": 0.0081, "u12_D9_T5_B33_L2_r1_ave_partial_streamed": 0.0076,
    "u16_D16_T2_B33_L3_r3_None_all_resident": 0.021}

GUARD = 1024
SENTINEL = 0.75
PAD_ROW, PAD_SAMPLE = 3, 5          # floats behind every step's row and behind every sample's block
E_UNSUPPORTED = -5


def dev(a, device):
    return torch.tensor(np.asarray(a), device=device)       # (a copy: the cases' arrays are shared)


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def padded3(a, device, fill=-3.5):
    """[B, T, E] inside a buffer with PAD_ROW floats behind every row and PAD_SAMPLE behind every sample; (buffer, view)."""
    B, T, E = a.shape
    buf = torch.full((B, T * (E + PAD_ROW) + PAD_SAMPLE), fill, device=device)
    view = buf[:, :T * (E + PAD_ROW)].view(B, T, E + PAD_ROW)[:, :, :E]
    view.copy_(dev(a.astype(np.float32), device))
    return buf, view


def pad_mask(B, T, E, device):
    m = torch.ones(B, T * (E + PAD_ROW) + PAD_SAMPLE, dtype=torch.bool, device=device)
    m[:, :T * (E + PAD_ROW)].view(B, T, E + PAD_ROW)[:, :, :E] = False
    return m


def flat_grads(G):
    return [g for layer in G["d_layers"] for g in layer]


@functools.lru_cache(maxsize=None)
def _reference(name):
    """Case, inputs, oracle and g0 of a case: computed once, never modified."""
    case = RB.CASE_BY_NAME[name]
    x, layers, masks, d_out = RB.case_inputs(case)
    G, T = RB.case_oracle(case)
    rng = np.random.RandomState(11 + case.seed)
    g0 = [(rng.standard_normal(g.shape) * max(float(np.sqrt(np.mean(np.square(g)))), 1e-3)).astype(np.float32) for g in flat_grads(G)]
    return case, x, layers, masks, d_out, G, T, g0


def _operands(device, x, layers, masks, d_out, merge):
    xbuf, xd = padded3(x, device)
    wd = [[dev(w, device) for w in layer] for layer in layers]
    md = None if masks is None else [None if m is None else dev(m, device) for m in masks]
    if merge is None:
        pairs = [padded3(d, device) for d in d_out]
        dbufs, dd = [p[0] for p in pairs], tuple(p[1] for p in pairs)
    else:
        dbuf, dd = padded3(d_out, device)
        dbufs = [dbuf]
    return xbuf, xd, wd, md, dbufs, dd


def _call(device, name, dx_mode, calls=1, outputs="all"):
    """``calls`` identical calls from g0; returns (dx of each call, weight gradients of each call)."""
    from deepctr_amd import ops
    case, x, layers, masks, d_out, G, T, g0 = _reference(name)
    B, Tn, Din = x.shape
    xbuf, xd, wd, md, dbufs, dd = _operands(device, x, layers, masks, d_out, case.merge)
    _, tape = ops.bilstm_train(xd, wd, md, case.res, case.merge)
    need = ops.bilstm_bwd_workspace_bytes(B, Tn, Din, case.u, case.L, case.res, case.merge, case.route)
    assert need > 0 and need % 4 == 0
    inputs = [xbuf, tape] + dbufs + [w for layer in wd for w in layer] + [m for m in (md or []) if m is not None]
    snap = [bits(t) for t in inputs]
    mask = pad_mask(B, Tn, Din, device)
    dxs, grads = [], []
    for _ in range(calls):
        dxbuf, dx = padded3(np.zeros_like(x), device, fill=SENTINEL)
        dx.fill_(float("nan") if dx_mode == "write" else SENTINEL)
        ws = torch.full((need // 4 + GUARD,), float("nan"), device=device)
        gd = [dev(g, device) for g in g0]
        ops.bilstm_bwd(xd, wd, tape, dd, md, case.res, case.merge, dx=dx if outputs != "weights" else None, accumulate=dx_mode == "add",
                       d_weights=gd if outputs != "dx" else None, max_blocks=case.max_blocks, route=case.route, workspace=ws[:need // 4])
        torch.cuda.synchronize()
        assert torch.isnan(ws[need // 4:]).all(), "%s: the workspace's guard was written" % name
        assert (bits(dxbuf[mask]) == bits(torch.full_like(dxbuf[mask], SENTINEL))).all(), "%s: dx's padding changed" % name
        dxs.append(dx.cpu().numpy())
        grads.append([g.cpu().numpy() for g in gd])
    for t, s in zip(inputs, snap):
        assert (bits(t) == s).all(), "%s: an input changed" % name
    return dxs, grads


def _compare(name, dx_mode, dxs, grads, weights=True):
    case, x, layers, masks, d_out, G, T, g0 = _reference(name)
    worst = {}
    base = SENTINEL if dx_mode == "add" else 0.0
    assert np.isfinite(dxs[0]).all(), "%s: dx holds what it held before (NaN) or a NaN was read" % name
    n0 = len(TERMS_REPORT)
    assert_close_terms(dxs[0].astype(np.float64) - base, G["dx"], T["dx"] + abs(base), what="%s dx (%s)" % (name, dx_mode))
    worst["dx"] = TERMS_REPORT[n0][4]
    if weights:
        for k, (g, ref, terms, z) in enumerate(zip(grads[0], flat_grads(G), flat_grads(T), g0)):
            n0 = len(TERMS_REPORT)
            assert_close_terms(g.astype(np.float64) - z, ref, terms + np.abs(z), what="%s d layer %d %d" % (name, k // 6, k % 6))
            worst["w%d" % k] = TERMS_REPORT[n0][4]
    print("[bilstm_bwd] %s %s: worst err / bar %.3g (%s)" % (name, dx_mode, max(worst.values()),
                                                            ", ".join("%s %.2g" % kv for kv in sorted(worst.items()))))
    return worst


@pytest.mark.parametrize("name", [c.name for c in RB.CASES])
def test_op_against_the_oracle(device, name):
    """Both dx modes; the second of two identical calls repeats dx AND the weight gradients bit for bit (no atomics anywhere)."""
    dxs, grads = _call(device, name, "write", calls=2)
    _compare(name, "write", dxs, grads)
    assert (dxs[0].view(np.int32) == dxs[1].view(np.int32)).all()
    assert all((a.view(np.int32) == b.view(np.int32)).all() for a, b in zip(*grads))
    _compare(name, "add", *_call(device, name, "add"))


@pytest.mark.parametrize("name", [c.name for c in RB.CASES])
def test_training_forward(device, name):
    """Without masks the training forward gives dctr_bilstm_fwd's bits; with the case's masks the oracle's values, and the tape holds
    the oracle's h_t and c_t at the documented place."""
    from deepctr_amd import ops
    case, x, layers, masks, d_out, G, T, g0 = _reference(name)
    B, Tn, Din = x.shape
    xbuf, xd, wd, md, _, _ = _operands(device, x, layers, masks, d_out, case.merge)
    plain = ops.bilstm(xd, wd, case.res, case.merge)
    got, _ = ops.bilstm_train(xd, wd, None, case.res, case.merge)
    for a, b in zip(*((plain, got) if case.merge is None else ((plain,), (got,)))):
        assert (bits(a) == bits(b)).all(), "%s: the training forward without masks is not dctr_bilstm_fwd's" % name
    got, tape = ops.bilstm_train(xd, wd, md, case.res, case.merge)
    ref, (_, _, sf, sb) = RB.forward(x, layers, masks, case.res, case.merge)
    for a, r, what in zip(*(((got,), (ref,)) if case.merge is not None else (got, ref)), ("out", "out_bw")):
        assert_close(a.cpu().numpy(), r, rtol=1e-4, atol=2e-5, what="%s: %s with masks" % (name, what))
    tp = tape[:case.L * 2 * Tn * 2 * B * case.u].view(case.L, 2, Tn, 2, B, case.u).cpu().numpy()
    for d, st in enumerate((sf, sb)):
        if st is None:
            continue
        for l in range(case.L):
            steps = st[l][5]
            c = np.stack([s[5] for s in steps])
            h = np.stack([s[3] * np.tanh(s[5]) for s in steps])
            assert_close(tp[l, d, :, 0], h, rtol=1e-4, atol=2e-5, what="%s: tape h, layer %d direction %d" % (name, l, d))
            assert_close(tp[l, d, :, 1], c, rtol=1e-4, atol=2e-5, what="%s: tape c, layer %d direction %d" % (name, l, d))


@pytest.mark.parametrize("name", [RB.CASES[3].name, RB.CASES[-2].name, RB.CASES[16].name])
def test_optional_outputs(device, name):
    """dx alone and the weight gradients alone: what is asked for equals the full call's bit for bit; with some entries of d_weights
    None the others do too."""
    from deepctr_amd import ops
    full = _call(device, name, "write")
    only_dx = _call(device, name, "write", outputs="dx")
    assert (full[0][0].view(np.int32) == only_dx[0][0].view(np.int32)).all()
    case, x, layers, masks, d_out, G, T, g0 = _reference(name)
    assert all((g == z).all() for g, z in zip(only_dx[1][0], g0))       # not asked for: not touched
    only_w = _call(device, name, "write", outputs="weights")
    assert np.isnan(only_w[0][0]).all()
    assert all((a.view(np.int32) == b.view(np.int32)).all() for a, b in zip(full[1][0], only_w[1][0]))
    xbuf, xd, wd, md, dbufs, dd = _operands(device, x, layers, masks, d_out, case.merge)
    _, tape = ops.bilstm_train(xd, wd, md, case.res, case.merge)
    gd = [dev(g, device) if k % 2 else None for k, g in enumerate(g0)]
    ops.bilstm_bwd(xd, wd, tape, dd, md, case.res, case.merge, d_weights=gd, max_blocks=case.max_blocks, route=case.route)
    for k, (g, f) in enumerate(zip(gd, full[1][0])):
        assert g is None or (bits(g) == f.view(np.int32)).all(), k


@pytest.mark.parametrize("merge", ["ave", None, "mul"])
def test_saturated_gates(device, merge):
    """Biases of +-30 whose signs alternate over the units of every sample, small kernels: every gate and candidate saturates.  All
    outputs finite and within the bar (both layers residual, so dx is not all zeros) with the terms floored at the tensor's max |ref| (float64 leaves 1e-13 residues where float32
    leaves 0)."""
    from deepctr_amd import ops
    rng = np.random.RandomState(17)
    B, Tn, u, L = 19, 4, 10, 2
    x = rng.randn(B, Tn, u).astype(np.float32)
    layers = []
    for l in range(L):
        layer = []
        for d in range(2):
            sign = np.where((np.arange(4 * u) + l + d) % 2 == 0, -30.0, 30.0).astype(np.float32)
            layer += [(0.05 * rng.randn(u, 4 * u)).astype(np.float32), (0.05 * rng.randn(u, 4 * u)).astype(np.float32), sign]
        layers.append(layer)
    masks = [((rng.rand(B, u) >= 0.2) / 0.8).astype(np.float32) for _ in range(2 * L)]
    d_out = rng.randn(B, Tn, u).astype(np.float32)
    d_out = (d_out, rng.randn(B, Tn, u).astype(np.float32)) if merge is None else d_out
    G, T = RB.bilstm_bwd(x, layers, masks, L, merge, d_out)
    xd, wd, md = dev(x, device), [[dev(w, device) for w in layer] for layer in layers], [dev(m, device) for m in masks]
    dd = tuple(dev(d, device) for d in d_out) if merge is None else dev(d_out, device)
    out, tape = ops.bilstm_train(xd, wd, md, L, merge)
    assert all(torch.isfinite(o).all() for o in (out if merge is None else (out,)))
    dx = torch.full_like(xd, float("nan"))
    gd = [torch.zeros_like(w) for layer in wd for w in layer]
    ops.bilstm_bwd(xd, wd, tape, dd, md, L, merge, dx=dx, d_weights=gd)
    for k, (g, ref, terms) in enumerate(zip([dx] + gd, [G["dx"]] + flat_grads(G), [T["dx"]] + flat_grads(T))):
        g = g.cpu().numpy()
        assert np.isfinite(g).all(), (merge, k)
        assert_close_terms(g, ref, np.maximum(terms, np.abs(ref).max()), what="saturated %s: output %d" % (merge, k))


@pytest.mark.parametrize("why", ["hard_sigmoid", "oversized"])
def test_a_refusal_raises_writes_nothing_and_falls_back(device, why, monkeypatch):
    from deepctr_amd import _C, ops, training
    B, Tn, L = 5, 5, 2
    u = 12 if why == "hard_sigmoid" else 65
    act = "hard_sigmoid" if why == "hard_sigmoid" else "sigmoid"
    rng = np.random.RandomState(3)
    x = dev(rng.randn(B, Tn, u).astype(np.float32), device)
    wd = [[dev((rng.randn(*s) * 0.1).astype(np.float32), device) for s in ((u, 4 * u), (u, 4 * u), (4 * u,)) * 2] for _ in range(L)]
    dy = dev(rng.randn(B, Tn, u).astype(np.float32), device)
    assert not ops.bilstm_bwd_supported(Tn, u, u, L, recurrent_activation=act)
    assert ops.bilstm_bwd_supported(Tn, u - 1, u - 1, L) and ops.bilstm_bwd_supported(Tn, 64, 64, L)
    tape = torch.full((L * 2 * Tn * 2 * B * u,), SENTINEL, device=device)
    dx = torch.full_like(x, SENTINEL)
    gd = [torch.full_like(w, SENTINEL) for layer in wd for w in layer]
    with pytest.raises(_C.DctrError) as err:
        ops.bilstm_bwd(x, wd, tape, dy, recurrent_activation=act, dx=dx, d_weights=gd)
    assert err.value.rc == E_UNSUPPORTED
    if why == "oversized":      # (the training forward has no workspace route either; hard_sigmoid it runs)
        out = torch.full_like(x, SENTINEL)
        with pytest.raises(_C.DctrError) as err:
            ops.bilstm_train(x, wd, out=out, tape=tape)
        assert err.value.rc == E_UNSUPPORTED
        gd.append(out)
    torch.cuda.synchronize()
    for t in [dx, tape] + gd:
        assert (bits(t) == bits(torch.full_like(t, SENTINEL))).all()
    # the autograd step then takes the torch loop
    calls = []
    monkeypatch.setattr(ops, "bilstm_bwd", lambda *a, **k: calls.append(1))
    ws = [[w.clone().requires_grad_(True) for w in layer] for layer in wd]
    xg = x.clone().requires_grad_(True)
    y = training.bilstm(xg, ws, recurrent_activation=act)
    assert torch.equal(y, training._bilstm(xg, ws, recurrent_activation=act))
    y.backward(dy)
    assert not calls and xg.grad is not None and all(w.grad is not None for layer in ws for w in layer)


# ---------------------------------------------------------------------------------------------------
# the function
# ---------------------------------------------------------------------------------------------------
def _normalised(got, ref, gmax, what, rtol=5e-4, atol=1e-5):
    """The bar of tests/test_gpu_gru_bwd.py:_normalised: relative to the tensor's largest gradient, at least 1e-2 of the step's."""
    scale = max(float(np.abs(ref).max()), 1e-2 * gmax)
    assert_close(np.asarray(got) / scale, np.asarray(ref) / scale, rtol=rtol, atol=atol, what=what)


@pytest.mark.parametrize("merge", RB.MERGES)
def test_function_is_differentiable(device, merge, monkeypatch):
    """BiLSTMFunction against float32 autograd of _bilstm under one seed: two layers, the upper one residual, dropout 0.2."""
    from deepctr_amd import ops, training
    case = RB.Case("fn", 12, 9, 5, 37, 2, 1, merge, "none", None, 0, 90)
    x, layers, _, d_out = RB.case_inputs(case)
    dy = tuple(dev(d, device) for d in d_out) if merge is None else dev(d_out, device)

    def run(fn, rate=0.2, train=True):
        xg = dev(x, device).requires_grad_(True)
        ws = [[dev(w, device).requires_grad_(True) for w in layer] for layer in layers]
        torch.manual_seed(5)
        y = fn(xg, ws, 1, merge, "sigmoid", rate, train)
        if merge is None:
            torch.autograd.backward(y, dy)
        else:
            y.backward(dy)
        ys = y if merge is None else (y,)
        return [t.detach().cpu().numpy() for t in ys], [(torch.zeros_like(t) if t.grad is None else t.grad).cpu().numpy() for t in [xg] + [w for layer in ws for w in layer]]

    seen = []
    real = ops.bilstm_bwd
    monkeypatch.setattr(ops, "bilstm_bwd", lambda *a, **k: (seen.append(1), real(*a, **k))[1])
    y_hip, got = run(training.bilstm)
    assert len(seen) == 1
    y_ref, ref = run(training._bilstm)
    assert len(seen) == 1
    for a, b in zip(y_hip, y_ref):
        assert_close(a, b, rtol=1e-4, atol=2e-5, what="%s: forward under the same masks" % (merge,))
    gmax = max(float(np.abs(r).max()) for r in ref)
    walked = {"fw": (0, 1, 2), "bw": (3, 4, 5)}.get(merge, range(6))
    for k, (g, r) in enumerate(zip(got, ref)):
        _normalised(g, r, gmax, "%s: gradient %d" % (merge, k))
        assert k == 0 or ((k - 1) % 6 in walked) == bool(np.abs(g).max() > 0), (merge, k)
    # without dropout the forward's value is dctr_bilstm_fwd's
    y_plain, _ = run(training.bilstm, 0.0, False)
    plain = ops.bilstm(dev(x, device), [[dev(w, device) for w in layer] for layer in layers], 1, merge)
    for a, b in zip(y_plain, plain if merge is None else (plain,)):
        assert (a == b.cpu().numpy()).all()
    assert len(seen) == 2
    # under no_grad, and with nothing requiring grad: the torch loop
    with torch.no_grad():
        training.bilstm(dev(x, device).requires_grad_(True), [[dev(w, device) for w in layer] for layer in layers], 1, merge)
    training.bilstm(dev(x, device), [[dev(w, device) for w in layer] for layer in layers], 1, merge)
    assert len(seen) == 2


# ---------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------
def _loss_and_grads(model, staged, n, y, params, seed):
    from deepctr_amd import training
    model._begin()
    torch.manual_seed(seed)
    logit = training.model_logits(model, staged, 0, n, training=True)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(logit, y)
    grads = torch.autograd.grad(loss, params, allow_unused=True)
    return float(loss.detach()), [None if g is None else g.cpu().numpy() for g in grads]


@pytest.mark.parametrize("bias", [False, True])
def test_model_gradients_with_the_switch_on_and_off(device, bias, monkeypatch):
    """DSIN as it is built (two layers, dropout 0.2, no residual): every parameter's gradient under one seed."""
    from deepctr_amd import engine, ops, training
    from deepctr_amd.models import DSIN
    from tests.dsin_util import dsin_problem, randomise
    n = 203
    rng = np.random.RandomState(8)
    cols, names, feed = dsin_problem(rng, n, vocab=20)
    model = DSIN(cols, names, sess_max_count=3, bias_encoding=bias, att_embedding_size=3, att_head_num=4, dnn_hidden_units=(16, 8), device=device)
    randomise(model, rng)
    assert model.bilstm.dropout_rate == 0.2
    y = dev(rng.randint(0, 2, n).astype(np.float32), device)
    staged = engine.Staged(n)
    model._stage_inputs(feed, staged)
    frozen = training.frozen_weights(model)
    named = [(k, t) for k, t in model.named_weights() if "moving_" not in k and t.data_ptr() not in frozen]
    params = [t for _, t in named]
    seen = []
    real = ops.bilstm_bwd
    monkeypatch.setattr(ops, "bilstm_bwd", lambda *a, **k: (seen.append(1), real(*a, **k))[1])
    try:
        for t in params:
            t.requires_grad_(True)
        monkeypatch.setattr(training, "HIP_AUTOGRAD_OPS", False)
        loss_off, g_off = _loss_and_grads(model, staged, n, y, params, 21)
        assert not seen
        monkeypatch.setattr(training, "HIP_AUTOGRAD_OPS", True)
        loss_on, g_on = _loss_and_grads(model, staged, n, y, params, 21)
        assert len(seen) == 1
    finally:
        for t in params:
            t.requires_grad_(False)
    assert abs(loss_on - loss_off) <= 1e-5 * abs(loss_off)
    gmax = max(float(np.abs(g).max()) for g in g_off if g is not None)
    lstm = 0
    for (k, _), a, b in zip(named, g_on, g_off):
        assert (a is None) == (b is None), k
        if a is not None:
            _normalised(a, b, gmax, "bias_encoding=%d: d %s" % (bias, k))
            lstm += "lstm" in k and float(np.abs(a).max()) > 0
    assert lstm == 12


def test_a_bare_layer_with_a_residual(device, monkeypatch):
    """BiLSTM as a layer of its own with a residual layer and concat, through training.bilstm and the layer's operands."""
    from deepctr_amd import ops, training
    from deepctr_amd.layers.sequence import BiLSTM
    rng = np.random.RandomState(12)
    B, Tn, u = 70, 4, 8
    layer = BiLSTM(u, layers=3, res_layers=2, merge_mode="concat", dropout_rate=0.3, device=device).build_for(u)
    x = dev(rng.randn(B, Tn, u).astype(np.float32), device)
    dy = dev(rng.randn(B, Tn, 2 * u).astype(np.float32), device)
    params = [w for ws in layer.operands() for w in ws]
    seen = []
    real = ops.bilstm_bwd
    monkeypatch.setattr(ops, "bilstm_bwd", lambda *a, **k: (seen.append(1), real(*a, **k))[1])
    res = {}
    try:
        for t in params:
            t.requires_grad_(True)
        for on in (False, True):
            monkeypatch.setattr(training, "HIP_AUTOGRAD_OPS", on)
            xg = x.clone().requires_grad_(True)
            torch.manual_seed(3)
            out = training.bilstm(xg, layer.operands(), layer.res_layers, layer.merge_mode, layer.recurrent_activation, layer.dropout_rate, True)
            res[on] = [g.cpu().numpy() for g in torch.autograd.grad(out, [xg] + params, dy)]
            assert len(seen) == int(on)
    finally:
        for t in params:
            t.requires_grad_(False)
    gmax = max(float(np.abs(g).max()) for g in res[False])
    for k, (a, b) in enumerate(zip(res[True], res[False])):
        _normalised(a, b, gmax, "bare BiLSTM: gradient %d" % k)


def test_fit_runs_the_bilstm_backward_on_hip(device, monkeypatch):
    from deepctr_amd import ops, training_hip
    from deepctr_amd.models import DSIN
    from tests.dsin_util import dsin_problem
    rng = np.random.RandomState(9)
    n = 1024
    cols, names, feed = dsin_problem(rng, n, vocab=20)
    y = ((feed["item"] % 2) ^ (feed["sess_0_item"][:, 0] % 2)).astype(np.float32)
    model = DSIN(cols, names, sess_max_count=3, att_embedding_size=3, att_head_num=4, dnn_hidden_units=(32, 16), device=device)
    assert not training_hip.supported(model)
    before = [w.clone() for ws in model.bilstm.operands() for w in ws]
    seen = []
    real = ops.bilstm_bwd
    monkeypatch.setattr(ops, "bilstm_bwd", lambda *a, **k: (seen.append(1), real(*a, **k))[1])
    model.compile("adam", "binary_crossentropy")
    hist = model.fit(feed, y, batch_size=256, epochs=4, verbose=0)
    loss = hist.history["loss"]
    assert np.isfinite(loss).all() and loss[-1] < loss[0], loss
    assert len(seen) == 4 * (n // 256)
    after = [w for ws in model.bilstm.operands() for w in ws]
    assert len(after) == 12 and all(not torch.equal(a, b) for a, b in zip(after, before))
