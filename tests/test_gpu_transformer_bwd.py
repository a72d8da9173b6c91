"""GPU: dctr_transformer_train_fwd / dctr_transformer_bwd (deepctr_amd/csrc/transformer_kernels.hip, transformer_bwd_kernels.hip) against
the float64 oracle of tests/ref_transformer_bwd.py on every case of the table there, the differentiable stack
(ops.TransformerFunction, training.transformer) and its fallbacks, and BST and DSIN on the autograd step with the Transformer on HIP.
The oracle, the table and the room the bar leaves are pinned without a GPU by tests/test_transformer_bwd_oracle_cpu.py.

Bar of the op: tests.util.assert_close_terms' defaults — 1e-4 of the result plus 2e-6 of the summed magnitude — for every case and
output; none has a bar of its own.  The tape is the kernel's own forward (ops.transformer_train).  Weight gradients ACCUMULATE, so
each starts at a random non-zero g0 of the result's magnitude and ``g - g0`` is compared, |g0| added to ``terms``.  dx is exercised
written onto NaN and accumulated onto a sentinel; x, d_out and dx sit on padded sample and row strides: the padding of dx comes back
bit-identical, the inputs unchanged.  The caller's workspace has a guard tail that comes back untouched.

Worst err / bar per case, largest over the outputs (for judging a later change of the bar):
  float32 torch autograd on the CPU (test_transformer_bwd_oracle_cpu.py -s): see that file's docstring
  these tests on an MI355X (MEASURED_GPU below; nothing varies from call to call): at most 0.069 (sum_general, d_fw2 of the last layer)."""
import functools

import numpy as np
import pytest
import torch

from tests import ref_transformer_bwd as RT
from tests.util import TERMS_REPORT, assert_close, assert_close_terms

pytestmark = pytest.mark.gpu

# case -> worst err / bar over its outputs and both dx modes, on an MI355X
MEASURED_GPU = {"bst": 0.023, "dsin_pe": 0.017, "dsin_t1": 0.0082, "sum_general": 0.069, "no_res": 0.0056, "no_ffn": 0.021}

GUARD = 1024
SENTINEL = 0.75
PAD_ROW, PAD_SAMPLE = 3, 5          # floats behind every position's row and behind every sample's block
E_NULL, E_DIM, E_ENUM, E_UNSUPPORTED = -1, -2, -4, -5


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


def padded2(a, device, fill=-3.5):
    B, E = a.shape
    buf = torch.full((B, E + PAD_ROW), fill, device=device)
    buf[:, :E].copy_(dev(a.astype(np.float32), device))
    return buf, buf[:, :E]


def pad_mask(B, T, E, device):
    m = torch.ones(B, T * (E + PAD_ROW) + PAD_SAMPLE, dtype=torch.bool, device=device)
    m[:, :T * (E + PAD_ROW)].view(B, T, E + PAD_ROW)[:, :, :E] = False
    return m


@functools.lru_cache(maxsize=None)
def _reference(name):
    """Case, inputs, oracle and g0 of a case: computed once, never modified."""
    case = RT.CASE_BY_NAME[name]
    inp = RT.case_inputs(case)
    G, T = RT.transformer_bwd(inp.x, inp.layers, case.cfg, inp.qmask, inp.kmask, inp.d_out)
    rng = np.random.RandomState(11)
    g0 = {k: (rng.standard_normal(G[k].shape) * max(float(np.sqrt(np.mean(np.square(G[k])))), 1e-3)).astype(np.float32)
          for k, _, _ in RT.grad_keys(case.cfg)}
    return case, inp, G, T, g0


def _flags(cfg):
    return dict(use_positional_encoding=cfg.pe, use_res=cfg.res, use_feed_forward=cfg.ffn, use_layer_norm=cfg.ln, blinding=cfg.blind,
                output_type=cfg.out)


def _operands(device, case, inp):
    xbuf, xd = padded3(inp.x, device)
    wd = [{k: (None if w is None else dev(w, device)) for k, w in W.items()} for W in inp.layers]
    dbuf, dd = padded3(inp.d_out, device) if case.cfg.out is None else padded2(inp.d_out, device)
    if case.masks == "lengths":
        lens = dev(inp.lengths, device)
        masks = dict(query_lengths=lens, key_lengths=lens)
    elif case.masks is None:
        masks = {}
    else:
        masks = dict(query_mask=dev(inp.qmask.astype(np.uint8), device), key_mask=dev(inp.kmask.astype(np.uint8), device))
    return xbuf, xd, wd, dbuf, dd, masks


def _call(device, name, dx_mode, calls=1, outputs=None):
    """``calls`` identical calls from g0; returns (dx of each call, {key: weight gradient} of each call)."""
    from deepctr_amd import ops
    case, inp, G, T, g0 = _reference(name)
    cfg = case.cfg
    outputs = case.outputs if outputs is None else outputs
    B = case.B
    xbuf, xd, wd, dbuf, dd, masks = _operands(device, case, inp)
    _, tape = ops.transformer_train(xd, wd, cfg.H, route=case.route, **masks, **_flags(cfg))
    need = ops.transformer_bwd_workspace_bytes(B, cfg.T, cfg.E, cfg.H, cfg.L, cfg.pe, cfg.res, cfg.ffn, cfg.ln, cfg.blind, cfg.out, case.route,
                                               case.max_blocks)
    assert need == RT.plan(cfg, B, case.route, case.max_blocks).workspace_bytes and need % 4 == 0
    inputs = [xbuf, tape, dbuf] + [w for W in wd for w in W.values() if w is not None] + list(masks.values())
    snap = [bits(t) if t.dtype == torch.float32 else t.cpu().numpy().copy() for t in inputs]
    mask = pad_mask(B, cfg.T, cfg.E, device)
    dxs, grads = [], []
    for _ in range(calls):
        dxbuf, dx = padded3(np.zeros_like(inp.x), device, fill=SENTINEL)
        dx.fill_(float("nan") if dx_mode == "write" else SENTINEL)
        ws = torch.full((need // 4 + GUARD,), float("nan"), device=device)
        gd = {k: dev(g, device) for k, g in g0.items()}
        flat = [None] * (9 * cfg.L)
        for k, l, m in RT.grad_keys(cfg):
            flat[9 * l + m] = gd[k]
        ops.transformer_bwd(xd, wd, cfg.H, tape, dd, dx=dx if outputs != "weights" else None, accumulate=dx_mode == "add",
                            d_weights=flat if outputs != "dx" else None, max_blocks=case.max_blocks, route=case.route,
                            workspace=ws[:need // 4], **masks, **_flags(cfg))
        torch.cuda.synchronize()
        assert torch.isnan(ws[need // 4:]).all(), "%s: the workspace's guard was written" % name
        assert (bits(dxbuf[mask]) == bits(torch.full_like(dxbuf[mask], SENTINEL))).all(), "%s: dx's padding changed" % name
        dxs.append(dx.cpu().numpy())
        grads.append({k: g.cpu().numpy() for k, g in gd.items()})
    for t, s in zip(inputs, snap):
        assert ((bits(t) if t.dtype == torch.float32 else t.cpu().numpy()) == s).all(), "%s: an input changed" % name
    return dxs, grads


def _compare(name, dx_mode, dxs, grads, outputs=None):
    case, inp, G, T, g0 = _reference(name)
    outputs = case.outputs if outputs is None else outputs
    worst = {}
    base = SENTINEL if dx_mode == "add" else 0.0
    if outputs != "weights":
        assert np.isfinite(dxs[0]).all(), "%s: dx holds what it held before (NaN) or a NaN was read" % name
        n0 = len(TERMS_REPORT)
        assert_close_terms(dxs[0].astype(np.float64) - base, G["dx"], T["dx"] + abs(base), what="%s dx (%s)" % (name, dx_mode))
        worst["dx"] = TERMS_REPORT[n0][4]
    else:
        assert (np.isnan(dxs[0]) if dx_mode == "write" else dxs[0] == SENTINEL).all(), "%s: dx was not asked for" % name
    for k, g in grads[0].items():
        if outputs == "dx":
            assert (g == g0[k]).all(), "%s: %s was not asked for" % (name, k)
            continue
        n0 = len(TERMS_REPORT)
        assert_close_terms(g.astype(np.float64) - g0[k], G[k], T[k] + np.abs(g0[k]), what="%s %s" % (name, k))
        worst[k] = TERMS_REPORT[n0][4]
    print("[transformer_bwd] %s %s: worst err / bar %.3g (%s)" % (name, dx_mode, max(worst.values()),
                                                                 ", ".join("%s %.2g" % kv for kv in sorted(worst.items()))))
    return worst


@pytest.mark.parametrize("name", [c.name for c in RT.CASES])
def test_op_against_the_oracle(device, name):
    """Both dx modes; the second of two identical calls repeats dx AND the weight gradients bit for bit (no atomics anywhere)."""
    dxs, grads = _call(device, name, "write", calls=2)
    _compare(name, "write", dxs, grads)
    assert (dxs[0].view(np.int32) == dxs[1].view(np.int32)).all()
    assert all((grads[0][k].view(np.int32) == grads[1][k].view(np.int32)).all() for k in grads[0])
    _compare(name, "add", *_call(device, name, "add"))


@pytest.mark.parametrize("name", [c.name for c in RT.CASES])
def test_training_forward(device, name):
    """The training forward gives dctr_transformer_fwd's bits, and the tape holds the oracle's layer inputs at the documented place."""
    from deepctr_amd import ops
    case, inp, G, T, g0 = _reference(name)
    cfg = case.cfg
    xbuf, xd, wd, _, _, masks = _operands(device, case, inp)
    plain = ops.transformer(xd, wd, cfg.H, route=case.route, **masks, **_flags(cfg))
    got, tape = ops.transformer_train(xd, wd, cfg.H, route=case.route, **masks, **_flags(cfg))
    assert (bits(plain) == bits(got)).all(), "%s: the training forward is not dctr_transformer_fwd's" % name
    assert tuple(tape.shape) == (cfg.L - 1, case.B, cfg.T, cfg.E) and tape.numel() * 4 == RT.plan(cfg, case.B).tape_bytes
    keep, out = RT.forward(inp.x, inp.layers, cfg, inp.qmask, inp.kmask)
    tp = tape.cpu().numpy()
    for l in range(1, cfg.L):
        assert_close_terms(tp[l - 1], keep[l]["X"], keep[l]["tX"], what="%s: tape, input of layer %d" % (name, l))
    assert np.isfinite(got.cpu().numpy()).all()


@pytest.mark.parametrize("name", ["bst", "dsin_pe"])
def test_optional_outputs(device, name):
    """dx alone and the weight gradients alone: what is asked for equals the full call's bit for bit; with some entries of d_weights
    None the others do too."""
    from deepctr_amd import ops
    case, inp, G, T, g0 = _reference(name)
    cfg = case.cfg
    full = _call(device, name, "write", outputs="both")
    only_dx = _call(device, name, "write", outputs="dx")
    assert (full[0][0].view(np.int32) == only_dx[0][0].view(np.int32)).all()
    assert all((only_dx[1][0][k] == g0[k]).all() for k in g0)       # not asked for: not touched
    only_w = _call(device, name, "write", outputs="weights")
    assert np.isnan(only_w[0][0]).all()
    assert all((full[1][0][k].view(np.int32) == only_w[1][0][k].view(np.int32)).all() for k in g0)
    xbuf, xd, wd, dbuf, dd, masks = _operands(device, case, inp)
    _, tape = ops.transformer_train(xd, wd, cfg.H, **masks, **_flags(cfg))
    flat, kept = [None] * (9 * cfg.L), {}
    for i, (k, l, m) in enumerate(RT.grad_keys(cfg)):
        if i % 2:
            flat[9 * l + m] = kept[k] = dev(g0[k], device)
    ops.transformer_bwd(xd, wd, cfg.H, tape, dd, d_weights=flat, max_blocks=case.max_blocks, **masks, **_flags(cfg))
    for k, g in kept.items():
        assert (bits(g) == full[1][0][k].view(np.int32)).all(), k


def test_argument_errors_launch_nothing(device):
    from deepctr_amd import _C, ops
    case, inp, G, T, g0 = _reference("bst")
    cfg = case.cfg
    xbuf, xd, wd, dbuf, dd, masks = _operands(device, case, inp)
    _, tape = ops.transformer_train(xd, wd, cfg.H, **masks, **_flags(cfg))
    dx = torch.full_like(dev(inp.x, device), SENTINEL)
    gd = [None] * (9 * cfg.L)
    for k, l, m in RT.grad_keys(cfg):
        gd[9 * l + m] = torch.full_like(dev(g0[k], device), SENTINEL)

    def refused(rc, **kw):
        args = dict(dx=dx, d_weights=gd, **masks, **_flags(cfg))
        args.update(kw)
        layers = args.pop("layers", wd)
        with pytest.raises(_C.DctrError) as err:
            ops.transformer_bwd(xd, layers, cfg.H, args.pop("tape", tape), dd, **args)
        assert err.value.rc == rc, (kw.keys(), err.value.rc)

    refused(E_UNSUPPORTED, keys=xd.clone())                                   # separate keys
    refused(E_UNSUPPORTED, layers=wd * 5, tape=torch.zeros(9 * tape[0].numel(), device=device), d_weights=None)      # ten layers
    refused(E_ENUM, max_blocks=-1)
    lens = masks["query_lengths"]
    # a lower-level call: both mask forms on one side, a NULL d_out, a short tape, no workspace
    import ctypes
    t = ops._transformer_train_shape(case.B, cfg.T, cfg.E, cfg.H, cfg.L, cfg.pe, cfg.res, cfg.ffn, cfg.ln, cfg.blind, cfg.out, None)
    lp = ops._ptr_array([W[k] for W in wd for k in RT.WEIGHTS])
    t.fwd.layers = ctypes.cast(lp, ctypes.c_void_p)
    xc = dev(inp.x, device)
    t.fwd.queries, t.fwd.query_lengths, t.fwd.key_lengths = xc.data_ptr(), lens.data_ptr(), lens.data_ptr()
    dc = dev(inp.d_out, device)
    t.tape, t.tape_bytes, t.dx = tape.data_ptr(), tape.numel() * 4, dx.data_ptr()
    call = lambda: _C.lib().dctr_transformer_bwd(ctypes.byref(t), _C.stream_ptr())      # noqa: E731
    assert call() == E_NULL                                                 # d_out
    t.d_out = dc.data_ptr()
    assert call() == E_NULL                                                 # the workspace
    need = _C.lib().dctr_transformer_bwd_workspace_bytes(ctypes.byref(t))
    ws = torch.empty(need // 4, device=device)
    t.workspace, t.workspace_bytes = ws.data_ptr(), need - 4
    assert call() == E_NULL
    t.workspace_bytes, t.tape_bytes = need, tape.numel() * 4 - 4
    assert call() == E_NULL                                                 # a short tape
    t.tape_bytes = tape.numel() * 4
    t.fwd.query_mask = lens.data_ptr()
    assert call() == E_ENUM                                                 # both mask forms on the query side
    t.fwd.query_mask = None
    t.fwd.use_res = 2
    assert call() == E_ENUM
    t.fwd.use_res = 1
    t.dx_row_stride = cfg.E - 1
    assert call() == E_DIM
    t.dx_row_stride = cfg.E
    torch.cuda.synchronize()
    for g in [dx] + [g for g in gd if g is not None]:
        assert (bits(g) == bits(torch.full_like(g, SENTINEL))).all()
    assert call() == 0                                                      # and the same struct, complete, runs
    torch.cuda.synchronize()
    assert_close_terms(dx.cpu().numpy(), G["dx"], T["dx"], what="the low-level call")


# ---------------------------------------------------------------------------------------------------
# the function
# ---------------------------------------------------------------------------------------------------
def _normalised(got, ref, gmax, what, rtol=5e-4, atol=1e-5):
    """The bar of tests/test_gpu_bilstm_bwd.py:_normalised: relative to the tensor's largest gradient, at least 1e-2 of the step's."""
    scale = max(float(np.abs(ref).max()), 1e-2 * gmax)
    assert_close(np.asarray(got) / scale, np.asarray(ref) / scale, rtol=rtol, atol=atol, what=what)


def _count(monkeypatch):
    from deepctr_amd import ops, training
    seen = {"hip": 0, "torch": 0}
    real_bwd, real_torch = ops.transformer_bwd, training._transformer
    monkeypatch.setattr(ops, "transformer_bwd", lambda *a, **k: (seen.__setitem__("hip", seen["hip"] + 1), real_bwd(*a, **k))[1])
    monkeypatch.setattr(training, "_transformer", lambda *a, **k: (seen.__setitem__("torch", seen["torch"] + 1), real_torch(*a, **k))[1])
    return seen


@pytest.mark.parametrize("name", ["bst", "dsin_pe", "no_res", "sum_general"])
def test_function_is_differentiable(device, name, monkeypatch):
    """training.transformer (one TransformerFunction for the stack) against float32 autograd of _transformer on the same device: the
    loss, dx and every weight gradient."""
    from deepctr_amd import training
    case, inp, G, T, g0 = _reference(name)
    cfg = case.cfg
    seen = _count(monkeypatch)
    dy = dev(inp.d_out, device)
    qm, km = dev(inp.qmask, device), dev(inp.kmask, device)

    def run(hip):
        monkeypatch.setattr(training, "HIP_AUTOGRAD_OPS", hip)
        layers = [RT.TorchLayer(W, cfg, torch.float32, device) for W in inp.layers]
        for layer in layers[:-1]:       # a pooled stack pools after its last layer
            layer.output_type = None
        xg = dev(inp.x, device).requires_grad_(True)
        y = training.transformer(layers, xg, qm, km, False, lengths=None if inp.lengths is None else dev(inp.lengths, device))
        if cfg.out is not None:
            assert tuple(y.shape) == (case.B, 1, cfg.E)
            y = y.squeeze(1)
        loss = (y * dy).sum()
        loss.backward()
        grads = {"dx": xg.grad.cpu().numpy()}
        for l, layer in enumerate(layers):
            for k, g in layer.grads().items():
                grads["%s%d" % (k, l)] = g
        return float(loss.detach()), grads

    loss_hip, got = run(True)
    assert seen == {"hip": 1, "torch": 0}
    loss_ref, ref = run(False)
    assert seen == {"hip": 1, "torch": cfg.L}
    assert abs(loss_hip - loss_ref) <= 1e-4 * max(abs(loss_ref), float(np.abs(T["dx"]).mean()))
    gmax = max(float(np.abs(r).max()) for r in ref.values())
    assert set(got) == set(ref)
    for k in ref:
        _normalised(got[k], ref[k], gmax, "%s: %s" % (name, k))
        if k in G:
            assert_close_terms(got[k], G[k], T[k], what="%s through the function: %s" % (name, k))


@pytest.mark.parametrize("why", ["dropout", "keys", "no_grad", "switch", "unsupported", "nothing_requires_grad", "min_rows"])
def test_fallbacks_take_the_torch_ops(device, why, monkeypatch):
    from deepctr_amd import ops, training
    case, inp, G, T, g0 = _reference("bst")
    cfg = case.cfg
    seen = _count(monkeypatch)
    n_layers = 9 if why == "unsupported" else cfg.L
    layers = [RT.TorchLayer(inp.layers[i % cfg.L], cfg, torch.float32, device, dropout_rate=0.5 if why == "dropout" else 0.0)
              for i in range(n_layers)]
    xg = dev(inp.x, device).requires_grad_(why != "nothing_requires_grad")
    qm = dev(inp.qmask, device)
    kw = {}
    if why == "keys":
        kw["keys"] = xg.detach().clone()
    if why == "switch":
        monkeypatch.setattr(training, "HIP_AUTOGRAD_OPS", False)
    if why == "min_rows":
        monkeypatch.setattr(training, "TRANSFORMER_HIP_MIN_ROWS", case.B + 1)
    if why == "nothing_requires_grad":
        for layer in layers:
            for t in layer.t.values():
                t.requires_grad_(False)
    if why == "unsupported":
        assert not ops.transformer_bwd_supported(cfg.T, cfg.E, cfg.H, n_layers, **_flags(cfg))
    torch.manual_seed(3)
    if why == "no_grad":
        with torch.no_grad():
            y = training.transformer(layers, xg, qm, qm, True, **kw)
    else:
        y = training.transformer(layers, xg, qm, qm, True, **kw)
        if why != "nothing_requires_grad":
            y.sum().backward()
            assert xg.grad is not None and torch.isfinite(xg.grad).all()
    assert seen == {"hip": 0, "torch": n_layers} and torch.isfinite(y).all()
    # and the same call without the reason goes to the HIP op
    if why in ("switch", "min_rows"):
        monkeypatch.undo()
        seen = _count(monkeypatch)
        xg = dev(inp.x, device).requires_grad_(True)
        training.transformer(layers, xg, qm, qm, True).sum().backward()
        assert seen == {"hip": 1, "torch": 0}


# ---------------------------------------------------------------------------------------------------
# the models
# ---------------------------------------------------------------------------------------------------
def _two_steps(model_fn, feed, y, hip, monkeypatch, seen):
    """Two SGD steps of fit() from the same seed: (losses, {name: weight after}, {name: weight before})."""
    from deepctr_amd import training
    monkeypatch.setattr(training, "HIP_AUTOGRAD_OPS", hip)
    model = model_fn()
    before = {k: t.detach().cpu().numpy().copy() for k, t in model.named_weights()}
    model.compile("sgd", "binary_crossentropy")
    torch.manual_seed(17)
    hist = model.fit(feed, y, batch_size=len(y), epochs=2, verbose=0, shuffle=False)
    after = {k: t.detach().cpu().numpy().copy() for k, t in model.named_weights()}
    return hist.history["loss"], after, before


def _check_models(model_fn, feed, y, monkeypatch, expect_hip, expect_bilstm=0):
    from deepctr_amd import ops
    seen = _count(monkeypatch)
    lstm = []
    real = ops.bilstm_bwd
    monkeypatch.setattr(ops, "bilstm_bwd", lambda *a, **k: (lstm.append(1), real(*a, **k))[1])
    loss_on, w_on, w0 = _two_steps(model_fn, feed, y, True, monkeypatch, seen)
    assert seen["hip"] == expect_hip and seen["torch"] == 0 and len(lstm) == expect_bilstm
    loss_off, w_off, _ = _two_steps(model_fn, feed, y, False, monkeypatch, seen)
    assert seen["hip"] == expect_hip and seen["torch"] > 0 and len(lstm) == expect_bilstm
    assert np.isfinite(loss_on).all() and len(loss_on) == 2
    for a, b in zip(loss_on, loss_off):
        assert abs(a - b) <= 1e-5 * abs(b), (loss_on, loss_off)
    steps = {k: w_off[k] - w0[k] for k in w0}
    smax = max(float(np.abs(s).max()) for s in steps.values())
    moved = 0
    for k in w0:
        # the bar of _normalised on the two-step update, plus what storing a float32 weight costs: half an ulp of the weight per step
        # and route, 4 x 2^-23 |w| in all (the update is a difference of stored weights)
        scale = max(float(np.abs(steps[k]).max()), 1e-2 * smax)
        err = np.abs((w_on[k] - w0[k]).astype(np.float64) - steps[k])
        bar = 5e-4 * np.abs(steps[k]) + 1e-5 * scale + 4 * 2.0 ** -23 * np.abs(w_off[k])
        assert (err <= bar).all(), "update of %s: max err / bar = %.3g" % (k, float((err / bar).max()))
        moved += ("transformer" in k or "position_encoding" in k or "layer_normalization" in k) and float(np.abs(w_on[k] - w0[k]).max()) > 0
    return moved


def test_bst_trains_through_the_hip_transformer(device, monkeypatch):
    from deepctr_amd.models import BST
    from tests.test_gpu_bst import _bst_problem, _randomise
    rng = np.random.RandomState(9)
    n = 96
    cols, names, feed = _bst_problem(rng, n, T=6, vocab=20)
    y = rng.randint(0, 2, n).astype(np.float32)

    def build():
        model = BST(cols, names, transformer_num=2, att_head_num=2, dnn_hidden_units=(16, 8), device=device)
        _randomise(model, np.random.RandomState(4))
        return model
    moved = _check_models(build, feed, y, monkeypatch, expect_hip=2)
    assert moved >= 2 * 9 - 2


def test_dsin_trains_through_the_hip_transformer_and_bilstm(device, monkeypatch):
    from deepctr_amd.models import DSIN
    from tests.dsin_util import dsin_problem, randomise
    rng = np.random.RandomState(8)
    n = 96
    cols, names, feed = dsin_problem(rng, n, vocab=20)
    y = rng.randint(0, 2, n).astype(np.float32)

    def build():
        model = DSIN(cols, names, sess_max_count=3, bias_encoding=False, att_embedding_size=3, att_head_num=4, dnn_hidden_units=(16, 8),
                     device=device)
        randomise(model, np.random.RandomState(4))
        return model
    moved = _check_models(build, feed, y, monkeypatch, expect_hip=2, expect_bilstm=2)
    assert moved >= 5
