"""GPU: EDCN's training forward (ops.edcn_train: dctr_edcn_train_fwd) against ops.edcn and the float64 tower, its backward
(ops.edcn_bwd: dctr_edcn_bwd) against the float64 oracle of tests/ref_edcn_bwd.py evaluated on the device's own tape, the slice
counts of the weight-gradient pass, ops.EDCNTowerFunction under autograd against torch double autograd, and the model: the gate, the
gradients with the switch on against off, and fit()."""
import numpy as np
import pytest
import torch

from tests import ref_edcn as RE
from tests import ref_edcn_bwd as RB
from tests.test_edcn_bwd_oracle_cpu import _autograd
from tests.test_edcn_cpu import ref_tower, tower_case
from tests.test_gpu_edcn import _cols, _feed, deep_dev, dev
from tests.util import assert_close_terms

pytestmark = pytest.mark.gpu

BAR = dict(rtol=1e-4, rtol_terms=RB.BWD_RTOL_TERMS)
FWD_BAR = dict(rtol=1e-4, rtol_terms=RE.TOWER_RTOL_TERMS)
WORST = {}


def _operands(device, F, d, L, B, bridge_type, par, off, seed=None):
    case = tower_case(F, d, L, B, bridge_type, par, off, (0.5, 2.0)[(F + off) % 2], F * 100 + d + off if seed is None else seed)
    t = {k: (deep_dev(v, device) if k not in ("tau", "off") else v) for k, v in case.items()}
    return case, t


def _args(t, F, d):
    return [t["xbuf"], F, d, t["gates"], t["cross_kernels"], t["cross_biases"], t["dnn_kernels"], t["dnn_biases"]]


def _kw(t, bridge_type, par, act):
    return dict(bridge_type=bridge_type, parameterization=par, tau=t["tau"], activation=act, bridge_weights=t["bridge_weights"],
                bridge_activation=act, x_offset=t["off"], head_w=t["head"])


def _flat_tensors(t):
    out = [t["xbuf"], t["head"]] + t["gates"] + t["cross_kernels"] + t["cross_biases"] + t["dnn_kernels"] + t["dnn_biases"]
    if t["bridge_weights"] is not None:
        out += [w for bw in t["bridge_weights"] for w in bw]
    return out


def _nan_like(ws):
    return [torch.full(tuple(w.shape), float("nan"), device=w.device) for w in ws]


def _result(res):
    names = ("dx", "d_gates", "d_cross_w", "d_cross_b", "d_dnn_w", "d_dnn_b", "d_bridge_w", "d_bridge_b", "d_head_w")
    return {n: v for n, v in zip(names, res)}


def _np(v):
    if v is None:
        return None
    if isinstance(v, dict):
        return {k: _np(e) for k, e in v.items()}
    if isinstance(v, (list, tuple)):
        return [_np(e) for e in v]
    return v.cpu().numpy()


def _compare(got, ref, mag, what):
    """Every output the oracle has against the op's; returns the worst err / bar."""
    worst = 0.0
    fg, fr, fm = RB.flatten(got), RB.flatten(ref), RB.flatten(mag)
    assert [n for n, _ in fg] == [n for n, _ in fr], what
    for (n, a), (_, r), (_, m) in zip(fg, fr, fm):
        assert a.shape == r.shape, (what, n)
        err = np.abs(a.astype(np.float64) - r)
        worst = max(worst, float((err / (BAR["rtol"] * np.abs(r) + BAR["rtol_terms"] * m + 1e-30)).max()))
        assert_close_terms(a, r, m, what="%s, %s" % (n, what), **BAR)
    return worst


@pytest.mark.parametrize("par", ["vector", "matrix"])
@pytest.mark.parametrize("bridge_type", RB.BRIDGES_BWD)
def test_train_forward_has_the_forward_bits_and_the_tape(device, bridge_type, par):
    from deepctr_amd import ops
    for (F, d, L, B) in RB.SWEEP_BWD:
        for off, act in ((3, "relu"), (4, "linear")):
            D = F * d
            case, t = _operands(device, F, d, L, B, bridge_type, par, off)
            what = "F=%d d=%d L=%d B=%d %s %s off=%d %s" % (F, d, L, B, bridge_type, par, off, act)
            kw = _kw(t, bridge_type, par, act)
            logit0, out0 = ops.edcn(*_args(t, F, d), logit=True, out=True, **kw)
            obuf = torch.full((B, 3 * D + 9), float("nan"), device=device)
            logit, out, tape = ops.edcn_train(*_args(t, F, d), logit=True, out=obuf, out_offset=2, **kw)
            assert out is obuf and tuple(tape.shape) == (L, B, 3 * D)
            assert torch.equal(logit, logit0), what
            assert torch.equal(obuf[:, 2:2 + 3 * D], out0) and torch.isnan(obuf[:, :2]).all() and torch.isnan(obuf[:, 2 + 3 * D:]).all(), what
            assert torch.equal(tape[L - 1], out0), what
            ref = RB.tower_tape(case, F, d, bridge_type, par, act, act)
            mag = np.stack([RE.tower_op(case["xbuf"], F, d, case["gates"][:2 * i + 2], case["cross_kernels"][:i + 1], case["cross_biases"][:i + 1],
                                        case["dnn_kernels"][:i + 1], case["dnn_biases"][:i + 1], bridge_type=bridge_type, parameterization=par,
                                        tau=case["tau"], activation=act, bridge_activation=act, x_offset=off, absolute=True,
                                        bridge_weights=None if case["bridge_weights"] is None else case["bridge_weights"][:i + 1])[1]
                            for i in range(L)])
            assert_close_terms(tape.cpu().numpy(), ref, mag, what="tape, " + what, **FWD_BAR)
            # the tape alone (no out), into the caller's tensor
            mine = torch.full((L, B, 3 * D), float("nan"), device=device)
            l2, none, tp2 = ops.edcn_train(*_args(t, F, d), tape=mine, **kw)
            assert none is None and tp2 is mine and torch.equal(mine, tape) and torch.equal(l2, logit0)


@pytest.mark.parametrize("shape", RB.SWEEP_BWD, ids=lambda s: "F%d_d%d_L%d_B%d" % s)
@pytest.mark.parametrize("par", ["vector", "matrix"])
@pytest.mark.parametrize("bridge_type", RB.BRIDGES_BWD)
def test_backward_matches_the_float64_oracle(device, bridge_type, par, shape):
    """Every output against the oracle on the device's own tape, offsets {3, 4} x relu / linear; worst err / bar per row of SWEEP_BWD
    over the bridges and parameterizations (printed by this test; MI355X):
        (1, 1, 1, 5)       0.003 - 0.012
        (2, 3, 2, 17)      0.015 - 0.037
        (3, 4, 1, 65)      0.012 - 0.031
        (9, 4, 3, 33)      0.016 - 0.064
        (5, 17, 2, 40)     0.024 - 0.054
        (26, 16, 2, 130)   0.053 - 0.101
        (39, 16, 4, 20)    0.032 - 0.071"""
    from deepctr_amd import ops
    F, d, L, B = shape
    D = F * d
    concat = bridge_type == "concatenation"
    worst = 0.0
    for off in (3, 4):
        for act in ("relu", "linear"):
            case, t = _operands(device, F, d, L, B, bridge_type, par, off)
            what = "F=%d d=%d L=%d B=%d %s %s off=%d %s" % (F, d, L, B, bridge_type, par, off, act)
            kw = _kw(t, bridge_type, par, act)
            _, _, tape = ops.edcn_train(*_args(t, F, d), logit=True, **kw)
            tape_np = tape.cpu().numpy()
            dl_np, do_np = RB.seeds(case, F, d, off)
            dl, do = dev(dl_np, device), dev(do_np, device)
            before = [x.clone() for x in _flat_tensors(t) + [tape, dl, do]]
            dxbuf = torch.full((B, off + D + 7), float("nan"), device=device)
            outs = dict(d_gates=_nan_like(t["gates"]), d_cross_w=_nan_like(t["cross_kernels"]), d_cross_b=_nan_like(t["cross_biases"]),
                        d_dnn_w=_nan_like(t["dnn_kernels"]), d_dnn_b=_nan_like(t["dnn_biases"]),
                        d_head_w=torch.full((3 * D, 1), float("nan"), device=device))
            if concat:
                outs["d_bridge_w"] = _nan_like([bw[0] for bw in t["bridge_weights"]])
                outs["d_bridge_b"] = _nan_like([bw[1] for bw in t["bridge_weights"]])
            res = _result(ops.edcn_bwd(*_args(t, F, d), tape, d_logit=dl, d_out=do, dx=dxbuf, dx_offset=off, **dict(kw, **outs)))
            assert res["dx"] is dxbuf and torch.isnan(dxbuf[:, :off]).all() and torch.isnan(dxbuf[:, off + D:]).all(), what
            for a, b in zip(before, _flat_tensors(t) + [tape, dl, do]):
                assert torch.equal(a, b), "an input changed, " + what
            got = _np(dict(res, dx=dxbuf[:, off:off + D]))
            okw = dict(d_logit=dl_np, d_out=do_np)
            ref = RB.oracle(case, F, d, tape_np, bridge_type, par, act, act, **okw)
            mag = RB.oracle(case, F, d, tape_np, bridge_type, par, act, act, absolute=True, **okw)
            worst = max(worst, _compare(got, ref, mag, what))
            # accumulate adds to dx; outputs that are not asked for are skipped and the others keep their bits
            acc = torch.ones(B, off + D + 7, device=device)
            part = _result(ops.edcn_bwd(*_args(t, F, d), tape, d_logit=dl, d_out=do, dx=acc, dx_offset=off, accumulate=True,
                                        d_dnn_w=[None] * (L - 1) + [torch.full((D, D), float("nan"), device=device)],
                                        d_gates=True, **kw))
            assert torch.equal(acc[:, off:off + D], 1.0 + dxbuf[:, off:off + D]) and (acc[:, :off] == 1).all() and (acc[:, off + D:] == 1).all()
            assert part["d_cross_w"] is None and part["d_cross_b"] is None and part["d_dnn_b"] is None and part["d_head_w"] is None
            assert part["d_dnn_w"][:L - 1] == [None] * (L - 1) and torch.equal(part["d_dnn_w"][L - 1], res["d_dnn_w"][L - 1]), what
            assert all(torch.equal(a, b) for a, b in zip(part["d_gates"], res["d_gates"])), what
            # one seed at a time
            if off == 3:
                for only in (dict(d_logit=dl), dict(d_out=do)):
                    r1 = _result(ops.edcn_bwd(*_args(t, F, d), tape, dx=True, d_gates=True, d_cross_w=True, d_cross_b=True, d_dnn_w=True,
                                              d_dnn_b=True, d_bridge_w=concat, d_bridge_b=concat, d_head_w="d_logit" in only,
                                              **dict(kw, **only)))
                    o1 = {k: _np(v) for k, v in only.items()}
                    ref1 = RB.oracle(case, F, d, tape_np, bridge_type, par, act, act, **o1)
                    mag1 = RB.oracle(case, F, d, tape_np, bridge_type, par, act, act, absolute=True, **o1)
                    worst = max(worst, _compare(_np(r1), ref1, mag1, what + " " + "/".join(only)))
    WORST[(shape, bridge_type, par)] = worst
    print("edcn_bwd %s %s %s: worst err / bar %.3f" % (shape, bridge_type, par, worst))


@pytest.mark.parametrize("shape", [(9, 4, 3, 33), (26, 16, 2, 130)], ids=lambda s: "F%d_d%d_L%d_B%d" % s)
def test_slice_counts(device, shape):
    """Slice counts (0, 1, 3, 64, 3): all inside the bar; equal counts give equal bits; only the [D, D] / [2D, D] weight gradients depend
    on the count; two calls on the same operands give the same bits."""
    from deepctr_amd import ops
    F, d, L, B = shape
    bridge_type, par, act = "concatenation", "matrix", "relu"
    case, t = _operands(device, F, d, L, B, bridge_type, par, 4)
    kw = _kw(t, bridge_type, par, act)
    _, _, tape = ops.edcn_train(*_args(t, F, d), logit=True, **kw)
    dl_np, do_np = RB.seeds(case, F, d)
    dl, do = dev(dl_np, device), dev(do_np, device)
    ref = RB.oracle(case, F, d, tape.cpu().numpy(), bridge_type, par, act, act, d_logit=dl_np, d_out=do_np)
    mag = RB.oracle(case, F, d, tape.cpu().numpy(), bridge_type, par, act, act, d_logit=dl_np, d_out=do_np, absolute=True)
    runs = []
    for S in (0, 1, 3, 64, 3, 0):
        res = _result(ops.edcn_bwd(*_args(t, F, d), tape, d_logit=dl, d_out=do, dx=True, d_gates=True, d_cross_w=True, d_cross_b=True,
                                   d_dnn_w=True, d_dnn_b=True, d_bridge_w=True, d_bridge_b=True, d_head_w=True, slices=S, **kw))
        _compare(_np(res), ref, mag, "slices=%d %s" % (S, shape))
        runs.append(dict(RB.flatten(_np(res))))
    sliced = ("d_cross_w", "d_dnn_w", "d_bridge_w")
    for n in runs[0]:
        assert np.array_equal(runs[2][n], runs[4][n]) and np.array_equal(runs[0][n], runs[5][n]), n
        if not n.startswith(sliced):
            assert all(np.array_equal(runs[0][n], r[n]) for r in runs), n
    assert any(not np.array_equal(runs[1][n], runs[3][n]) for n in runs[0] if n.startswith(sliced))      # (the count does reach the sums)


@pytest.mark.parametrize("shape", [(9, 4, 3, 33), (26, 16, 2, 130)], ids=lambda s: "F%d_d%d_L%d_B%d" % s)
@pytest.mark.parametrize("par", ["vector", "matrix"])
@pytest.mark.parametrize("bridge_type", RB.BRIDGES_BWD)
def test_function_against_torch_double_autograd(device, bridge_type, par, shape):
    """ops.EDCNTowerFunction under autograd against _EDCN._autograd_logit's expression in torch float64: the logit by the forward's bar,
    every gradient by the backward's.  End to end the tape is an intermediate, not an operand: the terms are the oracle's magnitude mode
    over the magnitudes c / h / br were summed at (``tape_terms``), not over |tape| — the float32 forward's own error, which its bar
    allows, reaches the gradients through the tape (with |tape| as the terms the float32 NumPy oracle itself sits up to 25 x off)."""
    from deepctr_amd import ops
    F, d, L, B = shape
    D = F * d
    act = "relu"
    case, t = _operands(device, F, d, L, B, bridge_type, par, 0)
    dl_np, _ = RB.seeds(case, F, d)
    ref, tape64 = _autograd(case, F, d, bridge_type, par, act, act, dl_np, None)
    mag = RB.oracle(case, F, d, tape64, bridge_type, par, act, act, d_logit=dl_np, absolute=True,
                    tape_terms=RB.tower_tape(case, F, d, bridge_type, par, act, act, absolute=True))
    x = t["xbuf"][:, :D].reshape(B, F, d).clone().requires_grad_(True)
    head = t["head"].clone().requires_grad_(True)
    groups = [t["gates"], t["cross_kernels"], t["cross_biases"], t["dnn_kernels"], t["dnn_biases"]]
    if bridge_type == "concatenation":
        groups += [[bw[0] for bw in t["bridge_weights"]], [bw[1] for bw in t["bridge_weights"]]]
    leaves = [[w.clone().requires_grad_(True) for w in g] for g in groups]
    logit = ops.EDCNTowerFunction.apply(x, (bridge_type, par, case["tau"], act, act), head, *[w for g in leaves for w in g])
    ref_l, _ = ref_tower(case, F, d, bridge_type, par, act, extras=False)
    mag_l, _ = ref_tower(case, F, d, bridge_type, par, act, extras=False, absolute=True)
    what = "%s %s %s" % (shape, bridge_type, par)
    assert_close_terms(logit.detach().cpu().numpy(), ref_l, mag_l, what="logit, " + what, **FWD_BAR)
    (logit * dev(dl_np, device)).sum().backward()
    names = ("d_gates", "d_cross_w", "d_cross_b", "d_dnn_w", "d_dnn_b", "d_bridge_w", "d_bridge_b")
    got = dict(dx=x.grad.reshape(B, D).cpu().numpy(), d_head_w=head.grad.cpu().numpy())
    for n, g in zip(names, leaves):
        got[n] = [w.grad.cpu().numpy() for w in g]
    _compare(got, ref, mag, "function, " + what)
    # only what needs a gradient is formed
    x2 = t["xbuf"][:, :D].reshape(B, F, d).clone().requires_grad_(True)
    logit2 = ops.EDCNTowerFunction.apply(x2, (bridge_type, par, case["tau"], act, act), t["head"], *[w for g in groups for w in g])
    assert torch.equal(logit2, logit)
    (logit2 * dev(dl_np, device)).sum().backward()
    assert torch.equal(x2.grad, x.grad)


def _spy(monkeypatch):
    from deepctr_amd import ops
    seen = []
    real = ops.edcn_bwd
    monkeypatch.setattr(ops, "edcn_bwd", lambda *a, **k: (seen.append(1), real(*a, **k))[1])
    return seen


def _model_grads(model, feed, rows):
    """One batch through the autograd step's forward: the gradient of sum(logit) for every float weight."""
    from deepctr_amd import engine, training
    staged = engine.Staged(rows)
    params = [(k, t) for k, t in model.named_weights() if t.is_floating_point()]
    model._stage_inputs(feed, staged)
    try:
        for _, t in params:
            t.requires_grad_(True)
        model._begin()
        training.model_logits(model, staged, 0, rows, training=True).sum().backward()
        return {k: (None if t.grad is None else t.grad.detach().cpu().numpy().copy()) for k, t in params}
    finally:
        for _, t in params:
            t.requires_grad_(False)
            t.grad = None


@pytest.mark.parametrize("par", ["vector", "matrix"])
@pytest.mark.parametrize("bridge_type", RB.BRIDGES_BWD)
def test_model_gradients_with_the_switch_on_against_off(device, bridge_type, par, monkeypatch):
    """6 fields x 8, 256 rows, one batch: the gradient of every weight, embeddings included, with HIP_AUTOGRAD_OPS on against off; one
    ops.edcn_bwd call per step with the switch on and none with it off.  The bar: both sides are float32 sums over at most 256 rows x 48
    columns, each within ~1e-6 of the magnitude it was summed at; with the cancellation of these sums below a hundredfold, 1e-4 of the
    tensor's largest gradient (the north star's fraction) bounds their difference."""
    from deepctr_amd import training, training_hip
    from deepctr_amd.models import EDCN
    rng = np.random.RandomState(4)
    cols = _cols(6, 8)
    feed = _feed(rng, cols, 256)
    monkeypatch.setattr(training, "EDCN_HIP_MIN_ROWS", 0)
    seen = _spy(monkeypatch)
    model = EDCN(cols, cols, cross_num=2, cross_parameterization=par, bridge_type=bridge_type, tau=0.5, seed=3, device=device)
    assert not training_hip.supported(model)
    grads = {}
    for on in (True, False):
        monkeypatch.setattr(training, "HIP_AUTOGRAD_OPS", on)
        del seen[:]
        grads[on] = _model_grads(model, feed, 256)
        assert len(seen) == (1 if on else 0)
    assert sorted(grads[True]) == sorted(grads[False])
    checked = 0
    for k in sorted(grads[False]):
        a, b = grads[True][k], grads[False][k]
        assert (a is None) == (b is None), k
        if b is None:
            continue
        err = np.abs(a.astype(np.float64) - b)
        assert (err <= 1e-4 * np.abs(b).max() + 1e-30).all(), "%s: %.3g of the largest gradient" % (k, err.max() / (np.abs(b).max() + 1e-30))
        checked += np.abs(b).max() > 0
    assert checked >= 6 + 2 * 4 + 4          # the embeddings, the gates, and the tower's kernels at least


@pytest.mark.parametrize("kw", [dict(dnn_use_bn=True), dict(bridge_type="attention_pooling"), dict(dnn_dropout=0.5),
                                dict(dnn_activation="sigmoid")], ids=["bn", "attention_pooling", "dropout", "sigmoid"])
def test_what_the_backward_refuses_keeps_the_torch_ops(device, kw, monkeypatch):
    from deepctr_amd import training
    from deepctr_amd.models import EDCN
    rng = np.random.RandomState(5)
    cols = _cols(6, 8)
    feed = _feed(rng, cols, 64)
    monkeypatch.setattr(training, "EDCN_HIP_MIN_ROWS", 0)
    seen = _spy(monkeypatch)
    model = EDCN(cols, cols, cross_num=2, device=device, **kw)
    g = _model_grads(model, feed, 64)
    assert not seen and any(v is not None and np.abs(v).max() > 0 for v in g.values())
    x = torch.zeros(64, 6, 8, device=device)
    assert not training._edcn_on_hip(model, x, True)
    plain = EDCN(cols, cols, cross_num=2, device=device)
    assert training._edcn_on_hip(plain, x, True) and not training._edcn_on_hip(plain, x.double(), True)
    with torch.no_grad():
        assert not training._edcn_on_hip(plain, x, True)
    monkeypatch.setattr(training, "EDCN_HIP_MIN_ROWS", 65)
    assert not training._edcn_on_hip(plain, x, True)
    monkeypatch.setattr(training, "EDCN_HIP_MIN_ROWS", 64)
    assert training._edcn_on_hip(plain, x, True)
    monkeypatch.setattr(training, "EDCN_HIP_MAX_ROWS", 63)
    assert not training._edcn_on_hip(plain, x, True)


def test_fit_trains_through_the_op(device, monkeypatch):
    from deepctr_amd import training
    from deepctr_amd.models import EDCN
    rng = np.random.RandomState(9)
    cols = _cols(6, 8)
    feed = _feed(rng, cols, 2048)
    y = ((feed["C0"] % 2) ^ (feed["C1"] % 3 == 0)).astype(np.float32)          # planted signal
    monkeypatch.setattr(training, "EDCN_HIP_MIN_ROWS", 0)
    seen = _spy(monkeypatch)
    model = EDCN(cols, cols, cross_num=2, bridge_type="concatenation", tau=0.5, device=device)
    gates0 = [r.g.clone() for r in model.regulations]
    dense0 = model.bridges[0].dense.w("kernel").clone()
    model.compile("adam", "binary_crossentropy")
    hist = model.fit(feed, y, batch_size=256, epochs=2, verbose=0)
    assert len(seen) == 16                                                      # one call a step
    assert hist.history["loss"][1] < hist.history["loss"][0]
    assert all(not torch.equal(r.g, g0) for r, g0 in zip(model.regulations, gates0))       # the field weights trained
    assert not torch.equal(model.bridges[0].dense.w("kernel"), dense0)                     # and the bridge's Dense
