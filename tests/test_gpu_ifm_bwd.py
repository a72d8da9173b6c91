"""GPU: dctr_ifm_bwd against the float64 oracle (tests/ref_ifm_bwd.py) over the sweep of shapes with softmax off and on, its batch
slices, its skipped outputs, ops.InputAwareFMFunction against the torch ops under autograd, and IFM's and DIFM's fit() with the switch on
against off.

Worst err / bar per sweep row under assert_close_terms' defaults (1e-4 of the result + 2e-6 of the summed magnitude), as printed by
test_op_vs_float64_oracle on an MI355X: between 0.0042 (F = 600, d = 2, softmax) and 0.030 (F = 16, d = 16, B = 129, softmax) over the
28 runs of the sweep; the Criteo-shaped rows 0.025 (IFM, B = 1001) and 0.023 (DIFM, K = 2,496 + 64).  The slices test's dkernel sits
at 0.01 of the bar for every slice count."""
import numpy as np
import pytest
import torch

from tests import ref_ifm_bwd as RB
from tests.test_gpu_ffm_bwd import _normalised
from tests.util import TERMS_REPORT, assert_close, assert_close_terms

pytestmark = pytest.mark.gpu


def _t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _operands(c, F, d, device):
    """The case on the device, every matrix a view narrower than its storage (row stride != width) where the case is padded."""
    pad = c["pad"]
    view = lambda a, w: _t(a, device)[:, :w + (pad and 1)]       # noqa: E731
    kw = dict(x=view(c["x"], F * d), fields=F, dim=d, factor=view(c["m"], F), d_out=_t(c["d_out"], device))
    kw["sources"] = [(_t(a, device)[:, :a.shape[1] - pad], _t(w, device)) for a, w in c["sources"]]
    if c["terms"] is not None:
        kw["terms"] = view(c["terms"], F)
    return kw


def _nan(rows, cols, pad, device):
    buf = torch.full((rows, cols + pad), float("nan"), device=device)
    return buf, buf[:, :cols + (pad and 1)]


def _outputs(c, F, d, B, Ks, device, dmprime=True, dterms=True):
    """NaN-filled buffers of every output: (dict name -> full buffer (or list), kwargs of ops.ifm_bwd)."""
    pad = c["pad"]
    full, kw = {}, {}
    for name, cols, want in (("dx", F * d, True), ("dterms", F, dterms), ("dmprime", F, dmprime)):
        if want:
            full[name], kw[name] = _nan(B, cols, pad, device)
    acts = [_nan(B, K, pad, device) for K in Ks]
    kers = [_nan(K, F, pad, device) for K in Ks]
    full["dact"], kw["dact"] = [a[0] for a in acts], [a[1] for a in acts]
    full["dkernel"], kw["dkernel"] = [k[0] for k in kers], [k[1] for k in kers]
    return full, kw


def _compare(full, ref, mag, widths, what, names):
    """Every wanted element finite and inside the bar, every padding column still NaN.  Returns the worst err / bar."""
    worst = 0.0
    for name in names:
        bufs = full[name] if isinstance(full[name], list) else [full[name]]
        refs = ref[name] if isinstance(ref[name], list) else [ref[name]]
        mags = mag[name] if isinstance(mag[name], list) else [mag[name]]
        for s, (buf, r, t) in enumerate(zip(bufs, refs, mags)):
            w = widths[name][s] if isinstance(widths[name], list) else widths[name]
            got = buf[:, :w].cpu().numpy()
            assert np.isfinite(got).all(), "%s %s[%d]: not finite" % (what, name, s)
            assert torch.isnan(buf[:, w:]).all(), "%s %s[%d]: written behind its width" % (what, name, s)
            n0 = len(TERMS_REPORT)
            assert_close_terms(got, r.reshape(got.shape), t.reshape(got.shape), what="%s %s[%d]" % (what, name, s))
            worst = max(worst, TERMS_REPORT[n0][4])
    return worst


@pytest.mark.parametrize("F,d,B,Ks,mprime,terms,pad", RB.SWEEP)
def test_op_vs_float64_oracle(device, F, d, B, Ks, mprime, terms, pad, capsys):
    from deepctr_amd import ops
    widths = dict(dx=F * d, dterms=F, dmprime=F, dact=list(Ks), dkernel=[F] * len(Ks))
    for softmax in (False, True):
        c = RB.case(F, d, B, Ks, mprime, terms, pad, softmax)
        ref, mag = RB.oracle(c, F, d, softmax), RB.oracle(c, F, d, softmax, absolute=True)
        kw = _operands(c, F, d, device)
        guard = {k: v.clone() for k, v in kw.items() if isinstance(v, torch.Tensor)}
        guard_s = [(a.clone(), w.clone()) for a, w in kw["sources"]]
        what = "ifm_bwd F=%d d=%d B=%d K=%s softmax=%d" % (F, d, B, Ks, softmax)
        names = ["dx"] + (["dterms"] if terms else []) + ["dact", "dkernel"]
        # dm' to dmprime where the forward was handed an m' (or has no source); else it waits in the workspace
        first = bool(mprime or not Ks)
        full, okw = _outputs(c, F, d, B, Ks, device, dmprime=first, dterms=terms)
        ops.ifm_bwd(softmax=softmax, **dict(kw, **okw))
        worst = _compare(full, ref, mag, widths, what, names + (["dmprime"] if first else []))
        if not first:
            # the same call with dmprime asked for: dm' itself, and everything else the same bits
            full2, okw = _outputs(c, F, d, B, Ks, device, dmprime=True, dterms=terms)
            ops.ifm_bwd(softmax=softmax, **dict(kw, **okw))
            worst = max(worst, _compare(full2, ref, mag, widths, what + " (dmprime)", ["dmprime"]))
            for name in names:
                a, b = full[name], full2[name]
                for u, v in zip(a if isinstance(a, list) else [a], b if isinstance(b, list) else [b]):
                    assert torch.equal(torch.nan_to_num(u, nan=7.0), torch.nan_to_num(v, nan=7.0)), what + " " + name
        assert all(torch.equal(v, kw[k]) for k, v in guard.items())                     # the inputs are unchanged
        assert all(torch.equal(a, b[0]) and torch.equal(w, b[1]) for (a, w), b in zip(guard_s, kw["sources"]))
        with capsys.disabled():
            print("\n[ifm_bwd] F=%d d=%d B=%d K=%s softmax=%d: worst err / bar %.3g" % (F, d, B, Ks, softmax, worst))


def _bits(t):
    return torch.nan_to_num(t, nan=7.0)


@pytest.mark.parametrize("F,d,B,Ks", [(39, 4, 257, (2496, 64)), (5, 2, 64, (64,))])
def test_slices(device, F, d, B, Ks):
    """dkernel is summed over batch slices in a fixed order: inside the bar for every slice count, the same bits from call to call;
    nothing else depends on the slices."""
    from deepctr_amd import ops
    widths = dict(dx=F * d, dterms=F, dmprime=F, dact=list(Ks), dkernel=[F] * len(Ks))
    c = RB.case(F, d, B, Ks, False, True, 0, True)
    ref, mag = RB.oracle(c, F, d, True), RB.oracle(c, F, d, True, absolute=True)
    kw = _operands(c, F, d, device)
    runs = []
    for slices in (0, 1, 3, 64, 3):
        full, okw = _outputs(c, F, d, B, Ks, device)
        ops.ifm_bwd(softmax=True, slices=slices, **dict(kw, **okw))
        _compare(full, ref, mag, widths, "slices=%d" % slices, ["dkernel"])
        runs.append(full)
    for full in runs[1:]:
        for name in ("dx", "dterms", "dmprime"):
            assert torch.equal(_bits(full[name]), _bits(runs[0][name])), name
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(full["dact"], runs[0]["dact"]))
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(runs[2]["dkernel"], runs[4]["dkernel"]))      # slices = 3, twice
    full, okw = _outputs(c, F, d, B, Ks, device)
    ops.ifm_bwd(softmax=True, **dict(kw, **okw))
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(full["dkernel"], runs[0]["dkernel"]))         # the default, twice
    with pytest.raises(ValueError):
        ops.ifm_bwd(softmax=True, slices=257, **dict(kw, **okw))


def test_skipped_outputs(device):
    """A NULL output is not formed and the others do not change; a buffer that is not named is not touched."""
    from deepctr_amd import ops
    F, d, B, Ks = 13, 17, 40, (65, 130)
    c = RB.case(F, d, B, Ks, False, True, 7, False)
    kw = _operands(c, F, d, device)
    base, okw = _outputs(c, F, d, B, Ks, device, dmprime=False)
    ops.ifm_bwd(**dict(kw, **okw))
    for skip in ("dx", "dact", "dkernel"):
        full, okw = _outputs(c, F, d, B, Ks, device, dmprime=False)
        passed = dict(okw)
        passed[skip] = None if skip == "dx" else [None] * len(Ks)
        ops.ifm_bwd(**dict(kw, **passed))
        for name in ("dx", "dterms", "dact", "dkernel"):
            a, b = full[name], base[name]
            a, b = (a if isinstance(a, list) else [a]), (b if isinstance(b, list) else [b])
            if name == skip:
                assert all(torch.isnan(u).all() for u in a), skip                       # passed over: untouched
            else:
                assert all(torch.equal(_bits(u), _bits(v)) for u, v in zip(a, b)), (skip, name)
    # one source's pair alone
    full, okw = _outputs(c, F, d, B, Ks, device, dmprime=False)
    ops.ifm_bwd(**dict(kw, dx=None, dterms=None, dact=[None, okw["dact"][1]], dkernel=[okw["dkernel"][0], None]))
    assert torch.isnan(full["dx"]).all() and torch.isnan(full["dterms"]).all()
    assert torch.isnan(full["dact"][0]).all() and torch.isnan(full["dkernel"][1]).all()
    assert torch.equal(_bits(full["dact"][1]), _bits(base["dact"][1])) and torch.equal(_bits(full["dkernel"][0]), _bits(base["dkernel"][0]))


def _torch_logit(x, sources, softmax, terms):
    """InputAwareModel._autograd_logit's expression."""
    mp = sum(a @ w for a, w in sources)
    m = x.shape[1] * torch.softmax(mp, dim=1) if softmax else mp
    r = x * m.unsqueeze(-1)
    logit = 0.5 * (r.sum(1).pow(2) - (r * r).sum(1)).sum(-1)
    return logit if terms is None else logit + (terms * m).sum(-1)


@pytest.mark.parametrize("with_terms", [False, True])
@pytest.mark.parametrize("shape", ["ifm", "difm"])
def test_function_vs_torch_ops_under_autograd(device, shape, with_terms, monkeypatch):
    from deepctr_amd import ops, training
    B, F, d = 300, 6, 8
    Ks, softmax = ((16,), True) if shape == "ifm" else ((48, 16), False)
    rng = np.random.RandomState(3)
    x = _t((rng.standard_normal((B, F, d)) * 0.5).astype(np.float32), device).requires_grad_(True)
    srcs = [(_t(rng.standard_normal((B, K)).astype(np.float32), device).requires_grad_(True),
             _t((rng.standard_normal((K, F)) / np.sqrt(K)).astype(np.float32), device).requires_grad_(True)) for K in Ks]
    terms = _t((rng.standard_normal((B, F)) * 0.3).astype(np.float32), device).requires_grad_(True) if with_terms else None
    srcs[0][0].requires_grad_(False)                      # the first source's activations: no gradient wanted
    g = _t(rng.standard_normal(B).astype(np.float32), device)
    leaves = [x] + ([terms] if with_terms else []) + [t for a, w in srcs for t in (a, w) if t.requires_grad]
    seen = []
    real = ops.ifm_bwd
    monkeypatch.setattr(ops, "ifm_bwd", lambda *a, **k: (seen.append((k, real(*a, **k))), seen[-1][1])[1])
    assert training._ifm_on_hip(x)
    got = training.input_aware_fm(x, srcs, softmax, terms=terms)
    ref = _torch_logit(x, srcs, softmax, terms)
    assert_close(got.detach().cpu().numpy(), ref.detach().cpu().numpy(), rtol=1e-4, atol=2e-5, what=shape + " forward")
    g_hip = torch.autograd.grad((got * g).sum(), leaves)
    g_ref = torch.autograd.grad((ref * g).sum(), leaves)
    assert len(seen) == 1
    k, ret = seen[0]
    assert k["dact"][0] is False and ret[3][0] is None                # requires_grad=False: not formed, None
    assert k["dmprime"] is False and ret[2] is None and (k["dterms"] is True) == with_terms
    gmax = max(float(t.abs().max()) for t in g_ref)
    for i, (a, b) in enumerate(zip(g_hip, g_ref)):
        assert a.shape == b.shape
        _normalised(a.cpu().numpy(), b.cpu().numpy(), gmax, "%s terms=%d: gradient %d" % (shape, with_terms, i))
    with torch.no_grad():
        assert not training._ifm_on_hip(x)
    monkeypatch.setattr(training, "HIP_AUTOGRAD_OPS", False)
    assert not training._ifm_on_hip(x)


def _small(rng, n, d=8):
    from deepctr_amd.feature_column import DenseFeat, SparseFeat, VarLenSparseFeat
    cols = [SparseFeat("C%d" % i, 50, d) for i in range(5)] + [VarLenSparseFeat(SparseFeat("S", 30, d), maxlen=4, combiner="mean"),
                                                                 DenseFeat("I0", 1)]
    feed = {"C%d" % i: rng.randint(0, 50, n).astype(np.int32) for i in range(5)}
    feed["S"] = rng.randint(0, 30, (n, 4)).astype(np.int32)
    feed["S"][:, 0] = np.maximum(feed["S"][:, 0], 1)
    feed["I0"] = rng.rand(n).astype(np.float32)
    return cols, feed


def _ctor(kind):
    from deepctr_amd import models
    return getattr(models, kind), (dict(att_embedding_size=4, att_head_num=2) if kind == "DIFM" else {})


def _count_calls(monkeypatch):
    from deepctr_amd import ops
    seen = []
    real = ops.ifm_bwd
    monkeypatch.setattr(ops, "ifm_bwd", lambda *a, **k: (seen.append(1), real(*a, **k))[1])
    return seen


@pytest.mark.parametrize("kind", ["IFM", "DIFM"])
def test_fit_with_the_switch_on_against_off(device, kind, monkeypatch):
    from deepctr_amd import training, training_hip
    rng = np.random.RandomState(9)
    n = 768
    cols, feed = _small(rng, n)
    y = ((feed["C0"] % 2) ^ (feed["C1"] % 3 == 0)).astype(np.float32)
    seen = _count_calls(monkeypatch)
    monkeypatch.setattr(training, kind + "_HIP_MIN_ROWS", 0)
    ctor, kw = _ctor(kind)
    ends, w0 = {}, None
    for on in (True, False):
        model = ctor(cols, cols, dnn_hidden_units=(32, 16), seed=5, device=device, **kw)        # a linear part of equal field count
        assert not training_hip.supported(model)
        if w0 is None:
            w0 = model.get_weights_by_name()
        else:
            model.set_weights_by_name(w0)
        monkeypatch.setattr(training, "HIP_AUTOGRAD_OPS", on)
        del seen[:]
        model.compile("adam", "binary_crossentropy")
        hist = model.fit(feed, y, batch_size=256, epochs=1, shuffle=False, verbose=0)          # three steps
        assert np.isfinite(hist.history["loss"]).all()
        assert len(seen) == (3 if on else 0)
        ends[on] = model.get_weights_by_name()
    gmax = max(float(np.abs(v).max()) for v in ends[False].values())
    moved = 0
    for k in sorted(w0):
        _normalised(ends[True][k], ends[False][k], gmax, "%s after three steps: %s" % (kind, k))
        moved += not np.array_equal(ends[True][k], w0[k])
    assert moved >= 12
    assert not np.array_equal(ends[True]["dense/kernel"], w0["dense/kernel"])
    assert not np.array_equal(ends[True]["linear0sparse_emb_C1/embeddings"], w0["linear0sparse_emb_C1/embeddings"])


def test_default_row_threshold(device, monkeypatch):
    """The gate follows training.IFM_HIP_MIN_ROWS (DIFM: DIFM_HIP_MIN_ROWS), whatever profiles/ifm_bwd.txt made the defaults: below it
    the torch ops run."""
    from deepctr_amd import engine, training
    for name in ("IFM_HIP_MIN_ROWS", "DIFM_HIP_MIN_ROWS"):
        assert isinstance(getattr(training, name), int) and getattr(training, name) >= 0
    rng = np.random.RandomState(6)
    cols, feed = _small(rng, 32)
    seen = _count_calls(monkeypatch)
    for kind in ("IFM", "DIFM"):
        staged = engine.Staged(32)
        ctor, kw = _ctor(kind)
        model = ctor(cols, cols, dnn_hidden_units=(8,), device=device, **kw)
        monkeypatch.setattr(training, kind + "_HIP_MIN_ROWS", 32)
        params = [t for k, t in model.named_weights() if k.startswith("sparse_emb_") or k.startswith("dense")]
        model._stage_inputs(feed, staged)
        try:
            for t in params:
                t.requires_grad_(True)
            for B, want in ((31, 0), (32, 1)):
                del seen[:]
                model._begin()
                training.model_logits(model, staged, 0, B, training=True).sum().backward()
                assert len(seen) == want, (kind, B, seen)
        finally:
            for t in params:
                t.requires_grad_(False)
                t.grad = None
    x = torch.zeros(40, 6, 8, device=device, requires_grad=True)
    for rows in (0, 40, 41, 1 << 40):
        assert training._ifm_on_hip(x, rows) is (rows <= 40)
