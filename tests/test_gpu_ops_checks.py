"""GPU: the operand checks of the seven wrappers that fill an args struct (interacting, senet_bilinear, fieldpair, ffm, ifm, fieldwise,
fieldwise_bwd) at the smallest shapes that exercise their stride arithmetic: B = 5 (a ragged tile) and B = 1 (the single-row pitch),
F = 3, E = 4, and F = 2 for fieldpair (one pair: ``pairs`` is a single column).  An input read in place and an output view at an offset
give the bits of the contiguous call and leave the other columns alone; one valid call per wrapper against its float64 oracle; every
malformed operand raises before anything is launched; a caller's workspace is taken at exactly the bytes asked for."""
import numpy as np
import pytest
import torch

from tests import ref_flen as RL
from tests import ref_ifm as RI
from tests import ref_onn as RO
from tests.test_gpu_flen import _case as flen_case, _normalised, _torch_fieldwise
from tests.test_gpu_ifm import _case as ifm_case
from tests.test_gpu_onn import _case as onn_case
from tests.util import assert_close_terms

pytestmark = pytest.mark.gpu

F, E, PAD = 3, 4, 7
D_ATT, HEADS = 2, 2
NAN = float("nan")


def _t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)


def _nan(device, *shape):
    return torch.full(shape, NAN, device=device)


def _x(rng, B, fields, device, offset=0):
    """([B, fields, E] values, the same values from column ``offset`` of a [B, fields*E + 7] buffer of other numbers)."""
    x = (rng.standard_normal((B, fields, E)) * 0.5).astype(np.float32)
    buf = rng.standard_normal((B, fields * E + PAD)).astype(np.float32)
    buf[:, offset:offset + fields * E] = x.reshape(B, -1)
    return _t(x, device), _t(buf, device)


def _bad_rows(t, cols):
    """A valid 2-D operand that has to hold ``cols`` columns, gone wrong in each way the check knows."""
    bad = [t.double(), t[:t.shape[0] - 1], t[:, :cols - 1]]
    if cols > 1:
        bad.append(torch.zeros(t.shape[0], 2 * t.shape[1], device=t.device)[:, ::2])             # column stride 2
    return bad


def _bad_vec(t):
    n = t.numel()
    bad = [t.double(), torch.zeros(n - 1, device=t.device)]
    if n > 1:
        bad.append(torch.zeros(2 * n, device=t.device)[::2])
    return bad


def _refused(device, call, kw, bad, outs):
    """Every (overrides, exception class) of ``bad`` raises, and after a synchronize no output has lost its NaN sentinel."""
    assert bad
    for over, exc in bad:
        with pytest.raises(exc):
            call(**dict(kw, **over))
    torch.cuda.synchronize(device)
    for o in outs:
        assert torch.isnan(o).all()


def _interacting_weights(rng, device, n_layers=1):
    dH = D_ATT * HEADS
    return [[_t(rng.standard_normal((E if l == 0 else dH, dH)) * 0.3, device) for _ in range(4)] for l in range(n_layers)]


@pytest.mark.parametrize("B", [1, 5])
def test_interacting_in_place(device, B):
    from deepctr_amd import ops
    rng = np.random.RandomState(B)
    x, buf = _x(rng, B, F, device)
    weights = _interacting_weights(rng, device)
    W = F * D_ATT * HEADS
    ref = ops.interacting(x, weights, D_ATT, HEADS, True, True)
    assert tuple(ref.shape) == (B, W) and torch.isfinite(ref).all()
    wide = _nan(device, B, W + 5)
    kw = dict(x=buf, weights=weights, att_embedding_size=D_ATT, head_num=HEADS, use_res=True, scaling=True, fields=F, dim=E, out=wide[:, 2:])
    bad = [(dict(x=b), ValueError) for b in _bad_rows(buf, F * E)] + [(dict(out=b), ValueError) for b in _bad_rows(_nan(device, B, W), W)]
    _refused(device, ops.interacting, kw, bad, [wide])
    assert ops.interacting(**kw) is kw["out"]
    assert torch.equal(wide[:, 2:2 + W], ref) and torch.isnan(wide[:, :2]).all() and torch.isnan(wide[:, 2 + W:]).all()


@pytest.mark.parametrize("B", [1, 5])
def test_senet_bilinear_in_place(device, B):
    from deepctr_amd import ops
    rng = np.random.RandomState(10 + B)
    x, buf = _x(rng, B, F, device)
    P = F * (F - 1) // 2
    mats = lambda: [_t(rng.standard_normal((E, E)) * 0.3, device) for _ in range(P)]       # noqa: E731
    w = dict(senet_w=(_t(rng.standard_normal((F, 2)), device), _t(rng.standard_normal((2, F)), device)), senet_bilinear_w=mats(),
             bilinear_w=mats(), bilinear_type="interaction")
    W = 2 * P * E
    ref = ops.senet_bilinear(x, **w)
    assert tuple(ref.shape) == (B, W) and torch.isfinite(ref).all()
    wide = _nan(device, B, W + 5)
    kw = dict(w, x=buf, fields=F, dim=E, out=wide[:, 2:])
    bad = [(dict(x=b), ValueError) for b in _bad_rows(buf, F * E)] + [(dict(out=b), ValueError) for b in _bad_rows(_nan(device, B, W), W)]
    _refused(device, ops.senet_bilinear, kw, bad, [wide])
    assert ops.senet_bilinear(**kw) is kw["out"]
    assert torch.equal(wide[:, 2:2 + W], ref) and torch.isnan(wide[:, :2]).all() and torch.isnan(wide[:, 2 + W:]).all()


@pytest.mark.parametrize("kind", ["fefm", "fwfm"])
@pytest.mark.parametrize("fields", [2, 3])
@pytest.mark.parametrize("B", [1, 5])
def test_fieldpair_in_place(device, B, fields, kind):
    from deepctr_amd import ops
    rng = np.random.RandomState(100 * B + fields)
    x, buf = _x(rng, B, fields, device, offset=3)
    P = fields * (fields - 1) // 2
    add = _t(rng.standard_normal(B), device)
    if kind == "fefm":
        weights = [_t(rng.standard_normal((E, E)) * 0.3, device) for _ in range(P)]
        ref_pairs, ref_logit = ops.fieldpair(x, weights, "fefm", pairs=True, logit=True, add=add)
        assert tuple(ref_pairs.shape) == (B, P) and torch.isfinite(ref_pairs).all()
    else:
        weights = _t(rng.standard_normal((fields, fields)), device)
        ref_pairs, ref_logit = ops.fieldpair(x, weights, "fwfm", add=add)
        assert ref_pairs is None
    assert tuple(ref_logit.shape) == (B,) and torch.isfinite(ref_logit).all()
    wide, logit = _nan(device, B, P + 5), _nan(device, B)
    kw = dict(x=buf, weights=weights, kind=kind, fields=fields, dim=E, x_offset=3, logit=logit, add=add)
    bad = [(dict(x=b), ValueError) for b in _bad_rows(buf, 3 + fields * E)] + [(dict(x_offset=-1), ValueError), (dict(x_offset=PAD + 1), ValueError)]
    bad += [(dict(logit=b), ValueError) for b in _bad_vec(logit)]
    bad += [(dict(add=add.double()), TypeError), (dict(add=torch.zeros(B + 1, device=device)), ValueError)]
    if kind == "fefm":
        kw.update(pairs=wide, pairs_offset=2)
        bad += [(dict(pairs=b), ValueError) for b in _bad_rows(_nan(device, B, P + 2), P + 2)] + [(dict(pairs_offset=-1), ValueError)]
    _refused(device, ops.fieldpair, kw, bad, [wide, logit])
    ops.fieldpair(**kw)
    assert torch.equal(logit, ref_logit)
    if kind == "fefm":
        assert torch.equal(wide[:, 2:2 + P], ref_pairs) and torch.isnan(wide[:, :2]).all() and torch.isnan(wide[:, 2 + P:]).all()
    if kind == "fefm" and P == 1:
        col = _nan(device, 1, B).t()                    # one column: [B, 1] with strides (1, B), rows one float apart
        ops.fieldpair(**dict(kw, pairs=col, pairs_offset=0))
        assert torch.equal(col, ref_pairs)


@pytest.mark.parametrize("B", [1, 5])
def test_ffm_valid_call_and_malformed_operands(device, B):
    from deepctr_amd import ops
    nd, off = 2, 3
    dev_kw, ref_kw, rng = onn_case(device, F, E, B, 7 + B, True, nd, False, off, True)
    W = F * (F - 1) // 2 * E
    scale, shift = (1.0 + 0.2 * rng.standard_normal(W)).astype(np.float32), (0.1 * rng.standard_normal(W)).astype(np.float32)
    ref = RO.ffm_pairs(scale=scale, shift=shift, **ref_kw)
    terms = RO.ffm_pairs(scale=scale, shift=shift, absolute=True, **ref_kw)
    stride = (off + W + nd + 7 + 3) // 4 * 4
    outbuf = _nan(device, B, stride)
    kw = dict(dev_kw, scale=_t(scale, device), shift=_t(shift, device), out=outbuf, out_offset=off)
    valid = _nan(device, B, off + W + nd)
    bad = [(dict(out=b), ValueError) for b in _bad_rows(valid, off + W + nd)] + [(dict(out_offset=-1), ValueError)]
    bad += [(dict(dense=b), ValueError) for b in _bad_rows(dev_kw["dense"][:, :nd], nd)]
    bad += [(dict(scale=kw["scale"].double()), TypeError), (dict(scale=kw["scale"][:W - 1]), ValueError), (dict(shift=None), ValueError)]
    _refused(device, ops.ffm, kw, bad, [outbuf])
    assert ops.ffm(**kw) is outbuf
    blk = outbuf[:, off:off + W + nd].cpu().numpy()
    assert torch.isnan(outbuf[:, :off]).all() and torch.isnan(outbuf[:, off + W + nd:]).all()
    assert_close_terms(blk, ref, terms, what="ffm B=%d" % B)
    assert np.array_equal(blk[:, W:], ref_kw["dense"])


def _ifm_operands(device, B):
    dev_kw, ref_kw = ifm_case(device, F, E, B, (5,), True, True, False, (1,), 3, 1, 40 + B)
    return dev_kw, {k: v for k, v in ref_kw.items() if not k.startswith("_")}


@pytest.mark.parametrize("B", [1, 5])
def test_ifm_valid_call_and_malformed_operands(device, B):
    from deepctr_amd import ops
    dev_kw, ref_kw = _ifm_operands(device, B)
    ref, m = RI.ifm_op(**ref_kw)
    terms, m_terms = RI.ifm_op(absolute=True, **ref_kw)
    out, fac = _nan(device, B), _nan(device, B, F + 3)
    kw = dict(dev_kw, out=out, factor_out=fac[:, :F + 1])
    act, kernel = dev_kw["sources"][0]
    bad = [(dict(x=b), ValueError) for b in _bad_rows(dev_kw["x"], F * E)]
    bad += [(dict(sources=[(b, kernel)]), ValueError) for b in _bad_rows(act, act.shape[1])[:2]]
    bad += [(dict(sources=[(torch.zeros(B, 2 * act.shape[1], device=device)[:, ::2], kernel)]), ValueError)]
    bad += [(dict(mprime=b), ValueError) for b in _bad_rows(dev_kw["mprime"], F)]
    bad += [(dict(factor_out=b), ValueError) for b in _bad_rows(_nan(device, B, F), F)]
    bad += [(dict(out=b), ValueError) for b in _bad_vec(out)] + [(dict(add=[b]), ValueError) for b in _bad_vec(dev_kw["add"][0])]
    _refused(device, ops.ifm, kw, bad, [out, fac])
    assert ops.ifm(**kw) is out
    assert_close_terms(out.cpu().numpy(), ref, terms, what="ifm B=%d" % B)
    assert_close_terms(fac[:, :F].cpu().numpy(), m, m_terms, what="ifm B=%d factor_out" % B)
    assert torch.isnan(fac[:, F:]).all()


def _fieldwise_operands(device, B, off=3):
    groups, xbuf, w, head, add = flen_case(2, (1, 2), E, B, "packed", off, 60 + B)          # 1 + 2 = F fields in two groups
    return groups, xbuf, w, head, add, {k: _t(v, device) for k, v in w.items()}


@pytest.mark.parametrize("B", [1, 5])
def test_fieldwise_valid_call_and_malformed_operands(device, B):
    from deepctr_amd import ops
    off = 3
    groups, xbuf, w, head, add, wt = _fieldwise_operands(device, B)
    span = F * E
    ref_y, ref_l = RL.fieldwise_op(xbuf, groups, E, w["kernel_mf"], w["kernel_fm"], w["bias_mf"], w["bias_fm"], x_offset=off, head_w=head, add=add)
    mag_y, mag_l = RL.fieldwise_op(xbuf, groups, E, w["kernel_mf"], w["kernel_fm"], w["bias_mf"], w["bias_fm"], x_offset=off, head_w=head, add=add,
                                   absolute=True)
    xt, addt = _t(xbuf, device), _t(add, device)
    ybuf, logit = _nan(device, B, E + 9), _nan(device, B)
    kw = dict(x=xt, groups=groups, dim=E, x_offset=off, y=ybuf, y_offset=2, head_w=_t(head, device), add=addt, logit=logit, **wt)
    bad = [(dict(x=b), ValueError) for b in _bad_rows(xt, off + span)] + [(dict(x_offset=-1), ValueError), (dict(groups=[(-1, 1), (4, 2)]), ValueError)]
    bad += [(dict(y=b), ValueError) for b in _bad_rows(_nan(device, B, 2 + E), 2 + E)] + [(dict(y_offset=-1), ValueError)]
    bad += [(dict(logit=b), ValueError) for b in _bad_vec(logit)]
    bad += [(dict(add=addt.double()), TypeError), (dict(add=torch.zeros(B + 1, device=device)), ValueError), (dict(head_w=None), ValueError),
            (dict(kernel_mf=wt["kernel_mf"].double()), TypeError), (dict(groups=groups[:1]), ValueError)]
    _refused(device, ops.fieldwise, kw, bad, [ybuf, logit])
    y, lg = ops.fieldwise(**kw)
    assert y is ybuf and lg is logit
    assert torch.isnan(ybuf[:, :2]).all() and torch.isnan(ybuf[:, 2 + E:]).all()
    assert_close_terms(ybuf[:, 2:2 + E].cpu().numpy(), ref_y, mag_y, what="fieldwise y B=%d" % B)
    assert_close_terms(logit.cpu().numpy(), ref_l, mag_l, what="fieldwise logit B=%d" % B)


@pytest.mark.parametrize("form", ["dy", "dlogit"])
@pytest.mark.parametrize("B", [1, 5])
def test_fieldwise_bwd_valid_call_and_malformed_operands(device, B, form):
    """The oracle is float64 autograd over test_gpu_flen's torch form of the layer (itself held against ref_flen.fieldwise_op here), at
    the bar of test_gpu_flen.test_fieldwise_bwd_vs_autograd."""
    from deepctr_amd import ops
    off = 3
    groups, xbuf, w, head, _, wt = _fieldwise_operands(device, B)
    rng = np.random.RandomState(B)
    x64 = torch.from_numpy(xbuf).double().requires_grad_(True)
    leaves = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in w.items()}
    head64 = torch.from_numpy(head).double().requires_grad_(True)
    y = _torch_fieldwise(x64, groups, E, off, leaves["kernel_mf"].reshape(-1), leaves["kernel_fm"].reshape(-1), leaves["bias_mf"], leaves["bias_fm"])
    ref_y, _ = RL.fieldwise_op(xbuf, groups, E, w["kernel_mf"], w["kernel_fm"], w["bias_mf"], w["bias_fm"], x_offset=off)
    assert np.allclose(y.detach().numpy(), ref_y, rtol=1e-12, atol=1e-12)          # (two float64 sums of a dozen terms)
    names = ["kernel_mf", "kernel_fm", "bias_mf", "bias_fm"]
    wanted = [x64] + [leaves[k] for k in names]
    if form == "dy":
        dybuf = _t(rng.standard_normal((B, E + 3)), device)
        up = dict(dy=dybuf[:, 1:1 + E])
        loss = (y * up["dy"].cpu().double()).sum()
    else:
        dl = _t(rng.standard_normal(B), device)
        up = dict(dlogit=dl, head_w=_t(head, device))
        loss = ((y @ head64).reshape(-1) * dl.cpu().double()).sum()
        wanted.append(head64)
    grads = [g.numpy() for g in torch.autograd.grad(loss, wanted)]
    gmax = max(float(np.abs(g).max()) for g in grads)
    xt = _t(xbuf, device)
    dx = _nan(device, *xbuf.shape)
    outs = {"d_" + k: _nan(device, *w[k].shape) for k in names}
    if form == "dlogit":
        outs["d_head_w"] = _nan(device, E, 1)
    kw = dict(x=xt, groups=groups, dim=E, x_offset=off, dx=dx, dx_offset=off, **wt, **outs, **up)
    bad = [(dict(x=b), ValueError) for b in _bad_rows(xt, off + F * E)] + [(dict(dx=b), ValueError) for b in _bad_rows(dx, off + F * E)]
    bad += [(dict(dx_offset=-1), ValueError), (dict(dy=None, dlogit=None), ValueError)]
    if form == "dy":
        bad += [(dict(dy=b), ValueError) for b in _bad_rows(up["dy"], E)] + [(dict(d_head_w=torch.zeros(E, device=device)), ValueError)]
    else:
        bad += [(dict(dlogit=b), ValueError) for b in _bad_vec(dl)] + [(dict(head_w=b), ValueError) for b in _bad_vec(up["head_w"])]
        bad += [(dict(head_w=None), ValueError)]
    for name, t in outs.items():
        bad += [({name: b}, ValueError) for b in _bad_vec(t)]
    _refused(device, ops.fieldwise_bwd, kw, bad, [dx] + list(outs.values()))
    for t in outs.values():
        t.fill_(0.5)                                    # (the weight gradients are accumulated)
    ops.fieldwise_bwd(**kw)
    cols = np.zeros(xbuf.shape[1], dtype=bool)
    cols[off:off + F * E] = True
    got = dx.cpu().numpy()
    assert np.isnan(got[:, ~cols]).all() and np.isfinite(got[:, cols]).all()
    what = "fieldwise_bwd B=%d %s: " % (B, form)
    _normalised(got[:, cols], grads[0][:, cols], gmax, what + "dx")
    for name, gref in zip(names + ["head_w"], grads[1:]):
        _normalised((outs["d_" + name] - 0.5).cpu().numpy(), gref, gmax, what + "d " + name)


def _interacting_head_only(device, B, rng):
    from deepctr_amd import ops
    n_layers = 33               # (the head alone over a stack this deep keeps a layer's rows in the workspace)
    x, _ = _x(rng, B, F, device)
    kw = dict(x=x, weights=_interacting_weights(rng, device, n_layers), att_embedding_size=D_ATT, head_num=HEADS, use_res=True, scaling=True,
              head_w=_t(rng.standard_normal(F * D_ATT * HEADS), device))
    return ops.interacting, kw, ops.interacting_workspace_bytes(B, F, E, n_layers, D_ATT, HEADS, with_out=False)


def _ifm_workspace_route(device, B, rng):
    from deepctr_amd import ops
    dev_kw, _ = _ifm_operands(device, B)
    return ops.ifm, dict(dev_kw, route="workspace"), ops.ifm_workspace_bytes(B, F, E, 1, route="workspace")


def _senet_bilinear_small(device, B, rng):
    from deepctr_amd import ops
    return ops.senet_bilinear, None, max(ops.senet_bilinear_workspace_bytes(B, F, E, t, m, 2) for t in ("all", "each", "interaction")
                                         for m in (0, 1, 2))


def _fieldpair_small(device, B, rng):
    from deepctr_amd import ops
    return ops.fieldpair, None, max(ops.fieldpair_workspace_bytes(B, f, E, k) for f in (2, 3) for k in ("fefm", "fwfm"))


@pytest.mark.parametrize("case", [_interacting_head_only, _senet_bilinear_small, _fieldpair_small, _ifm_workspace_route])
def test_caller_workspace_at_exactly_the_bytes_asked_for(device, case):
    B = 5
    call, kw, need = case(device, B, np.random.RandomState(3))
    if not need:
        pytest.skip("%s needs no workspace at B=%d, F=%d, E=%d: its workspace route starts at shapes far larger" % (call.__name__, B, F, E))
    assert need % 4 == 0
    ref = call(**kw)                                                         # the per-stream scratch
    with pytest.raises(ValueError, match=r">= %d bytes" % need):
        call(workspace=torch.zeros(need // 4 - 1, device=device), **kw)
    ws = _nan(device, need // 4)
    got = call(workspace=ws, **kw)
    assert torch.equal(got, ref) and torch.isfinite(got).all()
