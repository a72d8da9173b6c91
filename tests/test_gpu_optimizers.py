"""GPU: dctr_opt_apply and dctr_grad_clip_scales (csrc/opt_kernels.hip) against the float64 oracle of tests/ref_optimizers.py, the
four old kinds on the new entry point bit for bit, and whole models compiled with optimizer objects on the HIP step against the
autograd step.

The error bar of the rule tests is measured: a case's float32 torch restatement (training.KerasOptimizer) has some largest error E
against the float64 oracle on the same inputs; the kernel — another float32 evaluation of the same formulas, differing in operation
order, fused multiply-adds and sqrt / pow rounding — may sit at most 4 E plus one float32 ulp of the weight from the oracle.
Measured on an MI355X (largest kernel error over E): 0.70 - 1.19 for every rule but Adam, whose 3.42 (clipvalue) / 4.00 / 4.40 (amsgrad)
come from `1 - beta_2` formed in float32, as dctr_adam_multi forms it.
The rule tests, the clip pre-pass and the in-launch l2 penalty also run on a second layout (_layout_l2) that puts l2 > 0 where real models
have it and _layout() does not: the touched table, the unaligned segment, the tail-only segments.  The penalty's bar is derived
(_penalty_bar), not measured.

The whole-model tests hold the HIP fit's UPDATES (w3 - w0) to the bars of tests/test_gpu_train_reg.py::_autograd_check against the
torch restatement fed the gradients the HIP step itself produced (_updates_match), the two fits' losses to tests/test_gpu_fit.py's bar and
their weights to _autograd_check's; the two fits' update distance is printed: it also carries the rounding of three dependent backward
passes (measured: up to 3.6e-4 of the largest update for DIN under Nesterov SGD)."""
import os
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_optimizers as RO  # noqa: E402

from tests.util import assert_close  # noqa: E402

pytestmark = pytest.mark.gpu

UPDATES = 5
SIZES = (1, 3, 4, 5, 1023, 4096 + 7)          # + one more 1,023 off the 16-byte grid, one 4,103 with l2 > 0, one [64, 8] table
TABLE = (64, 8)


def _layout():
    """(n, l2, kind) per segment: "plain", "offset" (every buffer 4 bytes past a 16-byte boundary), "table" (touched bytes)."""
    return [(n, 0.0, "plain") for n in SIZES] + [(1023, 0.0, "offset"), (4096 + 7, 0.01, "plain"), (TABLE[0] * TABLE[1], 0.0, "table")]


def _layout_l2():
    """_layout()'s segments with l2 > 0 on every route a regulariser can take: the touched table (every embedding table of a real model),
    the offset segment (element by element), the segments of 1, 3 and 5 elements (tail loop only) and one plain 4,103; three segments
    stay at l2 = 0.  One value per segment, so that a swapped l2 shows."""
    l2 = {1: 0.02, 3: 0.03, 4: 0.0, 5: 0.04, 1023: 0.0, 4096 + 7: 0.0}
    return [(n, l2[n], "plain") for n in SIZES] + [(1023, 0.05, "offset"), (4096 + 7, 0.01, "plain"), (TABLE[0] * TABLE[1], 0.025, "table")]


def _buf(n, kind, device, fill=0.0):
    if kind == "offset":
        return torch.full((n + 1,), fill, dtype=torch.float32, device=device)[1:]
    return torch.full((n,), fill, dtype=torch.float32, device=device)


class Segments(object):
    """The device side of one case: w / g / slots per segment, the touched map of the table, dctr_opt_seg_t array."""

    def __init__(self, device, ws, inits, lay=None):
        from deepctr_amd import ops
        self.lay = _layout() if lay is None else lay
        self.w = [_buf(n, k, device) for n, _, k in self.lay]
        self.g = [_buf(n, k, device) for n, _, k in self.lay]
        self.slots = [[_buf(n, k, device, v) for v in inits] for n, _, k in self.lay]
        for t, w in zip(self.w, ws):
            t.copy_(torch.from_numpy(w))
        assert self.w[6].data_ptr() % 16 == 4 and all(t.data_ptr() % 16 == 0 for i, t in enumerate(self.w) if i != 6)
        self.touched = torch.zeros(self.lay[-1][0] // 4, dtype=torch.uint8, device=device)
        self.segs, self.n_segs, self.max_n = ops.make_opt_segments(
            [(w, g, s, l2, self.touched if k == "table" else None) for w, g, s, (_, l2, k) in zip(self.w, self.g, self.slots, self.lay)], device)

    def load_grads(self, gs, mask):
        """gs: the effective gradients (zero where the table's group is untouched); the device table gets NaN there instead."""
        for t, g in zip(self.g[:-1], gs[:-1]):
            t.copy_(torch.from_numpy(g))
        tab = gs[-1].reshape(-1, 4).copy()
        tab[~mask] = np.nan
        self.g[-1].copy_(torch.from_numpy(tab.reshape(-1)))
        self.touched.copy_(torch.from_numpy(mask.astype(np.uint8)))


def _inputs(case, seed, lay=None):
    """weights, per-update effective gradients and touched maps (about a tenth of the table's groups set) of a case."""
    cid, name, kw, rule, okw = case
    rng = np.random.RandomState(seed)
    lay = _layout() if lay is None else lay
    shapes, l2s = [(n,) for n, _, _ in lay], [l2 for _, l2, _ in lay]
    masks = [rng.rand(lay[-1][0] // 4) < 0.1 for _ in range(UPDATES)]

    def mask_table(gs):
        for g, m in zip(gs, masks):
            g[-1].reshape(-1, 4)[~m] = 0.0
        return gs
    if rule == "ftrl":              # draws with |z| within 1e-6 of l1 are taken again on the CPU (the masked gradients are part of the draw)
        ws, gs = RO.ftrl_draw(rng, shapes, l2s, UPDATES, kw["learning_rate"], okw, transform=mask_table)
        return ws, gs, masks, l2s
    ws = [rng.uniform(-0.5, 0.5, s).astype(np.float32) for s in shapes]
    gs = mask_table([[rng.normal(0, 0.1, s).astype(np.float32) for s in shapes] for _ in range(UPDATES)])
    return ws, gs, masks, l2s


def _run_hip(device, opt, ws, gs, masks, lay=None):
    from deepctr_amd import ops
    rule = dict(opt._rule(), clipvalue=opt.clipvalue)
    sg = Segments(device, ws, rule["slots"], lay)
    clip = ops.grad_clip_workspace(sg.n_segs, sg.max_n, device) if (opt.clipnorm or opt.global_clipnorm) else None
    for t, (g, m) in enumerate(zip(gs, masks), 1):
        sg.load_grads(g, m)
        scale = None
        if clip is not None:
            ops.grad_clip_scales(sg.segs, sg.n_segs, sg.max_n, opt.global_clipnorm or opt.clipnorm, clip[0], clip[1],
                                 global_norm=opt.global_clipnorm is not None)
            scale = clip[1]
        ops.opt_apply(rule, sg.segs, sg.n_segs, sg.max_n, opt._step_lr(t), zero_grad=True, clip_scale=scale)
        torch.cuda.synchronize()
        # zero_grad: set bytes and their gradients are cleared; clear groups were neither read (their NaN would be in w) nor cleared
        assert int(sg.touched.sum()) == 0
        tab = sg.g[-1].cpu().numpy().reshape(-1, 4)
        assert np.all(tab[m] == 0.0) and np.all(np.isnan(tab[~m]))
        assert all(float(x.abs().max()) == 0.0 for x in sg.g[:-1])
    return [w.cpu().numpy() for w in sg.w], sg


def _run_torch(opt, ws, gs, lay, dtype):
    from deepctr_amd import training
    l2s = [l2 for _, l2, _ in lay]
    params = [torch.tensor(w, dtype=dtype) for w in ws]
    ko = training.KerasOptimizer(params, opt)
    for g in gs:
        for p, gg, l2 in zip(params, g, l2s):
            p.grad = torch.tensor(gg, dtype=dtype) + (2.0 * l2) * p.detach()
        ko.step()
    return [p.detach().numpy() for p in params]


@pytest.mark.parametrize("case", RO.CASES, ids=RO.CASE_IDS)
def test_opt_apply_matches_the_float64_oracle(device, case):
    _updates_against_the_oracle(device, case, _layout())


@pytest.mark.parametrize("case", RO.CASES, ids=RO.CASE_IDS)
def test_opt_apply_matches_the_float64_oracle_with_l2_on_every_route(device, case):
    """The same comparison at the same bar on _layout_l2(): 2 l2 w enters on the touched table — where nine groups in ten have a clear byte
    and move by the l2 term alone —, on the element-by-element route and in the tail loop."""
    _updates_against_the_oracle(device, case, _layout_l2())


def _updates_against_the_oracle(device, case, lay):
    from deepctr_amd import optimizers
    cid, name, kw, rule, okw = case
    ws, gs, masks, l2s = _inputs(case, zlib.crc32(cid.encode()) % 1000, lay)
    oracle = RO.Oracle(rule, **okw)
    want = [w.astype(np.float64) for w in ws]
    for g in gs:
        oracle.update(want, g, l2s, kw["learning_rate"])
    if l2s[-1] > 0:
        # groups of the table no update touched: the oracle moved every element of them (by the l2 term alone), so the comparison below
        # says something about the kernel's clear-byte path
        never = ~np.any(masks, axis=0)
        assert never.sum() >= 32 and np.all(want[-1].reshape(-1, 4)[never] != ws[-1].reshape(-1, 4)[never].astype(np.float64))
    t32 = _run_torch(getattr(optimizers, name)(**kw), ws, gs, lay, torch.float32)
    opt = getattr(optimizers, name)(**kw)
    got, _ = _run_hip(device, opt, ws, gs, masks, lay)
    e_torch = max(float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(t32, want))
    worst = 0.0
    for i, (a, b) in enumerate(zip(got, want)):
        assert np.isfinite(a).all(), "segment %d: a poisoned gradient was read" % i
        err = np.abs(a.astype(np.float64) - b)
        # (the Adam cases use this bar up: the kernel forms 1 - beta_2 in float32 as dctr_adam_multi does, 3e-5 off in relative terms,
        # which is 1.5e-7 of bias per update at lr 0.01 against the restatement's 1e-7 of rounding — measured ratios 3.42 / 4.00 / 4.40,
        # the last two inside the bar by its ulp term only; the inputs are seeded, so the figures repeat)
        bar = 4.0 * e_torch + np.spacing(np.abs(b).astype(np.float32)).astype(np.float64)
        worst = max(worst, float(err.max()))
        assert np.all(err <= bar), "%s segment %d (n %d): off by %.3g, torch float32 by %.3g" % (cid, i, a.size, float(err.max()), e_torch)
        if rule == "ftrl":
            assert np.array_equal(a == 0.0, b == 0.0), "%s segment %d: Ftrl's exact zeros" % (cid, i)
    print("opt_apply %s: largest error %.3g, torch float32 %.3g, ratio %.2f" % (cid, worst, e_torch, worst / max(e_torch, 1e-30)))


def test_ftrl_keeps_the_oracles_zeros_exactly(device):
    """l1 such that the oracle holds at least a third of the weights at zero and at least a third away from it."""
    from deepctr_amd import optimizers
    kw = dict(learning_rate=0.05, l1_regularization_strength=0.15)
    okw = dict(l1_regularization_strength=0.15)
    case = ("ftrl_zeros", "Ftrl", kw, "ftrl", okw)
    ws, gs, masks, l2s = _inputs(case, 77)
    want = [w.astype(np.float64) for w in ws]
    oracle = RO.Oracle("ftrl", **okw)
    for g in gs:
        oracle.update(want, g, l2s, kw["learning_rate"])
    dense = np.concatenate([b for b, (_, _, k) in zip(want, _layout()) if k != "table"])
    frac = float((dense == 0).mean())
    assert 1.0 / 3 <= frac <= 2.0 / 3, frac
    got, _ = _run_hip(device, optimizers.Ftrl(**kw), ws, gs, masks)
    for a, b in zip(got, want):
        assert np.array_equal(a == 0.0, b == 0.0)
        assert np.all(a[b == 0.0] == 0.0)


@pytest.mark.parametrize("kind", ["adam", "adagrad", "rmsprop", "sgd"])
def test_the_old_kinds_give_dctr_opt_multis_bits(device, kind):
    from deepctr_amd import _C, ops
    rng = np.random.RandomState(9)
    lay = [(n, l2, k) for n, l2, k in _layout() if k != "offset"]        # (dctr_opt_multi takes 16-byte aligned buffers only)
    ws = [rng.uniform(-0.5, 0.5, n).astype(np.float32) for n, _, _ in lay]
    mk = lambda w, fill=None: (torch.from_numpy(w).to(device) if fill is None else torch.full((w.size,), fill, device=device))   # noqa: E731
    acc = 0.1 if kind == "adagrad" else 0.0
    old = [dict(w=mk(w), m=mk(w, 0.0), v=mk(w, acc), g=mk(w, 0.0)) for w in ws]
    new = [dict(w=mk(w), m=mk(w, 0.0), v=mk(w, acc), g=mk(w, 0.0)) for w in ws]
    t_old = torch.zeros(lay[-1][0] // 4, dtype=torch.uint8, device=device)
    t_new = torch.zeros_like(t_old)
    segs_old = ops.make_adam_segments([(p["w"], p["m"], p["v"], p["g"], l2, t_old if k == "table" else None)
                                       for p, (_, l2, k) in zip(old, lay)], device)
    slots = {"adam": lambda p: [p["m"], p["v"]], "adagrad": lambda p: [p["v"]], "rmsprop": lambda p: [p["v"]], "sgd": lambda p: []}[kind]
    segs_new = ops.make_opt_segments([(p["w"], p["g"], slots(p), l2, t_new if k == "table" else None) for p, (_, l2, k) in zip(new, lay)], device)
    rule = dict(kind=_C.OPT_CODES[kind], beta1=0.9, beta2=0.999 if kind == "adam" else 0.9, eps=1e-7)
    for t in range(1, 4):
        mask = rng.rand(lay[-1][0] // 4) < 0.1
        for po, pn, (n, _, k) in zip(old, new, lay):
            g = rng.normal(0, 0.1, n).astype(np.float32)
            if k == "table":
                g.reshape(-1, 4)[~mask] = np.nan
            po["g"].copy_(torch.from_numpy(g))
            pn["g"].copy_(torch.from_numpy(g))
        t_old.copy_(torch.from_numpy(mask.astype(np.uint8)))
        t_new.copy_(t_old)
        lr = 0.01 * (np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t) if kind == "adam" else 1.0)
        ops.opt_multi(kind, segs_old[0], segs_old[1], segs_old[2], lr, rule["beta1"], rule["beta2"], rule["eps"])
        ops.opt_apply(rule, segs_new[0], segs_new[1], segs_new[2], lr)
        for po, pn in zip(old, new):
            for key in ("w", "m", "v"):
                a, b = po[key].cpu().numpy(), pn[key].cpu().numpy()
                assert np.array_equal(a, b), (kind, t, key, a.size)
            assert torch.equal(torch.nan_to_num(po["g"]), torch.nan_to_num(pn["g"]))
        assert torch.equal(t_old, t_new)
    # the l2 penalties ride the launch as they do dctr_opt_multi_l2's
    pen_old, pen_new = torch.zeros(1, dtype=torch.float64, device=device), torch.zeros(1, dtype=torch.float64, device=device)
    want = 200.0 * _penalty64([p["w"] for p in old], lay)          # (of the weights BEFORE the update)
    ops.opt_multi(kind, segs_old[0], segs_old[1], segs_old[2], 0.01, rule["beta1"], rule["beta2"], rule["eps"], penalty=pen_old, penalty_scale=200.0)
    ops.opt_apply(rule, segs_new[0], segs_new[1], segs_new[2], 0.01, penalty=pen_new, penalty_scale=200.0)
    assert float(pen_old) > 0 and abs(float(pen_old) - float(pen_new)) <= 1e-12 * float(pen_old)
    for po, pn in zip(old, new):
        assert torch.equal(po["w"], pn["w"])
    assert want > 0
    assert abs(float(pen_old) - want) <= _penalty_bar(lay) * want and abs(float(pen_new) - want) <= _penalty_bar(lay) * want, (
        float(pen_old), float(pen_new), want)


def _penalty64(ws, lay):
    """sum over the segments of l2 * sum(w^2) in float64, from host copies of the weights (device tensors or arrays)."""
    host = [w.detach().cpu().numpy() if torch.is_tensor(w) else np.asarray(w) for w in ws]
    return sum(l2 * float((w.astype(np.float64) ** 2).sum()) for w, (_, l2, _) in zip(host, lay))


def _penalty_bar(lay):
    """The relative error the in-launch penalty may have against float64.  A thread adds its squares up in float32 and everything
    behind that — the sum over the workgroup, the products with l2 and penalty_scale, the atomic add — is float64.  Every segment gets
    at least one workgroup of 256 threads, each thread takes every 256th group (or element) at the closest, so no thread adds more than
    k = ceil(n_max / 256) squares: each square carries one rounding (2^-24 relative) and a float32 sum of k non-negative terms k - 1
    more, which bounds a thread's share, and so the sum of the shares, by k 2^-24 relative; the segment's l2 is a float32 (one more
    rounding of the Python value the reference multiplies by) and one 2^-24 is kept for the second-order terms: (k + 2) 2^-24."""
    n_max = max(n for n, _, _ in lay)
    return (-(-n_max // 256) + 2) * 2.0 ** -24


APPLY_RULES = {      # one rule per number of state slots of dctr_opt_apply's kernel (NS), and Ftrl
    "sgd_ns0": ("SGD", dict(learning_rate=0.05)), "adagrad_ns1": ("Adagrad", dict(learning_rate=0.1)),
    "adam_ns2": ("Adam", dict(learning_rate=0.01)), "adam_amsgrad_ns3": ("Adam", dict(learning_rate=0.01, amsgrad=True)),
    "ftrl_ns2": ("Ftrl", dict(learning_rate=0.05, l1_regularization_strength=0.01)),
}


def _penalty_grads(rng, lay, sg_g, touched):
    """One update's gradients on the device: NaN in the clear groups of the table, a tenth of its bytes set."""
    mask = rng.rand(lay[-1][0] // 4) < 0.1
    for t, (n, _, k) in zip(sg_g, lay):
        g = rng.normal(0, 0.1, n).astype(np.float32)
        if k == "table":
            g.reshape(-1, 4)[~mask] = np.nan
        t.copy_(torch.from_numpy(g))
    touched.copy_(torch.from_numpy(mask.astype(np.uint8)))


@pytest.mark.parametrize("entry", sorted(APPLY_RULES) + ["multi_adam", "multi_adagrad", "multi_rmsprop", "multi_sgd"])
def test_the_launch_adds_the_float64_l2_penalty(device, entry):
    """penalty += penalty_scale * sum_segments l2 * sum(w^2) of the weights BEFORE the update, against float64 from host copies at
    _penalty_bar; a second launch ADDS the penalty at the then-current weights; with every l2 at 0 the accumulator stays exactly 0.0.
    dctr_opt_multi takes 16-byte aligned buffers only: the offset segment runs on dctr_opt_apply alone."""
    from deepctr_amd import ops, optimizers
    multi = entry.startswith("multi_")
    full = [s for s in _layout_l2() if not (multi and s[2] == "offset")]
    scale = 200.0
    for lay in (full, [(n, 0.0, k) for n, _, k in full]):
        rng = np.random.RandomState(zlib.crc32(entry.encode()) % 1000)
        ws = [rng.uniform(-0.5, 0.5, n).astype(np.float32) for n, _, _ in lay]
        pen = torch.zeros(1, dtype=torch.float64, device=device)
        if multi:
            kind = entry[len("multi_"):]
            mk = lambda w, fill: torch.full((w.size,), fill, dtype=torch.float32, device=device)     # noqa: E731
            ps = [dict(w=torch.from_numpy(w).to(device), m=mk(w, 0.0), v=mk(w, 0.1 if kind == "adagrad" else 0.0), g=mk(w, 0.0)) for w in ws]
            touched = torch.zeros(lay[-1][0] // 4, dtype=torch.uint8, device=device)
            segs = ops.make_adam_segments([(p["w"], p["m"], p["v"], p["g"], l2, touched if k == "table" else None)
                                           for p, (_, l2, k) in zip(ps, lay)], device)
            w_dev, g_dev = [p["w"] for p in ps], [p["g"] for p in ps]
            launch = lambda t: ops.opt_multi(kind, segs[0], segs[1], segs[2], 0.01, 0.9, 0.999 if kind == "adam" else 0.9, 1e-7,    # noqa: E731
                                             penalty=pen, penalty_scale=scale)
        else:
            name, kw = APPLY_RULES[entry]
            opt = getattr(optimizers, name)(**kw)
            rule = dict(opt._rule(), clipvalue=opt.clipvalue)
            assert "ns%d" % len(rule["slots"]) in entry
            sg = Segments(device, ws, rule["slots"], lay)
            w_dev, g_dev, touched = sg.w, sg.g, sg.touched
            launch = lambda t: ops.opt_apply(rule, sg.segs, sg.n_segs, sg.max_n, opt._step_lr(t), penalty=pen, penalty_scale=scale)  # noqa: E731
        want = 0.0
        for t in (1, 2):
            _penalty_grads(rng, lay, g_dev, touched)
            want += scale * _penalty64(w_dev, lay)
            before = [w.clone() for w in w_dev]
            launch(t)
            torch.cuda.synchronize()
            assert all(not torch.equal(a, b) and bool(torch.isfinite(b).all()) for a, b in zip(before, w_dev)), "the update itself ran"
            got = float(pen)
            if all(l2 == 0.0 for _, l2, _ in lay):
                assert got == 0.0 and want == 0.0
            else:
                assert want > 0 and abs(got - want) <= _penalty_bar(lay) * want, (entry, t, got, want, abs(got - want) / want, _penalty_bar(lay))
                print("%s launch %d: penalty off by %.3g relative, bar %.3g" % (entry, t, abs(got - want) / want, _penalty_bar(lay)))


def test_grad_clip_scales(device):
    _clip_scales_against_float64(device, _layout())


def test_grad_clip_scales_with_l2_on_every_route(device):
    """clipnorm and global_clipnorm over g + 2 l2 w on _layout_l2(): the table's clear groups add (2 l2 w)^2 without their (poisoned)
    gradient being read, the offset segment and the tails carry the term element by element."""
    _clip_scales_against_float64(device, _layout_l2())


def _clip_scales_against_float64(device, lay):
    from deepctr_amd import _C, ops
    rng = np.random.RandomState(13)
    ws = [rng.uniform(-0.5, 0.5, n).astype(np.float32) for n, _, _ in lay]
    amp = [0.5, 0.001, 0.3, 0.001, 0.02, 0.01, 0.02, 0.01, 0.05]            # some norms above the clip value, some below
    gs = [(rng.normal(0, a, n)).astype(np.float32) for (n, _, _), a in zip(lay, amp)]
    mask = rng.rand(lay[-1][0] // 4) < 0.1
    gs[-1].reshape(-1, 4)[~mask] = 0.0
    sg = Segments(device, ws, [], lay)
    ws_, scale = ops.grad_clip_workspace(sg.n_segs, sg.max_n, device)
    eff = [g.astype(np.float64) + 2.0 * l2 * w.astype(np.float64) for g, w, (_, l2, _) in zip(gs, ws, lay)]
    out = {}
    for mode, clip in ((False, 0.25), (True, 0.9), (True, 100.0)):
        sg.load_grads(gs, mask)                     # (NaN in the clear groups: the touched-skipping route must not read them)
        ops.grad_clip_scales(sg.segs, sg.n_segs, sg.max_n, clip, ws_, scale, global_norm=mode)
        first = scale.cpu().numpy().copy()
        scale.fill_(-1.0)
        ops.grad_clip_scales(sg.segs, sg.n_segs, sg.max_n, clip, ws_, scale, global_norm=mode)
        again = scale.cpu().numpy()
        assert np.array_equal(first.view(np.uint32), again.view(np.uint32)), "two calls, two results"
        want = np.array(RO.clip_scales(eff, None if mode else clip, clip if mode else None))
        assert np.all(np.abs(first - want) <= 1.5 * np.spacing(want.astype(np.float32))), (first, want)
        below = np.array([np.sqrt((e ** 2).sum()) for e in eff]) < clip if not mode else np.full(len(eff), np.sqrt(sum((e ** 2).sum() for e in eff)) < clip)
        assert np.all(first[below] == 1.0)
        out[(mode, clip)] = first
    assert (out[(False, 0.25)] == 1.0).any() and (out[(False, 0.25)] < 1.0).any() and np.all(out[(True, 0.9)] < 1.0) and np.all(out[(True, 100.0)] == 1.0)
    # the dense route (no touched map, zeros where the map is clear) gives the touched route's bits
    dense = Segments(device, ws, [], lay)
    for t, g in zip(dense.g, gs):
        t.copy_(torch.from_numpy(g))
    dsegs = ops.make_opt_segments([(w, g, [], l2) for w, g, (_, l2, _) in zip(dense.w, dense.g, lay)], device)
    ops.grad_clip_scales(dsegs[0], dsegs[1], dsegs[2], 0.25, ws_, scale, global_norm=False)
    assert np.array_equal(scale.cpu().numpy().view(np.uint32), out[(False, 0.25)].view(np.uint32))
    # a workspace smaller than the query's: DCTR_E_NULL, nothing launched
    scale.fill_(-1.0)
    with pytest.raises(_C.DctrError) as e:
        ops.grad_clip_scales(sg.segs, sg.n_segs, sg.max_n, 0.25, ws_[:ws_.numel() - 1], scale)
    torch.cuda.synchronize()
    assert e.value.rc == _C.E_NULL and float(scale.max()) == -1.0


# ---- whole models ------------------------------------------------------------------------------------------------------------------
def _objects():
    from deepctr_amd.optimizers import SGD, Adagrad, Adam, Ftrl, schedules
    return {"adagrad": lambda: Adagrad(0.1), "ftrl": lambda: Ftrl(0.05, l1_regularization_strength=1e-4),
            "sgd_nesterov_clip": lambda: SGD(0.05, momentum=0.9, nesterov=True, global_clipnorm=0.5),
            "adam_amsgrad_schedule_clip": lambda: Adam(schedules.ExponentialDecay(0.01, 2, 0.5), amsgrad=True, clipvalue=0.01)}


def _model(kind, device, rng):
    from deepctr_amd import models
    from deepctr_amd.feature_column import DenseFeat, SparseFeat
    from tests.test_gpu_din_train import _din, _din_feed
    from tests.test_gpu_models import _randomise
    from tests.test_gpu_train import _feed
    n = 600
    if kind == "DIN":
        make = lambda: _din(device, "dice")[0]          # noqa: E731
        feed = _din_feed(rng, n)
    else:
        cols = [SparseFeat("a", 50, 8), SparseFeat("b", 47, 8, use_hash=True), SparseFeat("c", 9, 8), DenseFeat("d", 1)]
        kw = dict(dnn_hidden_units=(16, 8), l2_reg_embedding=1e-3, l2_reg_linear=1e-3, l2_reg_dnn=1e-3, device=device)
        make = (lambda: models.DeepFM(cols, cols, **kw)) if kind == "DeepFM" else (lambda: models.DCN(cols, cols, cross_num=2, **kw))
        feed = _feed(rng, cols, n)
    probe = make()
    w0 = _randomise(probe, rng)
    return make, w0, feed, (rng.rand(n) > 0.5).astype(np.float32)


def _weights_close(what, w0, w_hip, w_ref, rtol=5e-4, atol=1e-5):
    """The two fits' weights after three updates, per tensor over max(the autograd step's largest element, 1 % of the largest weight of
    any tensor).  A coarse end-to-end check — three updates of ~1e-2 sit on weights of ~0.5 — beside _updates_match, which holds the
    updates themselves; the two fits' update distance is printed (it carries three dependent backward passes' rounding)."""
    names = [k for k in w_ref if "moving_" not in k]
    wmax = max(float(np.abs(w_ref[k]).max()) for k in names)
    dmax = max(float(np.abs(w_ref[k] - w0[k]).max()) for k in names)
    for k in names:
        scale = max(float(np.abs(w_ref[k]).max()), 1e-2 * wmax)
        d_ref, d_hip = (w_ref[k] - w0[k]).astype(np.float64), (w_hip[k] - w0[k]).astype(np.float64)
        dscale = max(float(np.abs(d_ref).max()), 1e-2 * dmax)
        print("%s: %s: weights off by %.3g of their scale, updates (largest %.3g) by %.3g of theirs"
              % (what, k, float(np.abs(w_hip[k] - w_ref[k]).max()) / scale, float(np.abs(d_ref).max()), float(np.abs(d_hip - d_ref).max()) / dscale))
        assert float(np.abs(d_ref).max()) > 0, "%s: %s did not move" % (what, k)
        assert_close(w_hip[k].astype(np.float64) / scale, w_ref[k].astype(np.float64) / scale, rtol=rtol, atol=atol, what="%s: %s" % (what, k))


class _Recorder(object):
    """Records what every HipTrainer.apply_update of a fit() meets: the weights before the first one and each update's gradients."""

    def __init__(self, monkeypatch):
        from deepctr_amd.training_hip import HipTrainer
        self.w0, self.grads, self.tr = None, [], None
        real = HipTrainer.apply_update
        rec = self

        def apply_update(tr):
            if rec.tr is None:
                rec.tr, rec.w0 = tr, [p.w.clone() for p in tr.params]
            if tr is rec.tr:
                rec.grads.append([p.g.clone() for p in tr.params])      # (zero wherever a table's touched byte is clear)
            return real(tr)
        monkeypatch.setattr(HipTrainer, "apply_update", apply_update)
        self.undo = lambda: monkeypatch.setattr(HipTrainer, "apply_update", real)


def _updates_match(what, rec, make_opt, rtol=5e-4, atol=1e-5):
    """tests/test_gpu_train_reg.py::_autograd_check's method and bars on the UPDATES w3 - w0 of the HIP fit, tensor by tensor over
    max(the reference update's largest element, 1 % of the largest update of any tensor), plus float32's resolution of the weights
    the updates are read from (three ulp: see below).  The reference is the autograd step's optimizer
    (training.KerasOptimizer with a fresh object of the same kind) fed the very gradients the HIP step's three backward passes produced,
    from the same starting weights: whatever the trainer wires — state slots and their initial values, the schedule, iterations, the l2
    term, the clip pre-pass, clipvalue — is in the comparison, and the backward's rounding, which the existing gradient tests of these
    models hold to the same bars, is not."""
    from deepctr_amd import training
    tr = rec.tr
    assert len(rec.grads) == 3
    params = [w.clone() for w in rec.w0]
    ko = training.KerasOptimizer(params, make_opt())
    for gs in rec.grads:
        for p, g, q in zip(params, gs, tr.params):
            p.grad = g + (2.0 * q.l2) * p
        ko.step()
    d_ref = [(p - w).double().cpu().numpy() for p, w in zip(params, rec.w0)]
    d_hip = [(q.w - w).double().cpu().numpy() for q, w in zip(tr.params, rec.w0)]
    dmax = max(float(np.abs(d).max()) for d in d_ref)
    assert dmax > 0
    worst = 0.0
    for i, (a, b) in enumerate(zip(d_hip, d_ref)):
        scale = max(float(np.abs(b).max()), 1e-2 * dmax)
        # An update is read off as a difference of float32 weights, and each of the three updates rounds the weight once in either
        # evaluation (half an ulp each): beside _autograd_check's bar, the two may stand 3 x (1/2 + 1/2) ulp of the weight apart.  On an
        # embedding of ~0.1 that moves by ~2e-4 one ulp of the weight is already 2e-5 of the update's scale, twice that bar's atol.
        wmag = np.maximum(rec.w0[i].abs().cpu().numpy(), tr.params[i].w.abs().cpu().numpy())
        bar = scale * (atol + rtol * np.abs(b / scale)) + 3.0 * np.spacing(wmag.astype(np.float32)).astype(np.float64)
        err = np.abs(a - b)
        worst = max(worst, float((err / bar).max()))
        assert np.all(err <= bar), "%s: update of parameter %d %s (largest %.3g): off by %.3g of its scale, %.2f x the bar" % (
            what, i, tuple(tr.params[i].w.shape), float(np.abs(b).max()), float(err.max()) / scale, float((err / bar).max()))
    print("%s: updates of the HIP step against the torch restatement on its own gradients: at most %.2f of the bar" % (what, worst))


def _continues_then_rebuilds(model, opt, make_opt, fit, compile_args=()):
    """A second fit() with the same object continues — the trainer, its state buffers (not reset) and the update count — and compile()
    with a new object rebuilds the trainer."""
    tr = model._hip_trainer
    inits = opt._rule()["slots"]
    assert tr.optimizer is opt and tr.t == 3 and all(len(p.slots) == len(inits) for p in tr.params)
    slot_ptrs = [s.data_ptr() for p in tr.params for s in p.slots]
    witness = tr.p_kernels[0] if tr.p_kernels else tr.params[-1]
    before = [s.clone() for s in witness.slots]
    fit()
    assert model._hip_trainer is tr and opt.iterations == 6 and tr.t == 6
    assert [s.data_ptr() for p in tr.params for s in p.slots] == slot_ptrs
    # the same buffers, carried on from where the first fit() left them: some state moved, and none is back at its initial fill
    # (Ftrl's accumulator alone may stand still: once its weights have shrunk, g^2 is below float32's resolution of n >= 0.1)
    assert any(not torch.equal(a, b) for a, b in zip(before, witness.slots)) or not before
    assert all(not torch.equal(s, torch.full_like(s, v)) for s, v in zip(witness.slots, inits))
    other = make_opt()
    model.compile(other, *compile_args)
    fit()
    assert model._hip_trainer is not tr and model._hip_trainer.optimizer is other and other.iterations == 3 and opt.iterations == 6


@pytest.mark.parametrize("obj", sorted(_objects()))
@pytest.mark.parametrize("kind", ["DeepFM", "DCN", "DIN"])
def test_models_train_on_the_hip_step_with_optimizer_objects(device, kind, obj, monkeypatch):
    """B = 200, three updates from the same weights on both steps: the same loss (tests/test_gpu_fit.py's bar for the l2-inclusive
    loss), the HIP step's updates at _autograd_check's bars (_updates_match), the same weights; then a second fit() continues the
    optimizer's state, and a new object rebuilds the trainer."""
    rng = np.random.RandomState(zlib.crc32((kind + obj).encode()) % 1000)
    make, w0, feed, y = _model(kind, device, rng)
    out = {}
    for hip in (True, False):
        model = make()
        model.set_weights_by_name(w0)
        model.hip_training = hip
        opt = _objects()[obj]()
        model.compile(opt, "binary_crossentropy")
        rec = _Recorder(monkeypatch) if hip else None
        h = model.fit(feed, y, batch_size=200, epochs=1, verbose=0, shuffle=False)
        assert (getattr(model, "_hip_trainer", None) is not None) == hip, "fit() took the wrong step"
        assert opt.iterations == 3
        if hip:
            rec.undo()
            _updates_match("%s %s" % (kind, obj), rec, _objects()[obj])
        out[hip] = (model, opt, h.history["loss"], model.get_weights_by_name())
    assert_close(np.array(out[True][2]), np.array(out[False][2]), rtol=2e-5, atol=1e-7, what="%s %s: fit loss, HIP step vs autograd step" % (kind, obj))
    _weights_close("%s %s" % (kind, obj), w0, out[True][3], out[False][3])
    model, opt = out[True][0], out[True][1]
    _continues_then_rebuilds(model, opt, _objects()[obj], lambda: model.fit(feed, y, batch_size=200, epochs=1, verbose=0, shuffle=False),
                             ("binary_crossentropy",))


def test_mmoe_trains_on_the_hip_step_with_centered_momentum_rmsprop(device, monkeypatch):
    from deepctr_amd import models
    from deepctr_amd.optimizers import RMSprop
    from tests.test_gpu_mtl import _fuzz_feed
    from tests.test_gpu_mtl_train import _build, _labels, _step_cols
    cols, n = _step_cols(), 600
    kw = dict(num_experts=3, expert_dnn_hidden_units=(16, 8), tower_dnn_hidden_units=(8,), l2_reg_dnn=1e-3, l2_reg_embedding=1e-3)
    probe, w0 = _build("MMOE", device, 11, cols, **kw)
    rng = np.random.RandomState(12)
    feed, ys = _fuzz_feed(rng, cols, n), _labels(rng, probe.task_types, n)
    make_opt = lambda: RMSprop(0.01, momentum=0.5, centered=True)      # noqa: E731
    out = {}
    for hip in (True, False):
        model = models.MMOE(cols, device=device, **kw)
        model.set_weights_by_name(w0)
        model.hip_training = hip
        opt = make_opt()
        model.compile(opt)
        rec = _Recorder(monkeypatch) if hip else None
        h = model.fit(feed, ys, batch_size=200, epochs=1, verbose=0, shuffle=False).history
        assert (getattr(model, "_hip_trainer", None) is not None) == hip and opt.iterations == 3
        if hip:
            rec.undo()
            _updates_match("MMOE rmsprop", rec, make_opt)
        out[hip] = (model, opt, h, model.get_weights_by_name())
    assert_close(out[True][2]["loss"], out[False][2]["loss"], rtol=2e-5, atol=1e-7, what="MMOE: fit loss, HIP step vs autograd step")
    _weights_close("MMOE rmsprop", w0, out[True][3], out[False][3])
    model, opt = out[True][0], out[True][1]
    assert all(len(p.slots) == 3 for p in model._hip_trainer.params)            # ms, mg, mom
    _continues_then_rebuilds(model, opt, make_opt, lambda: model.fit(feed, ys, batch_size=200, epochs=1, verbose=0, shuffle=False))


def test_state_slots_follow_the_rule(device):
    from deepctr_amd.feature_column import SparseFeat
    from deepctr_amd.models import DeepFM
    from deepctr_amd.optimizers import SGD, Adadelta, Adagrad, Adam, Adamax, Ftrl, RMSprop
    from deepctr_amd.training_hip import HipTrainer
    cols = [SparseFeat("a", 10, 8), SparseFeat("b", 7, 8)]
    model = DeepFM(cols, cols, dnn_hidden_units=(8,), device=device)
    for opt, n, fills in ((SGD(0.1), 0, []), (SGD(0.1, momentum=0.5), 1, [0.0]), (Adagrad(0.1, 0.25), 1, [0.25]), (RMSprop(), 1, [0.0]),
                          (RMSprop(centered=True), 2, [0.0] * 2), (RMSprop(momentum=0.1, centered=True), 3, [0.0] * 3), (Adam(), 2, [0.0] * 2),
                          (Adam(amsgrad=True), 3, [0.0] * 3), (Adamax(), 2, [0.0] * 2), (Adadelta(), 2, [0.0] * 2),
                          (Ftrl(initial_accumulator_value=0.3), 2, [0.3, 0.0])):
        tr = HipTrainer(model, opt)
        for p in tr.params:
            assert len(p.slots) == n and [float(s.flatten()[0]) for s in p.slots] == [np.float32(f) for f in fills], type(opt).__name__


def test_a_name_still_launches_dctr_opt_multi_with_todays_bits(device, monkeypatch):
    """compile("adam"): what launches is ops.opt_multi, and every launch moves the weights and moments exactly as a HipTrainer(model, "adam")
    built by hand moves them from the same inputs — replayed launch by launch on a twin, since the float atomics of the backward make two
    whole runs differ in the last bit.  compile(Adam()) launches ops.opt_apply instead."""
    from deepctr_amd import ops
    from deepctr_amd.optimizers import Adam
    from deepctr_amd.training_hip import HipTrainer
    rng = np.random.RandomState(5)
    make, w0, feed, y = _model("DeepFM", device, rng)
    model, twin_model = make(), make()
    model.set_weights_by_name(w0)
    twin_model.set_weights_by_name(w0)
    twin = HipTrainer(twin_model, "adam")
    calls = {"multi": 0, "apply": 0}
    real_multi, real_apply = ops.opt_multi, ops.opt_apply

    def multi(kind, segs, *a, **kw):
        tr = model._hip_trainer
        if segs is not tr.segs:                 # the twin's own launch
            return real_multi(kind, segs, *a, **kw)
        assert kind == "adam"
        calls["multi"] += 1
        for p, q in zip(tr.params, twin.params):
            q.w.copy_(p.w), q.m.copy_(p.m), q.v.copy_(p.v), q.g.copy_(p.g)
            assert q.l2 == p.l2 and (q.touched is None) == (p.touched is None)
            if p.touched is not None:
                q.touched.copy_(p.touched)
        real_multi(kind, segs, *a, **kw)
        twin.t = tr.t - 1
        twin.penalty_acc = None if kw.get("penalty") is None else torch.zeros_like(kw["penalty"])
        twin.penalty_rows = tr.penalty_rows
        twin.apply_update()
        for p, q in zip(tr.params, twin.params):
            assert torch.equal(p.w, q.w) and torch.equal(p.m, q.m) and torch.equal(p.v, q.v) and torch.equal(p.g, q.g)

    def apply(*a, **kw):
        calls["apply"] += 1
        return real_apply(*a, **kw)
    monkeypatch.setattr(ops, "opt_multi", multi)
    monkeypatch.setattr(ops, "opt_apply", apply)
    model.compile("adam", "binary_crossentropy")
    model.fit(feed, y, batch_size=200, epochs=1, verbose=0, shuffle=False)
    assert calls == {"multi": 3, "apply": 0} and model._hip_trainer.optimizer == "adam" and model._hip_trainer.opt is None
    assert len(model._hip_trainer.params) == len(twin.params)
    model.compile(Adam(), "binary_crossentropy")
    model.fit(feed, y, batch_size=200, epochs=1, verbose=0, shuffle=False)
    assert calls == {"multi": 3, "apply": 3} and model._hip_trainer.opt is not None


def test_the_readme_example_trains_a_deepfm_on_the_hip_step(device):
    from deepctr_amd.feature_column import DenseFeat, SparseFeat
    from deepctr_amd.models import DeepFM
    from deepctr_amd.optimizers import Adagrad
    rng = np.random.RandomState(0)
    n = 2048
    cols = [SparseFeat("a", 20, 8), SparseFeat("b", 30, 8), DenseFeat("d", 2)]
    feed = {"a": rng.randint(0, 20, n), "b": rng.randint(0, 30, n), "d": rng.rand(n, 2).astype(np.float32)}
    y = ((feed["a"] % 2) ^ (feed["d"][:, 0] > 0.5)).astype(np.float32)
    model = DeepFM(cols, cols, dnn_hidden_units=(16, 8), device=device)
    model.compile(Adagrad(0.1024), "binary_crossentropy")
    h = model.fit(feed, y, batch_size=256, epochs=6, verbose=0)
    assert model._hip_trainer is not None and model._hip_trainer.kind == "adagrad" and model._hip_trainer.opt.iterations == 6 * 8
    assert h.history["loss"][-1] < h.history["loss"][0] - 0.02, h.history["loss"]
