"""GPU parity tests, op level, of dctr_mlp_bwd (deepctr_amd/csrc/dnn_train_kernels.hip, deepctr_amd/csrc/mlp_bwd_kernels.hip, the grouped
GEMM of deepctr_amd/csrc/gemm_kernels.hip) on both of its forms — chained (widest layer <= 1216) and layered (wider, and Dice) — against
the float64 oracle of tests/ref_mlp_bwd.py, which restates the op's contract (act' from the SAVED outputs) and is pinned without a GPU
by tests/test_mlp_bwd_oracle_cpu.py together with the form every case of the table takes.

Bar: tests.util.assert_close_terms' defaults — 1e-4 of the result plus 2e-6 of the summed magnitude.  The op ACCUMULATES into d_kernels /
d_biases / d_head_w, so each starts at a random non-zero g0 and ``g - g0`` is compared; g0 is one more summand of the fp32 sum the
kernels form, so |g0| joins the oracle's ``terms``.  dx starts at a sentinel: columns past in_dim come back bit-identical.  Every call
gets a caller-owned workspace filled with NaN and longer than dctr_mlp_bwd_workspace_bytes asks for: the tail must come back untouched
(the two layout computations agree), and finite results within the bar mean nothing unwritten was read.  The requested size is the
larger of the two forms' layouts, so for a chained case the tail is decisive only where the chained layout is the larger one: the small
batches under wide layers, listed by tests/test_mlp_bwd_oracle_cpu.py::test_the_workspace_guard_is_decisive_for_these_chained_cases
(chain-tight-B257 is there for the sliced layout).  At chain-B4097, chain-B8193, chain-rt4 and chain-widest the layered layout is the
larger one, and an overrun of the chained carving by less than the difference would go unseen."""
import functools

import numpy as np
import pytest
import torch

from tests import ref_mlp_bwd as RM
from tests.util import assert_close_terms

pytestmark = pytest.mark.gpu

GUARD = 4096                                # floats behind the requested workspace
SENTINEL = -123.25
CASE = {c.id: c for c in RM.CASES}


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def _reference(case_id, act):
    """Inputs, oracle and g0 of a case, never modified; computed once for the cases that more than one test runs."""
    return _shared_reference(case_id, act) if case_id in ACCUMULATE + DETERMINISTIC else _make_reference(case_id, act)


def _make_reference(case_id, act):
    case = CASE[case_id]
    d = RM.make_data(case, act)
    g, t = RM.oracle(case, d, act)
    rng = np.random.RandomState(len(case_id) + 7 * case.batch)

    def g0_like(ref):                      # the magnitude of what is added to it
        return (rng.standard_normal(ref.shape) * max(float(np.sqrt(np.mean(np.square(ref)))), 1e-3)).astype(np.float32)
    g0 = {"dW": [g0_like(a) for a in g["dW"]], "db": [g0_like(a) for a in g["db"]],
          "d_head_w": None if g["d_head_w"] is None else g0_like(g["d_head_w"])}
    return d, g, t, g0


ACCUMULATE = ("chain-B33", "chain-B513", "layer-B33", "layer-B1024", "layer-N1300-B1024", "headless3-chain-B513", "headless3-layer-B1024")
DETERMINISTIC = ("chain-B257", "chain-B8193", "chain-pad64", "headless3-chain-B513", "nobias-first-chain-B513")
_shared_reference = functools.lru_cache(maxsize=None)(_make_reference)


class Run:
    """One or more identical ops.mlp_bwd calls of a case from g0, a sentinel dx and a NaN workspace with a guard tail."""

    def __init__(self, device, case, act, calls=1, dw_stream=None):
        from deepctr_amd import ops
        self.case, self.act, self.calls = case, act, calls
        d, self.g, self.t, self.g0 = _reference(case.id, act)
        w, B = case.widths, case.batch
        self.x = dev(d["x"], device)
        x_before = bits(self.x)
        ks, acts = [dev(k, device) for k in d["kernels"]], [dev(a, device) for a in d["acts"]]
        hw = dl = dout = self.dhw = None
        if case.head:
            if case.head_offset:
                hw = torch.zeros(w[-1] + 1, device=device)[1:]
                hw.copy_(dev(d["head_w"], device))
                assert hw.data_ptr() % 16 == 4
            else:
                hw = dev(d["head_w"], device)
            dl, self.dhw = dev(d["dlogit"], device), dev(self.g0["d_head_w"], device)
        else:
            dout = dev(d["d_out"], device)[:, :w[-1]]
            assert dout.stride(0) == w[-1] + 2
        self.dk = [dev(a, device) for a in self.g0["dW"]]
        self.db = [dev(a, device) if case.bias[l] else None for l, a in enumerate(self.g0["db"])]
        self.dx = torch.full((B, w[0] + 2), SENTINEL, device=device) if case.dx else None
        need = RM.workspace_bytes(B, list(w))
        assert need % 4 == 0
        self.ws = torch.full((need // 4 + GUARD,), float("nan"), device=device)
        guard_before = bits(self.ws[need // 4:])
        holder = {"ws": self.ws}
        for _ in range(calls):
            ops.mlp_bwd(self.x, w[0], ks, acts, act, hw, dl, self.dk, self.db, self.dhw, dx=self.dx, d_out=dout, dw_stream=dw_stream,
                        workspace=holder)
        if dw_stream is not None:
            torch.cuda.current_stream().wait_stream(dw_stream)
        torch.cuda.synchronize()
        assert holder["ws"] is self.ws, "the op replaced a workspace that was large enough"
        assert (bits(self.ws[need // 4:]) == guard_before).all(), "%s: the op wrote past dctr_mlp_bwd_workspace_bytes()" % self.tag()
        assert (bits(self.x) == x_before).all(), "%s: x (padding included) changed" % self.tag()

    def tag(self):
        return "%s %s" % (self.case.id, self.act)

    def _acc(self, got, g0, ref, terms, what):
        got, g0 = got.cpu().numpy().astype(np.float64), g0.astype(np.float64)
        assert np.isfinite(got).all(), "%s %s: not finite" % (what, self.tag())
        assert_close_terms(got - g0, self.calls * ref, self.calls * terms + np.abs(g0), what="%s %s" % (what, self.tag()))

    def check(self):
        case, L = self.case, len(self.case.widths) - 1
        for l in range(L):
            self._acc(self.dk[l], self.g0["dW"][l], self.g["dW"][l], self.t["dW"][l], "dW%d" % l)
            if case.bias[l]:
                self._acc(self.db[l], self.g0["db"][l], self.g["db"][l], self.t["db"][l], "db%d" % l)
        if case.head:
            self._acc(self.dhw, self.g0["d_head_w"], self.g["d_head_w"], self.t["d_head_w"], "d_head_w")
        if case.dx:
            k0 = case.widths[0]
            got = self.dx[:, :k0].cpu().numpy().astype(np.float64)
            assert np.isfinite(got).all(), "dx %s: not finite" % self.tag()
            assert_close_terms(got, self.g["dx"], self.t["dx"], what="dx " + self.tag())      # written, not accumulated: no factor `calls`
            assert (bits(self.dx[:, k0:]) == bits(torch.full((case.batch, 2), SENTINEL))).all(), "dx %s: columns past in_dim changed" % self.tag()
        return self


@pytest.mark.parametrize("act", RM.ACTS)
@pytest.mark.parametrize("case_id", RM.CASE_IDS)
def test_mlp_bwd_matches_the_float64_oracle(device, case_id, act):
    Run(device, CASE[case_id], act).check()


@pytest.mark.parametrize("act", RM.ACTS)
@pytest.mark.parametrize("case_id", ACCUMULATE)
def test_a_second_call_adds_the_same_gradient_again(device, case_id, act):
    """Gradients are accumulated on both routes: two identical calls leave g0 + 2 x the oracle, within the same bar."""
    Run(device, CASE[case_id], act, calls=2).check()


@pytest.mark.parametrize("act", ("relu", "tanh"))
@pytest.mark.parametrize("case_id", DETERMINISTIC)
def test_the_chained_form_is_deterministic_and_dw_stream_changes_no_bit(device, case_id, act):
    """dW, db and dx of the chained form are sums in a fixed order (row slices + one sum, no atomics): the same bits from the same
    start, and the same bits again with the weight-gradient half on a second stream.  d_head_w goes through atomics: the bar only."""
    case = CASE[case_id]
    assert case.route == "chained"
    a = Run(device, case, act).check()
    b = Run(device, case, act).check()
    c = Run(device, case, act, dw_stream=torch.cuda.Stream(device=device)).check()
    for other, how in ((b, "a second call"), (c, "dw_stream")):
        for l in range(len(case.widths) - 1):
            assert (bits(a.dk[l]) == bits(other.dk[l])).all(), "dW%d differs in %s" % (l, how)
            if case.bias[l]:
                assert (bits(a.db[l]) == bits(other.db[l])).all(), "db%d differs in %s" % (l, how)
        if case.dx:
            assert (bits(a.dx) == bits(other.dx)).all(), "dx differs in %s" % how


@pytest.mark.parametrize("widths", [(13, 8, 5), (1217, 8, 5)])
def test_batch_zero_returns_at_once_and_changes_nothing(device, widths):
    from deepctr_amd import ops
    rng = np.random.RandomState(5)
    L = len(widths) - 1
    x = torch.empty(0, widths[0] + 3, device=device)
    ks = [dev(rng.standard_normal((k, n)).astype(np.float32), device) for k, n in zip(widths[:-1], widths[1:])]
    acts = [torch.empty(0, n, device=device) for n in widths[1:]]
    hw, dl = dev(rng.standard_normal(widths[-1]).astype(np.float32), device), torch.empty(0, device=device)
    dk, db = [torch.full_like(k, 0.5) for k in ks], [torch.full((n,), 0.25, device=device) for n in widths[1:]]
    dhw, dx = torch.full_like(hw, 0.75), torch.full((0, widths[0]), SENTINEL, device=device)
    ws = torch.full((GUARD,), float("nan"), device=device)
    ops.mlp_bwd(x, widths[0], ks, acts, "relu", hw, dl, dk, db, dhw, dx=dx, workspace={"ws": ws})
    torch.cuda.synchronize()
    assert all(float((dk[l] - 0.5).abs().max()) == 0.0 and float((db[l] - 0.25).abs().max()) == 0.0 for l in range(L))
    assert float((dhw - 0.75).abs().max()) == 0.0 and bool(torch.isnan(ws).all())


def test_nine_layers_are_rejected_before_any_launch(device):
    """MAX_LAYERS = 8 (the eight-layer case of the table runs): nine is an argument error of the host, every buffer stays as it was."""
    from deepctr_amd import _C, ops
    rng = np.random.RandomState(6)
    B, widths = 37, [11, 9, 12, 7, 8, 6, 10, 5, 4, 3]
    x = dev(rng.standard_normal((B, widths[0] + 3)).astype(np.float32), device)
    ks = [dev(rng.standard_normal((k, n)).astype(np.float32), device) for k, n in zip(widths[:-1], widths[1:])]
    acts = [dev(rng.rand(B, n).astype(np.float32), device) for n in widths[1:]]
    hw, dl = dev(rng.standard_normal(widths[-1]).astype(np.float32), device), dev(rng.standard_normal(B).astype(np.float32), device)
    dk, db = [torch.full_like(k, 0.5) for k in ks], [torch.full((n,), 0.25, device=device) for n in widths[1:]]
    dhw, dx = torch.full_like(hw, 0.75), torch.full((B, widths[0] + 2), SENTINEL, device=device)
    ws = torch.full((1 << 16,), float("nan"), device=device)
    with pytest.raises(_C.DctrError) as e:
        ops.mlp_bwd(x, widths[0], ks, acts, "relu", hw, dl, dk, db, dhw, dx=dx, workspace={"ws": ws})
    assert e.value.rc == -2                     # DCTR_E_DIM
    torch.cuda.synchronize()
    assert all(float((dk[l] - 0.5).abs().max()) == 0.0 and float((db[l] - 0.25).abs().max()) == 0.0 for l in range(len(ks)))
    assert float((dhw - 0.75).abs().max()) == 0.0 and float((dx - SENTINEL).abs().max()) == 0.0 and bool(torch.isnan(ws).all())


# ---------------------------------------------------------------------------------------------------
# Dice: always layered.  Checker: torch double autograd over tests/ref_dice.py's restatement of Dice.call, at its bar (scaled_close) —
# both shared with tests/test_gpu_din_train.py; widths [12, 6]: the 16-B Dice kernels (N = 12) and the scalar ones (N = 6) both run.
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch_stats", [False, True])
def test_mlp_bwd_dice_accumulates_and_stays_inside_its_workspace(device, batch_stats):
    from deepctr_amd import ops
    from tests.ref_dice import dice_dnn, scaled_close as _scaled
    rng = np.random.RandomState(28 + batch_stats)
    B, K, units = 211, 24, [12, 6]
    dims, L = [K] + units, len(units)
    f32 = lambda a: np.asarray(a, dtype=np.float32)                                            # noqa: E731
    x = f32(rng.standard_normal((B, K + 3)) + 0.3)
    Ws = [f32(rng.standard_normal((dims[i], dims[i + 1])) / np.sqrt(dims[i])) for i in range(L)]
    bs = [f32(rng.standard_normal(n) * 0.5 + (1.0 if batch_stats else 0.0)) for n in units]
    al = [f32(rng.standard_normal(n) * 0.3) for n in units]
    mu = [f32(rng.standard_normal(n) * 0.2) for n in units]
    va = [f32(rng.uniform(0.5, 1.5, n)) for n in units]
    hw, dl = f32(rng.standard_normal((units[-1], 1))), f32(rng.standard_normal(B))
    # checker: float64 autograd on the CPU
    leaves = [torch.tensor(a.astype(np.float64), requires_grad=True) for a in [x] + Ws + bs + al + [hw]]
    xa, Wa, ba, aa, ha = leaves[0], leaves[1:1 + L], leaves[1 + L:1 + 2 * L], leaves[1 + 2 * L:1 + 3 * L], leaves[-1]
    stored = ([torch.tensor(a.astype(np.float64)) for a in mu], [torch.tensor(a.astype(np.float64)) for a in va])
    h, _ = dice_dnn(xa[:, :K], Wa, ba, aa, *((None, None) if batch_stats else stored), eps=1e-9)
    ((h @ ha).reshape(-1) * torch.tensor(dl.astype(np.float64))).sum().backward()
    # HIP forward (saves what the backward reads), then the backward from g0 with a NaN workspace and a guard tail
    xd, Wd, bd, ad = dev(x, device), [dev(a, device) for a in Ws], [dev(a, device) for a in bs], [dev(a, device) for a in al]
    md, vd, hd, dld = [dev(a, device) for a in mu], [dev(a, device) for a in va], dev(hw, device), dev(dl, device)
    acts = [torch.empty(B, n, device=device) for n in units]
    extra = {}
    if batch_stats:
        zs, stats, xin, kin = [torch.empty(B, n, device=device) for n in units], [], xd, K
        for i in range(L):
            ops.mlp(xin, [Wd[i]], [bd[i]], "linear", in_dim=kin, out=zs[i])
            stats.append(ops.dice_train_fwd(zs[i], ad[i], md[i], vd[i], acts[i], eps=1e-9, momentum=0.99))
            xin, kin = acts[i], units[i]
        extra = dict(dice_batch=stats)
    else:
        ops.mlp(xd, Wd, bd, "dice", dice=list(zip(ad, md, vd)), head_w=hd, in_dim=K, out=torch.empty(B, device=device), save_acts=acts)
    g0 = lambda t: dev(f32(rng.standard_normal(tuple(t.shape)) * 0.5), device)                  # noqa: E731
    gW, gb, ga, ghw = [g0(t) for t in Wd], [g0(t) for t in bd], [g0(t) for t in ad], g0(hd)
    start = [t.clone() for t in gW + gb + ga + [ghw]]
    dx = torch.full((B, K + 2), SENTINEL, device=device)
    need = RM.workspace_bytes(B, dims, dice=True)
    ws = torch.full((need // 4 + GUARD,), float("nan"), device=device)
    holder, guard_before = {"ws": ws}, bits(ws[need // 4:])
    ops.mlp_bwd(xd, K, Wd, acts, "dice", hd, dld, gW, gb, ghw, dx=dx, biases=bd, dice=list(zip(ad, md, vd)), d_dice_alpha=ga,
                workspace=holder, **extra)
    torch.cuda.synchronize()
    assert holder["ws"] is ws and (bits(ws[need // 4:]) == guard_before).all(), "the op wrote past dctr_mlp_bwd_workspace_bytes()"
    added = [(t.double() - s.double()).cpu() for t, s in zip(gW + gb + ga + [ghw], start)]
    assert all(bool(torch.isfinite(t).all()) for t in added) and bool(torch.isfinite(dx).all())
    _scaled(dx[:, :K].double(), xa.grad[:, :K], "dx")
    assert (bits(dx[:, K:]) == bits(torch.full((B, 2), SENTINEL))).all()
    for i in range(L):
        _scaled(added[i], Wa[i].grad, "dW%d" % i)
        # (with batch statistics d loss / d bias cancels to ~0 through the batch mean: the absolute floor of the test this restates)
        _scaled(added[L + i], ba[i].grad, "db%d" % i, **(dict(atol=2e-5) if batch_stats else {}))
        _scaled(added[2 * L + i], aa[i].grad, "dalpha%d" % i)
    _scaled(added[3 * L], ha.grad, "dhead")
