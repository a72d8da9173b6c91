"""GPU parity tests, op level, of the backward ops between dctr_mlp_bwd and the embedding scatter in NFM, PNN, AFM, DCN and DCNMix —
dctr_bi_interaction_bwd, dctr_inner_product_bwd, dctr_afm_bwd (deepctr_amd/csrc/interaction_bwd_kernels.hip), dctr_crossnet_bwd in its
three forms and dctr_crossnet_mix_bwd (deepctr_amd/csrc/crossnet_bwd_kernels.hip) — against the float64 oracles of
tests/ref_interaction_bwd.py, on every route of the table there.  The oracles, the routes and the room the bar leaves are pinned
without a GPU by tests/test_interaction_bwd_oracle_cpu.py; here every case is resolved again and one that no longer reaches its route
FAILS.

Bar: tests.util.assert_close_terms' defaults — 1e-4 of the result plus 2e-6 of the summed magnitude — for every case; none has a bar of
its own.  On the non-negative data of the inner product and the CrossNet nothing cancels, ``terms`` is |ref| and the comparison is the
literal 1e-4 relative bar (the bi-interaction's contract is the difference sum_f' x - x_f: its terms exceed |ref| there too).
Measured, for judging a later change of a bar — worst err / bar per op and kind of data (signed | non-negative):
                                                          bi             ip              afm     vec             mat             mix
  float32 torch autograd on the CPU against the oracle    0.036 | 0.034  0.036 | 0.0039  0.072   0.044 | 0.0092  0.14 | 0.0080   0.078
  (tests/test_interaction_bwd_oracle_cpu.py -s)
  these tests on an MI355X                                0.033 | 0.020  0.025 | 0.017   0.089   0.026 | 0.014   0.13 | 0.019    0.081
  compared elements outside 1e-4 |ref| alone, percent     0.054 | 0.054  0.0099 | 0      5.8     0.16 | 0       0.19 | 0        0.16
  (what tests.util.TERMS_REPORT counts: how much of the comparison leaned on the 2e-6 term)
(afm's 5.8 % is the accumulated dx of afm-5x62x64x8, 30 % of its elements: a gradient of 1e-3 added onto the sentinel 0.75.)
The worst GPU cases: mat-130x300x3-signed recompute, dk (0.13); afm-9x30x64x4-signed, dx (0.089); mix-300x429x2x4x32-signed, dU (0.081).

Weight gradients ACCUMULATE, so each starts at a random non-zero g0 of the result's magnitude and ``g - g0`` is compared, |g0| added to
``terms``.  dx is exercised written onto a sentinel and accumulated onto it; x, dy and dx sit on row strides 3, 1 and 2 wider than the
row: the padding of dx comes back bit-identical, x, dy and the weights unchanged.  dctr_crossnet_bwd and dctr_crossnet_mix_bwd get a
caller-owned workspace filled with NaN with a guard tail behind the restated size: the op must keep it, the guard must come back
untouched, and finite results within the bar mean nothing unwritten was read.  The matrix form's saved_u / saved_x are the oracle's own
u_l / x_l rounded to float32, so the backward is tested by itself.  Shapes an op refuses raise its documented error and leave every
output bit-identical.

The two model-level tests at the end are for a gap the table's refused rows led to: training_hip.supported() said yes to an AFM past
160 KiB of backward LDS and to a DCNMix with more than 16 experts, and fit() raised in the middle of the first step.  Both tests were
run once on an MI355X against the Python tree of the commit before dctr_afm_bwd_supported / dctr_crossnet_mix_bwd_supported and failed
there with the op's refusal (MEASURED_BAR["parent"]).  No op-level case failed: the kernels are that commit's, the change in the two
.hip files is the host predicate each op now shares with its dry check."""
import functools

import numpy as np
import pytest
import torch

from tests import ref_interaction_bwd as R
from tests.util import assert_close_terms

pytestmark = pytest.mark.gpu

# what the two model-level tests did on the parent commit's Python tree
MEASURED_BAR = {"parent": {
    "test_an_afm_past_the_backward_lds_trains_on_the_autograd_step": "DctrError: dctr_afm_bwd failed (rc=-5): afm_bwd: needs 165008 B of LDS",
    "test_a_dcnmix_with_17_experts_trains_on_the_autograd_step":
        "DctrError: dctr_crossnet_mix_bwd failed (rc=-2): crossnet_mix_bwd: bad sizes (batch=64 dim=13 layers=2 experts=17 (max 16) low_rank=2)"}}

GUARD = 4096                                # floats behind the restated workspace size
SENTINEL = 0.75                             # what dx holds before the call: of the gradient's magnitude
PAD_X, PAD_DY, PAD_DX = 3, 1, 2
CASE = {c.id: c for c in R.CASES}
E_DIM, E_UNSUPPORTED = -2, -5               # include/dctr.h


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def padded(a, pad, device, fill=-3.5):
    """[B, n + pad] device buffer with ``a`` (anything [B, ...]) in its first n columns."""
    a = np.asarray(a, dtype=np.float32).reshape(a.shape[0], -1)
    buf = np.full((a.shape[0], a.shape[1] + pad), fill, dtype=np.float32)
    buf[:, :a.shape[1]] = a
    return dev(buf, device)


@functools.lru_cache(maxsize=None)
def _reference(case_id):
    """Case, resolved routes, inputs, oracle and g0 of a case: computed once, never modified."""
    case = CASE[case_id]
    info = R.resolve(case)
    d = R.make_data(case)
    g, t = R.oracle(case, d)
    rng = np.random.RandomState(len(case_id) + 7 * case.shape[0])
    g0 = {k: (rng.standard_normal(g[k].shape) * max(float(np.sqrt(np.mean(np.square(g[k])))) if g[k].size else 0.0, 1e-3)).astype(np.float32)
          for k in R.WEIGHT_GRADS[case.op] if g.get(k) is not None}
    return case, info, d, g, t, g0


class Run:
    """``calls`` identical calls of a case's op from g0 and a sentinel dx.  dx_mode: "write" or "add" (accumulate onto the sentinel);
    mode: a matrix case's "recompute" / "saved".  ``refused``: the call must raise DctrError with that code and change nothing."""

    def __init__(self, device, case_id, dx_mode, calls=1, mode=None, refused=None):
        from deepctr_amd import _C, ops
        self.case, self.info, d, self.g, self.t, self.g0 = _reference(case_id)
        case, self.dx_mode, self.calls, self.mode = self.case, dx_mode, calls, mode
        op, s = case.op, case.shape
        self.n = n = int(np.prod(d["x"].shape[1:]))
        x, dx = padded(d["x"], PAD_X, device), torch.full((s[0], n + PAD_DX), SENTINEL, device=device)
        dy = dev(d["dy"], device) if op == "afm" else padded(d["dy"], PAD_DY, device)
        assert (x.stride(0), dx.stride(0)) == (n + PAD_X, n + PAD_DX) or s[0] == 1
        wnames = {"afm": ("W", "b", "h", "p"), "vec": ("kernels", "bias"), "mat": ("kernels", "bias"), "mix": ("U", "V", "C", "G", "bias")}.get(op, ())
        w = [None if d[k] is None else dev(d[k], device) for k in wnames]
        self.grads = {k: dev(a, device) for k, a in self.g0.items()}                  # (none at L = 0 of the CrossNet)
        gl = [self.grads.get(k) for k in R.WEIGHT_GRADS[op]]
        self.dx, holder, self.ws = dx, None, None
        if op in ("vec", "mat", "mix"):
            need = self.info["ws_bytes"]
            lib = (R.library_mix_ws_bytes(*s) if s[2] else need) if op == "mix" else R.library_crossnet_ws_bytes("vector" if op == "vec" else "matrix", *s)
            assert lib == need or refused, "%s: the restated workspace size is not the library's" % self.tag()
            self.ws = torch.full((need // 4 + GUARD,), float("nan"), device=device)
            holder = {"ws": self.ws}
        saved_u = saved_x = None
        if mode == "saved":
            su, sx = R.saved_for_matrix(d)
            saved_u, saved_x = dev(su, device), None if sx is None else dev(sx, device)
        keep = [(t_, bits(t_)) for t_ in [x, dy] + [t_ for t_ in w if t_ is not None] + ([saved_u] if saved_u is not None else [])]
        acc = dx_mode == "add"

        def call():
            if op == "bi":
                ops.bi_interaction_bwd(x, s[1], s[2], dy, dx, accumulate=acc)
            elif op == "ip":
                ops.inner_product_bwd(x, s[1], s[2], dy, dx, accumulate=acc)
            elif op == "afm":
                ops.afm_bwd(x, s[1], s[2], w[0], w[1], w[2], w[3], dy, dx, *gl, accumulate=acc)
            elif op == "mix":
                ops.crossnet_mix_bwd(x, s[1], w, dy, gl, dx, accumulate=acc, workspace=holder)
            else:
                ops.crossnet_bwd(x, s[1], w[0], w[1], "vector" if op == "vec" else "matrix", dy, gl[0], gl[1], dx,
                                 accumulate=acc, saved_u=saved_u, saved_x=saved_x, workspace=holder)
        if refused is not None:
            before = [bits(dx)] + [bits(t_) for t_ in gl]                               # (refused: afm and mix, every gradient present)
            with pytest.raises(_C.DctrError) as err:
                call()
            torch.cuda.synchronize()
            assert err.value.rc == refused, "%s: rc %r" % (self.tag(), err.value.rc)
            assert all((a == bits(t_)).all() for a, t_ in zip(before, [dx] + gl)), "%s: a refused call changed an output" % self.tag()
        else:
            for _ in range(calls):
                call()
            torch.cuda.synchronize()
        if holder is not None:
            assert holder["ws"] is self.ws, "%s: the library asks for more workspace than the restated size" % self.tag()
            tail = bits(self.ws[self.info["ws_bytes"] // 4:])
            assert (tail == bits(torch.full((GUARD,), float("nan")))).all(), "%s: the op wrote past its workspace size" % self.tag()
        for t_, b in keep:
            assert (bits(t_) == b).all(), "%s: an input (padding included) changed" % self.tag()

    def tag(self):
        return "%s%s dx=%s" % (self.case.id, " " + self.mode if self.mode else "", self.dx_mode)

    def check(self):
        for k in self.grads:
            if not self.g[k].size:
                continue
            got, g0 = self.grads[k].cpu().numpy().astype(np.float64).reshape(self.g[k].shape), self.g0[k].astype(np.float64)
            assert np.isfinite(got).all(), "%s %s: not finite" % (self.tag(), k)
            assert_close_terms(got - g0, self.calls * self.g[k], self.calls * self.t[k] + np.abs(g0), what="%s %s" % (self.tag(), k))
        got = self.dx[:, :self.n].cpu().numpy().astype(np.float64)
        ref, terms = self.g["dx"].reshape(got.shape), self.t["dx"].reshape(got.shape)
        assert np.isfinite(got).all(), "%s dx: not finite" % self.tag()
        if self.dx_mode == "add":
            assert_close_terms(got - SENTINEL, self.calls * ref, self.calls * terms + SENTINEL, what="%s dx" % self.tag())
        else:                                                               # written: no factor `calls`
            assert_close_terms(got, ref, terms, what="%s dx" % self.tag())
        assert (bits(self.dx[:, self.n:]) == bits(torch.full((self.case.shape[0], PAD_DX), SENTINEL))).all(), "%s: dx padding changed" % self.tag()
        return self


def _variants():
    out = []
    for c in R.CASES:
        for mode in (R.MATRIX_MODES if c.op == "mat" else (None,)):
            out.append(pytest.param(c.id, mode, id=c.id + ("-" + mode if mode else "")))
    return out


@pytest.mark.parametrize("case_id,mode", _variants())
def test_the_op_matches_the_float64_oracle(device, case_id, mode):
    case = CASE[case_id]
    assert R.resolve(case)["route"] == case.route
    if case.route == "refused":
        Run(device, case_id, "write", refused=E_UNSUPPORTED if case.op == "afm" else E_DIM)
        return
    for dx_mode in ("write", "add"):
        Run(device, case_id, dx_mode, mode=mode).check()


# one case per op and form
TWICE = (("bi-70x26x16-signed", None), ("ip-70x26x16-signed", None), ("afm-70x26x16x8-signed", None), ("vec-70x429x2-signed", None),
         ("vec-19x1138x3-signed", None), ("mat-1030x12x2-signed", "recompute"), ("mat-37x45x2-signed", "saved"), ("mix-70x45x3x2x4-signed", None))


@pytest.mark.parametrize("case_id,mode", TWICE, ids=[c + ("-" + m if m else "") for c, m in TWICE])
def test_two_identical_calls_accumulate_twice_the_gradient(device, case_id, mode):
    """Two calls in a row into the same gradients and, accumulating, the same dx: g0 + 2 x the oracle and the sentinel + 2 x the oracle."""
    Run(device, case_id, "add", calls=2, mode=mode).check()


def test_inner_product_bwd_with_dy_a_column_slice_of_the_dx_buffer(device):
    """As models/pnn.py calls it: dy is the columns of the DNN step's dx behind the embeddings, dx the same buffer, accumulated."""
    from deepctr_amd import ops
    case, info, d, g, t, _ = _reference("ip-70x26x16-signed")
    B, F, E = case.shape
    n, P = F * E, F * (F - 1) // 2
    host = np.full((B, n + 5 + P + 1), SENTINEL, dtype=np.float32)
    host[:, n + 5:n + 5 + P] = d["dy"]
    buf, x = dev(host, device), padded(d["x"], PAD_X, device)
    ops.inner_product_bwd(x, F, E, buf[:, n + 5:], buf, accumulate=True)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:, n:].view(np.int32) == host[:, n:].view(np.int32)).all(), "columns behind the embeddings changed"
    assert_close_terms(got[:, :n].astype(np.float64) - SENTINEL, g["dx"].reshape(B, n), t["dx"].reshape(B, n) + SENTINEL, what="ip dy-in-dx dx")


def test_the_workspace_holders_are_filled_kept_and_replaced_when_too_small(device):
    """ops.crossnet_bwd / ops.crossnet_mix_bwd(workspace=): an empty holder receives a tensor of the library's size, a large enough one
    is kept, a smaller one is replaced; without a holder a fresh tensor per call, as before."""
    for case_id, mode in (("mat-37x45x2-signed", "recompute"), ("mix-70x45x3x2x4-signed", None)):
        from deepctr_amd import ops
        case, info, d, g, t, g0 = _reference(case_id)
        s = case.shape
        names = ("kernels", "bias") if case.op == "mat" else ("U", "V", "C", "G", "bias")
        x, dy, w = dev(d["x"], device), dev(d["dy"], device), [dev(d[k], device) for k in names]
        outs = []
        for holder in ({}, None, {"ws": torch.empty(3, device=device)}):
            for _ in range(2):
                gl, dx = [dev(g0[k], device) for k in R.WEIGHT_GRADS[case.op]], torch.empty(s[0], s[1], device=device)
                if case.op == "mat":
                    ops.crossnet_bwd(x, s[1], w[0], w[1], "matrix", dy, gl[0], gl[1], dx, workspace=holder)
                else:
                    ops.crossnet_mix_bwd(x, s[1], w, dy, gl, dx, workspace=holder)
                if holder is not None:
                    assert holder["ws"].numel() * 4 == info["ws_bytes"] and holder["ws"].dtype == torch.float32
                    kept = holder.setdefault("kept", holder["ws"])
                    assert holder["ws"] is kept
            outs.append(dx.cpu().numpy())
        for o in outs[1:]:
            assert_close_terms(o, g["dx"], t["dx"], what="%s dx with a holder" % case_id)


def _fit_one_epoch(model, cols, device):
    from deepctr_amd.training_hip import supported
    from tests.test_gpu_train import _feed
    rng = np.random.RandomState(5)
    feed = _feed(rng, cols, 128)
    y = (rng.rand(128) > 0.5).astype(np.float32)
    model.compile("adam", "binary_crossentropy")
    h = model.fit(feed, y, batch_size=64, epochs=1, verbose=0)                        # must not raise
    assert np.isfinite(h.history["loss"]).all()
    assert (getattr(model, "_hip_trainer", None) is not None) == supported(model)
    return supported(model)


def test_an_afm_past_the_backward_lds_trains_on_the_autograd_step(device):
    """63 fields of embedding_dim 64 with attention_factor 8: dctr_afm_fwd streams it, dctr_afm_bwd needs 165,008 B of LDS and refuses.
    supported() must say so (dctr_afm_bwd_supported) and fit() take the autograd step.  Before the dry check: fit() raised
    DCTR_E_UNSUPPORTED out of dctr_afm_bwd."""
    from deepctr_amd.feature_column import SparseFeat
    from deepctr_amd.models import AFM
    cols = [SparseFeat("C%d" % i, 10, 64) for i in range(63)]
    model = AFM(cols, cols, attention_factor=8, device=device)
    assert not _fit_one_epoch(model, cols, device)
    small = [SparseFeat("C%d" % i, 10, 8) for i in range(5)]
    assert _fit_one_epoch(AFM(small, small, attention_factor=8, device=device), small, device)      # and the HIP step where the op takes it


def test_a_dcnmix_with_17_experts_trains_on_the_autograd_step(device):
    """num_experts = 17: dctr_crossnet_mix_fwd takes it, dctr_crossnet_mix_bwd keeps a row's gate in 16 registers and answers
    DCTR_E_DIM.  supported() must say so (dctr_crossnet_mix_bwd_supported).  Before the dry check: fit() raised out of dctr_crossnet_mix_bwd."""
    from deepctr_amd.feature_column import DenseFeat, SparseFeat
    from deepctr_amd.models import DCNMix
    cols = [SparseFeat("C%d" % i, 10, 4) for i in range(3)] + [DenseFeat("I0", 1)]
    assert not _fit_one_epoch(DCNMix(cols, cols, cross_num=2, dnn_hidden_units=(8,), low_rank=2, num_experts=17, device=device), cols, device)
    assert _fit_one_epoch(DCNMix(cols, cols, cross_num=2, dnn_hidden_units=(8,), low_rank=2, num_experts=16, device=device), cols, device)
