"""GPU parity tests, op level, of dctr_cin_bwd (deepctr_amd/csrc/cin_layered_kernels.hip) on every route of its two MFMA kernels
(deepctr_amd/csrc/cin_bwd_kernels.hip: cin_dz_fused_kernel<KS>, cin_dw_fused_kernel<TW, NH, XK4>) and on the GEMM route, against the
float64 oracle of tests/ref_cin_bwd.py.  The oracle restates the op's contract (act' and x_k from the SAVED layer outputs) and is pinned
without a GPU by tests/test_cin_bwd_oracle_cpu.py, together with the route every case of the table takes; here the table is resolved
again with the device's CU count (the slices-* cases choose their rows from it) and a case that no longer reaches its route FAILS.

Bar: tests.util.assert_close_terms' defaults — 1e-4 of the result plus 2e-6 of the summed magnitude — for every case; none needed a bar
of its own (slices-3, the longest reduction: 8,193 rows at 256 CUs).  The op ACCUMULATES into d_filters / d_biases, so each starts at a
random non-zero g0 of the result's magnitude and ``g - g0`` is compared; g0 is one more summand of the fp32 sum, so |g0| joins the
oracle's ``terms``.  dx is exercised written, accumulated onto a sentinel and absent, on a row stride wider than F0*D: the columns past
F0*D come back bit-identical, x unchanged.  Every call gets a caller-owned workspace filled with NaN and longer than the restated
dctr_cin_bwd_workspace_bytes, which must equal the library's at this device's CU count: the op must keep it, the tail must come
back untouched, and finite results within the bar mean nothing unwritten was read (dxk, the dW slices, the y slots of the re-run).

On the kernels as they were before the dpre staging covered the tile for every H (a row step of 256 / (H/4) per element: rows 60..63
of every 64-row block partly unstaged at H = 48, 80, 96, 112) every case with such a layer and more than 60 rows failed here, 74 of the
table's 131, by 115 to 6.8e7 x the bar; rows-1 and rows-15, whose blocks end before row 60, and every other case passed.

The saved outputs come from ops.cin(save_y=) once per case; the oracle is computed once per case from those very values and never
modified."""
import functools

import numpy as np
import pytest
import torch

from tests import ref_cin_bwd as RC
from tests.util import assert_close_terms

pytestmark = pytest.mark.gpu

GUARD = 4096                                # floats behind the restated workspace size
SENTINEL = 0.75                             # what dx holds before the call: of the gradient's magnitude, so that accumulating onto it costs no bar
CASE = {c.id: c for c in RC.CASES}


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


@functools.lru_cache(maxsize=None)
def _reference(case_id, device):
    """Resolved case, routes, inputs, the forward kernel's saved outputs, oracle and g0 of a case: computed once, never modified."""
    from deepctr_amd import ops
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    case, rt = RC.resolve(CASE[case_id], cus)
    d = RC.make_data(case)
    sy = [torch.full((case.B * case.D, h), float("nan"), device=device) for h in case.layers]
    ops.cin(dev(d["x"], device), [dev(f, device) for f in d["filters"]], [dev(b, device) for b in d["biases"]], list(case.layers),
            case.split, case.act, fields=case.F0, dim=case.D, save_y=sy)
    sy = [t.cpu().numpy() for t in sy]
    for k, (got, ref) in enumerate(zip(sy, d["ys"])):           # the forward is not under test here: only that the oracle's input is sane
        assert np.isfinite(got).all() and (np.abs(got - ref) <= 2e-4 * np.abs(ref) + 2e-5).all(), "%s: saved y%d" % (case_id, k)
    g, t = RC.oracle(case, d, ys=sy)
    rng = np.random.RandomState(len(case_id) + 7 * case.B)

    def g0_like(ref):                      # the magnitude of what is added to it
        return (rng.standard_normal(ref.shape) * max(float(np.sqrt(np.mean(np.square(ref)))), 1e-3)).astype(np.float32)
    g0 = {"dW": [g0_like(a) for a in g["dW"]], "db": [g0_like(a) for a in g["db"]]}
    lib_need, fwd_ws = RC.library_bytes(case.B, case.F0, case.D, case.layers, case.split)
    need = 4 * RC.workspace_floats(case.B, case.F0, case.D, case.layers, case.split, fwd_ws, cus)
    assert lib_need == need, "%s: the restated routes do not give the library's workspace size at %d CUs" % (case_id, cus)
    return case, rt, d, sy, g, t, g0, need


class Run:
    """``calls`` identical ops.cin_bwd calls of a case from g0 and a sentinel dx, with a NaN workspace and a guard tail.
    dx_mode: "write", "add" (accumulate onto the sentinel) or None (no dx)."""

    def __init__(self, device, case_id, saved, dx_mode, calls=1):
        from deepctr_amd import ops
        self.case, self.rt, d, sy, self.g, self.t, self.g0, need = _reference(case_id, device)
        case = self.case
        self.saved, self.dx_mode, self.calls = saved, dx_mode, calls
        self.n = case.F0 * case.D
        self.x = dev(d["x"], device)
        assert self.x.stride(0) == self.n + 5
        x_before = bits(self.x)
        fs, bs = [dev(f, device) for f in d["filters"]], [dev(b, device) for b in d["biases"]]
        self.dW, self.db = [dev(a, device) for a in self.g0["dW"]], [dev(a, device) for a in self.g0["db"]]
        self.dx = torch.full((case.B, self.n + 2), SENTINEL, device=device) if dx_mode else None
        self.ws = torch.full((need // 4 + GUARD,), float("nan"), device=device)
        guard_before = bits(self.ws[need // 4:])
        holder = {"ws": self.ws}
        for _ in range(calls):
            ops.cin_bwd(self.x, fs, bs, list(case.layers), case.split, case.act, dev(d["d_out"], device), self.dW, self.db, dx=self.dx,
                        accumulate=dx_mode == "add", fields=case.F0, dim=case.D, saved_y=[dev(y, device) for y in sy] if saved else None,
                        workspace=holder)
        torch.cuda.synchronize()
        assert holder["ws"] is self.ws, "%s: dctr_cin_bwd_workspace_bytes() asks for more than the restated size" % self.tag()
        assert (bits(self.ws[need // 4:]) == guard_before).all(), "%s: the op wrote past dctr_cin_bwd_workspace_bytes()" % self.tag()
        assert (bits(self.x) == x_before).all(), "%s: x (padding included) changed" % self.tag()

    def tag(self):
        return "%s %s dx=%s" % (self.case.id, "saved_y" if self.saved else "re-run", self.dx_mode)

    def _acc(self, got, g0, ref, terms, what):
        got, g0 = got.cpu().numpy().astype(np.float64), g0.astype(np.float64)
        assert np.isfinite(got).all(), "%s %s: not finite" % (what, self.tag())
        assert_close_terms(got - g0, self.calls * ref, self.calls * terms + np.abs(g0), what="%s %s" % (what, self.tag()))

    def check(self):
        for k in range(len(self.case.layers)):
            self._acc(self.dW[k], self.g0["dW"][k], self.g["dW"][k], self.t["dW"][k], "dW%d" % k)
            self._acc(self.db[k], self.g0["db"][k], self.g["db"][k], self.t["db"][k], "db%d" % k)
        if self.dx_mode:
            got = self.dx[:, :self.n].cpu().numpy().astype(np.float64)
            assert np.isfinite(got).all(), "dx %s: not finite" % self.tag()
            if self.dx_mode == "add":
                assert_close_terms(got - SENTINEL, self.calls * self.g["dx"], self.calls * self.t["dx"] + SENTINEL, what="dx " + self.tag())
            else:                                                            # written: no factor `calls`
                assert_close_terms(got, self.g["dx"], self.t["dx"], what="dx " + self.tag())
            assert (bits(self.dx[:, self.n:]) == bits(torch.full((self.case.B, 2), SENTINEL))).all(), "dx %s: columns past F0*D changed" % self.tag()
        return self


@pytest.mark.parametrize("saved", [True, False], ids=["saved_y", "rerun"])
@pytest.mark.parametrize("case_id", RC.CASE_IDS)
def test_cin_bwd_matches_the_float64_oracle(device, case_id, saved):
    for dx_mode in ("write", "add", None):
        Run(device, case_id, saved, dx_mode).check()


# one case per dW ending and per kind of hand-over, two of them with long reductions
REPEATED = ("det-tpi2", "det-F2", "hole-H96-ks6-R135-F26", "tpi-3-Fk48-F5-split", "tpi-4-Fk64-F32-whole", "mixed-nf-f-f", "mixed-f-nf-f",
            "nonfused-R131-gemm1", "nonfused-R135-batched", "slices-2")


@pytest.mark.parametrize("case_id", REPEATED)
def test_a_second_call_from_the_same_start(device, case_id):
    """Two separate identical calls from the same g0, and one run of two calls in a row (the gradients accumulate: g0 + 2 x the oracle,
    dx accumulated twice), all within the bar.  Equal BITS are asserted where the sums have a fixed order, which
    tests.ref_cin_bwd.bit_reproducible derives from the kernels (its docstring has the reading).  In short: the dz kernel's LDS float
    atomics make dxk / dx0 of a layer order-dependent unless no element receives more than two adds (TPI = 2, or TPI = 1 with at most
    two fields), and everything below such a layer inherits it through dpre.  Where the layers above are reproducible,
      dW of a fused layer is — launch_sum_parts adds the slices' partial products, which the dW kernel stored without atomics, in index
        order onto d_filters; the batched-GEMM ending goes through the same sum but its partial products through dctr_gemm, and the
        single GEMM with beta = 1 through dctr_gemm alone, whose K split adds with float atomics: the bar only;
      db is where the column-sum pass is ONE workgroup (several leave with one float atomic each onto d_bias).
    det-tpi2 and det-F2 are in the table for this: everything holds there.  (Observed on an MI355X: dW1 of mixed-nf-f-f and dW0 of
    mixed-f-nf-f, both below a TPI = 1 layer of seven fields, do differ between two calls.)"""
    a = Run(device, case_id, True, "write").check()
    b = Run(device, case_id, True, "write").check()
    Run(device, case_id, True, "add", calls=2).check()
    dx_ok, db_ok, dw_ok = RC.bit_reproducible(a.case.F0, a.rt, a.case.B * a.case.D)
    if case_id.startswith("det-"):
        assert dx_ok and all(db_ok) and all(dw_ok)
    for k in range(len(a.case.layers)):
        if dw_ok[k]:
            assert (bits(a.dW[k]) == bits(b.dW[k])).all(), "dW%d differs in a second call" % k
        if db_ok[k]:
            assert (bits(a.db[k]) == bits(b.db[k])).all(), "db%d differs in a second call" % k
    if dx_ok:
        assert (bits(a.dx) == bits(b.dx)).all(), "dx differs in a second call"


def test_the_workspace_holder_is_filled_kept_and_replaced_when_too_small(device):
    """ops.cin_bwd(workspace=): an empty holder receives a tensor of the library's size, a large enough one is kept, a smaller one is
    replaced; the results do not depend on which."""
    from deepctr_amd import ops
    case, rt, d, sy, g, t, g0, need = _reference("det-tpi2", device)
    outs = []
    for holder in ({}, None, {"ws": torch.empty(3, device=device)}):
        dW, db = [dev(a, device) for a in g0["dW"]], [dev(a, device) for a in g0["db"]]
        ops.cin_bwd(dev(d["x"], device), [dev(f, device) for f in d["filters"]], [dev(b, device) for b in d["biases"]], list(case.layers),
                    case.split, case.act, dev(d["d_out"], device), dW, db, fields=case.F0, dim=case.D, workspace=holder)
        if holder is not None:
            assert holder["ws"].numel() * 4 == need and holder["ws"].dtype == torch.float32
            kept = holder["ws"]
            ops.cin_bwd(dev(d["x"], device), [dev(f, device) for f in d["filters"]], [dev(b, device) for b in d["biases"]],
                        list(case.layers), case.split, case.act, dev(d["d_out"], device), [w.clone() for w in dW], [b.clone() for b in db],
                        fields=case.F0, dim=case.D, workspace=holder)
            assert holder["ws"] is kept
        outs.append([bits(w) for w in dW])
    assert all((a == b).all() for o in outs[1:] for a, b in zip(outs[0], o))
