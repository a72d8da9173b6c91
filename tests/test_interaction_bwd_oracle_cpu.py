"""Pins, without a GPU, what tests/test_gpu_interaction_bwd.py checks the interaction and CrossNet backward ops against
(tests/ref_interaction_bwd.py):
  * every oracle against torch float64 autograd over the differentiable restatement of the reference layer (the ones of
    tests/test_gpu_train.py and models/*._autograd_*), on every case of the table, to 1e-12 of each gradient's largest element;
  * that tests.util.assert_close_terms' default bar leaves room: torch FLOAT32 autograd on the CPU, whose sums run in another order
    than any kernel's, stays within half of it on every case;
  * that the bar can fail: a restatement that leaves one summand out of one reduction misses it;
  * the restated routes and workspace sizes against the table and against the library's host-only calls, AFM's ReLU margin, and the two
    dry checks ops.afm_bwd_supported / ops.crossnet_mix_bwd_supported at their limits.
Run with -s for the worst float32 err / bar per op; tests/test_gpu_interaction_bwd.py quotes them."""
import functools

import numpy as np
import pytest
import torch

from tests import ref_interaction_bwd as R

CASE = {c.id: c for c in R.CASES}
WORST32 = {}


@functools.lru_cache(maxsize=None)
def _reference(case_id):
    case = CASE[case_id]
    info = R.resolve(case)
    d = R.make_data(case)
    g, t = R.oracle(case, d)
    return case, info, d, g, t


def _ratio(got, ref, terms):
    """Worst error in units of tests.util.assert_close_terms' default bar."""
    return float((np.abs(got - ref) / (1e-4 * np.abs(ref) + 2e-6 * np.abs(terms) + 1e-30)).max()) if ref.size else 0.0


def autograd(case, d, dtype):
    """The gradients of a case by torch autograd over the reference layer's arithmetic in ``dtype``, as float64 NumPy, keyed as the oracle."""
    T = lambda a: torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True)          # noqa: E731
    C = lambda a: torch.tensor(np.asarray(a), dtype=dtype)                             # noqa: E731
    out = lambda **kw: {k: (None if v is None else v.grad.double().numpy()) for k, v in kw.items()}     # noqa: E731
    x, dy = T(d["x"]), C(d["dy"])
    if case.op == "bi":
        (0.5 * (x.sum(1).pow(2) - (x * x).sum(1)) * dy).sum().backward()
        return out(dx=x)
    if case.op == "ip":
        ii, jj = (torch.tensor(a) for a in R.pair_indices(case.shape[1]))
        ((x[:, ii] * x[:, jj]).sum(-1) * dy).sum().backward()
        return out(dx=x)
    if case.op == "afm":                                                                # interaction.py:116-146
        W, b, h, p = T(d["W"]), T(d["b"]), T(d["h"]), T(d["p"])
        ii, jj = (torch.tensor(a) for a in R.pair_indices(case.shape[1]))
        bi = x[:, ii] * x[:, jj]
        score = torch.softmax(torch.relu(bi @ W + b) @ h, dim=1)
        (((score * bi).sum(1) @ p).reshape(-1) * dy).sum().backward()
        return out(dx=x, dW=W, db=b, dh=h, dp=p)
    if case.op in ("vec", "mat"):                                                       # interaction.py:405-424
        L = case.shape[2]
        k, b = (T(d["kernels"]), T(d["bias"])) if L else (None, None)
        xl = x
        for l in range(L):
            xl = x * (xl @ k[l]).unsqueeze(1) + b[l] + xl if case.op == "vec" else x * (xl @ k[l].T + b[l]) + xl
        (xl * dy).sum().backward()
        return out(dx=x, dk=k, db=b)
    U, V, Cc, G, b = T(d["U"]), T(d["V"]), T(d["C"]), T(d["G"]), T(d["bias"])           # interaction.py:511-549
    L, ne = case.shape[2], case.shape[3]
    xl = x
    for l in range(L):
        gate = torch.softmax(xl @ G.T, dim=-1)
        moe = torch.zeros_like(xl)
        for e in range(ne):
            v = torch.tanh(torch.tanh(xl @ V[l, e]) @ Cc[l, e].T)
            moe = moe + gate[:, e:e + 1] * (x * (v @ U[l, e].T + b[l]))
        xl = moe + xl
    (xl * dy).sum().backward()
    if L == 0:
        return dict(dx=x.grad.double().numpy(), **{k: np.zeros_like(d[n], dtype=np.float64) for k, n in
                                                  (("dU", "U"), ("dV", "V"), ("dC", "C"), ("dG", "G"), ("db", "bias"))})
    return out(dx=x, dU=U, dV=V, dC=Cc, dG=G, db=b)


def _keys(case, g):
    return [k for k in ("dx",) + R.WEIGHT_GRADS[case.op] if g.get(k) is not None and g[k].size]


@pytest.mark.parametrize("case_id", R.CASE_IDS)
def test_the_oracle_matches_double_autograd_and_float32_keeps_half_the_bar(case_id):
    case, info, d, g, t = _reference(case_id)
    a64 = autograd(case, d, torch.float64)
    for k in _keys(case, g):
        ref = a64[k].reshape(g[k].shape)
        assert np.abs(g[k] - ref).max() <= 1e-12 * np.abs(ref).max() + 1e-300, \
            "%s %s: %.3g of %.3g" % (case_id, k, np.abs(g[k] - ref).max(), np.abs(ref).max())
        assert (np.abs(g[k]) <= t[k] * (1 + 1e-12) + 1e-300).all(), "%s %s: terms below the value" % (case_id, k)
        if case.data == "nonneg" and case.op in ("ip", "vec", "mat"):      # nothing cancels: the bar is the literal 1e-4 relative one
            assert np.abs(t[k] - np.abs(g[k])).max() <= 1e-12 * np.abs(g[k]).max(), "%s %s: terms != |ref|" % (case_id, k)
    a32 = autograd(case, d, torch.float32)
    worst = {k: _ratio(a32[k].reshape(g[k].shape), g[k], t[k]) for k in _keys(case, g)}
    print("%s float32 autograd, err / bar: %s" % (case_id, "  ".join("%s %.3g" % kv for kv in worst.items())))
    w = max(worst.values())
    WORST32[case.op, case.data] = max(WORST32.get((case.op, case.data), 0.0), w)
    assert w <= 0.5, worst


def test_print_the_worst_float32_ratio_per_op():
    """(after the cases above, in file order) the figures the GPU test's docstring quotes."""
    for (op, kind), w in sorted(WORST32.items()):
        print("float32 CPU autograd, worst err / bar: %-4s %-7s %.3g" % (op, kind, w))
    assert all(w <= 0.5 for w in WORST32.values())


def _wrong(case):
    """The wrong restatements a case must catch: (corrupt, keys of which at least one must miss the bar)."""
    if case.op == "afm":
        return [("last_pair", ("dx", "dW", "db", "dh", "dp"))]
    if case.op in ("vec", "mat") and case.data == "nonneg" and case.shape[2] > 0:
        return [("ds_col", ("dx", "dk")), ("dw_row", ("dk",))]
    if case.op == "mix" and case.shape[2] > 0:
        return [("dw_row", ("dV",))] + ([("gate_col", ("dG", "dx"))] if case.shape[3] > 1 else [])
    return []


@pytest.mark.parametrize("case_id", [c.id for c in R.CASES if _wrong(c)])
def test_a_dropped_summand_misses_the_bar(case_id):
    """One summand left out of one reduction: AFM's last pair out of every sum of the backward; CrossNet's last column out of the last
    layer's ds (vector) or g W step (matrix), or the last batch row out of layer 0's kernel gradient; CrossNetMix's last column out of
    the last layer's gate dot products, or the last batch row out of layer 0's dV.  Each must miss the bar in every non-negative
    CrossNet case and in every AFM and mix case (an expert alone has p = 1 and ds = 0: no gate restatement there)."""
    case, info, d, g, t = _reference(case_id)
    for corrupt, keys in _wrong(case):
        gc, _ = R.oracle(case, d, corrupt=corrupt)
        r = {k: _ratio(gc[k], g[k], t[k]) for k in keys}
        print("%s %s: %s x the bar" % (case_id, corrupt, "  ".join("%s %.3g" % kv for kv in r.items())))
        assert max(r.values()) > 1.0, (corrupt, r)


@pytest.mark.parametrize("case_id", R.CASE_IDS)
def test_the_case_reaches_its_route_and_the_restated_sizes_are_the_librarys(case_id):
    case = CASE[case_id]
    info = R.resolve(case)                                              # raises when the route is not the table's
    assert case.route in R.ROUTES[case.op]
    if case.op in ("vec", "mat"):
        B, d, L = case.shape
        assert info["ws_bytes"] == R.library_crossnet_ws_bytes("vector" if case.op == "vec" else "matrix", B, d, L), info
    if case.op == "mix" and case.shape[2] > 0:
        assert info["ws_bytes"] == R.library_mix_ws_bytes(*case.shape), info


def test_every_route_is_reached_and_every_cap_is_passed():
    reached = {(c.op, c.route) for c in R.CASES}
    assert reached == {(op, r) for op, rs in R.ROUTES.items() for r in rs}
    for op in R.CAP:
        assert any(c.op == op and c.cap2 for c in R.CASES), op
    for c in R.CASES:
        if c.op in ("bi", "ip", "vec", "mat"):                          # both kinds of data on every such route
            assert c.id.rsplit("-", 1)[0] + "-nonneg" in CASE and c.id.rsplit("-", 1)[0] + "-signed" in CASE
    assert len(set(R.CASE_IDS)) == len(R.CASE_IDS)
    # the edges the table is there for
    assert R.resolve(CASE["afm-5x62x64x8-signed"])["lds"] == 161968 and R.resolve(CASE["afm-5x63x64x8-signed"])["lds"] == 165008
    assert R.resolve(CASE["afm-9x30x64x4-signed"])["lds"] == 71024
    assert R.resolve(CASE["vec-19x1137x3-signed"])["lds"] == 163776 and R.resolve(CASE["vec-19x1138x3-signed"])["lds"] == 163920
    v = R.resolve(CASE["vec-520x2100x2-signed"])
    assert (v["slices"], v["last_rows"]) == (9, 56)
    assert [R.resolve(CASE["mat-%s-signed" % s])["parts"] for s in ("1031x12x2", "1030x12x2", "2048x45x1", "1030x1024x1")] == [1, 2, 4, 2]
    m = R.resolve(CASE["mix-1100x70x2x3x5-signed"])
    assert (m["slices"], m["last_rows"]) == (5, 204)
    assert {c.shape[3] for c in R.CASES if c.op == "mix"} >= {1, 2, 16, 17} and any(c.op == "mix" and c.shape[4] == 1 for c in R.CASES)
    assert {c.shape[0] % 4 for c in R.CASES if c.op == "afm"} >= {1, 3}
    assert [R.k_slices(b, 256) for b in (256, 257, 513, 4097, 8193)] == [1, 2, 3, 17, 29]
    assert [R.mlp_dw_parts(b, 144) for b in (1023, 1024, 8192)] == [1, 2, 16]


@pytest.mark.parametrize("case_id", [c.id for c in R.CASES if c.op == "afm"])
def test_the_afm_relu_margin_holds(case_id):
    case, info, d, g, t = _reference(case_id)
    assert R.afm_kink_margin(d["x"], d["W"], d["b"]).min() >= R.KINK_ULP
    assert len(d["redrawn"]) <= max(1, case.shape[0] // 2)
    again = R.make_data(case)
    assert all((again[k] == d[k]).all() for k in ("x", "W", "b", "h", "p", "dy"))          # deterministic, redraws included


def test_the_dry_checks_agree_with_the_restated_limits():
    from deepctr_amd import ops
    assert ops.afm_bwd_supported(62, 64, 8) and not ops.afm_bwd_supported(63, 64, 8)
    for c in R.CASES:
        if c.op == "afm":
            assert ops.afm_bwd_supported(*c.shape[1:]) == (R.afm_bwd_lds_bytes(*c.shape[1:]) <= R.LDS_MAX) == (c.route != "refused")
        if c.op == "mix":
            assert ops.crossnet_mix_bwd_supported(c.shape[1], c.shape[2], c.shape[3], c.shape[4]) == (c.route != "refused")
    assert ops.crossnet_mix_bwd_supported(8, 2, 16, 4) and not ops.crossnet_mix_bwd_supported(8, 2, 17, 4)
    assert not ops.afm_bwd_supported(1, 4, 2) and not ops.crossnet_mix_bwd_supported(8, 2, 0, 4)      # the ops' DCTR_E_DIM
