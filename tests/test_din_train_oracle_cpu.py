"""Pins, without a GPU, what tests/test_gpu_din_train_oracle.py checks the DIN step's kernels, the Dice passes, the lookup scatter and
the loss against (tests/ref_din_train.py):
  * every oracle against torch float64 autograd over the differentiable restatement of the reference layer (the expressions of
    tests/test_gpu_din_train.py, tests/ref_dice.dice_dnn, index_add_, binary_cross_entropy on sigmoid outputs), on every case small
    enough for the CPU, to 1e-12 of each gradient's largest element;
  * that tests.util.assert_close_terms' default bar leaves room: float32 torch autograd / float32 NumPy on the CPU, whose sums run in
    another order than any kernel's, stays within half of it on every case;
  * that the bar can fail: a weighted sum without one position, a variance divided by R - 1, a scatter without one run miss it;
  * the floor of the batch variance the batch-statistics backward is conditioned at, and the route every case is there for, restated
    from the constants of the .hip files.
Run with -s for the worst float32 err / bar per op; tests/test_gpu_din_train_oracle.py quotes them."""
import functools

import numpy as np
import pytest
import torch

from tests import ref_din_train as R
from tests.ref_dice import dice_dnn

DIN = {c.id: c for c in R.DIN_CASES}
LOOKUP = {c.id: c for c in R.LOOKUP_CASES}
DICE = {c.id: c for c in R.DICE_CASES}
CPU_MAX = 1 << 21                           # elements of a case's largest array up to which the autograd comparison runs here
WORST32 = {}


def _ratio(got, ref, terms):
    """Worst error in units of tests.util.assert_close_terms' default bar."""
    got, ref, terms = (np.asarray(a, dtype=np.float64) for a in (got, ref, terms))
    return float((np.abs(got - ref) / (1e-4 * np.abs(ref) + 2e-6 * np.abs(terms) + 1e-30)).max()) if ref.size else 0.0


def _pinned(got, ref, what, scale=None):
    """1e-12 of the reference's largest element (``scale``: of the summands' instead, for a sum that cancels)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64).reshape(np.shape(got))
    scale = (np.abs(ref).max() if ref.size else 0.0) if scale is None else scale
    assert np.abs(got - ref).max(initial=0.0) <= 1e-12 * scale + 1e-300, "%s: %.3g of %.3g" % (what, np.abs(got - ref).max(), scale)


def _note(op, case_id, worst):
    print("%s float32 on the CPU, err / bar: %s" % (case_id, "  ".join("%s %.3g" % kv for kv in worst.items())))
    w = max(worst.values())
    WORST32[op] = max(WORST32.get(op, 0.0), w)
    assert w <= 0.5, (case_id, worst)


# ---------------------------------------------------------------------------------------------------
# DIN's attention pieces
# ---------------------------------------------------------------------------------------------------
def _din_autograd(case, d, dtype):
    """Every piece of a case by torch in ``dtype``: the expressions of tests/test_gpu_din_train.py."""
    B, T, E = case.shape
    C = lambda a: torch.tensor(np.asarray(a), dtype=dtype)                             # noqa: E731
    L = lambda a: torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True)         # noqa: E731
    N = lambda t: t.detach().double().numpy()                                          # noqa: E731
    m = torch.tensor(d["mask"].astype(bool))
    out = {}
    if "att_in_bwd" in case.pieces:
        q, k = L(d["q"]), L(d["k"])
        qq = q[:, None, :].expand(-1, T, -1)
        (torch.cat([qq, k, qq - k, qq * k], dim=-1).reshape(B * T, 4 * E) * C(d["da"])).sum().backward()
        out["att_in_bwd"] = {"dq": N(q.grad), "dk": N(k.grad)}
    if "wsum" in case.pieces or "wsum_bwd" in case.pieces:
        s, k = L(d["score"]), L(d["k"])
        o = (torch.where(m, s.reshape(B, T), torch.zeros(B, T, dtype=dtype))[:, None, :] @ k).squeeze(1)
        out["wsum"] = N(o)
        if "wsum_bwd" in case.pieces:
            (o * C(d["d_out"])).sum().backward()
            out["wsum_bwd"] = {"d_score": N(s.grad).reshape(B, T), "dk": N(k.grad), "d_bias": float(s.grad.double().sum())}
    if "softmax" in case.pieces or "softmax_bwd" in case.pieces:
        s = L(d["score"])
        p = torch.softmax(torch.where(m, s.reshape(B, T), torch.full((B, T), -2.0 ** 32 + 1, dtype=dtype)), dim=1)
        out["softmax"] = N(p)
    if "softmax_bwd" in case.pieces:
        # the op takes p: differentiate softmax at the float32-rounded p's own scores is not possible, so autograd runs from the scores
        # and the oracle is handed autograd's p
        (p * C(d["dp"]).reshape(B, T)).sum().backward()
        out["softmax_bwd"] = {"d_score": N(s.grad).reshape(B, T), "d_bias": float(s.grad.double().sum()), "p": N(p)}
    return out


def _din_small(case):
    B, T, E = case.shape
    return B * T * E * 4 <= CPU_MAX


@pytest.mark.parametrize("case_id", [c.id for c in R.DIN_CASES if _din_small(c)])
def test_the_attention_oracles_match_double_autograd_and_float32_keeps_half_the_bar(case_id):
    case = DIN[case_id]
    B, T, E = case.shape
    d = R.make_din_data(case)
    a64, a32 = _din_autograd(case, d, torch.float64), _din_autograd(case, d, torch.float32)
    worst = {}
    if "att_in" in case.pieces:                 # exact: float32 torch gives the oracle's bits
        q, k = torch.tensor(d["q"]), torch.tensor(d["k"])
        qq = q[:, None, :].expand(-1, T, -1)
        ref = torch.cat([qq, k, qq - k, qq * k], dim=-1).reshape(B * T, 4 * E).numpy()
        assert (R.att_in(d["q"], d["k"])[0].view(np.int32) == ref.view(np.int32)).all()
    if "att_in_bwd" in case.pieces:
        g, t = R.att_in_bwd(d["da"], d["q"], d["k"])
        for key in ("dq", "dk"):
            _pinned(g[key], a64["att_in_bwd"][key], "%s att_in_bwd %s" % (case_id, key))
            assert (np.abs(g[key]) <= t[key] * (1 + 1e-12)).all()
            worst["att_in_bwd." + key] = _ratio(a32["att_in_bwd"][key], g[key], t[key])
    if "wsum" in case.pieces:
        g, t = R.wsum(d["score"], d["mask"], d["k"])
        _pinned(g, a64["wsum"], case_id + " wsum")
        assert (np.abs(g) <= t * (1 + 1e-12)).all()
        if case.mask == "none" or (case.mask == "random" and B > 2):
            assert (g[0] == 0).all() and (t[0] == 0).all()                          # a row without a valid position: an exact zero
        worst["wsum"] = _ratio(a32["wsum"], g, t)
    if "wsum_bwd" in case.pieces:
        g, t = R.wsum_bwd(d["d_out"], d["score"], d["mask"], d["k"])
        for key in ("d_score", "dk", "d_bias"):
            _pinned(g[key], a64["wsum_bwd"][key], "%s wsum_bwd %s" % (case_id, key))
            worst["wsum_bwd." + key] = _ratio(a32["wsum_bwd"][key], g[key], t[key])
    if "softmax" in case.pieces:
        g, t = R.din_softmax(d["score"].reshape(B, T), d["mask"])
        _pinned(g, a64["softmax"], case_id + " softmax")
        worst["softmax"] = _ratio(a32["softmax"], g, t)
    if "softmax_bwd" in case.pieces:
        (g, gb), (t, tb) = R.din_softmax_bwd(a64["softmax_bwd"]["p"], d["mask"], d["dp"].reshape(B, T))
        _pinned(g, a64["softmax_bwd"]["d_score"], case_id + " softmax_bwd")
        _pinned(gb, a64["softmax_bwd"]["d_bias"], case_id + " softmax_bwd d_bias", scale=np.abs(g).sum())
        worst["softmax_bwd"] = _ratio(a32["softmax_bwd"]["d_score"], g, t)
    for key, w in worst.items():
        WORST32[key] = max(WORST32.get(key, 0.0), w)
    print("%s float32 autograd, err / bar: %s" % (case_id, "  ".join("%s %.3g" % kv for kv in worst.items())))
    assert all(w <= 0.5 for w in worst.values()), worst


@pytest.mark.parametrize("case_id", [c.id for c in R.DIN_CASES if "wsum" in c.pieces and c.mask in ("random", "full", "alt") and _din_small(c)])
def test_a_weighted_sum_without_one_position_misses_the_bar(case_id):
    case = DIN[case_id]
    d = R.make_din_data(case)
    g, t = R.wsum(d["score"], d["mask"], d["k"])
    b, tt = [int(i) for i in np.argwhere(d["mask"] != 0)[-1]]                      # the last valid position of the batch
    gc, _ = R.wsum(d["score"], d["mask"], d["k"], drop=(b, tt))
    r = _ratio(gc, g, t)
    print("%s without position (%d, %d): %.3g x the bar" % (case_id, b, tt, r))
    assert r > 1.0


# ---------------------------------------------------------------------------------------------------
# the lookup scatter
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lookup_reference(case_id):
    case = LOOKUP[case_id]
    d = R.make_lookup_data(case)
    (g, touched), t = R.lookup_bwd(d["ids"], case.vocab, case.dim, case.hash_mode, d["d"])
    rows = R.RE.resolve_rows(d["ids"], case.vocab, case.hash_mode)
    return case, d, g, touched, t, rows


@pytest.mark.parametrize("case_id", [c.id for c in R.LOOKUP_CASES])
def test_the_scatter_oracle_matches_index_add_and_float32_keeps_half_the_bar(case_id):
    case, d, g, touched, t, rows = _lookup_reference(case_id)
    ok = (rows >= 0) & (rows < case.vocab)
    src = torch.tensor(d["d"][ok])
    idx = torch.tensor(rows[ok])
    _pinned(g, torch.zeros(case.vocab, case.dim, dtype=torch.float64).index_add_(0, idx, src.double()).numpy(), case_id)
    assert (np.abs(g) <= t * (1 + 1e-12)).all()
    _note("lookup_bwd", case_id, {"g": _ratio(torch.zeros(case.vocab, case.dim).index_add_(0, idx, src).numpy(), g, t)})
    hit = np.zeros(case.vocab, dtype=bool)
    hit[rows[ok]] = True
    assert (t[~hit] == 0).all()
    if case.dim % 4 == 0:
        assert touched.dtype == np.uint8 and (touched.reshape(case.vocab, case.dim // 4) == hit[:, None]).all()
    else:
        assert touched is None
    # the pattern is what the id says
    if case.pattern == "equal":
        assert np.unique(rows).size == 1 and ok.all()
    if case.pattern == "distinct":
        assert np.unique(rows).size == case.n and ok.all()
    if case.pattern == "padskew":
        zero = d["ids"] == 0
        assert 0.4 < zero.mean() < 0.6 and (rows[zero] == 0).all() and ok.all()
        assert np.bincount(rows[~zero]).max() >= 4                                  # skewed: some row is hit again and again
    if case.pattern == "oor_tile":
        lo = R.oor_tile_of(case) * R.LB_TILE
        assert not ok[lo:lo + R.LB_TILE].any() and ok[:lo].all() and ok[lo + R.LB_TILE:].all() and ok.any()
        assert (d["ids"][lo:lo + R.LB_TILE] < 0).any() and (d["ids"][lo:lo + R.LB_TILE] >= case.vocab).any()
    if case.hash_mode == 2 and case.pattern == "padskew":
        assert (rows[d["ids"] != 0] != 0).all()                                      # mask_zero: bucket 0 is the padding id's alone


@pytest.mark.parametrize("case_id", [c.id for c in R.LOOKUP_CASES])
def test_a_scatter_that_forgets_one_run_misses_the_bar(case_id):
    case, d, g, touched, t, rows = _lookup_reference(case_id)
    ok = (rows >= 0) & (rows < case.vocab)
    row = int(rows[ok][-1])
    (gc, _), _ = R.lookup_bwd(d["ids"], case.vocab, case.dim, case.hash_mode, d["d"], forget_row=row)
    assert _ratio(gc, g, t) > 1.0 and (gc[row] == 0).all()
    keep = np.arange(case.vocab) != row
    assert (gc[keep] == g[keep]).all()


# ---------------------------------------------------------------------------------------------------
# Dice
# ---------------------------------------------------------------------------------------------------
def _dice_autograd(d, mode, dtype):
    """dz, d_alpha, dW, db, dx of a case's layer by torch autograd over tests/ref_dice.dice_dnn (the bias as a full [R, N] leaf: its
    gradient is dz), and the layer's output and batch statistics."""
    Lf = lambda a: torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True)        # noqa: E731
    C = lambda a: torch.tensor(np.asarray(a), dtype=dtype)                             # noqa: E731
    x, W, al = Lf(d["x"]), Lf(d["W"]), Lf(d["alpha"])
    bfull = Lf(np.broadcast_to(d["b"], d["dy"].shape).copy())
    stored = ([C(d["moving_mean"])], [C(d["moving_var"])]) if mode == "stored" else (None, None)
    h, stats = dice_dnn(x, [W], [bfull], [al], *stored, eps=1e-9)
    (h * C(d["dy"])).sum().backward()
    N = lambda t: t.detach().double().numpy()                                          # noqa: E731
    return {"dz": N(bfull.grad), "d_alpha": N(al.grad), "dW": N(W.grad), "db": N(bfull.grad.sum(0)), "dx": N(x.grad), "y": N(h),
            "mean": N(stats[0][0]), "var": N(stats[0][1])}


BWD_DICE = [c.id for c in R.DICE_CASES if c.kind == "bwd"]


@pytest.mark.parametrize("mode", ["stored", "batch"])
@pytest.mark.parametrize("case_id", BWD_DICE)
def test_the_dice_backward_oracles_match_double_autograd_and_float32_keeps_half_the_bar(case_id, mode):
    case = DICE[case_id]
    d = R.make_dice_data(case)
    a64 = _dice_autograd(d, mode, torch.float64)
    if mode == "stored":
        G, T = R.dice_bwd_stored(d["z64"], d["dy"], d["alpha"], d["moving_mean"], d["moving_var"], zmag=d["zmag"])
    else:                                   # the formulas hold for the batch's own statistics: the exact float64 ones here
        G, T = R.dice_bwd_batch(d["z64"], d["dy"], d["alpha"], d["z64"].mean(0), d["z64"].var(0), zmag=d["zmag"])
    G, T = R.dense_bwd(d["x"], d["W"], G, T)
    keys = ("dz", "d_alpha", "dW", "db", "dx")
    for k in keys:
        # (db through the batch statistics is an exact zero that float64 autograd leaves at 1e-17: its scale is dz's)
        scale = np.abs(a64["dz"]).max() * case.R if k == "db" else np.abs(a64[k]).max()
        assert np.abs(G[k] - a64[k]).max() <= 1e-12 * scale, "%s %s %s: %.3g of %.3g" % (case_id, mode, k, np.abs(G[k] - a64[k]).max(), scale)
        assert (np.abs(G[k]) <= T[k] * (1 + 1e-12) + 1e-300).all(), k
    # what the GPU test hands the op — the batch statistics rounded to float32 — moves nothing near the bar
    Gr, Tr = R.dice_bwd_oracle(d, mode)
    assert max(_ratio(G[k], Gr[k], Tr[k]) for k in keys) <= 0.25
    a32 = _dice_autograd(d, mode, torch.float32)
    _note("dice_bwd_" + mode, case_id, {k: _ratio(a32[k], Gr[k], Tr[k]) for k in keys})


@pytest.mark.parametrize("case_id", [c.id for c in R.DICE_CASES])
def test_the_dice_forward_oracle_matches_torch_and_a_variance_over_r_minus_1_misses_the_bar(case_id):
    case = DICE[case_id]
    d = R.make_dice_data(case)
    z, bias = R.dice_fwd_input(case, d)
    G, T = R.dice_train_fwd(z, bias, d["alpha"], d["moving_mean"], d["moving_var"])
    zb = torch.tensor(z, dtype=torch.float64) + (0 if bias is None else torch.tensor(bias, dtype=torch.float64))
    al = torch.tensor(d["alpha"], dtype=torch.float64)
    mean, var = zb.mean(0), zb.var(0, unbiased=False)
    p = torch.sigmoid((zb - mean) / torch.sqrt(var + 1e-9))
    _pinned(G["mean"], mean.numpy(), case_id + " mean")
    _pinned(G["var"], var.numpy(), case_id + " var")
    _pinned(G["y"], (al * (1 - p) * zb + p * zb).numpy(), case_id + " y")
    mom = float(np.float32(0.99))
    _pinned(G["moving_mean"], d["moving_mean"].astype(np.float64) * mom + mean.numpy() * (1 - mom), case_id + " moving mean")
    _pinned(G["moving_var"], d["moving_var"].astype(np.float64) * mom + var.numpy() * (1 - mom), case_id + " moving variance")
    for k in G:
        assert (np.abs(G[k]) <= T[k] * (1 + 1e-12) + 1e-300).all(), k
    if case.kind == "var0":
        assert (G["var"] == 0).all() and (G["mean"] == zb.numpy()[0]).all()
        return
    # float32 torch, two passes like the kernel
    zf = torch.tensor(z) + (0 if bias is None else torch.tensor(bias))
    mf, vf = zf.mean(0), zf.var(0, unbiased=False)
    pf = torch.sigmoid((zf - mf) / torch.sqrt(vf + 1e-9))
    alf = torch.tensor(d["alpha"])
    _note("dice_train_fwd", case_id, {"mean": _ratio(mf.numpy(), G["mean"], T["mean"]), "var": _ratio(vf.numpy(), G["var"], T["var"]),
                                      "y": _ratio((alf * (1 - pf) * zf + pf * zf).numpy(), G["y"], T["y"])})
    if case.R <= 5000:
        Gw, _ = R.dice_train_fwd(z, bias, d["alpha"], d["moving_mean"], d["moving_var"], ddof=1)
        r = _ratio(Gw["var"], G["var"], T["var"])
        print("%s variance over R - 1: %.3g x the bar" % (case_id, r))
        assert r > 1.0


def test_the_batch_variance_floor_holds_where_the_backward_runs_through_the_statistics():
    """The gradient through the batch statistics carries 1 / sqrt(var + eps) twice: a column whose batch variance is nearly zero makes it
    ill-conditioned, and two rows always have xn = +-1.  So the smallest backward case has three rows and every case's seed is moved
    on until each column's batch variance is at least DICE_MIN_VAR (1 / sqrt(var) <= 4.5).  The terms of dice_bwd_batch carry that
    conditioning themselves ((|z| + |mean|) / sqrt(var + eps)): measured with them, float32 torch autograd over 40 seeds of an
    [R, 8] layer stays at 0.006 of the bar at R = 2 and 0.008 at R = 3."""
    assert min(DICE[c].R for c in BWD_DICE) == 3
    for cid in BWD_DICE:
        d = R.make_dice_data(DICE[cid])
        assert d["z64"].var(0).min() >= R.DICE_MIN_VAR, cid
        assert d["redraws"] < R.DICE_REDRAWS // 2
        again = R.make_dice_data(DICE[cid])
        assert all((again[k] == d[k]).all() for k in ("x", "W", "b", "alpha", "dy"))          # deterministic, redraws included
        # mean about 0.7, unit spread: E[z^2] - E[z]^2 would cancel
        if DICE[cid].R * DICE[cid].N >= 2000:
            assert 0.5 < d["z64"].mean() < 0.9 and 0.7 < d["z64"].std() < 1.4, cid


# ---------------------------------------------------------------------------------------------------
# the loss
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weight", R.BCE_WEIGHTS)
@pytest.mark.parametrize("task", R.BCE_TASKS)
@pytest.mark.parametrize("B", R.BCE_BATCHES)
def test_the_loss_oracle_matches_double_autograd_and_float32_keeps_half_the_bar(B, task, weight):
    pred, y, w = R.make_bce_data(B, task, weight)
    G, T = R.bce_grad(pred, y, task, w)
    # autograd through the sigmoid, on the predictions a finite logit reaches (the others: the closed form's own test below)
    # (mse belongs to PredictionLayer('regression'): the prediction IS the logit)
    inner = (pred > 0) & (pred < 1) if task == "binary" else np.ones(B, dtype=bool)
    p64 = torch.tensor(pred[inner].astype(np.float64))
    logit = torch.log(p64) - torch.log1p(-p64) if task == "binary" else p64.clone()
    logit.requires_grad_(True)
    p, t = torch.sigmoid(logit) if task == "binary" else logit, torch.tensor(y[inner].astype(np.float64))
    wt = torch.ones_like(p) if w is None else torch.tensor(w[inner].astype(np.float64))
    if task == "binary":
        pc = torch.clamp(p, float(R.BCE_LO), float(R.BCE_HI))                         # (inside the clip its gradient is 1)
        loss = -(wt * (t * torch.log(pc) + (1 - t) * torch.log(1 - pc)))
        unclipped = (pred[inner] > R.BCE_LO) & (pred[inner] < R.BCE_HI)                # (strictly inside: the round trip through the logit moves p by an ulp)
    else:
        loss = wt * (p - t) ** 2
        unclipped = np.ones(int(inner.sum()), dtype=bool)
    (loss.sum() / B).backward()
    ref = logit.grad.numpy()
    got = G["dlogit"][inner]
    scale = np.abs(ref).max() if ref.size else 0.0
    assert np.abs(got - ref)[unclipped].max(initial=0.0) <= 1e-12 * scale + 1e-300
    # the value: 1 - pc formed in float32 moves log(1 - pc) by at most 2^-24 / (1 - pc)
    if inner.any():
        mine = R.bce_grad(pred[inner], y[inner], task, None if w is None else w[inner])
        assert abs(mine[0]["loss_sum"] - float(loss.detach().sum())) <= 1e-5 * mine[1]["loss_sum"] + 1e-300
    assert G["loss_sum"] <= T["loss_sum"] * (1 + 1e-12) and abs(G["dlogit_sum"]) <= T["dlogit_sum"] * (1 + 1e-12)
    # float32 NumPy, the kernel's expressions
    f = np.float32
    if task == "binary":
        pc = np.minimum(np.maximum(pred, f(1e-7)), f(1) - f(1e-7))
        l32, d32 = -(y * np.log(pc) + (f(1) - y) * np.log(f(1) - pc)), (pred - y) / f(B)
    else:
        l32, d32 = (pred - y) * (pred - y), f(2) * (pred - y) / f(B)
    if w is not None:
        l32, d32 = l32 * w, d32 * w
    assert l32.dtype == np.float32 and d32.dtype == np.float32
    _note("bce_grad", "bce-%d-%s-%s" % (B, task, weight), {"dlogit": _ratio(d32, G["dlogit"], T["dlogit"]),
                                                           "loss_sum": _ratio(l32.sum(dtype=np.float32), G["loss_sum"], T["loss_sum"]),
                                                           "dlogit_sum": _ratio(d32.sum(dtype=np.float32), G["dlogit_sum"], T["dlogit_sum"])})
    if weight == "zero":
        assert G["loss_sum"] == 0 and G["dlogit_sum"] == 0 and (G["dlogit"] == 0).all()


def test_the_loss_oracle_at_the_clip():
    """The closed form at the edge predictions: the clip bounds are the float32 ones, 1 - pc is formed in float32, and the gradient is
    (pred - y) / B on both sides of the clip (the open point of the oracle's docstring)."""
    assert float(R.BCE_HI) == 1 - 2.0 ** -23 and float(R.BCE_LO) == float(np.float32(1e-7))
    p, y = R.bce_edges()
    assert p.size == 12 and set(y) == {0.0, 1.0}
    for pv, yv in zip(p, y):
        G, T = R.bce_grad([pv], [yv])
        pc = min(max(float(pv), float(R.BCE_LO)), float(R.BCE_HI))
        one_m = float(np.float32(1) - np.float32(pc))
        want = -np.log(pc) if yv else -np.log(one_m)
        assert abs(G["loss_sum"] - want) <= 1e-15 * abs(want), (pv, yv)
        assert G["dlogit"][0] == float(pv) - float(yv) and np.isfinite(G["loss_sum"])
    assert R.bce_grad([0.0], [1.0])[0]["loss_sum"] == -np.log(float(np.float32(1e-7)))
    assert R.bce_grad([1.0], [0.0])[0]["loss_sum"] == -np.log(2.0 ** -23)
    assert R.bce_grad([1.0 - 2.0 ** -24], [0.0])[0]["loss_sum"] == -np.log(2.0 ** -23)         # clipped: not -log(2^-24)
    assert R.bce_grad([1e-8], [1.0])[0]["loss_sum"] == R.bce_grad([0.0], [1.0])[0]["loss_sum"]


# ---------------------------------------------------------------------------------------------------
# routes
# ---------------------------------------------------------------------------------------------------
def test_every_case_reaches_its_route():
    for c in R.DIN_CASES:
        R.resolve_din(c)                                                             # raises when a cap is no longer passed
    for c in R.LOOKUP_CASES:
        R.resolve_lookup(c)
    for c in R.DICE_CASES:
        R.resolve_dice(c)
    ids = [c.id for c in R.DIN_CASES + R.LOOKUP_CASES + R.DICE_CASES]
    assert len(set(ids)) == len(ids)


def test_every_branch_of_the_issue_is_reached():
    # DIN: every launcher's 16,384 cap, sum_vec on several workgroups, the wave loops, every mask edge
    capped = {p for c in R.DIN_CASES for p in R.resolve_din(c)["cap2"]}
    assert capped == set(R.DIN_PIECES)
    assert any(R.resolve_din(c)["sum_vec_many"] and "wsum_bwd" in c.pieces for c in R.DIN_CASES)
    assert any(R.resolve_din(c)["sum_vec_many"] and "softmax_bwd" in c.pieces for c in R.DIN_CASES)
    assert R.sum_vec_grid(1400 * 50) == 35 and R.sum_vec_grid(66000 * 3) == 64 and R.sum_vec_grid(2048) == 1
    assert [R.din_grid("softmax", b, 3, 1)[0] > R.DIN_CAP for b in (65536, 65537)] == [False, True]
    assert {c.mask for c in R.DIN_CASES} == {"random", "none", "full", "alt"}
    for piece in R.DIN_PIECES:
        shapes = {c.shape for c in R.DIN_CASES if piece in c.pieces}
        assert {(1, 1, 1), (37, 6, 8), (5, 65, 70), (3, 130, 16)} <= shapes, piece
    for c in R.DIN_CASES:
        m = R.din_mask(c)
        if c.mask == "random" and c.shape[0] > 2:                                    # rows without a valid position among valid ones
            assert not m[0].any() and not m[-1].any() and m[1:-1].any()
    # the lookup: both routes at every edge of the window, the tile route's id patterns, id types, hash modes, layouts
    info = {c.id: R.resolve_lookup(c) for c in R.LOOKUP_CASES}
    tile = [c for c in R.LOOKUP_CASES if c.route == "tile"]
    assert {(c.dim, c.n) for c in tile} == {(3, 1024), (12, 1025), (64, 3000)}
    assert {(c.dim, c.n) for c in R.LOOKUP_CASES if c.route == "plain"} == {(2, 2048), (68, 62000), (16, 1023)}
    for dim, n in ((3, 1024), (12, 1025), (64, 3000)):
        assert {c.pattern for c in tile if (c.dim, c.n) == (dim, n)} >= {"equal", "distinct", "padskew"}
    assert {c.pattern for c in tile} == {"equal", "distinct", "padskew", "oor_tile", "random"}
    assert R.lookup_route(10, 2, 5000) == "plain" and R.lookup_route(10, 3, 1024) == "tile" and R.lookup_route(10, 3, 1023) == "plain"
    assert R.lookup_route(10, 64, 1024) == "tile" and R.lookup_route(10, 65, 1024) == "plain"
    d3, d12, d64 = (next(info[c.id] for c in tile if c.dim == dim) for dim in (3, 12, 64))
    assert (d3["dimP"], d3["idle_lanes"], d3["walkers_per_wave"], d3["per_walker"], d3["tiles"]) == (4, 1, 16, 16, 1)
    assert (d12["dimP"], d12["idle_lanes"], d12["walkers_per_wave"], d12["per_walker"], d12["tiles"]) == (16, 4, 4, 64, 2)
    assert (d64["dimP"], d64["idle_lanes"], d64["walkers_per_wave"], d64["per_walker"], d64["tiles"]) == (64, 0, 1, 256, 3)
    assert any(c.plain_cap2 and c.mark_cap2 for c in R.LOOKUP_CASES)
    assert {c.i64 for c in R.LOOKUP_CASES} == {False, True} and {c.hash_mode for c in R.LOOKUP_CASES} == {0, 1, 2}
    assert {c.strided for c in R.LOOKUP_CASES} == {False, True}
    assert any(c.dim % 4 == 0 and c.pattern == "oor_tile" for c in R.LOOKUP_CASES)                 # touched bytes stay clear
    # Dice: both forms, the row-lane form's extremes, the scalar form's column loop, the caps
    r = {c.id: R.resolve_dice(c) for c in R.DICE_CASES}
    assert (r["dice-300x80-bwd"]["RL"], r["dice-300x80-bwd"]["idle"]) == (12, 16)
    assert (r["dice-300x40-bwd"]["RL"], r["dice-300x40-bwd"]["idle"]) == (25, 6)
    assert r["dice-17x4-bwd"]["RL"] == 256 and r["dice-17x4-bwd"]["idle"] == 0 and r["dice-33x1024-bwd"]["RL"] == 1
    assert r["dice-33x1028-bwd"]["passes"] == 5 and r["dice-70x257-bwd"]["passes"] == 2
    assert r["dice-5000x6-bwd"]["grid"] == R.COLSUM_MAX_WG and r["dice-5000x6-bwd"]["strided_trips"] == 5
    big = r["dice-32773x40-bwd"]
    assert big["grid"] == 128 and big["apply_cap2"] and big["strided_trips"] > 1
    assert R.colsum_grid(32767, 25) == 64 and R.colsum_grid(32768, 25) == 128
    assert not any(v["apply_cap2"] for k, v in r.items() if k != "dice-32773x40-bwd")
    assert r["dice-37x12-stride14"]["form"] == "scalar" and r["dice-37x12-off4"]["form"] == "scalar" and r["dice-37x12-bias"]["form"] == "lane4"
    assert R.rowlane4_ok(1024, 1024) and not R.rowlane4_ok(1028, 1028) and not R.rowlane4_ok(12, 14) and not R.rowlane4_ok(12, 12, 4)
    assert R.rowlane4_ok(4, 4) and not R.rowlane4_ok(6, 6)
    assert {c.kind for c in R.DICE_CASES} == {"bwd", "var0", "stride14", "off4", "nobias", "bias"}
    # the loss: every remainder of the wave and of the workgroup
    assert {b % 64 for b in R.BCE_BATCHES} >= {0, 1, 63} and {b % 256 != 0 for b in R.BCE_BATCHES} == {False, True}


def test_print_the_worst_float32_ratio_per_op():
    """(after the cases above, in file order) the figures the GPU test's docstring quotes."""
    for op, w in sorted(WORST32.items()):
        print("float32 on the CPU, worst err / bar: %-22s %.3g" % (op, w))
    assert all(w <= 0.5 for w in WORST32.values())
