"""GPU parity tests, op level, of the kernels only the DIN training step uses and of the loss of every single-task step —
dctr_din_att_in_fwd / _bwd, dctr_din_wsum_fwd / _bwd, dctr_din_softmax_fwd / _bwd (deepctr_amd/csrc/din_train_kernels.hip),
dctr_embed_lookup_bwd on both routes (deepctr_amd/csrc/embed_bwd_kernels.hip), dctr_dice_train_fwd and the Dice branch of dctr_mlp_bwd in
both forms (deepctr_amd/csrc/dnn_train_kernels.hip), dctr_bce_grad / dctr_bce_grad_w (deepctr_amd/csrc/loss_kernels.hip) — against
the float64 oracles of tests/ref_din_train.py, on every case of the
tables there.  The oracles, the routes and the room the bar leaves are pinned without a GPU by tests/test_din_train_oracle_cpu.py; here
every case is resolved again and one that no longer reaches its route FAILS.

Bar: tests.util.assert_close_terms' defaults — 1e-4 of the result plus 2e-6 of the summed magnitude — for every case; none has a bar of
its own.  What is exact is compared bit for bit: the attention input, the touched bytes, every sentinel neighbour of a strided output,
the in-place softmax backward against the out-of-place one, a written output against its second writing.
Measured, for judging a later change of a bar — worst err / bar per op, float32 on the CPU (torch autograd, index_add_, NumPy; the
sums run in another order than any kernel's; tests/test_din_train_oracle_cpu.py -s):
  att_in_bwd dq 0.018, dk 0.015;  wsum 0.013;  wsum_bwd d_score 0.016, dk 0.0006, d_bias 0.0008;  softmax 0.0038;  softmax_bwd 0.042;
  lookup_bwd 0.031;  dice_train_fwd 0.023;  dice backward, stored statistics 0.024, batch statistics 0.0073;  bce_grad 0.0022
and these tests on an MI355X (the worst of both calls):
  att_in_bwd dq 0.036, dk 0.051;  wsum 0.014;  wsum_bwd d_score 0.032, dk 0.0006, d_bias 0.0019;  softmax 0.0036;  softmax_bwd d_score
  0.028, d_bias 0.0062;  lookup_bwd 0.051 (lookup-v4000-d64-n3000-padskew);  dice_train_fwd mean 0.0047, var 0.0042, moved statistics
  0.012, y 0.038;  dice backward, stored statistics dz 0.025, dx 0.027, dW 0.0096, db 0.014, d_alpha 0.013;  batch statistics dz 0.0096,
  dx 0.0064, dW 0.0041, db 0.0040, d_alpha 0.0084;  bce_grad dlogit 0.0014, loss_sum 0.037, dlogit_sum 0.016
No case failed: no kernel was changed.  0.015 % of the 45 million compared elements lay outside 1e-4 |ref| alone.

Everything an op ACCUMULATES into (d_bias, dk of the attention input, the dx columns, g_table, the weight gradients, d_alpha, loss_sum,
dlogit_sum) starts at a non-zero g0 and ``got - g0`` is compared, |g0| added to ``terms``; a second identical call must add the same
amount again.  What an op WRITES (the weighted sum, dk of its backward, d_score, the softmax, dlogit, dz) must come back
bit-identical from the second call — except dz through the BATCH statistics on more than one workgroup: its column means are atomic
sums over the workgroups, whose order is free, so the second call is held to the bar there and to the bits where one workgroup runs;
and except dx of the DNN, a dctr_gemm product whose k-slices add up in any order (N = 1024 showed it), held to the bar in both calls.  dz is read where dctr_mlp_bwd leaves it: the head of the caller-owned workspace ([R, N], tests/ref_mlp_bwd.layered_floats).
The backward's batch statistics and saved_z are the oracle's own, rounded to float32, so the backward is tested by itself."""
import functools

import numpy as np
import pytest
import torch

from tests import ref_din_train as R
from tests import ref_mlp_bwd as RM
from tests.util import assert_close_terms

pytestmark = pytest.mark.gpu

SENTINEL = 0.75
GUARD = 4096                                # floats behind the restated workspace size
DIN = {c.id: c for c in R.DIN_CASES}
LOOKUP = {c.id: c for c in R.LOOKUP_CASES}
DICE = {c.id: c for c in R.DICE_CASES}
E_NULL, E_DIM = -1, -2                      # include/dctr.h


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def same_bits(a, b):
    return bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def g0_like(shape, scale, seed, device):
    """A non-zero start of an accumulated output, of the result's magnitude: (host float32, device clone)."""
    h = (np.random.default_rng(seed).standard_normal(shape) * max(float(scale), 1e-3)).astype(np.float32)
    return h, dev(h, device)


def rms(a):
    a = np.asarray(a, dtype=np.float64)
    return float(np.sqrt(np.mean(np.square(a)))) if a.size else 0.0


def framed(a, left, right, device, fill=SENTINEL):
    """(buffer [B, left + n + right] filled with ``fill``, its view [:, left:left + n] holding ``a`` [B, n])."""
    a = np.asarray(a, dtype=np.float32)
    buf = np.full((a.shape[0], left + a.shape[1] + right), fill, dtype=np.float32)
    buf[:, left:left + a.shape[1]] = a
    t = dev(buf, device)
    return t, t[:, left:left + a.shape[1]]


def frame_intact(buf, left, n, fill=SENTINEL):
    ref = torch.full_like(buf, fill)
    return same_bits(buf[:, :left], ref[:, :left]) and same_bits(buf[:, left + n:], ref[:, left + n:])


# ---------------------------------------------------------------------------------------------------
# DIN's attention pieces
# ---------------------------------------------------------------------------------------------------
def _din_reference(case_id):
    """Case, inputs and oracles of a case (one test each: not kept, the largest holds a gigabyte)."""
    case = DIN[case_id]
    R.resolve_din(case)
    d = R.make_din_data(case)
    B, T, E = case.shape
    o = {}
    if "att_in" in case.pieces:
        o["att_in"] = R.att_in(d["q"], d["k"])[0]
    if "att_in_bwd" in case.pieces:
        o["att_in_bwd"] = R.att_in_bwd(d["da"], d["q"], d["k"])
    if "wsum" in case.pieces:
        o["wsum"] = R.wsum(d["score"], d["mask"], d["k"])
    if "wsum_bwd" in case.pieces:
        o["wsum_bwd"] = R.wsum_bwd(d["d_out"], d["score"], d["mask"], d["k"])
    if "softmax" in case.pieces:
        o["softmax"] = R.din_softmax(d["score"].reshape(B, T), d["mask"])
    if "softmax_bwd" in case.pieces:
        o["softmax_bwd"] = R.din_softmax_bwd(d["p"], d["mask"], d["dp"].reshape(B, T))
    return case, d, o


def _check_att_in(device, case, d, o):
    from deepctr_amd import ops
    B, T, E = case.shape
    q, k = dev(d["q"], device), dev(d["k"], device)
    a = ops.din_att_in(q, k, torch.full((B * T, 4 * E), float("nan"), device=device))
    assert (bits(a) == o["att_in"].view(np.int32)).all(), "%s: the attention input is not float32-exact" % case.id


def _check_att_in_bwd(device, case, d, o):
    from deepctr_amd import ops
    B, T, E = case.shape
    G, Tm = o["att_in_bwd"]
    q, k, da = dev(d["q"], device), dev(d["k"], device), dev(d["da"], device)
    # the query's columns in dx: neither contiguous nor monotone
    qcol_h = (1 + 2 * np.random.default_rng(E).permutation(E)).astype(np.int32)
    dk0_h, dk = g0_like((B, T, E), rms(G["dk"]), 11, device)
    dx0_h, dx = g0_like((B, 2 * E + 3), rms(G["dq"]), 12, device)
    qcol = dev(qcol_h, device)
    others = np.setdiff1d(np.arange(2 * E + 3), qcol_h)
    for calls in (1, 2):
        ops.din_att_in_bwd(da, q, k, dk, dx, qcol)
        torch.cuda.synchronize()
        assert_close_terms(f64(dk) - dk0_h, calls * G["dk"], calls * Tm["dk"] + np.abs(dk0_h), what="%s att_in_bwd dk x%d" % (case.id, calls))
        got = f64(dx)
        assert_close_terms(got[:, qcol_h] - dx0_h[:, qcol_h], calls * G["dq"], calls * Tm["dq"] + np.abs(dx0_h[:, qcol_h]),
                           what="%s att_in_bwd dq x%d" % (case.id, calls))
        assert (bits(dx)[:, others] == dx0_h.view(np.int32)[:, others]).all(), "%s: a dx column outside qcol changed" % case.id


def _check_wsum(device, case, d, o):
    from deepctr_amd import ops
    B, T, E = case.shape
    G, Tm = o["wsum"]
    score, mask, k = dev(d["score"], device), dev(d["mask"], device), dev(d["k"], device)
    buf, out = framed(np.full((B, E), np.nan), 1, 2, device)
    ops.din_wsum(score, mask, k, out)
    torch.cuda.synchronize()
    first = out.clone()
    assert_close_terms(f64(out), G, Tm, what=case.id + " wsum")
    assert frame_intact(buf, 1, E), "%s: wsum wrote beside its columns" % case.id
    empty = d["mask"].sum(1) == 0
    assert (f64(out)[empty] == 0).all(), "%s: a row without a valid position is not an exact zero" % case.id
    ops.din_wsum(score, mask, k, out)
    assert same_bits(out, first), "%s: the second writing of wsum differs" % case.id


def _check_wsum_bwd(device, case, d, o):
    from deepctr_amd import ops
    B, T, E = case.shape
    G, Tm = o["wsum_bwd"]
    score, mask, k = dev(d["score"], device), dev(d["mask"], device), dev(d["k"], device)
    gbuf, d_out = framed(d["d_out"], 2, 1, device)
    d_score = torch.full((B * T,), float("nan"), device=device)
    dk = torch.full((B, T, E), float("nan"), device=device)
    b0_h, d_bias = g0_like((1,), abs(G["d_bias"]), 13, device)
    keep = bits(gbuf)
    first = None
    for calls in (1, 2):
        ops.din_wsum_bwd(d_out, score, mask, k, d_score, dk, d_bias=d_bias)
        torch.cuda.synchronize()
        if first is None:
            first = (d_score.clone(), dk.clone())
            assert_close_terms(f64(d_score).reshape(B, T), G["d_score"], Tm["d_score"], what=case.id + " wsum_bwd d_score")
            assert_close_terms(f64(dk), G["dk"], Tm["dk"], what=case.id + " wsum_bwd dk")
        else:
            assert same_bits(d_score, first[0]) and same_bits(dk, first[1]), "%s: the second writing of d_score / dk differs" % case.id
        assert_close_terms(f64(d_bias) - b0_h, calls * G["d_bias"], calls * Tm["d_bias"] + np.abs(b0_h), what="%s wsum_bwd d_bias x%d" % (case.id, calls))
    assert (bits(gbuf) == keep).all()
    # without d_bias: the same d_score and dk
    ds2, dk2 = torch.full_like(d_score, float("nan")), torch.full_like(dk, float("nan"))
    ops.din_wsum_bwd(d_out, score, mask, k, ds2, dk2)
    assert same_bits(ds2, first[0]) and same_bits(dk2, first[1])


def _check_softmax(device, case, d, o):
    from deepctr_amd import ops
    B, T, E = case.shape
    G, Tm = o["softmax"]
    score, mask = dev(d["score"], device), dev(d["mask"], device)
    p = ops.din_softmax(score, mask, torch.full((B, T), float("nan"), device=device))
    torch.cuda.synchronize()
    assert_close_terms(f64(p), G, Tm, what=case.id + " softmax")
    empty = d["mask"].sum(1) == 0
    if empty.any():                         # a row without a valid position: the uniform 1 / T, as tf.nn.softmax gives it
        assert_close_terms(f64(p)[empty], np.full((int(empty.sum()), T), 1.0 / T), np.full((int(empty.sum()), T), 1.0 / T), what=case.id + " softmax, empty rows")


def _check_softmax_bwd(device, case, d, o):
    from deepctr_amd import ops
    B, T, E = case.shape
    (G, Gb), (Tm, Tb) = o["softmax_bwd"]
    p, mask, dp = dev(d["p"], device), dev(d["mask"], device), dev(d["dp"], device)
    d_score = torch.full((B * T,), float("nan"), device=device)
    b0_h, d_bias = g0_like((1,), max(abs(Gb), rms(G)), 14, device)
    for calls in (1, 2):
        ops.din_softmax_bwd(p, mask, dp, d_score, d_bias=d_bias)
        torch.cuda.synchronize()
        assert_close_terms(f64(d_bias) - b0_h, calls * Gb, calls * Tb + np.abs(b0_h), what="%s softmax_bwd d_bias x%d" % (case.id, calls))
    assert_close_terms(f64(d_score).reshape(B, T), G, Tm, what=case.id + " softmax_bwd d_score")
    assert (f64(d_score).reshape(B, T)[d["mask"] == 0] == 0).all(), "%s: a padded position received a gradient" % case.id
    # as models/din calls it: d_score IS dp
    inplace = dp.clone()
    ops.din_softmax_bwd(p, mask, inplace, inplace)
    assert same_bits(inplace, d_score), "%s: the in-place softmax backward differs from the out-of-place one" % case.id


_DIN_CHECKS = {"att_in": _check_att_in, "att_in_bwd": _check_att_in_bwd, "wsum": _check_wsum, "wsum_bwd": _check_wsum_bwd,
               "softmax": _check_softmax, "softmax_bwd": _check_softmax_bwd}


@pytest.mark.parametrize("case_id", [c.id for c in R.DIN_CASES])
def test_the_attention_pieces_match_the_float64_oracles(device, case_id):
    case, d, o = _din_reference(case_id)
    for piece in case.pieces:
        _DIN_CHECKS[piece](device, case, d, o)


def test_the_attention_pieces_leave_their_outputs_alone_at_batch_0(device):
    from deepctr_amd import ops
    T, E = 3, 4
    z = lambda *s: torch.zeros(*s, device=device)                                      # noqa: E731
    outs = [torch.full((5, 4 * E), SENTINEL, device=device) for _ in range(8)]
    keep = [bits(t) for t in outs]
    q, k, mask, score = z(0, E), z(0, T, E), torch.zeros(0, T, dtype=torch.uint8, device=device), z(0)
    qcol = torch.arange(E, dtype=torch.int32, device=device)
    ops.din_att_in(q, k, outs[0])
    ops.din_wsum(score, mask, k, outs[1])
    ops.din_wsum_bwd(z(0, E), score, mask, k, outs[2], outs[3], d_bias=outs[4])
    ops.din_softmax(score, mask, outs[5])
    ops.din_softmax_bwd(score, mask, score, outs[6], d_bias=outs[4])
    ops.din_att_in_bwd(z(0, 4 * E), q, k, outs[7], outs[5], qcol)
    torch.cuda.synchronize()
    assert all((bits(t) == b).all() for t, b in zip(outs, keep))


# ---------------------------------------------------------------------------------------------------
# the lookup scatter
# ---------------------------------------------------------------------------------------------------
def _lookup_reference(case_id):
    case = LOOKUP[case_id]
    info = R.resolve_lookup(case)
    d = R.make_lookup_data(case)
    (g, touched), t = R.lookup_bwd(d["ids"], case.vocab, case.dim, case.hash_mode, d["d"])
    return case, info, d, g, touched, t


@pytest.mark.parametrize("case_id", [c.id for c in R.LOOKUP_CASES])
def test_embed_lookup_bwd_matches_the_float64_scatter(device, case_id):
    from deepctr_amd import ops
    case, info, d, G, touched_ref, Tm = _lookup_reference(case_id)
    V, dim, n = case.vocab, case.dim, case.n
    idx = dev(d["ids"], device)
    if case.strided:
        dbuf, dview = framed(d["d"], 2, 2, device)
        assert dview.stride(0) == dim + 4 and dview.data_ptr() % 16 == 8
    else:
        dbuf = dview = dev(d["d"], device)
    keep = bits(dbuf)
    g0_h, g = g0_like((V, dim), 1.0, 15, device)
    touched = torch.zeros(V * dim // 4, dtype=torch.uint8, device=device) if dim % 4 == 0 else None
    for calls in (1, 2):
        ops.embed_lookup_bwd(idx, (V, dim), case.hash_mode, dview, g, touched=touched)
        torch.cuda.synchronize()
        assert_close_terms(f64(g) - g0_h, calls * G, calls * Tm + np.abs(g0_h), what="%s g_table x%d" % (case.id, calls))
        if touched is not None:
            assert (touched.cpu().numpy() == touched_ref).all(), "%s: the touched bytes are not those of the resolved rows" % case.id
    never = Tm.sum(1) == 0                   # rows no in-range id resolved to: not one bit of them moves
    assert (bits(g)[never] == g0_h.view(np.int32)[never]).all()
    assert (bits(dbuf) == keep).all()
    if dim % 4:
        from deepctr_amd import _C
        with pytest.raises(_C.DctrError) as err:           # touched bytes need whole 16-B groups
            ops.embed_lookup_bwd(idx, (V, dim), case.hash_mode, dview, g, touched=torch.zeros(V, dtype=torch.uint8, device=device))
        assert err.value.rc == E_DIM


def test_embed_lookup_bwd_leaves_its_outputs_alone_at_n_0(device):
    from deepctr_amd import ops
    g = torch.full((7, 8), SENTINEL, device=device)
    touched = torch.zeros(14, dtype=torch.uint8, device=device)
    ops.embed_lookup_bwd(torch.zeros(0, dtype=torch.int32, device=device), (7, 8), 0, torch.zeros(0, 8, device=device), g, touched=touched)
    torch.cuda.synchronize()
    assert same_bits(g, torch.full((7, 8), SENTINEL, device=device)) and not bool(touched.any())


# ---------------------------------------------------------------------------------------------------
# Dice
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dice_reference(case_id):
    case = DICE[case_id]
    info = R.resolve_dice(case)
    d = R.make_dice_data(case)
    z, bias = R.dice_fwd_input(case, d)
    fwd = R.dice_train_fwd(z, bias, d["alpha"], d["moving_mean"], d["moving_var"])
    bwd = {mode: R.dice_bwd_oracle(d, mode) for mode in ("stored", "batch")} if case.kind == "bwd" else {}
    return case, info, d, z, bias, fwd, bwd


@pytest.mark.parametrize("case_id", [c.id for c in R.DICE_CASES])
def test_dice_train_fwd_matches_the_float64_oracle(device, case_id):
    from deepctr_amd import ops
    case, info, d, z_h, bias_h, (G, Tm), _ = _dice_reference(case_id)
    Rr, N = case.R, case.N
    if case.kind == "stride14":
        zbuf, z = framed(z_h, 0, 2, device)
        assert z.stride(0) == 14
    elif case.kind == "off4":
        zbuf = torch.full((Rr * N + 1,), SENTINEL, device=device)
        zbuf[1:] = dev(z_h, device).reshape(-1)
        z = zbuf[1:].view(Rr, N)
        assert z.data_ptr() % 16 == 4 and z.is_contiguous()
    else:
        zbuf = z = dev(z_h, device)
    assert R.dice_route(Rr, N, z.stride(0), z.data_ptr() % 16)["form"] == case.form
    keep = bits(zbuf)
    bias = None if bias_h is None else dev(bias_h, device)
    alpha, mm, mv = dev(d["alpha"], device), dev(d["moving_mean"], device), dev(d["moving_var"], device)
    obuf, out = framed(np.full((Rr, N), np.nan), 1, 1, device)
    bm, bv = ops.dice_train_fwd(z, alpha, mm, mv, out, eps=1e-9, momentum=0.99, bias=bias)
    torch.cuda.synchronize()
    for key, got in (("mean", bm), ("var", bv), ("moving_mean", mm), ("moving_var", mv), ("y", out)):
        assert np.isfinite(f64(got)).all(), "%s %s: not finite" % (case.id, key)
        assert_close_terms(f64(got), G[key], Tm[key], what="%s dice_train_fwd %s" % (case.id, key))
    assert (f64(bv) >= 0).all()
    assert frame_intact(obuf, 1, N) and (bits(zbuf) == keep).all()


def test_dice_train_fwd_refuses_an_empty_batch(device):
    """rows >= 1 is this op's contract (the mean of no rows): refused before any launch, nothing touched."""
    from deepctr_amd import _C, ops
    N = 8
    mm, mv, out = (torch.full(s, SENTINEL, device=device) for s in ((N,), (N,), (3, N)))
    with pytest.raises(_C.DctrError) as err:
        ops.dice_train_fwd(torch.zeros(0, N, device=device), torch.zeros(N, device=device), mm, mv, out)
    torch.cuda.synchronize()
    assert err.value.rc in (E_NULL, E_DIM)      # (the pointers are looked at first, and torch hands out a null one for no elements)
    assert all(same_bits(t, torch.full_like(t, SENTINEL)) for t in (mm, mv, out))


BWD_MODES = ("stored", "batch-recompute", "batch-saved")


@pytest.mark.parametrize("mode", BWD_MODES)
@pytest.mark.parametrize("case_id", [c.id for c in R.DICE_CASES if c.kind == "bwd"])
def test_mlp_bwd_dice_matches_the_float64_oracle(device, case_id, mode):
    """One Dice layer [R, N] behind K = 8 inputs, headless: d_out is the gradient of the layer's output."""
    from deepctr_amd import ops
    case, info, d, _, _, fwd, bwd = _dice_reference(case_id)
    G, Tm = bwd["stored" if mode == "stored" else "batch"]
    Rr, N, K = case.R, case.N, R.DICE_K
    _, x = framed(d["x"], 0, 3, device)
    _, dy = framed(d["dy"], 0, 1, device)
    W, b, alpha = dev(d["W"], device), dev(d["b"], device), dev(d["alpha"], device)
    mm, mv = dev(d["moving_mean"], device), dev(d["moving_var"], device)
    acts = [dev(fwd[0]["y"].astype(np.float32), device)]
    extra = {}
    if mode != "stored":
        bm, bv = R.dice_batch_stats(d)
        extra["dice_batch"] = [(dev(bm, device), dev(bv, device))]
    if mode == "batch-saved":
        extra["saved_z"] = [dev(d["z64"].astype(np.float32), device)]
    g0 = {k: g0_like(G[k].shape, rms(G[k]), 20 + i, device) for i, k in enumerate(("dW", "db", "d_alpha"))}
    dxbuf, dx = torch.full((Rr, K + 2), SENTINEL, device=device), None
    need = RM.workspace_bytes(Rr, [K, N], dice=True)
    ws = torch.full((need // 4 + GUARD,), float("nan"), device=device)
    holder = {"ws": ws}
    one_workgroup = info["grid"] == 1
    first = None
    for calls in (1, 2):
        ops.mlp_bwd(x, K, [W], acts, "dice", None, None, [g0["dW"][1]], [g0["db"][1]], None, dx=dxbuf, d_out=dy, biases=[b],
                    dice=[(alpha, mm, mv)], d_dice_alpha=[g0["d_alpha"][1]], workspace=holder, **extra)
        torch.cuda.synchronize()
        assert holder["ws"] is ws, "%s: the library asks for more workspace than the restated size" % case.id
        assert bool(torch.isnan(ws[need // 4:]).all()), "%s: the op wrote past its workspace size" % case.id
        dz, dx = ws[:Rr * N].view(Rr, N), dxbuf[:, :K]
        for key in ("dW", "db", "d_alpha"):
            h, t = g0[key]
            assert np.isfinite(f64(t)).all()
            assert_close_terms(f64(t) - h, calls * G[key], calls * Tm[key] + np.abs(h), what="%s %s %s x%d" % (case.id, mode, key, calls))
        assert_close_terms(f64(dz), G["dz"], Tm["dz"], what="%s %s dz x%d" % (case.id, mode, calls))
        assert_close_terms(f64(dx), G["dx"], Tm["dx"], what="%s %s dx x%d" % (case.id, mode, calls))
        assert same_bits(dxbuf[:, K:], torch.full((Rr, 2), SENTINEL, device=device)), "%s: dx padding changed" % case.id
        if first is None:
            first = dz.clone()
        elif mode == "stored" or one_workgroup:
            assert same_bits(dz, first), "%s %s: the second writing of dz differs" % (case.id, mode)


# ---------------------------------------------------------------------------------------------------
# the loss
# ---------------------------------------------------------------------------------------------------
def _bce_run(device, pred_h, y_h, w_h, task, direct=False):
    """Two calls from non-zero accumulators; returns the oracle and checks both calls."""
    from deepctr_amd import _C, ops
    B = pred_h.size
    G, Tm = R.bce_grad(pred_h, y_h, task, w_h)
    pred, y = dev(pred_h, device), dev(y_h, device)
    w = None if w_h is None else dev(w_h, device)
    dlogit = torch.full((B + 3,), float("nan"), device=device)
    dlogit[B:] = SENTINEL
    l0, d0 = np.float32(3.25), np.float32(-1.5)
    ls, dsum = torch.full((1,), float(l0), device=device), torch.full((1,), float(d0), device=device)
    first = None
    for calls in (1, 2):
        if direct:
            _C.check(_C.lib().dctr_bce_grad(pred.data_ptr(), y.data_ptr(), B, 0 if task == "binary" else 1, dlogit.data_ptr(), ls.data_ptr(),
                                            dsum.data_ptr(), _C.stream_ptr()), "dctr_bce_grad")
        else:
            ops.bce_grad(pred, y, dlogit[:B], loss_sum=ls, dlogit_sum=dsum, task=task, weight=w)
        torch.cuda.synchronize()
        what = "bce B=%d %s x%d" % (B, task, calls)
        assert np.isfinite(f64(ls)).all() and np.isfinite(f64(dlogit)).all()
        assert_close_terms(f64(ls)[0] - float(l0), calls * G["loss_sum"], calls * Tm["loss_sum"] + abs(float(l0)), what=what + " loss_sum")
        assert_close_terms(f64(dsum)[0] - float(d0), calls * G["dlogit_sum"], calls * Tm["dlogit_sum"] + abs(float(d0)), what=what + " dlogit_sum")
        if first is None:
            first = dlogit.clone()
            assert_close_terms(f64(dlogit[:B]), G["dlogit"], Tm["dlogit"], what=what + " dlogit")
        else:
            assert same_bits(dlogit, first)
    assert same_bits(dlogit[B:], torch.full((3,), SENTINEL, device=device))
    return G


@pytest.mark.parametrize("weight", R.BCE_WEIGHTS)
@pytest.mark.parametrize("task", R.BCE_TASKS)
@pytest.mark.parametrize("B", R.BCE_BATCHES)
def test_bce_grad_matches_the_float64_oracle(device, B, task, weight):
    pred, y, w = R.make_bce_data(B, task, weight)
    _bce_run(device, pred, y, w, task)
    if weight == "none":
        _bce_run(device, pred, y, None, task, direct=True)          # dctr_bce_grad, the entry without weights


def test_bce_grad_at_the_clip_sample_by_sample(device):
    """B = 1 per edge prediction: loss_sum is that sample's loss alone — 16.1 at a saturated wrong prediction, never inf or nan."""
    p, y = R.bce_edges()
    for pv, yv in zip(p, y):
        G = _bce_run(device, np.asarray([pv], np.float32), np.asarray([yv], np.float32), None, "binary")
        assert np.isfinite(G["loss_sum"]) and G["loss_sum"] <= 16.2


def test_bce_grad_leaves_its_outputs_alone_at_batch_0(device):
    from deepctr_amd import ops
    e = torch.zeros(0, device=device)
    outs = [torch.full((4,), SENTINEL, device=device) for _ in range(3)]
    for task in R.BCE_TASKS:
        ops.bce_grad(e, e, outs[0], loss_sum=outs[1], dlogit_sum=outs[2], task=task)
    torch.cuda.synchronize()
    assert all(same_bits(t, torch.full((4,), SENTINEL, device=device)) for t in outs)
