"""Pins tests/ref_embed_bwd.py (the float64 oracle the GPU tests of dctr_embed_gather_fm_bwd / dctr_embed_pool_bwd compare with)
without a GPU: the forward (gather + FM + linear; weighted_sequence + sequence_pooling) is restated in torch double, the restatement is
checked against oracle/ref_numpy.py on the same inputs, and torch autograd through it must equal the oracle's closed forms.

Bar: 1e-12 of the summed magnitude of each element (the oracle's ``terms`` — both sides are float64 sums of the same summands in
different orders, so their difference scales with the magnitude summed, a few 1e-16 of it per summand)."""
import numpy as np
import pytest
import torch

from oracle import ref_numpy as R
from tests import ref_embed_bwd as RB


def _close(got, ref, terms, what):
    got, ref, terms = (np.asarray(a, np.float64) for a in (got, ref, terms))
    assert got.shape == ref.shape, what
    err = np.abs(got - ref)
    bar = 1e-12 * np.maximum(terms, np.abs(ref))
    assert (err <= bar).all(), "%s: max err %.3g at a bar of %.3g" % (what, err.max(), bar[np.unravel_index(err.argmax(), err.shape)])


def _t(a, grad=False):
    return torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=grad)


# ---------------------------------------------------------------------------------------------
# gather + concat + FM + linear
# ---------------------------------------------------------------------------------------------
def _gather_inputs(seed, B, dims, vocab, hash_modes, in_fm, offs, n_dense, dense_rows, n_lin_w, oor, ids64=False, identity=None):
    rng = np.random.RandomState(seed)
    F = len(dims)
    identity = identity or [0] * F
    fields = []
    for j in range(F):
        V = B if identity[j] else vocab[j]
        fields.append(dict(table=rng.standard_normal((V, dims[j])).astype(np.float32), lin_table=rng.standard_normal(V).astype(np.float32),
                           vocab=V, dim=dims[j], out_offset=offs[j], in_fm=in_fm[j], hash_mode=hash_modes[j], identity=identity[j]))
    ids = np.stack([rng.randint(0, 2 ** 31 - 1 if hash_modes[j] else vocab[j], B) for j in range(F)]).astype(np.int64 if ids64 else np.int32)
    if oor:
        for j in range(F):
            if not hash_modes[j] and not identity[j]:
                ids[j, j % B] = -1
                ids[j, (j + 2) % B] = vocab[j]
    dense = rng.rand(B, n_dense) if n_dense else None
    total = max([o + d for o, d in zip(offs, dims) if o >= 0] + [0])
    return dict(fields=fields, ids=ids, dense=dense, dense_rows=dense_rows, n_lin_w=n_lin_w if n_lin_w is not None else n_dense,
                d_in=rng.standard_normal((B, total + 3)), d_fm=rng.standard_normal(B), d_lin=rng.standard_normal(B),
                lin_w=rng.standard_normal(n_lin_w if n_lin_w is not None else n_dense) if n_dense else None, total=total)


def _gather_forward(c, tables, lins, lin_w):
    """torch double: dnn_in [B,total], fm [B], lin [B]; out-of-range rows read as zero."""
    fields, B = c["fields"], c["ids"].shape[1]
    rows = RB.field_rows(fields, c["ids"])
    e = []
    for f, t, (r, ok) in zip(fields, tables, rows):
        e.append(t[torch.from_numpy(np.where(ok, r, 0))] * torch.from_numpy(ok.astype(np.float64))[:, None])
    dnn_in = torch.zeros(B, c["total"], dtype=torch.float64)
    for f, ej in zip(fields, e):
        if f["out_offset"] >= 0:
            dnn_in = dnn_in + torch.nn.functional.pad(ej, (f["out_offset"], c["total"] - f["out_offset"] - f["dim"]))
    width = max(f["dim"] for f in fields)
    fm_e = [torch.nn.functional.pad(ej, (0, width - f["dim"])) for f, ej in zip(fields, e) if f["in_fm"]]
    fm = torch.zeros(B, dtype=torch.float64)
    if fm_e:
        x = torch.stack(fm_e, dim=1)                                                   # [B,F,E]
        fm = 0.5 * (x.sum(1) ** 2 - (x * x).sum(1)).sum(-1)
    lin = torch.zeros(B, dtype=torch.float64)
    for f, l_, (r, ok) in zip(fields, lins, rows):
        lin = lin + l_[torch.from_numpy(np.where(ok, r, 0))] * torch.from_numpy(ok.astype(np.float64))
    if c["dense"] is not None:
        to = np.arange(c["dense"].shape[1]) if c["dense_rows"] is None else np.asarray(c["dense_rows"])
        for k in range(c["dense"].shape[1]):
            if to[k] >= 0:
                lin = lin + _t(c["dense"][:, k]) * lin_w[int(to[k])]
    return dnn_in, fm, lin, e


GATHER_CASES = {
    "uniform":        dict(B=37, dims=[8] * 5, vocab=[5, 70, 9, 100, 3], hash_modes=[0] * 5, in_fm=[1] * 5, offs=[0, 8, 16, 24, 32], n_dense=3,
                           dense_rows=None, n_lin_w=None, oor=False),
    "mixed_hashed":   dict(B=41, dims=[10, 4, 8, 4], vocab=[3, 20, 4, 30], hash_modes=[0, 1, 0, 2], in_fm=[0, 1, 0, 1], offs=[0, 10, 14, 22],
                           n_dense=4, dense_rows=[2, -1, 0, 4], n_lin_w=5, oor=False, ids64=True),
    "oor_no_offset":  dict(B=29, dims=[4, 4, 4], vocab=[6, 7, 8], hash_modes=[0, 2, 0], in_fm=[1, 1, 1], offs=[0, -1, 4], n_dense=2,
                           dense_rows=[1, 0], n_lin_w=2, oor=True),
    "identity":       dict(B=21, dims=[8, 8, 8], vocab=[9, 21, 5], hash_modes=[0] * 3, in_fm=[1] * 3, offs=[0, 8, 16], n_dense=0, dense_rows=None,
                           n_lin_w=None, oor=True, identity=[0, 1, 0]),
}


@pytest.mark.parametrize("name", sorted(GATHER_CASES))
def test_gather_fm_bwd_oracle_is_the_derivative_of_the_forward(name):
    c = _gather_inputs(seed=len(name), **GATHER_CASES[name])
    fields = c["fields"]
    tables = [_t(f["table"], True) for f in fields]
    lins = [_t(f["lin_table"], True) for f in fields]
    lin_w = _t(c["lin_w"], True) if c["dense"] is not None else None
    dnn_in, fm, lin, e = _gather_forward(c, tables, lins, lin_w)
    # the restatement is the oracle's forward (in-range samples: ref_numpy refuses an out-of-range index, the kernels read it as zero)
    rows = RB.field_rows(fields, c["ids"])
    good = np.all([ok for _, ok in rows], axis=0)
    for f, ej, (r, ok) in zip(fields, e, rows):
        assert (ej.detach().numpy()[ok] == R.embedding(f["table"].astype(np.float64), r[ok])).all()
        assert (ej.detach().numpy()[~ok] == 0).all()
        if f["out_offset"] >= 0:
            assert (dnn_in.detach().numpy()[:, f["out_offset"]:f["out_offset"] + f["dim"]] == ej.detach().numpy()).all()
    fm_fields = [(f, ej) for f, ej in zip(fields, e) if f["in_fm"]]
    assert len({f["dim"] for f, _ in fm_fields}) == 1                     # (R.fm takes equal widths)
    x = np.stack([ej.detach().numpy() for _, ej in fm_fields], axis=1)
    _close(fm.detach().numpy(), R.fm(x)[:, 0], 0.5 * (np.square(np.abs(x).sum(1)) + np.square(x).sum(1)).sum(-1), "fm forward")
    sparse = np.stack([np.where(ok, f["lin_table"].astype(np.float64)[np.where(ok, r, 0)], 0.0) for f, (r, ok) in zip(fields, rows)], axis=1)
    if c["dense"] is not None:
        to = np.arange(c["dense"].shape[1]) if c["dense_rows"] is None else np.asarray(c["dense_rows"])
        kernel = np.where(to >= 0, c["lin_w"][np.maximum(to, 0)], 0.0)[:, None]          # the kernel rows the dense columns feed
        ref_lin = R.linear(sparse[:, None, :], c["dense"], kernel)[:, 0]
        mag = np.abs(sparse).sum(1) + np.abs(c["dense"]) @ np.abs(kernel[:, 0])
    else:
        ref_lin, mag = R.linear(sparse[:, None, :])[:, 0, 0], np.abs(sparse).sum(1)
    _close(lin.detach().numpy(), ref_lin, mag, "linear forward")
    assert good.sum() >= 0.8 * good.size
    # autograd of  <d_in, dnn_in> + <d_fm, fm> + <d_lin, lin>  against the oracle's closed form, every operand subset
    for use in ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0)):
        loss = torch.zeros((), dtype=torch.float64)
        if use[0]:
            loss = loss + (dnn_in * _t(c["d_in"][:, :c["total"]])).sum()
        if use[1]:
            loss = loss + (fm * _t(c["d_fm"])).sum()
        if use[2]:
            loss = loss + (lin * _t(c["d_lin"])).sum()
        leaves = tables + lins + ([lin_w] if lin_w is not None else [])
        grads = torch.autograd.grad(loss, leaves, allow_unused=True, retain_graph=True)
        grads = [torch.zeros_like(p) if g is None else g for g, p in zip(grads, leaves)]
        val, trm = RB.gather_fm_bwd(fields, c["ids"], d_in=c["d_in"] if use[0] else None, d_fm=c["d_fm"] if use[1] else None,
                                    d_lin=c["d_lin"] if use[2] else None, dense=c["dense"], dense_lin_rows=c["dense_rows"],
                                    n_lin_w=c["n_lin_w"])
        F = len(fields)
        for j in range(F):
            _close(grads[j].numpy(), val["g_table"][j], trm["g_table"][j], "%s g_table[%d] use=%s" % (name, j, use))
            _close(grads[F + j].numpy(), val["g_lin"][j], trm["g_lin"][j], "%s g_lin[%d] use=%s" % (name, j, use))
        if lin_w is not None:
            _close(grads[2 * F].numpy(), val["g_dense_lin_w"], trm["g_dense_lin_w"], "%s g_dense_lin_w use=%s" % (name, use))
    # touched_expected: exactly the rows with an in-range id (tables of width % 4 == 0 only)
    exp = RB.touched_expected(fields, c["ids"])
    assert sorted(exp) == [j for j, f in enumerate(fields) if f["dim"] % 4 == 0]
    for j, rset in exp.items():
        r, ok = rows[j]
        assert set(rset.tolist()) == {int(v) for v, k in zip(r, ok) if k} and all(0 <= v < fields[j]["vocab"] for v in rset)
    if GATHER_CASES[name]["oor"]:
        assert not good.all()


def test_gather_fm_bwd_oracle_skips_out_of_range_rows():
    """An out-of-range id leaves every gradient alone and counts as zero in the FM sum of its sample."""
    t = [np.arange(8, dtype=np.float32).reshape(2, 4) + 1, np.ones((3, 4), np.float32)]
    fields = [dict(table=t[j], lin_table=np.ones(t[j].shape[0], np.float32), vocab=t[j].shape[0], dim=4, out_offset=4 * j, in_fm=1)
              for j in range(2)]
    ids = np.array([[1, 2, -1], [0, 1, 3]])
    val, _ = RB.gather_fm_bwd(fields, ids, d_in=np.zeros((3, 8)), d_fm=np.ones(3), d_lin=np.ones(3))
    assert (val["g_table"][0] == np.array([[0, 0, 0, 0], [1, 1, 1, 1.]])).all()        # sample 0 only: S - e_0 = e_1
    assert (val["g_table"][1] == np.array([[5, 6, 7, 8.], [0, 0, 0, 0], [0, 0, 0, 0]])).all()   # sample 1: field 0 out of range -> S = e_1
    assert (val["g_lin"][0] == [0, 1]).all() and (val["g_lin"][1] == [1, 1, 0]).all()
    assert RB.touched_expected(fields, ids)[0].tolist() == [1] and RB.touched_expected(fields, ids)[1].tolist() == [0, 1]


# ---------------------------------------------------------------------------------------------
# weighted_sequence + sequence_pooling
# ---------------------------------------------------------------------------------------------
def _pool_inputs(seed, B, T, E, V, by_len, weighted, hash_mode=0, oor=False):
    rng = np.random.RandomState(seed)
    table = rng.standard_normal((V, E)).astype(np.float32)
    lin = rng.standard_normal(V).astype(np.float32)
    ids = rng.randint(1, 10 ** 6 if hash_mode else V, (B, T)).astype(np.int64 if hash_mode else np.int32)
    lens = rng.randint(0, T + 1, B).astype(np.int32)
    lens[0] = T
    if B > 1:
        lens[1] = 0
    ids[np.arange(T)[None, :] >= lens[:, None]] = 0
    if not by_len and B > 2 and T > 2:
        ids[2, 1] = 0
    if T >= 3:
        ids[0, 2] = ids[0, 0]                                              # one id twice inside a sample
    if oor:
        ids[0, 1], ids[B - 1, 0] = V, -1
    w = rng.standard_normal((B, T, 1)).astype(np.float32) if weighted is not None else None
    return table, lin, ids, lens, w


def _pool_forward(table, lin, ids, lens, w, combiner, by_len, weighted, hash_mode):
    """torch double restatement; max selects its position with the reference's float32 expression (RB.max_hist)."""
    V = table.shape[0]
    rows, ok, mask = RB.pool_masks(ids, V, hash_mode, lens if by_len else None)
    B, T = rows.shape
    safe, okf, m = torch.from_numpy(np.where(ok, rows, 0)), torch.from_numpy(ok.astype(np.float64)), torch.from_numpy(mask.astype(np.float64))
    outs = []
    for tab in (table, lin[:, None]):
        seq = tab[safe] * okf[:, :, None]                                  # [B,T,E]
        if w is not None:
            ww = _t(w)[:, :, 0]
            if weighted:
                ww = torch.softmax(torch.where(m > 0, ww, torch.full_like(ww, -2.0 ** 32 + 1)), dim=1)
            else:
                ww = ww * m
            seq = seq * ww[:, :, None]
        if combiner == "max":
            hist = seq - (1 - m)[:, :, None] * 1e9
            first = RB.max_hist(tab.detach().numpy().astype(np.float32), rows, ok, mask, w, bool(weighted)).argmax(axis=1)
            outs.append(torch.gather(hist, 1, torch.from_numpy(first)[:, None, :])[:, 0, :])
            continue
        out = (seq * m[:, :, None]).sum(1)
        if combiner == "mean":
            length = m.sum(1) if not by_len else _t(lens)
            out = out / (length[:, None] + 1e-8)
        outs.append(out)
    return outs[0], outs[1][:, 0], rows, ok, mask


@pytest.mark.parametrize("combiner", ["sum", "mean", "max"])
@pytest.mark.parametrize("by_len", [False, True])
@pytest.mark.parametrize("weighted", [None, True, False])
def test_pool_bwd_oracle_is_the_derivative_of_the_forward(combiner, by_len, weighted):
    for n, (B, T, E, V, hash_mode, oor) in enumerate(((37, 10, 8, 20, 0, False), (5, 1, 4, 3, 0, False), (9, 7, 3, 6, 0, True),
                                                      (23, 6, 5, 11, 2, False))):
        table, lin, ids, lens, w = _pool_inputs(10 * n + len(combiner), B, T, E, V, by_len, weighted, hash_mode, oor)
        tt, tl = _t(table, True), _t(lin, True)
        out, lout, rows, ok, mask = _pool_forward(tt, tl, ids, lens, w, combiner, by_len, weighted, hash_mode)
        # the restatement is oracle/ref_numpy.py's forward
        kw = dict(lengths=lens) if by_len else dict(mask=mask)
        for tab, got in ((table, out), (lin[:, None], lout[:, None])):
            seq = np.where(ok[:, :, None], tab.astype(np.float64)[np.where(ok, rows, 0)], 0.0)
            if w is not None:
                seq = R.weighted_sequence(seq, w.astype(np.float64), weight_normalization=bool(weighted), **kw)
            ref = R.sequence_pooling(seq, combiner, **kw)[:, 0, :]
            some = mask.any(1) if combiner == "max" else np.ones(B, bool)
            # (max over a sample without a valid position: every entry is -1e9 in float32, the first one by the rule the kernels
            # follow, while float64 still tells the entries apart — compared in float32 below)
            _close(got.detach().numpy()[some], ref[some], np.abs(ref[some]), "pool forward %s" % combiner)
            if combiner == "max":
                h32 = RB.max_hist(tab, rows, ok, mask, w, bool(weighted))
                seq32 = np.where(ok[:, :, None], tab.astype(np.float32)[np.where(ok, rows, 0)], np.float32(0))
                if w is not None:
                    seq32 = R.weighted_sequence(seq32, w, weight_normalization=bool(weighted), **kw)
                ref32 = R.sequence_pooling(seq32, "max", **kw)[:, 0, :]
                assert h32.dtype == np.float32 and (h32.max(axis=1) == ref32).all()       # bit for bit: the reference's own expression
                assert (np.take_along_axis(h32, h32.argmax(axis=1)[:, None, :], 1)[:, 0, :] == ref32).all()
        d_out, d_lin = np.random.RandomState(n).standard_normal((B, E)), np.random.RandomState(n + 50).standard_normal(B)
        g_t, g_l = torch.autograd.grad((out * _t(d_out)).sum() + (lout * _t(d_lin)).sum(), [tt, tl])
        (vt, vl), (at, al) = RB.pool_bwd(table, lin, ids, d_out, d_lin, combiner, lens if by_len else None, w, bool(weighted), hash_mode)
        _close(g_t.numpy(), vt, at, "pool g_table %s by_len=%s weighted=%s case %d" % (combiner, by_len, weighted, n))
        _close(g_l.numpy(), vl, al, "pool g_lin %s by_len=%s weighted=%s case %d" % (combiner, by_len, weighted, n))
        assert np.abs(vt).sum() > 0 and np.abs(vl).sum() > 0


def test_pool_bwd_oracle_max_goes_to_the_first_position():
    """A repeated id and an all-padding sample: the gradient of max lands once, on the first position that attains it."""
    table = np.array([[0.5, -1.0], [2.0, 3.0], [1.0, 4.0]], np.float32)
    ids = np.array([[1, 2, 1], [0, 0, 0]], np.int32)
    d = np.array([[1.0, 10.0], [100.0, 1000.0]])
    (g, _), _ = RB.pool_bwd(table, None, ids, d_out=d, combiner="max")
    assert (g == np.array([[100.0, 1000.0], [1.0, 0.0], [0.0, 10.0]])).all()


# ---------------------------------------------------------------------------------------------
# the small entry points
# ---------------------------------------------------------------------------------------------
def test_small_backward_oracles_match_autograd():
    rng = np.random.RandomState(0)
    x, d = rng.standard_normal((7, 5, 3)), rng.standard_normal(7)
    xt = _t(x, True)
    y = torch.from_numpy(R.fm(x)[:, 0])
    fm = 0.5 * (xt.sum(1) ** 2 - (xt * xt).sum(1)).sum(-1)
    _close(fm.detach().numpy(), y.numpy(), 0.5 * (np.square(np.abs(x).sum(1)) + np.square(x).sum(1)).sum(-1), "fm")
    v, t = RB.fm_bwd(x, d)
    _close(torch.autograd.grad((fm * _t(d)).sum(), xt)[0].numpy(), v, t, "fm_bwd")
    x2, w = rng.standard_normal((9, 6)), rng.standard_normal(6)
    d2 = rng.standard_normal(9)
    xt, wt = _t(x2, True), _t(w, True)
    gx, gw = torch.autograd.grad(((xt @ wt) * _t(d2)).sum(), [xt, wt])
    (vx, vw), (tx, tw) = RB.dense1_bwd(x2, w, d2)
    _close(gx.numpy(), vx, tx, "dense1 dx")
    _close(gw.numpy(), vw, tw, "dense1 d_w")
    s, dp = rng.standard_normal((6, 9)), rng.standard_normal((6, 9))
    mask = rng.rand(6, 9) < 0.6
    mask[0], mask[1] = True, False
    st = _t(s, True)
    p = torch.softmax(torch.where(torch.from_numpy(mask), st, torch.full_like(st, -2.0 ** 32 + 1)), dim=1)
    pv, _ = RB.din_softmax(s, mask)
    _close(p.detach().numpy(), pv, pv, "din_softmax")
    assert (pv[1] == 1.0 / 9).all()
    (ds, db), (dsa, dba) = RB.din_softmax_bwd(pv, mask, dp)
    _close(torch.autograd.grad((p * _t(dp)).sum(), st)[0].numpy(), ds, dsa, "din_softmax_bwd")
    assert (ds[1] == 0).all() and abs(db - ds.sum()) <= 1e-12 * dba
