"""GPU parity tests, op level, of the two scatter kernels every HIP training step ends in — dctr_embed_gather_fm_bwd and
dctr_embed_pool_bwd (csrc/embed_bwd_kernels.hip) — and of dctr_fm_bwd (csrc/interaction_bwd_kernels.hip), dctr_dense1_bwd
(csrc/dnn_train_kernels.hip), dctr_din_softmax_fwd/_bwd (csrc/din_train_kernels.hip) and dctr_seq_weight_fwd,
against the float64 oracle of tests/ref_embed_bwd.py (pinned without a GPU by tests/test_embed_bwd_oracle_cpu.py).

Bar: tests.util.assert_close_terms' defaults — 1e-4 of the result plus 2e-6 of the summed magnitude.  The kernels ACCUMULATE, so every
gradient buffer starts at a non-zero g0 and ``g - g0`` is compared; g0 is one more summand of the fp32 sum the kernel forms, so |g0|
joins the oracle's ``terms``.  Memory that must not change (rows no id resolved to, guard elements) and the touched bytes are compared
exactly.  The shapes are the smallest that reach each branch of the kernels (LPR instantiations, the chunk loop, VEC = 1, the LDS
accumulators' three limits, identity fields, hashing, out-of-range ids)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import ref_numpy as R
from tests import ref_embed_bwd as RB
from tests.util import assert_close_terms

pytestmark = pytest.mark.gpu


def dev(a, device, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(device)


def _lpr(width):
    """Lanes per row of the 16-B form of gather_fm_bwd_kernel / pool_bwd_kernel."""
    lpr = 1
    while lpr * 4 < width and lpr < 16:
        lpr <<= 1
    return lpr


def _check_scatter(got, g0, ref, terms, calls, hit_rows, what):
    """``got`` = g0 + calls * ref within the bar; rows outside ``hit_rows`` bit-identical to g0."""
    got, g0 = np.asarray(got), np.asarray(g0)
    assert_close_terms(got.astype(np.float64) - g0.astype(np.float64), calls * ref, calls * terms + np.abs(g0.astype(np.float64)), what=what)
    idle = np.ones(got.shape[0], bool)
    idle[hit_rows] = False
    assert (got[idle] == g0[idle]).all(), "%s: a row no id resolved to changed" % what


def _check_touched(touched, got, g0, hit_rows, what, superset_of=None):
    """The touched bytes of a [V, D] gradient table (D % 4 == 0; one byte per 16-B group): every group that changed has its byte set,
    the rows with a byte set are exactly ``hit_rows`` (or, with ``superset_of``: lie between that set and ``hit_rows``), rows never
    resolved have every byte clear, bytes are 0 or 1."""
    V, D = got.shape
    t = touched.cpu().numpy().reshape(V, D // 4)
    assert np.isin(t, (0, 1)).all(), "%s: a touched byte that is neither 0 nor 1" % what
    t = t.astype(bool)
    changed = (np.asarray(got) != np.asarray(g0)).reshape(V, D // 4, 4).any(-1)
    assert not (changed & ~t).any(), "%s: a 16-B group changed with its touched byte clear" % what
    hit = np.zeros(V, bool)
    hit[hit_rows] = True
    assert not t[~hit].any(), "%s: a touched byte set in a row no id resolved to" % what
    if superset_of is None:
        assert (t.any(1) == hit).all(), "%s: rows with a touched byte != rows resolved" % what
    else:
        need = np.zeros(V, bool)
        need[superset_of] = True
        assert not (need & ~t.any(1)).any() and not (t.any(1) & ~hit).any(), "%s: marked rows outside [expected, resolved]" % what


# ---------------------------------------------------------------------------------------------
# dctr_embed_gather_fm_bwd
# ---------------------------------------------------------------------------------------------
def _gather_bwd_case(device, B, dims, vocab, n_dense=0, hash_modes=None, ids64=False, in_fm=None, seed=0, lin=True, identity=None,
                     no_offset=(), frozen=(), use=("d_in", "d_fm", "d_lin"), keep_dnn_in=True, d_extra=0, dense_rows=None, n_lin_w=None,
                     dense_extra=0, oor=False, calls=1, what="gather_bwd"):
    """Forward (dctr_embed_gather_fm, args struct kept) -> gradient buffers at g0 -> ops.embed_gather_fm_bwd ``calls`` times ->
    g - g0 against the oracle.  ``no_offset``: fields outside the DNN input (out_offset -1); ``frozen``: fields whose g_table is NULL;
    ``keep_dnn_in`` False: fwd.dnn_in NULL in the backward (the FM term reads the tables); ``d_extra``: columns d_dnn_in is wider than the
    DNN input by; ``dense_rows`` / ``n_lin_w``: dense column -> row of a Linear.kernel of n_lin_w rows; ``oor``: ids -1 and vocab."""
    from deepctr_amd import _C, ops
    rng = np.random.RandomState(seed)
    F = len(dims)
    hash_modes = hash_modes or [0] * F
    in_fm = in_fm if in_fm is not None else [1] * F
    identity = identity or [0] * F
    vocab = [B if identity[j] else vocab[j] for j in range(F)]
    tables = [rng.standard_normal((vocab[j], dims[j])).astype(np.float32) * 0.3 for j in range(F)]
    lins = [rng.standard_normal(vocab[j]).astype(np.float32) * 0.1 if lin else None for j in range(F)]
    raw = np.stack([rng.randint(0, 2 ** 31 - 1 if hash_modes[j] else vocab[j], B) for j in range(F)]).astype(np.int64 if ids64 else np.int32)
    if oor:
        for j in range(F):
            if not hash_modes[j] and not identity[j]:
                raw[j, (3 * j) % B] = -1
                raw[j, (3 * j + 1) % B] = vocab[j]
    offs, end = [], 0
    for j in range(F):
        offs.append(-1 if j in no_offset else end)
        end += 0 if j in no_offset else dims[j]
    all4 = all(d % 4 == 0 for d in dims)
    stride = (end + n_dense + 3) // 4 * 4
    dense = rng.rand(B, n_dense + dense_extra).astype(np.float32) if n_dense else None
    linw = rng.standard_normal(n_dense).astype(np.float32) if n_dense else None
    n_lin_w = n_dense if n_lin_w is None else n_lin_w
    t_dev = [dev(t, device) for t in tables]
    l_dev = [None if l_ is None else dev(l_, device) for l_ in lins]
    spec = [dict(table=tables[j], lin_table=lins[j], vocab=vocab[j], dim=dims[j], out_offset=offs[j], in_fm=in_fm[j],
                 hash_mode=hash_modes[j], identity=identity[j]) for j in range(F)]
    desc = ops.make_field_descriptors([dict(spec[j], table=t_dev[j], lin_table=l_dev[j]) for j in range(F)], device)
    ids = dev(raw, device)
    dense_dev = None if dense is None else dev(dense, device)[:, :n_dense]
    linw_dev = None if linw is None else dev(linw, device)
    dnn_in = torch.full((B, stride), float("nan"), device=device)
    fm, ll, status = torch.empty(B, device=device), torch.empty(B, device=device), ops.new_status(device)

    def fwd_args(dnn_in):
        return ops.make_gather_args(desc, F, ids, B, 1, B, max(dims), all4, any(hash_modes), dense=dense_dev, dense_lin_w=linw_dev,
                                    dense_out_offset=end, dnn_in=dnn_in, out_stride=stride, fm_logit=fm, lin_logit=ll, status=status,
                                    any_identity=any(identity))
    args = fwd_args(dnn_in)
    _C.check(_C.lib().dctr_embed_gather_fm(ctypes.byref(args), _C.stream_ptr()), "dctr_embed_gather_fm")
    if not keep_dnn_in:
        args = fwd_args(None)
    # gradient buffers: a non-zero start everywhere; Linear.kernel's gradient with a guard element either side
    g0_t = [rng.standard_normal((vocab[j], dims[j])).astype(np.float32) * 0.5 for j in range(F)]
    g0_l = [rng.standard_normal(vocab[j]).astype(np.float32) * 0.5 for j in range(F)]
    g_t = [None if j in frozen else dev(g0_t[j], device) for j in range(F)]
    g_l = [dev(g0_l[j], device) if lin else None for j in range(F)]
    tch = [torch.zeros(vocab[j] * dims[j] // 4, dtype=torch.uint8, device=device)
           if (dims[j] % 4 == 0 and not identity[j] and g_t[j] is not None) else None for j in range(F)]
    grads = ops.make_field_grads([(g_t[j], g_l[j], tch[j]) for j in range(F)], device)
    d_cols = stride + d_extra
    d_in = rng.standard_normal((B, d_cols)).astype(np.float32)
    d_in[:, end:] = np.nan                                   # (the dense columns and everything past them: never read)
    d_fm, d_lin = rng.standard_normal(B).astype(np.float32), rng.standard_normal(B).astype(np.float32)
    g0_d = rng.standard_normal(n_lin_w + 2).astype(np.float32) * 0.5
    g_d = dev(g0_d, device) if n_dense else None
    rows_dev = None if dense_rows is None else dev(np.asarray(dense_rows, np.int32), device)
    d_in_dev, d_fm_dev, d_lin_dev = dev(d_in, device), dev(d_fm, device), dev(d_lin, device)
    for _ in range(calls):
        ops.embed_gather_fm_bwd(args, grads, d_dnn_in=d_in_dev if "d_in" in use else None, d_fm=d_fm_dev if "d_fm" in use else None,
                                d_lin=d_lin_dev if "d_lin" in use else None, g_dense_lin_w=None if g_d is None else g_d[1:1 + n_lin_w],
                                dense_lin_rows=rows_dev)
    torch.cuda.synchronize()
    val, trm = RB.gather_fm_bwd(spec, raw, d_in=d_in if "d_in" in use else None, d_fm=d_fm if "d_fm" in use else None,
                                d_lin=d_lin if "d_lin" in use else None, dense=None if dense is None else dense[:, :n_dense],
                                dense_lin_rows=dense_rows, n_lin_w=n_lin_w)
    hits = [r[ok] for r, ok in RB.field_rows(spec, raw)]
    exp = RB.touched_expected(spec, raw)
    for j in range(F):
        tag = "%s field %d (dim %d, vocab %d)" % (what, j, dims[j], vocab[j])
        if g_t[j] is not None:
            got = g_t[j].cpu().numpy()
            _check_scatter(got, g0_t[j], val["g_table"][j], trm["g_table"][j], calls, hits[j], tag + " g_table")
            if tch[j] is not None:
                _check_touched(tch[j], got, g0_t[j], exp[j], tag + " touched")
        if g_l[j] is not None:
            _check_scatter(g_l[j].cpu().numpy(), g0_l[j], val["g_lin"][j], trm["g_lin"][j], calls, hits[j], tag + " g_lin")
    if g_d is not None:
        got = g_d.cpu().numpy()
        assert got[0] == g0_d[0] and got[-1] == g0_d[-1], "%s: a guard element of g_dense_lin_w changed" % what
        fed = np.arange(n_dense) if dense_rows is None else np.asarray([r for r in dense_rows if r >= 0], np.int64)
        _check_scatter(got[1:-1], g0_d[1:-1], val["g_dense_lin_w"], trm["g_dense_lin_w"], calls, fed, what + " g_dense_lin_w")


@pytest.mark.parametrize("hashed", [False, True])
@pytest.mark.parametrize("width", [4, 8, 16, 32, 64, 12])
def test_gather_bwd_every_instantiation(device, width, hashed):
    """LPR 1, 2, 4, 8, 16 (and width 12: LPR 4 with a lane per sample that owns no chunk), HASH on and off; one sample, and two full waves
    of samples plus one (a ragged last workgroup whose other waves idle).  Vocabularies past 64: the global-atomics path."""
    for B in (1, 2 * (64 // _lpr(width)) + 1):
        _gather_bwd_case(device, B, [width] * 5, [70, 90, 100, 65, 200], n_dense=2, hash_modes=[1, 0, 2, 0, 0] if hashed else None,
                         seed=width + B, what="width %d B %d" % (width, B))


@pytest.mark.parametrize("width", [68, 128, 132, 3, 10, 17, 102])
def test_gather_bwd_chunk_loop(device, width):
    """Rows wider than the lanes of a sample hold at once: two and three trips of the chunk loop at VEC = 4 (68 / 128, 132), two and seven at
    VEC = 1 (17, 102; 3 and 10 take one) — FM on, so the barrier inside the loop and the per-chunk S run, on both the LDS (vocabulary 5) and
    the global path, with the touched bytes of every chunk."""
    for B in (1, 2 * 4 + 1, 37):                       # (16 lanes per sample in both forms: 4 samples per wave)
        _gather_bwd_case(device, B, [width] * 3, [70, 5, 90], n_dense=1, seed=width + B, what="width %d B %d" % (width, B))


def test_gather_bwd_mixed_widths(device):
    # DIN-like: one width that is no multiple of 4 puts every field on the element-per-lane form; touched bytes for the other three
    _gather_bwd_case(device, 37, [10, 4, 8, 4], [3, 2, 4, 3], n_dense=1, in_fm=[0, 1, 0, 1], seed=4, what="[10,4,8,4]")
    _gather_bwd_case(device, 37, [10, 4, 8, 4], [70, 80, 90, 100], n_dense=1, in_fm=[0, 1, 0, 1], seed=5, what="[10,4,8,4] global")
    # widths that differ, all multiples of 4: LPR from the widest, FM over the two equal ones
    _gather_bwd_case(device, 37, [8, 16, 4, 8], [50, 60, 70, 5], in_fm=[1, 0, 0, 1], seed=6, what="[8,16,4,8]")
    _gather_bwd_case(device, 37, [8, 16, 4], [50, 60, 70], in_fm=[0, 0, 0], seed=7, what="[8,16,4]")


LDS_CASES = {
    # (a) vocabularies 2, 7, 64: all three accumulate in LDS
    "all_fit": dict(dims=[8, 8, 8], vocab=[2, 7, 64]),
    # (b) SMALL_VOCAB: 64 rows in LDS, 65 rows by global atomics, same width
    "vocab_64_against_65": dict(dims=[8, 8], vocab=[64, 65]),
    # (c) SMALL_FLOATS: 64 * 17 floats fit, the second such field does not, (2, 16) fits again — both paths in one launch
    "budget_overflows_mid_list": dict(dims=[16, 16, 16], vocab=[64, 64, 2]),
    # (d) SMALL_FIELDS: 130 fields of 3 * 5 floats; the first 128 fill 1920 of the 2048 floats, fields 128 and 129 go global
    "more_than_128_fields": dict(dims=[4] * 130, vocab=[3] * 130),
    # (e) a frozen table with a trainable linear table: no LDS rows for it, its linear gradient by global atomics
    "frozen_table_trainable_linear": dict(dims=[8, 8, 8], vocab=[5, 6, 7], frozen=(1,)),
}


@pytest.mark.parametrize("name", sorted(LDS_CASES))
def test_gather_bwd_lds_accumulators(device, name):
    for B in (33, 100):                         # (LPR 2 / 4 / 1: several workgroups, each flushing its own accumulators)
        _gather_bwd_case(device, B, seed=B + len(name), what=name, **LDS_CASES[name])


@pytest.mark.parametrize("B", [21, 130])
def test_gather_bwd_identity_fields(device, B):
    """A pooled sequence enters the gather as an identity field whose "table" is the batch (row b for sample b): 21 rows accumulate in
    LDS, 130 go to global memory; with its linear vector."""
    _gather_bwd_case(device, B, [8, 8, 8], [50, 0, 6], identity=[0, 1, 0], n_dense=1, seed=B, what="identity B %d" % B)
    _gather_bwd_case(device, B, [8, 6], [0, 9], identity=[1, 0], seed=B + 1, what="identity, element per lane, B %d" % B)


@pytest.mark.parametrize("ids64", [False, True])
def test_gather_bwd_id_handling(device, ids64):
    """hash_mode 1 and 2 beside plain fields, both id types; ids -1 and vocab in the plain fields leave every gradient and every touched
    byte alone (the oracle skips them and counts them as zero in the FM sum of their sample)."""
    _gather_bwd_case(device, 70, [16] * 6, [1000, 30, 40, 7, 200, 64], hash_modes=[1, 2, 0, 0, 2, 1], ids64=ids64, n_dense=2, oor=True,
                     seed=11 + ids64, what="hashed + out of range")
    _gather_bwd_case(device, 41, [5, 8, 4], [9, 100, 3], hash_modes=[2, 0, 1], ids64=ids64, oor=True, seed=13 + ids64,
                     what="hashed + out of range, element per lane")
    _gather_bwd_case(device, 41, [8, 8, 8], [9, 100, 3], ids64=ids64, oor=True, seed=15 + ids64, what="out of range, no hashing")


OPERANDS = {
    "no_d_dnn_in": dict(use=("d_fm", "d_lin")),
    "no_d_fm": dict(use=("d_in", "d_lin")),
    "no_d_lin": dict(use=("d_in", "d_fm")),
    "field_outside_the_dnn_input": dict(no_offset=(1,)),
    "no_linear_tables": dict(lin=False),
    "fm_term_from_the_tables": dict(keep_dnn_in=False),
    "fm_term_from_dnn_in": dict(keep_dnn_in=True),
    "d_dnn_in_wider_than_the_fields": dict(d_extra=8),
}


@pytest.mark.parametrize("name", sorted(OPERANDS))
@pytest.mark.parametrize("dims", [[8, 8, 8, 8], [8, 6, 8, 3]])
def test_gather_bwd_operand_combinations(device, name, dims):
    kw = dict(OPERANDS[name])
    if name == "d_dnn_in_wider_than_the_fields" and any(d % 4 for d in dims):
        kw["d_extra"] = 7
    _gather_bwd_case(device, 70, dims, [100, 6, 80, 70], n_dense=3, in_fm=[1, 0, 1, 0] if any(d % 4 for d in dims) else None,
                     seed=len(name), what=name, **kw)


@pytest.mark.parametrize("n_dense", [1, 4, 7])
@pytest.mark.parametrize("rows", ["identity", "permutation", "with_gaps"])
def test_gather_bwd_dense_linear(device, n_dense, rows):
    """d Linear.kernel[rows[k]] += sum_b d_lin[b] dense[b, k]: every dense column by one wave (1, 4 and 7 columns over 4 waves), the row map
    NULL, a permutation into a longer kernel, or with -1 entries; dense rows wider than n_dense; the guard elements stay."""
    rng = np.random.RandomState(n_dense)
    n_w = n_dense + 3
    dense_rows = None if rows == "identity" else list(rng.permutation(n_w)[:n_dense])
    if rows == "with_gaps":
        dense_rows[0] = -1
        if n_dense > 4:
            dense_rows[5] = -1
    for B, dims in ((1, [8, 8]), (70, [8, 8]), (37, [6])):
        _gather_bwd_case(device, B, dims, [50] * len(dims), n_dense=n_dense, dense_rows=dense_rows, n_lin_w=None if dense_rows is None else n_w,
                         dense_extra=5, seed=B + n_dense, what="dense %d %s" % (n_dense, rows))


def test_gather_bwd_accumulates(device):
    """A second identical call doubles g - g0 (LDS and global rows, both forms), within the same bar."""
    _gather_bwd_case(device, 70, [16, 16, 16], [64, 64, 2], n_dense=2, calls=2, seed=21, what="two calls")
    _gather_bwd_case(device, 37, [10, 4, 8, 4], [3, 200, 4, 3], n_dense=1, in_fm=[0, 1, 0, 1], calls=2, seed=22, what="two calls, element per lane")


# ---------------------------------------------------------------------------------------------
# dctr_embed_pool_bwd
# ---------------------------------------------------------------------------------------------
POOL_SHAPES = ((37, 10, 8, 20), (5, 1, 4, 3), (70, 50, 32, 1000), (9, 7, 3, 6), (33, 5, 68, 12), (6, 3, 20, 4), (40, 6, 17, 9))


def _pool_ids(rng, B, T, V, by_len, hash_mode=0, ids64=False, oor=False):
    """As test_embed_pool builds them: a full row, an empty row, ids past the length zeroed, one interior zero under mask_zero — and, from
    T = 3 on, one id twice inside a sample."""
    ids = rng.randint(1, 10 ** 6 if hash_mode else V, (B, T)).astype(np.int64 if ids64 else np.int32)
    lens = rng.randint(0, T + 1, B).astype(np.int32)
    lens[0] = T
    if B > 1:
        lens[1] = 0
    ids[np.arange(T)[None, :] >= lens[:, None]] = 0
    if not by_len and B > 2 and T > 2:
        ids[2, 1] = 0
    if T >= 3:
        ids[0, 2] = ids[0, 0]
    if oor:
        ids[0, 1], ids[B - 1, 0] = V, -1
        if B > 3 and T > 1:
            ids[3, :] = V + 7                        # a sample of nothing but out-of-range ids
    return ids, lens


def _pool_bwd_case(device, shape, combiner, by_len, weighted, seed=0, hash_mode=0, ids64=False, oor=False, lin=True, lin_only=False,
                   strided=False, calls=1):
    from deepctr_amd import ops
    B, T, E, V = shape
    rng = np.random.RandomState(seed)
    table = rng.standard_normal((V, E)).astype(np.float32)          # (continuous: different rows never tie under max)
    lin_t = rng.standard_normal(V).astype(np.float32) if lin else None
    ids, lens = _pool_ids(rng, B, T, V, by_len, hash_mode, ids64, oor)
    w = rng.standard_normal((B, T, 1)).astype(np.float32) if weighted is not None else None
    keep = []
    ops.embed_pool(dev(ids, device), dev(table, device), combiner, length=dev(lens, device) if by_len else None,
                   weight=None if w is None else dev(w, device), weight_norm=bool(weighted), lin_table=None if lin_t is None else dev(lin_t, device),
                   hash_mode=hash_mode, keep_args=keep)
    a, _alive = keep[0]
    pad = 8 if E % 4 == 0 else 5
    d_full = rng.standard_normal((B, E + pad)).astype(np.float32)
    d_out = d_full[:, 4:4 + E] if strided else np.ascontiguousarray(d_full[:, :E])
    d_dev = dev(d_full, device)[:, 4:4 + E] if strided else dev(d_out, device)
    d_lin = rng.standard_normal(B).astype(np.float32)
    g0, g0_l = rng.standard_normal((V, E)).astype(np.float32) * 0.5, rng.standard_normal(V).astype(np.float32) * 0.5
    g = None if lin_only else dev(g0, device)
    g_l = dev(g0_l, device) if lin else None
    tch = torch.zeros(V * E // 4, dtype=torch.uint8, device=device) if (E % 4 == 0 and g is not None) else None
    for _ in range(calls):
        ops.embed_pool_bwd(a, d_out=None if lin_only else d_dev, d_lin_out=dev(d_lin, device) if lin else None, g_table=g, g_lin_table=g_l,
                           touched=tch)
    torch.cuda.synchronize()
    (vt, vl), (at, al) = RB.pool_bwd(table, lin_t, ids, None if lin_only else d_out, d_lin if lin else None, combiner,
                                     lens if by_len else None, w, bool(weighted), hash_mode)
    rows, ok, _ = RB.pool_masks(ids, V, hash_mode, lens if by_len else None)
    hit = np.unique(rows[ok])
    what = "pool_bwd %s by_len=%s weighted=%s %s" % (combiner, by_len, weighted, shape)
    if g is not None:
        got = g.cpu().numpy()
        _check_scatter(got, g0, vt, at, calls, hit, what + " g_table")
        if tch is not None:
            # mark_rows marks every row an id resolved to, masked ones included: expected rows <= marked rows <= rows resolved in range
            _check_touched(tch, got, g0, hit, what + " touched", superset_of=np.nonzero((vt != 0).any(1))[0])
    if g_l is not None:
        _check_scatter(g_l.cpu().numpy(), g0_l, vl, al, calls, hit, what + " g_lin")


@pytest.mark.parametrize("combiner", ["sum", "mean", "max"])
@pytest.mark.parametrize("by_len", [False, True])
@pytest.mark.parametrize("weighted", [None, True, False])
def test_pool_bwd(device, combiner, by_len, weighted):
    """Widths 8 / 4 / 32 / 68 / 20 (16-B form: LPR 2, 1, 8, 16 with two trips, 8 with idle lanes) and 3 / 17 (element per lane, 17 in two
    trips); weights none, softmax-normalised (True) and raw (False)."""
    for n, shape in enumerate(POOL_SHAPES):
        _pool_bwd_case(device, shape, combiner, by_len, weighted, seed=3 + n)


@pytest.mark.parametrize("combiner", ["sum", "mean", "max"])
@pytest.mark.parametrize("variant", ["hash_int64", "out_of_range", "no_lin_table", "linear_only", "strided_d_out", "two_calls"])
def test_pool_bwd_variants(device, combiner, variant):
    kw = {"hash_int64": dict(hash_mode=2, ids64=True), "out_of_range": dict(oor=True), "no_lin_table": dict(lin=False),
          "linear_only": dict(lin_only=True), "strided_d_out": dict(strided=True), "two_calls": dict(calls=2)}[variant]
    for n, shape in enumerate(((37, 10, 8, 20), (9, 7, 3, 6), (33, 5, 68, 12))):
        for by_len, weighted in ((False, None), (True, True), (False, False)):
            _pool_bwd_case(device, shape, combiner, by_len, weighted, seed=40 + n, **kw)


# ---------------------------------------------------------------------------------------------
# argument errors: refused before any launch
# ---------------------------------------------------------------------------------------------
def test_embed_bwd_argument_errors(device):
    from deepctr_amd import _C, ops
    B = 8
    # touched bytes beside a table whose width is no multiple of 4
    keep = []
    ops.embed_pool(torch.ones(B, 3, dtype=torch.int32, device=device), torch.ones(5, 6, device=device), "sum", keep_args=keep)
    g = torch.zeros(5, 6, device=device)
    with pytest.raises(_C.DctrError):
        ops.embed_pool_bwd(keep[0][0], d_out=torch.ones(B, 6, device=device), g_table=g, touched=torch.zeros(8, dtype=torch.uint8, device=device))
    # a d_out row stride that is no multiple of 4 beside a width that is
    keep = []
    ops.embed_pool(torch.ones(B, 3, dtype=torch.int32, device=device), torch.ones(5, 8, device=device), "sum", keep_args=keep)
    g8 = torch.zeros(5, 8, device=device)
    with pytest.raises(_C.DctrError):
        ops.embed_pool_bwd(keep[0][0], d_out=torch.ones(B, 9, device=device)[:, :8], g_table=g8)
    assert (g == 0).all() and (g8 == 0).all()
    # the same for d_dnn_in, and record-form tables (any_pitch) in the forward arguments
    table = torch.ones(5, 8, device=device)
    desc = ops.make_field_descriptors([dict(table=table, vocab=5, dim=8, out_offset=0, in_fm=1)], device)
    ids = torch.ones(1, B, dtype=torch.int32, device=device)
    gt = torch.zeros(5, 8, device=device)
    grads = ops.make_field_grads([(gt, None)], device)
    with pytest.raises(_C.DctrError):
        ops.embed_gather_fm_bwd(ops.make_gather_args(desc, 1, ids, B, 1, B, 8, True, False, out_stride=8), grads,
                                d_dnn_in=torch.ones(B, 9, device=device)[:, :8])
    with pytest.raises(_C.DctrError):
        ops.embed_gather_fm_bwd(ops.make_gather_args(desc, 1, ids, B, 1, B, 8, True, False, out_stride=8, any_pitch=True), grads,
                                d_dnn_in=torch.ones(B, 8, device=device))
    assert (gt == 0).all()


# ---------------------------------------------------------------------------------------------
# dctr_fm_bwd, dctr_dense1_bwd, dctr_din_softmax_fwd / _bwd, dctr_seq_weight_fwd
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,F,E", [(1, 1, 1), (70, 5, 5), (257, 26, 16)])
@pytest.mark.parametrize("accumulate", [False, True])
def test_fm_bwd(device, B, F, E, accumulate):
    """x and dx as column-offset views of wider buffers; accumulate False overwrites a NaN-filled dx, True adds to what is there."""
    from deepctr_amd import ops
    rng = np.random.RandomState(B)
    n = F * E
    xb = rng.standard_normal((B, n + 7)).astype(np.float32)
    d = rng.standard_normal(B).astype(np.float32)
    dx0 = rng.standard_normal((B, n + 9)).astype(np.float32)
    if not accumulate:
        dx0[:, 4:4 + n] = np.nan
    dxb = dev(dx0, device)
    ops.fm_bwd(dev(xb, device)[:, 3:3 + n], F, E, dev(d, device), dxb[:, 4:4 + n], accumulate=accumulate)
    got = dxb.cpu().numpy()
    ref, terms = RB.fm_bwd(xb[:, 3:3 + n].reshape(B, F, E), d)
    assert (got[:, :4] == dx0[:, :4]).all() and (got[:, 4 + n:] == dx0[:, 4 + n:]).all(), "guard columns of dx changed"
    start = dx0[:, 4:4 + n].astype(np.float64) if accumulate else np.zeros((B, n))
    assert_close_terms(got[:, 4:4 + n].astype(np.float64) - start, ref.reshape(B, n), terms.reshape(B, n) + np.abs(start), what="fm_bwd")


@pytest.mark.parametrize("n", [1, 5, 257, 1030, 8, 256])
@pytest.mark.parametrize("B", [1, 300])
def test_dense1_bwd(device, n, B):
    """Strided x and dx; d_w accumulates onto a non-zero start.  8 and 256 columns at 16-B aligned views take the 16-B form of the kernel,
    the other widths (and views at an odd column) the column-per-thread one."""
    from deepctr_amd import ops
    rng = np.random.RandomState(n + B)
    off, wide = (4, n + 8) if n % 4 == 0 else (3, n + 5)
    xb = rng.standard_normal((B, wide)).astype(np.float32)
    w, d = rng.standard_normal(n).astype(np.float32), rng.standard_normal(B).astype(np.float32)
    dx0 = rng.standard_normal((B, wide)).astype(np.float32)
    gw0 = rng.standard_normal(n + 2).astype(np.float32) if n % 4 else rng.standard_normal(n + 8).astype(np.float32)
    lo = 1 if n % 4 else 4
    dxb, gw = dev(dx0, device), dev(gw0, device)
    ops.dense1_bwd(dev(xb, device)[:, off:off + n], n, dev(w, device), dev(d, device), dxb[:, off:off + n], gw[lo:lo + n])
    got, got_w = dxb.cpu().numpy(), gw.cpu().numpy()
    (rx, rw), (tx, tw) = RB.dense1_bwd(xb[:, off:off + n], w, d)
    assert (got[:, :off] == dx0[:, :off]).all() and (got[:, off + n:] == dx0[:, off + n:]).all(), "guard columns of dx changed"
    assert (got_w[:lo] == gw0[:lo]).all() and (got_w[lo + n:] == gw0[lo + n:]).all(), "guard elements of d_w changed"
    assert_close_terms(got[:, off:off + n], rx, tx, what="dense1_bwd dx")
    start = gw0[lo:lo + n].astype(np.float64)
    assert_close_terms(got_w[lo:lo + n].astype(np.float64) - start, rw, tw + np.abs(start), what="dense1_bwd d_w")


@pytest.mark.parametrize("T", [1, 63, 64, 65, 130])
def test_din_softmax_fwd_bwd(device, T):
    """One wave per row, positions lane-strided (T below, at and past 64); a row without a valid position is exactly uniform forward and
    gets a zero d_score; d_score aliases dp as models/sequence/din.py calls it; d_bias accumulates."""
    from deepctr_amd import ops
    rng = np.random.RandomState(T)
    B = 7
    s, dp = rng.standard_normal((B, T)).astype(np.float32) * 2, rng.standard_normal((B, T)).astype(np.float32)
    mask = rng.rand(B, T) < 0.6
    mask[0], mask[1] = True, False
    m_dev = dev(mask.astype(np.uint8), device)
    p = ops.din_softmax(dev(s, device), m_dev, torch.full((B, T), float("nan"), device=device))
    ref, terms = RB.din_softmax(s, mask)
    got = p.cpu().numpy()
    assert (got[1] == np.float32(1) / np.float32(T)).all(), "a row without a valid position must be exactly uniform"
    assert_close_terms(got, ref, terms, what="din_softmax")
    b0 = np.float32(0.75)
    d_bias = torch.full((1,), float(b0), device=device)
    ds = dev(dp, device)
    ops.din_softmax_bwd(p, m_dev, ds, ds, d_bias)
    (rs, rb), (ts, tb) = RB.din_softmax_bwd(ref, mask, dp)
    got = ds.cpu().numpy()
    assert (got[1] == 0).all() and (got[~mask] == 0).all()
    assert_close_terms(got, rs, ts, what="din_softmax_bwd d_score")
    assert_close_terms(float(d_bias.item()) - float(b0), rb, tb + float(b0), what="din_softmax_bwd d_bias")


@pytest.mark.parametrize("by_len", [False, True])
@pytest.mark.parametrize("norm", [False, True])
def test_seq_weight(device, by_len, norm):
    from deepctr_amd import ops
    for n, (B, T, E) in enumerate(((9, 7, 5), (5, 70, 4), (1, 1, 1))):
        rng = np.random.RandomState(n)
        seq, w = rng.standard_normal((B, T, E)).astype(np.float32), rng.standard_normal((B, T, 1)).astype(np.float32)
        lens = rng.randint(1, T + 1, B).astype(np.int32)
        if B > 1:
            lens[1] = 0                                   # one row with every position masked
        mask = R.sequence_mask(lens, T)
        if not by_len and T > 2:
            mask[0, 1] = False                            # (a mask is no prefix)
        kw = dict(lengths=lens) if by_len else dict(mask=mask)
        ref = R.weighted_sequence(seq.astype(np.float64), w.astype(np.float64), weight_normalization=norm, **kw)
        out = ops.seq_weight(dev(seq, device), dev(w, device), mask=None if by_len else dev(mask, device),
                             length=dev(lens, device) if by_len else None, weight_norm=norm)
        assert_close_terms(out.cpu().numpy(), ref, np.abs(ref), what="seq_weight")
