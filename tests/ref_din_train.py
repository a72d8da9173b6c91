"""What tests/test_gpu_din_train_oracle.py and tests/test_din_train_oracle_cpu.py share:
  1. float64 NumPy oracles, closed form and without autograd, of the kernels only the DIN training step uses and of the loss of every
     single-task step: dctr_din_att_in_fwd / _bwd, dctr_din_wsum_fwd / _bwd, dctr_din_softmax_fwd / _bwd
     (deepctr_amd/csrc/din_train_kernels.hip), dctr_embed_lookup_bwd (deepctr_amd/csrc/embed_bwd_kernels.hip), dctr_dice_train_fwd and
     the Dice branch of dctr_mlp_bwd (deepctr_amd/csrc/dnn_train_kernels.hip) and dctr_bce_grad / dctr_bce_grad_w
     (deepctr_amd/csrc/loss_kernels.hip);
  2. a restatement of the host arithmetic that picks each kernel's form and sizes its grid;
  3. the tables of cases the GPU test runs, each with the route it is there for.
The CPU test pins 1 against torch double autograd and 2 and 3 against each other.

Every oracle returns (result, terms).  ``terms`` is the input of tests.util.assert_close_terms: the same computation over absolute
values, an upper bound of the magnitude each output element was summed at.  Dice's sigmoid takes a DIFFERENCE scaled by
1 / sqrt(var + eps): its argument is rounded at the magnitude c = (|z| + |mean|) / sqrt(var + eps), and that reaches every output
through p' = p (1 - p); the Dice terms carry p + p (1 - p) c where the value has p, and p (1 - p) (1 + c) where it has p (1 - p)."""
import collections
import zlib

import numpy as np

from tests import ref_embed_bwd as RE

din_softmax, din_softmax_bwd = RE.din_softmax, RE.din_softmax_bwd           # layers/sequence.py:283-289 and its derivative


def _f64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


# ---------------------------------------------------------------------------------------------------
# the oracles: DIN's attention pieces
# ---------------------------------------------------------------------------------------------------
def att_in(q, k):
    """LocalActivationUnit's input (reference layers/core.py:94-108): a[b T + t] = [q_b, k_bt, q_b - k_bt, q_b * k_bt], q [B, E],
    k [B, T, E] -> [B T, 4 E].  One float32 operation per element: the result is exact in float32 and the comparison is of bits,
    so this one oracle is float32 NumPy and its terms are None."""
    q, k = np.asarray(q, np.float32), np.asarray(k, np.float32)
    B, T, E = k.shape
    qq = np.broadcast_to(q[:, None, :], (B, T, E))
    return np.concatenate([qq, k, qq - k, qq * k], axis=-1).reshape(B * T, 4 * E), None


def att_in_bwd(da, q, k):
    """Derivative of att_in (layers/core.py:94-108), da [B T, 4 E] = (d0, d1, d2, d3):
        dq[b, e] = sum_t (d0 + d2 + d3 k[b, t, e])  — the op adds it into the columns ``qcol`` of dx;
        dk[b, t, e] = d1 - d2 + d3 q[b, e]          — the op adds it to dk."""
    q, k = _f64(q), _f64(k)
    B, T, E = k.shape
    d = _f64(da).reshape(B, T, 4, E)
    a = np.abs(d)
    G = {"dq": (d[:, :, 0] + d[:, :, 2] + d[:, :, 3] * k).sum(1), "dk": d[:, :, 1] - d[:, :, 2] + d[:, :, 3] * q[:, None, :]}
    T_ = {"dq": (a[:, :, 0] + a[:, :, 2] + a[:, :, 3] * np.abs(k)).sum(1), "dk": a[:, :, 1] + a[:, :, 2] + a[:, :, 3] * np.abs(q)[:, None, :]}
    return G, T_


def wsum(score, mask, k, drop=None):
    """AttentionSequencePoolingLayer without weight normalization (layers/sequence.py:286-296): out[b, e] = sum_t (mask ? score : 0)
    k[b, t, e].  score [B T] or [B, T], mask [B, T], k [B, T, E].  ``drop`` = (b, t): that position is left out of row b's sums — the
    wrong restatement of the CPU test."""
    k = _f64(k)
    B, T, E = k.shape
    s = np.where(np.asarray(mask).reshape(B, T) != 0, _f64(score).reshape(B, T), 0.0)
    if drop is not None:
        s[drop] = 0.0
    return np.einsum("bt,bte->be", s, k), np.einsum("bt,bte->be", np.abs(s), np.abs(k))


def wsum_bwd(d_out, score, mask, k):
    """Derivative of wsum: d_score[b, t] = mask ? <d_out[b], k[b, t]> : 0;  dk[b, t] = (mask ? score : 0) d_out[b] (WRITTEN);
    d_bias = sum d_score (the bias of the unit's Dense(1), layers/core.py:106; ADDED)."""
    k, g = _f64(k), _f64(d_out)
    B, T, E = k.shape
    m = np.asarray(mask).reshape(B, T) != 0
    s = np.where(m, _f64(score).reshape(B, T), 0.0)
    ds, tds = np.where(m, np.einsum("be,bte->bt", g, k), 0.0), np.where(m, np.einsum("be,bte->bt", np.abs(g), np.abs(k)), 0.0)
    dk = s[:, :, None] * g[:, None, :]
    return {"d_score": ds, "dk": dk, "d_bias": ds.sum()}, {"d_score": tds, "dk": np.abs(dk), "d_bias": tds.sum()}


# ---------------------------------------------------------------------------------------------------
# the scatter of dctr_embed_lookup
# ---------------------------------------------------------------------------------------------------
def lookup_bwd(ids, vocab, dim, hash_mode, d, forget_row=None):
    """Backward of embedding_lookup (reference inputs.py:101-117) on n ids: g[row(ids[i]), :] += d[i, :dim], ids that resolve outside
    [0, vocab) skipped.  Returns ((g [vocab, dim], touched), terms): ``touched`` the expected touched bytes — one per 16-B group of
    every row some id resolved to — or None when dim % 4 != 0 (such tables carry none).  ``forget_row``: the run of that row is left
    out — the wrong restatement of the CPU test."""
    rows = RE.resolve_rows(np.asarray(ids).reshape(-1), vocab, hash_mode)
    ok = (rows >= 0) & (rows < vocab)
    if forget_row is not None:
        ok &= rows != forget_row
    d = _f64(d).reshape(rows.size, dim)
    r = rows[ok]
    g = np.stack([np.bincount(r, weights=d[ok, c], minlength=vocab) for c in range(dim)], axis=1).reshape(vocab, dim)
    t = np.stack([np.bincount(r, weights=np.abs(d[ok, c]), minlength=vocab) for c in range(dim)], axis=1).reshape(vocab, dim)
    touched = None
    if dim % 4 == 0:
        hit = np.zeros(vocab, dtype=np.uint8)
        hit[r] = 1
        touched = np.repeat(hit, dim // 4)
    return (g, touched), t


# ---------------------------------------------------------------------------------------------------
# Dice (reference layers/activation.py:51-64)
# ---------------------------------------------------------------------------------------------------
def _dice_parts(z, mean, var, eps, zmag):
    """rs, xn, p and the magnitude c the sigmoid's argument was formed at."""
    rs = 1.0 / np.sqrt(var + eps)
    xn = (z - mean) * rs
    p = 1.0 / (1.0 + np.exp(-xn))
    return rs, xn, p, (zmag + np.abs(mean)) * rs


def dice_train_fwd(z, bias, alpha, moving_mean, moving_var, eps=1e-9, momentum=0.99, ddof=0):
    """Dice.call under training=True (layers/activation.py:51-64: BatchNormalization(center=False, scale=False, epsilon=1e-9) with
    the training flag) on pre-activations z [R, N] (+ bias [N] or None): this batch's mean and BIASED variance over every row, the
    stored statistics moved by ``momentum`` (float32, as the layer holds it), y = z (alpha + (1 - alpha) p),
    p = sigmoid((z - mean) / sqrt(var + eps)).  ``ddof`` = 1 divides the variance by R - 1: the wrong restatement of the CPU test."""
    z = _f64(z)
    b = np.zeros(z.shape[1]) if bias is None else _f64(bias)
    al, zb, zmag = _f64(alpha), z + b, np.abs(z) + np.abs(b)
    R = z.shape[0]
    mean = zb.sum(0) / R
    var = np.square(zb - mean).sum(0) / (R - ddof)
    tmean, tvar = zmag.sum(0) / R, np.square(zmag + np.abs(mean)).sum(0) / (R - ddof)
    mom = float(np.float32(momentum))
    one_m = float(np.float32(1) - np.float32(momentum))
    rs, xn, p, c = _dice_parts(zb, mean, var, eps, zmag)
    G = {"mean": mean, "var": var, "moving_mean": _f64(moving_mean) * mom + mean * one_m, "moving_var": _f64(moving_var) * mom + var * one_m,
         "y": zb * (al + (1 - al) * p)}
    T = {"mean": tmean, "var": tvar, "moving_mean": np.abs(_f64(moving_mean)) * mom + tmean * one_m,
         "moving_var": np.abs(_f64(moving_var)) * mom + tvar * one_m, "y": zmag * (np.abs(al) + (1 + np.abs(al)) * (p + p * (1 - p) * c))}
    return G, T


def dice_bwd_stored(z, dy, alpha, mean, var, eps=1e-9, zmag=None):
    """Dice with given (stored) statistics, the comment block above dice_bwd_kernel (dnn_train_kernels.hip):
        dz = dy (alpha + (1 - alpha) p + z (1 - alpha) p (1 - p) rs);   d_alpha = sum_rows dy z (1 - p)
    z [R, N] with the bias in it, ``zmag`` the magnitude z was summed at (default |z|)."""
    z, dy, al = _f64(z), _f64(dy), _f64(alpha)
    zmag = np.abs(z) if zmag is None else _f64(zmag)
    rs, xn, p, c = _dice_parts(z, _f64(mean), _f64(var), eps, zmag)
    a1, ady = 1 + np.abs(al), np.abs(dy)
    tp, tq = p + p * (1 - p) * c, p * (1 - p) * (1 + c)
    G = {"dz": dy * (al + (1 - al) * p + z * (1 - al) * p * (1 - p) * rs), "d_alpha": (dy * z * (1 - p)).sum(0)}
    T = {"dz": ady * (np.abs(al) + a1 * tp + zmag * a1 * tq * rs), "d_alpha": (ady * zmag * (1 - p + p * (1 - p) * c)).sum(0)}
    return G, T


def dice_bwd_batch(z, dy, alpha, mean, var, eps=1e-9, zmag=None):
    """Dice under training=True, ``mean`` / ``var`` this batch's statistics, the gradient flows through them (the comment block above
    dice_colstat_kernel, dnn_train_kernels.hip):
        xn = (z - mean) rs;  dxn = dy z (1 - alpha) p (1 - p);  d_alpha = sum_rows dy z (1 - p)
        dz = dy (alpha + (1 - alpha) p) + rs (dxn - mean_rows(dxn) - xn mean_rows(dxn xn))"""
    z, dy, al = _f64(z), _f64(dy), _f64(alpha)
    zmag = np.abs(z) if zmag is None else _f64(zmag)
    rs, xn, p, c = _dice_parts(z, _f64(mean), _f64(var), eps, zmag)
    a1, ady = 1 + np.abs(al), np.abs(dy)
    tp, tq = p + p * (1 - p) * c, p * (1 - p) * (1 + c)
    dxn, tdxn = dy * z * (1 - al) * p * (1 - p), ady * zmag * a1 * tq
    G = {"dz": dy * (al + (1 - al) * p) + rs * (dxn - dxn.mean(0) - xn * (dxn * xn).mean(0)), "d_alpha": (dy * z * (1 - p)).sum(0)}
    m2 = (dxn * xn).mean(0)
    T = {"dz": ady * (np.abs(al) + a1 * tp) + rs * (tdxn + tdxn.mean(0) + np.abs(xn) * (tdxn * c).mean(0) + c * np.abs(m2)),
         "d_alpha": (ady * zmag * (1 - p + p * (1 - p) * c)).sum(0)}
    return G, T


def dense_bwd(x, W, G, T):
    """What dctr_mlp_bwd makes of a one-layer DNN's dz: dW += x^T dz, db += sum_rows dz, dx = dz W^T (written).  Adds them to G / T."""
    x, W = _f64(x), _f64(W)
    G.update(dW=x.T @ G["dz"], db=G["dz"].sum(0), dx=G["dz"] @ W.T)
    T.update(dW=np.abs(x).T @ T["dz"], db=T["dz"].sum(0), dx=T["dz"] @ np.abs(W).T)
    return G, T


# ---------------------------------------------------------------------------------------------------
# the loss
# ---------------------------------------------------------------------------------------------------
BCE_LO = np.float32(1e-7)                                   # tf.keras backend.epsilon(), in float32 as float32 Keras holds it
BCE_HI = np.float32(1) - np.float32(1e-7)


def bce_grad(pred, y, task="binary", weight=None):
    """dctr_bce_grad / dctr_bce_grad_w as include/dctr.h and the comment in bce_grad_kernel state them, B = pred.size:
      binary: loss_b = -(y log pc + (1 - y) log(1 - pc)), pc = clip(pred, 1e-7, 1 - 1e-7);  dlogit_b = (pred - y) / B
      mse:    loss_b = (pred - y)^2;  dlogit_b = 2 (pred - y) / B
      weight (tf.keras' sample_weight, reduction SUM_OVER_BATCH_SIZE): loss_b and dlogit_b times weight_b
      loss_sum = sum_b loss_b, dlogit_sum = sum_b dlogit_b (both ADDED to by the op).
    The clip bounds and 1 - pc are FLOAT32 values, as float32 Keras forms them; the logarithms are float64.
    Open, and not settled here: Keras' gradient through clip_by_value is zero outside the clip, the op returns (pred - y) / B
    everywhere.  Nothing pins which of the two the training step should follow; this oracle restates the op's contract."""
    p32 = np.asarray(pred, np.float32).reshape(-1)
    p, t = _f64(p32), _f64(y).reshape(-1)
    B = p.size
    if task == "binary":
        pc = np.minimum(np.maximum(p32, BCE_LO), BCE_HI)
        la, lb = np.log(_f64(pc)), np.log(_f64(np.float32(1) - pc))
        l, tl = -(t * la + (1 - t) * lb), np.abs(t * la) + np.abs((1 - t) * lb)
        ds, tds = (p - t) / B, (np.abs(p) + np.abs(t)) / B
    elif task == "mse":
        l, tl = np.square(p - t), np.square(np.abs(p) + np.abs(t))
        ds, tds = 2 * (p - t) / B, 2 * (np.abs(p) + np.abs(t)) / B
    else:
        raise ValueError(task)
    if weight is not None:
        w = _f64(weight).reshape(-1)
        l, tl, ds, tds = l * w, tl * np.abs(w), ds * w, tds * np.abs(w)
    return {"dlogit": ds, "loss_sum": l.sum(), "dlogit_sum": ds.sum()}, {"dlogit": tds, "loss_sum": tl.sum(), "dlogit_sum": tds.sum()}


# ---------------------------------------------------------------------------------------------------
# the host arithmetic of the routes, restated from the .hip files
# ---------------------------------------------------------------------------------------------------
DIN_CAP = 16384             # din_train_kernels.hip: workgroups of every launcher there
COLSUM_MAX_WG = 64          # train_common.h
BWD_ROWS = 16               # train_common.h: rows per trip of the one-thread-per-column Dice passes
LB_TILE = 1024              # embed_bwd_kernels.hip: positions a workgroup of lookup_bwd_tile_kernel sorts
LOOKUP_PLAIN_CAP, MARK_ROWS_CAP, DICE_APPLY_CAP = 16384, 4096, 4096


def _ceil_div(a, b):
    return -(-a // b)


def din_grid(piece, B, T, E):
    """(workgroups wanted, cap) of a DIN piece's main kernel: one thread per element, one wave per (b, t) or one wave per row."""
    want = {"att_in": _ceil_div(B * T * E, 256), "att_in_bwd": _ceil_div(B * E, 256), "wsum": _ceil_div(B * E, 256),
            "wsum_bwd": _ceil_div(B * T, 4), "softmax": _ceil_div(B, 4), "softmax_bwd": _ceil_div(B, 4)}[piece]
    return want, DIN_CAP


def sum_vec_grid(n):
    """sum_vec_kernel behind dctr_din_wsum_bwd / dctr_din_softmax_bwd (d_bias): 2048 elements per workgroup, at most COLSUM_MAX_WG."""
    return min(max(_ceil_div(n, 256 * 8), 1), COLSUM_MAX_WG)


def lookup_route(vocab, dim, n):
    """dctr_embed_lookup_bwd: the sorted-tile kernel for 3 <= dim <= 64 from LB_TILE positions on, else one atomic per element."""
    return "tile" if 3 <= dim <= 64 and vocab < 0xffffffff and n >= LB_TILE else "plain"


def lookup_dimP(dim):
    p = 1
    while p < dim:
        p <<= 1
    return p


def rowlane4_ok(N, stride, offset_bytes=0):
    """train_common.h: the shapes the 16-B row-lane kernels take."""
    return N % 4 == 0 and 4 <= N <= 1024 and stride % 4 == 0 and offset_bytes % 16 == 0


def colsum_grid(rows, RL):
    return max(1, min(_ceil_div(rows, RL * 4), 128 if rows >= 32768 else COLSUM_MAX_WG))


def rows_grid(rows, column_sums=True):
    return max(1, min(_ceil_div(rows, BWD_ROWS), COLSUM_MAX_WG if column_sums else 16384))


def dice_route(R, N, stride=None, offset_bytes=0):
    """The form of the Dice passes for z [R, N] on row stride ``stride`` (default N): dict(form, and per form RL / idle threads / grid /
    column passes), apply_cap2: dice_apply_kernel's grid-stride loop takes a second trip."""
    stride = N if stride is None else stride
    info = {"apply_cap2": _ceil_div(R * N, 256) > DICE_APPLY_CAP}
    if rowlane4_ok(N, stride, offset_bytes):
        N4 = N // 4
        RL = 256 // N4
        info.update(form="lane4", RL=RL, idle=256 - RL * N4, grid=colsum_grid(R, RL), strided_trips=_ceil_div(R, RL * colsum_grid(R, RL)))
    else:
        info.update(form="scalar", passes=_ceil_div(N, 256), grid=rows_grid(R), strided_trips=_ceil_div(_ceil_div(R, BWD_ROWS), rows_grid(R)))
    return info


# ---------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------
def _seed(*key):
    return zlib.crc32("/".join(str(k) for k in key).encode()) & 0x7fffffff


def _normal(rng, *shape):
    return rng.standard_normal(shape, dtype=np.float32)


# --- DIN's attention pieces.  pieces: which ops run the case;  mask: "random" (70 % valid, row 0 and the last row without a valid
# position when B > 2), "none", "full", "alt" ((b + t) odd);  cap2: the pieces whose grid-stride loop takes a second trip, else the case
# no longer reaches what it was made for and the tests FAIL;  sum_vec_many: sum_vec_kernel runs on more than one workgroup
DinCase = collections.namedtuple("DinCase", "id shape pieces mask cap2 sum_vec_many why")
DIN_PIECES = ("att_in", "att_in_bwd", "wsum", "wsum_bwd", "softmax", "softmax_bwd")


def _din_cases():
    out = []

    def add(shape, pieces=DIN_PIECES, mask="random", cap2=(), svm=False, why=""):
        out.append(DinCase("din-%s-%s" % ("x".join(str(s) for s in shape), mask), tuple(shape), tuple(pieces), mask, tuple(cap2), svm, why))
    add((1, 1, 1), mask="full", why="smallest shape")
    add((1, 1, 1), mask="none", why="one row, no valid position")
    add((37, 6, 8), why="ordinary small shape")
    for kind in ("none", "full", "alt"):
        add((37, 6, 8), mask=kind, why="mask edge")
    add((5, 65, 70), why="the wave loop e += 64 runs twice; T past one wave in softmax")
    add((3, 130, 16), why="longer history, T past two waves")
    add((66000, 3, 1), pieces=("softmax", "softmax_bwd"), cap2=("softmax", "softmax_bwd"), svm=True, why="B / 4 > 16,384")
    add((1400, 50, 8), pieces=("wsum_bwd",), cap2=("wsum_bwd",), svm=True, why="B T / 4 > 16,384; sum_vec on 35 workgroups")
    add((65600, 2, 64), pieces=("wsum", "att_in_bwd"), cap2=("wsum", "att_in_bwd"), why="B E > 16,384 * 256")
    add((2100, 50, 40), pieces=("att_in",), cap2=("att_in",), why="B T E > 16,384 * 256")
    return out


DIN_CASES = _din_cases()


def resolve_din(case):
    B, T, E = case.shape
    cap2 = tuple(p for p in case.pieces if din_grid(p, B, T, E)[0] > din_grid(p, B, T, E)[1])
    svm = sum_vec_grid(B * T) > 1 and any(p in case.pieces for p in ("wsum_bwd", "softmax_bwd"))
    assert cap2 == case.cap2 and svm == case.sum_vec_many, "%s no longer reaches its route: cap2=%r sum_vec_many=%r" % (case.id, cap2, svm)
    return {"cap2": cap2, "sum_vec_many": svm}


def din_mask(case):
    B, T, E = case.shape
    rng = np.random.default_rng(_seed(case.id, "mask"))
    if case.mask == "random":
        m = rng.random((B, T)) > 0.3
        if B > 2:
            m[0] = m[-1] = False
    elif case.mask == "alt":
        m = (np.arange(B)[:, None] + np.arange(T)[None, :]) % 2 == 1
    else:
        m = np.full((B, T), case.mask == "full")
    return m.astype(np.uint8)


def make_din_data(case):
    """Deterministic float32 inputs of a case, only those its pieces read: q [B, E], k [B, T, E], score [B T], mask [B, T] uint8,
    d_out [B, E], da [B T, 4 E], and for the softmax backward p (the oracle's softmax rounded to float32) and dp [B T]."""
    B, T, E = case.shape
    rng = np.random.default_rng(_seed(case.id))
    need = set(case.pieces)
    d = {"mask": din_mask(case)}
    if need & {"att_in", "att_in_bwd"}:
        d["q"] = _normal(rng, B, E)
    if need & {"att_in", "att_in_bwd", "wsum", "wsum_bwd"}:
        d["k"] = _normal(rng, B, T, E)
    if need & {"wsum", "wsum_bwd", "softmax", "softmax_bwd"}:
        d["score"] = _normal(rng, B * T)
    if "wsum_bwd" in need:
        d["d_out"] = _normal(rng, B, E)
    if "att_in_bwd" in need:
        d["da"] = _normal(rng, B * T, 4 * E)
    if "softmax_bwd" in need:
        d["p"] = din_softmax(d["score"].reshape(B, T), d["mask"])[0].astype(np.float32)
        d["dp"] = _normal(rng, B * T)
    return d


# --- dctr_embed_lookup_bwd.  pattern: "random", "equal" (one id: a run across every walker boundary), "distinct" (no two alike),
# "padskew" (half padding id 0, the rest skewed), "oor_tile" (the tile ``oor`` holds only ids outside [0, vocab), negative ones among
# them);  strided: d is the columns 2 .. 2 + dim of a buffer 4 wider (row stride > dim, 8 bytes off its 16-B boundary)
LookupCase = collections.namedtuple("LookupCase", "id vocab dim n pattern i64 hash_mode strided route plain_cap2 mark_cap2 why")


def _lookup_cases():
    out = []

    def add(vocab, dim, n, pattern, i64=False, hash_mode=0, strided=True, route="tile", plain_cap2=False, mark_cap2=False, why=""):
        cid = "lookup-v%d-d%d-n%d-%s-%s-h%d%s" % (vocab, dim, n, pattern, "i64" if i64 else "i32", hash_mode, "" if strided else "-dense")
        out.append(LookupCase(cid, vocab, dim, n, pattern, i64, hash_mode, strided, route, plain_cap2, mark_cap2, why))
    add(50, 2, 2048, "random", route="plain", why="plain route because dim < 3")
    add(1500, 3, 1024, "equal", why="tile route floor, exactly one tile; dimP 4 with an idle lane; one run over all 64 walkers")
    add(1500, 3, 1024, "distinct", i64=True, strided=False)
    add(1500, 3, 1024, "padskew", hash_mode=2)
    add(1500, 3, 1024, "random", i64=True, hash_mode=1)
    add(2000, 12, 1025, "equal", i64=True, why="dimP 16, 4 masked lanes per walker; a second tile of 1 position")
    add(2000, 12, 1025, "distinct", strided=False)
    add(2000, 12, 1025, "padskew", i64=True, hash_mode=2)
    add(2000, 12, 1025, "oor_tile", why="tile 0 only out-of-range ids: nothing added but the last position's row")
    add(2000, 12, 1025, "random", hash_mode=1)
    add(4000, 64, 3000, "padskew", why="widest tile-route shape: one walker per wave")
    add(4000, 64, 3000, "equal", hash_mode=1)
    add(4000, 64, 3000, "distinct", i64=True)
    add(4000, 64, 3000, "oor_tile", i64=True, why="the middle tile only out-of-range ids")
    add(300, 68, 62000, "random", route="plain", plain_cap2=True, mark_cap2=True, why="plain route by width; n dim > 16,384 * 256 and n dim / 4 > 4096 * 256")
    add(40, 16, 1023, "random", i64=True, hash_mode=1, route="plain", why="plain route by n")
    return out


LOOKUP_CASES = _lookup_cases()


def resolve_lookup(case):
    route = lookup_route(case.vocab, case.dim, case.n)
    plain_cap2 = route == "plain" and _ceil_div(case.n * case.dim, 256) > LOOKUP_PLAIN_CAP
    mark_cap2 = case.dim % 4 == 0 and _ceil_div(case.n * (case.dim // 4), 256) > MARK_ROWS_CAP
    assert (route, plain_cap2, mark_cap2) == (case.route, case.plain_cap2, case.mark_cap2), "%s no longer reaches its route" % case.id
    info = {"route": route, "plain_cap2": plain_cap2, "mark_cap2": mark_cap2, "tiles": _ceil_div(case.n, LB_TILE)}
    if route == "tile":
        dimP = lookup_dimP(case.dim)
        info.update(dimP=dimP, walkers_per_wave=64 // dimP, per_walker=LB_TILE // (4 * (64 // dimP)), idle_lanes=dimP - case.dim)
    return info


def oor_tile_of(case):
    """The tile an "oor_tile" case fills with out-of-range ids: the first of two tiles, the middle one of three."""
    return 0 if _ceil_div(case.n, LB_TILE) <= 2 else 1


def make_lookup_data(case):
    """ids [n] (int32 or int64) and d [n, dim] float32 of a case."""
    rng = np.random.default_rng(_seed(case.id))
    V, n = case.vocab, case.n
    span = 10 ** 6 if case.hash_mode else V                   # hashed ids are raw: any value resolves inside the table
    if case.pattern in ("random", "oor_tile"):
        ids = rng.integers(0, span, n)
        if case.pattern == "oor_tile":
            assert case.hash_mode == 0
            lo = oor_tile_of(case) * LB_TILE
            m = min(LB_TILE, n - lo)
            ids[lo:lo + m] = np.where(rng.random(m) < 0.5, V + rng.integers(0, 1000, m), -1 - rng.integers(0, 1000, m))
            ids[lo] = V                                       # the first id past the table
    elif case.pattern == "equal":
        ids = np.full(n, 7 if not case.hash_mode else 123457)
    elif case.pattern == "distinct":
        assert case.hash_mode == 0 and V >= n
        ids = rng.permutation(V)[:n]
    elif case.pattern == "padskew":
        ids = np.where(rng.random(n) < 0.5, 0, 1 + ((span - 1) * rng.random(n) ** 4).astype(np.int64))
    else:
        raise ValueError(case.pattern)
    return {"ids": ids.astype(np.int64 if case.i64 else np.int32), "d": _normal(rng, n, case.dim)}


# --- Dice on one layer [R, N] behind K = 8 inputs.  kind: "bwd" (dctr_dice_train_fwd, then dctr_mlp_bwd with stored statistics, with
# batch statistics recomputing z and with batch statistics from saved_z) or a forward-only variant: "var0" (one row), "stride14"
# (z the first 12 columns of a [R, 14] buffer), "off4" (z a contiguous view one float into its buffer), "nobias" / "bias"
DiceCase = collections.namedtuple("DiceCase", "id R N kind form why")
DICE_K = 8
DICE_MIN_VAR = 0.05         # smallest batch variance of a column in a case whose backward runs through the batch statistics
DICE_REDRAWS = 64


def _dice_cases():
    out = []

    def add(R, N, form, kind="bwd", why=""):
        out.append(DiceCase("dice-%dx%d-%s" % (R, N, kind), R, N, kind, form, why))
    add(3, 8, "lane4", why="smallest backward through the batch statistics: three rows, every column's batch variance >= DICE_MIN_VAR")
    add(17, 4, "lane4", why="N4 = 1, RL = 256: rows < RL, one workgroup")
    add(211, 12, "lane4", why="the float64 point of tests/test_gpu_mlp_bwd.py")
    add(300, 80, "lane4", why="DIN's first attention width: N4 = 20, RL = 12, 16 idle threads")
    add(300, 40, "lane4", why="DIN's second attention width: N4 = 10, RL = 25, 6 idle threads")
    add(33, 1024, "lane4", why="RL = 1")
    add(33, 1028, "scalar", why="five column passes")
    add(70, 257, "scalar", why="odd N, two column passes")
    add(5000, 6, "scalar", why="grid-stride over the row blocks")
    add(32773, 40, "lane4", why="colsum_grid's 128 cap (rows >= 32,768) and dice_apply's 4096 cap")
    add(1, 8, "lane4", kind="var0", why="variance exactly 0")
    add(37, 12, "scalar", kind="stride14", why="row stride 14: the scalar form")
    add(37, 12, "scalar", kind="off4", why="4 bytes off 16-B alignment: the scalar form")
    add(37, 12, "lane4", kind="nobias")
    add(37, 12, "lane4", kind="bias")
    return out


DICE_CASES = _dice_cases()
DICE_FWD_LAYOUT = {"stride14": (14, 0), "off4": (None, 4)}                  # kind -> (row stride, byte offset) of z


def resolve_dice(case):
    stride, off = DICE_FWD_LAYOUT.get(case.kind, (None, 0))
    info = dice_route(case.R, case.N, stride, off)
    assert info["form"] == case.form, "%s no longer reaches its form: %r" % (case.id, info)
    return info


def make_dice_data(case):
    """x [R, K], W [K, N], b [N] with z = x W + b of mean about 0.7 and unit spread (E[z^2] - E[z]^2 would cancel), alpha, the stored
    statistics, dy [R, N];  z64 (x W + b in float64), zmag (|x| |W| + |b|);  redraws: how often the seed moved on until every column's
    batch variance reached DICE_MIN_VAR (R >= 3; ``var0`` is there for the opposite)."""
    R, N, K = case.R, case.N, DICE_K
    for attempt in range(DICE_REDRAWS):
        rng = np.random.default_rng(_seed("dice", R, N, attempt))       # (the forward-only variants of one shape share their draws)
        x, W = _normal(rng, R, K), _normal(rng, K, N) / np.float32(np.sqrt(K))
        b = (0.7 + 0.2 * _normal(rng, N)).astype(np.float32)
        z64 = _f64(x) @ _f64(W) + _f64(b)
        if R < 3 or z64.var(0).min() >= DICE_MIN_VAR:
            break
    else:
        raise AssertionError("%s: no seed with every batch variance >= %g" % (case.id, DICE_MIN_VAR))
    return dict(x=x, W=W, b=b, z64=z64, zmag=np.abs(_f64(x)) @ np.abs(_f64(W)) + np.abs(_f64(b)), alpha=0.3 * _normal(rng, N),
                moving_mean=0.2 * _normal(rng, N), moving_var=rng.uniform(0.5, 1.5, N).astype(np.float32), dy=_normal(rng, R, N), redraws=attempt)


def dice_fwd_input(case, d):
    """(z float32 [R, N], bias or None) dctr_dice_train_fwd gets: x W rounded to float32 and the bias; "nobias": x W + b rounded."""
    if case.kind == "nobias":
        return d["z64"].astype(np.float32), None
    return (d["z64"] - _f64(d["b"])).astype(np.float32), d["b"]


def dice_bwd_oracle(d, mode):
    """(G, T) with dz, d_alpha, dW, db, dx of a case's layer.  mode "stored": the stored statistics;  "batch": the float64 batch
    statistics of z64 rounded to float32, as the GPU test hands them to the op."""
    if mode == "stored":
        G, T = dice_bwd_stored(d["z64"], d["dy"], d["alpha"], d["moving_mean"], d["moving_var"], zmag=d["zmag"])
    else:
        G, T = dice_bwd_batch(d["z64"], d["dy"], d["alpha"], *dice_batch_stats(d), zmag=d["zmag"])
    return dense_bwd(d["x"], d["W"], G, T)


def dice_batch_stats(d):
    return d["z64"].mean(0).astype(np.float32), d["z64"].var(0).astype(np.float32)


# --- the loss
BCE_BATCHES = (1, 63, 64, 65, 256, 257, 1000)
BCE_TASKS = ("binary", "mse")
BCE_WEIGHTS = ("none", "random", "zero")
BCE_EDGE_PREDS = (0.0, 1e-8, 1e-7, 0.5, 1.0 - 2.0 ** -24, 1.0)             # each against y = 0 and y = 1


def bce_edges():
    """(pred, y) float32 pairs at and around the clip."""
    p = np.asarray([v for v in BCE_EDGE_PREDS for _ in (0, 1)], dtype=np.float32)
    return p, np.asarray([0.0, 1.0] * len(BCE_EDGE_PREDS), dtype=np.float32)


def make_bce_data(B, task, weight):
    """pred, y, weight (or None): the edge pairs first, as many as fit, then ordinary sigmoid outputs (labels 0 / 1; mse: any target)."""
    rng = np.random.default_rng(_seed("bce", B, task, weight))
    pred = (1.0 / (1.0 + np.exp(-2.0 * rng.standard_normal(B)))).astype(np.float32)
    y = (rng.random(B) > 0.5).astype(np.float32) if task == "binary" else _normal(rng, B)
    ep, ey = bce_edges()
    m = min(B, ep.size)
    start = 0 if B >= ep.size else (B * 5) % ep.size          # (a batch shorter than the edges takes a slice of them)
    idx = (start + np.arange(m)) % ep.size
    pred[:m] = ep[idx]
    if task == "binary":
        y[:m] = ey[idx]
    w = {"none": None, "random": rng.uniform(0.0, 2.0, B).astype(np.float32), "zero": np.zeros(B, np.float32)}[weight]
    return pred, y, w
