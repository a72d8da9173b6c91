"""float64 NumPy oracle of the two scatter kernels every HIP training step ends in — dctr_embed_gather_fm_bwd and dctr_embed_pool_bwd
(include/dctr.h) — and of the small backward entry points beside them.  Every function returns ``(value, terms)``: ``terms`` is the same
sum taken over the absolute values of its summands, the magnitude tests.util.assert_close_terms scales its fp32 bar by.

The formulas are the derivatives of the forward expressions in oracle/ref_numpy.py (embedding gather + concat, FM, the linear logit;
weighted_sequence followed by sequence_pooling); tests/test_embed_bwd_oracle_cpu.py pins them against torch autograd in double."""
import numpy as np

from oracle import farmhash as fh
from oracle import ref_numpy as R


def resolve_rows(ids, vocab, hash_mode=0):
    """The table row of every id: the id itself, or Hash.call on it (hash_mode 1: every bucket, 2: mask_zero — bucket 0 kept for id 0)."""
    ids = np.asarray(ids)
    return fh.hash_bucket_int(ids, vocab, hash_mode == 2) if hash_mode else ids.astype(np.int64)


def field_rows(fields, ids):
    """Per field of a gather: (rows [B] int64, in-range [B] bool).  An identity field's "vocabulary" is the batch: row b for sample b."""
    ids = np.asarray(ids)
    B = ids.shape[1]
    out = []
    for j, f in enumerate(fields):
        r = np.arange(B, dtype=np.int64) if f.get("identity") else resolve_rows(ids[j], f["vocab"], f.get("hash_mode", 0))
        out.append((r, (r >= 0) & (r < f["vocab"])))
    return out


def gather_fm_bwd(fields, ids, d_in=None, d_fm=None, d_lin=None, dense=None, dense_lin_rows=None, n_lin_w=None):
    """Backward of gather + concat + FM + linear logit.  ``fields``: dicts(table [V,D], lin_table [V] or None, vocab, dim, out_offset
    (-1: not in the DNN input), in_fm, hash_mode, identity); ``ids`` [F,B]; ``d_in`` [B, >= columns], ``d_fm`` / ``d_lin`` [B] or None;
    ``dense`` [B,n] with ``dense_lin_rows`` [n] (the row of Linear.kernel a dense column feeds, -1: none; None: the identity) and
    ``n_lin_w`` rows of Linear.kernel.  Value and terms are dicts: g_table / g_lin (lists per field, None without a linear table) and
    g_dense_lin_w.  Out-of-range rows contribute nothing and count as zero in the FM sum."""
    F = len(fields)
    ids = np.asarray(ids)
    B = ids.shape[1] if F else np.asarray(dense).shape[0]
    rows = field_rows(fields, ids)
    d_in = None if d_in is None else np.asarray(d_in, np.float64)
    d_fm = None if d_fm is None else np.asarray(d_fm, np.float64).reshape(B)
    d_lin = None if d_lin is None else np.asarray(d_lin, np.float64).reshape(B)
    e = []
    for f, (r, ok) in zip(fields, rows):
        t = np.asarray(f["table"], np.float64)
        e.append(np.where(ok[:, None], t[np.where(ok, r, 0)], 0.0))
    width = max([f["dim"] for f in fields] + [1])
    S, Sa = np.zeros((B, width)), np.zeros((B, width))          # element i of S sums the FM fields that are wider than i
    for f, ej in zip(fields, e):
        if f.get("in_fm"):
            S[:, :f["dim"]] += ej
            Sa[:, :f["dim"]] += np.abs(ej)
    val = dict(g_table=[], g_lin=[], g_dense_lin_w=None)
    trm = dict(g_table=[], g_lin=[], g_dense_lin_w=None)
    for f, ej, (r, ok) in zip(fields, e, rows):
        D, off = f["dim"], f.get("out_offset", -1)
        g, ga = np.zeros((B, D)), np.zeros((B, D))
        if off >= 0 and d_in is not None:
            g += d_in[:, off:off + D]
            ga += np.abs(d_in[:, off:off + D])
        if f.get("in_fm") and d_fm is not None:
            g += d_fm[:, None] * (S[:, :D] - ej)
            ga += np.abs(d_fm)[:, None] * (Sa[:, :D] + np.abs(ej))
        gt, gta = np.zeros((f["vocab"], D)), np.zeros((f["vocab"], D))
        np.add.at(gt, r[ok], g[ok])
        np.add.at(gta, r[ok], ga[ok])
        val["g_table"].append(gt)
        trm["g_table"].append(gta)
        if f.get("lin_table") is None:
            val["g_lin"].append(None)
            trm["g_lin"].append(None)
            continue
        gl, gla = np.zeros(f["vocab"]), np.zeros(f["vocab"])
        if d_lin is not None:
            np.add.at(gl, r[ok], d_lin[ok])
            np.add.at(gla, r[ok], np.abs(d_lin[ok]))
        val["g_lin"].append(gl)
        trm["g_lin"].append(gla)
    if dense is not None:
        dense = np.asarray(dense, np.float64)
        n = dense.shape[1]
        to = np.arange(n) if dense_lin_rows is None else np.asarray(dense_lin_rows).astype(np.int64)
        gw, gwa = np.zeros(n if n_lin_w is None else n_lin_w), np.zeros(n if n_lin_w is None else n_lin_w)
        if d_lin is not None:
            for k in range(n):
                if to[k] >= 0:
                    gw[to[k]] += (d_lin * dense[:, k]).sum()
                    gwa[to[k]] += np.abs(d_lin * dense[:, k]).sum()
        val["g_dense_lin_w"], trm["g_dense_lin_w"] = gw, gwa
    return val, trm


def pool_masks(ids, vocab, hash_mode=0, lengths=None):
    """rows [B,T], in-range [B,T], mask [B,T] of a pooled sequence: by length, or mask_zero on the resolved (post-hash) row."""
    rows = resolve_rows(ids, vocab, hash_mode)
    ok = (rows >= 0) & (rows < vocab)
    mask = R.sequence_mask(lengths, rows.shape[1]) if lengths is not None else rows != 0
    return rows, ok, mask


def pool_weights(mask, weight=None, weight_norm=True, dtype=np.float64):
    """The factor weighted_sequence multiplies position t by ([B,T]; ones without weights — the mask is sequence_pooling's)."""
    if weight is None:
        return np.ones(mask.shape, dtype)
    one = np.ones(mask.shape + (1,), dtype)
    return R.weighted_sequence(one, np.asarray(weight).reshape(mask.shape + (1,)).astype(dtype), mask=mask,
                               weight_normalization=weight_norm)[:, :, 0]


def max_hist(rows_of, rows, ok, mask, weight=None, weight_norm=True):
    """What sequence_pooling('max') takes the maximum of, in float32 exactly as the reference writes it: seq * w - (1 - mask) * 1e9
    (layers/sequence.py:97 after :183).  ``rows_of`` [V,E] float32; out-of-range rows read as zero.  Returns [B,T,E] float32."""
    t = np.asarray(rows_of, np.float32)
    seq = np.where(ok[:, :, None], t[np.where(ok, rows, 0)], np.float32(0))
    if weight is not None:
        seq = R.weighted_sequence(seq, np.asarray(weight, np.float32).reshape(mask.shape + (1,)), mask=mask, weight_normalization=weight_norm)
    m3 = np.repeat(mask.astype(np.float32)[:, :, None], seq.shape[2], axis=2)
    return seq - (1 - m3) * np.float32(1e9)


def pool_bwd(table, lin_table, ids, d_out=None, d_lin_out=None, combiner="mean", lengths=None, weight=None, weight_norm=True, hash_mode=0):
    """Derivative of weighted_sequence followed by sequence_pooling with respect to the table rows and the 1-wide linear table rows
    (``lin_table`` may be None).  max: the gradient goes to the FIRST position attaining the maximum, selected in float32 (max_hist)."""
    table = np.asarray(table)
    V, E = table.shape
    rows, ok, mask = pool_masks(ids, V, hash_mode, lengths)
    B, T = rows.shape
    w = pool_weights(mask, weight, weight_norm)
    d_out = np.zeros((B, E)) if d_out is None else np.asarray(d_out, np.float64)
    d_lin_out = np.zeros(B) if d_lin_out is None else np.asarray(d_lin_out, np.float64).reshape(B)
    gt, gta = np.zeros((V, E)), np.zeros((V, E))
    gl, gla = (None, None) if lin_table is None else (np.zeros(V), np.zeros(V))
    if combiner == "max":
        bi = np.arange(B)
        first = max_hist(table, rows, ok, mask, weight, weight_norm).argmax(axis=1)              # [B,E]: np.argmax takes the first
        for c in range(E):
            t = first[:, c]
            r, k = rows[bi, t], ok[bi, t]
            np.add.at(gt[:, c], r[k], (d_out[:, c] * w[bi, t])[k])
            np.add.at(gta[:, c], r[k], np.abs(d_out[:, c] * w[bi, t])[k])
        if lin_table is not None:
            t = max_hist(np.asarray(lin_table).reshape(V, 1), rows, ok, mask, weight, weight_norm).argmax(axis=1)[:, 0]
            r, k = rows[bi, t], ok[bi, t]
            np.add.at(gl, r[k], (d_lin_out * w[bi, t])[k])
            np.add.at(gla, r[k], np.abs(d_lin_out * w[bi, t])[k])
        return (gt, gl), (gta, gla)
    f = w * mask
    if combiner == "mean":
        length = mask.sum(axis=1) if lengths is None else np.asarray(lengths).reshape(B)
        f = f / (length.astype(np.float64)[:, None] + 1e-8)
    elif combiner != "sum":
        raise ValueError(combiner)
    g = d_out[:, None, :] * f[:, :, None]                       # [B,T,E]
    np.add.at(gt, rows[ok], g[ok])
    np.add.at(gta, rows[ok], np.abs(g[ok]))
    if lin_table is not None:
        np.add.at(gl, rows[ok], (d_lin_out[:, None] * f)[ok])
        np.add.at(gla, rows[ok], np.abs(d_lin_out[:, None] * f)[ok])
    return (gt, gl), (gta, gla)


def touched_expected(fields, ids):
    """Per table with dim % 4 == 0 (the only ones that carry touched bytes): {field index: the rows some in-range id resolved to}."""
    out = {}
    for j, (f, (r, ok)) in enumerate(zip(fields, field_rows(fields, ids))):
        if f["dim"] % 4 == 0:
            out[j] = np.unique(r[ok])
    return out


def fm_bwd(x, dlogit):
    """x [B,F,E], dlogit [B] -> dx[b,f,:] = dlogit[b] * (sum_f' x[b,f',:] - x[b,f,:])."""
    x = np.asarray(x, np.float64)
    d = np.asarray(dlogit, np.float64).reshape(-1, 1, 1)
    return d * (x.sum(1, keepdims=True) - x), np.abs(d) * (np.abs(x).sum(1, keepdims=True) + np.abs(x))


def dense1_bwd(x, w, dlogit):
    """Dense(1, use_bias=False): ((dx [B,n], d_w [n]), their terms)."""
    x, w, d = np.asarray(x, np.float64), np.asarray(w, np.float64).reshape(-1), np.asarray(dlogit, np.float64).reshape(-1)
    return (d[:, None] * w[None, :], d @ x), (np.abs(d[:, None] * w[None, :]), np.abs(d) @ np.abs(x))


def din_softmax(score, mask):
    """softmax over all T positions of where(mask, score, -2^32 + 1) (layers/sequence.py:283-289): ((p [B,T]), terms)."""
    s = np.where(np.asarray(mask, bool), np.asarray(score, np.float64), -2.0 ** 32 + 1)
    e = np.exp(s - s.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    return p, p


def din_softmax_bwd(p, mask, dp):
    """d_score = p (dp - <p, dp>) where the mask is set (a padded position's input is the constant), d_bias = sum d_score."""
    p, dp, m = np.asarray(p, np.float64), np.asarray(dp, np.float64), np.asarray(mask, bool)
    dot, dota = (p * dp).sum(1, keepdims=True), np.abs(p * dp).sum(1, keepdims=True)
    ds, dsa = np.where(m, p * (dp - dot), 0.0), np.where(m, np.abs(p) * (np.abs(dp) + dota), 0.0)
    return (ds, ds.sum()), (dsa, dsa.sum())
