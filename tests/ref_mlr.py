"""NumPy oracle of MLR (reference deepctr/models/mlr.py:17-74), float64 or float32.

``mlr_model`` / ``run_fixture``: the whole model from the reference's per-name weights, on the shared oracle helpers (the linear part's
lookups, sequence pooling, Hash).  ``mutate`` replaces one piece of the graph by a wrong one — what the fixture recipe and the CPU test
use to show that the fixtures would notice: 'no_sigmoid' (learners without their sigmoid), 'swap' (region and learner tables swapped),
'no_bias' (the bias factor dropped), 'uniform' (softmax replaced by 1 / R).

``mlr_op``: the op-level oracle of dctr_mlr_fwd / dctr_mlr_bwd over fused rows: z, out, dz, the table / pooled-row gradients, and the
``terms`` magnitudes (the sum of |summands| per element) tests.util.assert_close_terms wants."""
import json

import numpy as np

from oracle.ref_models import _embed_groups, _is_dense


def _sigmoid(z):
    z = np.asarray(z)
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e)).astype(z.dtype)


def mix(z, R, bias, task, mutate=None):
    """z [B, K] -> dict(s, a, g, u, out): the mixture of include/dctr.h (MLR)."""
    zr = z[:, :R]
    e = np.exp(zr - zr.max(axis=1, keepdims=True))
    s = e / e.sum(axis=1, keepdims=True)
    if mutate == "uniform":
        s = np.full_like(s, 1.0 / R)
    a = _sigmoid(z[:, R:2 * R]) if (task == "binary" and mutate != "no_sigmoid") else z[:, R:2 * R]
    u = (s * a).sum(axis=1)
    g = _sigmoid(z[:, 2 * R]) if (bias and mutate != "no_bias") else np.ones_like(u)
    return dict(s=s, a=a, g=g, u=u, out=u * g)


def mutations(meta):
    """The mutations that apply to a fixture: 'uniform' always; 'no_sigmoid' for binary learners; 'swap' where the base columns are
    the region columns (the tables have the same shapes); 'no_bias' where there is a bias part."""
    out = ["uniform"]
    if meta["kwargs"].get("task", "binary") == "binary":
        out.append("no_sigmoid")
    if not meta.get("base"):
        out.append("swap")
    if meta.get("bias"):
        out.append("no_bias")
    return out


def linear_logit(cols, feed, weights, prefix, linear_name, dt):
    """One linear logit [B] of get_linear_logit(prefix=prefix, units=1): tables ``<prefix>0sparse_emb_<name>``, Linear ``linear_name``."""
    groups, dense = _embed_groups(list(cols), feed, weights, prefix + "0", dt)
    sparse = [e for g in groups.values() for e in g]
    n = next(iter(feed.values())).shape[0]
    z = np.zeros(n, dt)
    for e in sparse:
        z = z + e.reshape(n, -1).sum(-1)
    if dense:
        d = np.concatenate([x.reshape(n, -1) for x in dense], axis=-1)
        z = z + (d @ weights[linear_name + "/linear_kernel"].astype(dt)).reshape(n)
    return z


def mlr_model(region_cols, base_cols, bias_cols, weights, feed, region_num=4, task="binary", dtype=np.float64, mutate=None, **_):
    dt = np.dtype(dtype).type
    R = int(region_num)
    base_cols = list(base_cols or []) or list(region_cols)
    bias_cols = list(bias_cols or [])
    lin = lambda k: "linear" if k == 0 else "linear_%d" % k     # noqa: E731  (keras' auto names, in creation order)
    rp, lp = ("learner_", "region_") if mutate == "swap" else ("region_", "learner_")
    if mutate == "swap":
        # the region logits from the learners' tables and the other way round (possible when both lists are the same columns)
        zr = [linear_logit(region_cols, feed, weights, "%s%d" % (rp, r + 1), lin(R + r), dt) for r in range(R)]
        zl = [linear_logit(base_cols, feed, weights, "%s%d" % (lp, r + 1), lin(r), dt) for r in range(R)]
    else:
        zr = [linear_logit(region_cols, feed, weights, "%s%d" % (rp, r + 1), lin(r), dt) for r in range(R)]
        zl = [linear_logit(base_cols, feed, weights, "%s%d" % (lp, r + 1), lin(R + r), dt) for r in range(R)]
    zs = zr + zl
    if bias_cols:
        zs.append(linear_logit(bias_cols, feed, weights, "bias_1", lin(2 * R), dt))
    z = np.stack(zs, axis=1)
    return mix(z, R, bool(bias_cols), task, mutate)["out"].reshape(-1, 1), z


def run_fixture(g, dtype=np.float64, mutate=None, weights=None, want_z=False):
    """The oracle over a tests/golden/model_mlr*.npz fixture -> y [n, 1] (``want_z``: (y, z [n, K]))."""
    from tests.spec import columns_from_spec
    meta = json.loads(bytes(g["meta"]).decode())
    feed = {k[5:]: v for k, v in g.items() if k.startswith("feed/")}
    if weights is None:
        weights = {k[2:]: v for k, v in g.items() if k.startswith("w/")}
    cols = lambda key: columns_from_spec(meta[key]) if meta.get(key) else None     # noqa: E731
    y, z = mlr_model(cols("region"), cols("base"), cols("bias"), weights, feed, dtype=dtype, mutate=mutate, **meta["kwargs"])
    return (y, z) if want_z else y


def mlr_op(fields, batch, region_num, bias=False, task="binary", dense=None, dense_w=None, d_out=None, z=None):
    """fields: list of dict(rows [V, >= width] (pre-pooled: [>= B, >= width]), ids [B] or None, col0, width); an id outside [0, V)
    counts as a zero row and gets no gradient.  float64 throughout.  ``z``: use this z (the forward's saved one) for the backward instead
    of the oracle's own.  Returns dict(z, z_terms, out, s, a, g, u, dout_dz, sum_terms (what out_bar reads), and with d_out: dz, dz_terms, grads,
    grad_terms — per field an array shaped like rows[:, :width], None entries never produced)."""
    R, B = int(region_num), int(batch)
    K = 2 * R + int(bool(bias))
    zz = np.zeros((B, K))
    zt = np.zeros((B, K))
    picked = []
    for f in fields:
        rows = np.asarray(f["rows"], dtype=np.float64)[:, :f["width"]]
        if f.get("ids") is None:
            idx, ok = np.arange(B), np.ones(B, dtype=bool)
        else:
            idx = np.asarray(f["ids"]).astype(np.int64)
            ok = (idx >= 0) & (idx < rows.shape[0])
        v = np.where(ok[:, None], rows[np.where(ok, idx, 0)], 0.0)
        zz[:, f["col0"]:f["col0"] + f["width"]] += v
        zt[:, f["col0"]:f["col0"] + f["width"]] += np.abs(v)
        picked.append((idx, ok))
    if dense is not None:
        d, w = np.asarray(dense, dtype=np.float64), np.asarray(dense_w, dtype=np.float64)
        zz += d @ w
        zt += np.abs(d) @ np.abs(w)
    res = dict(z=zz, z_terms=zt)
    zb = zz if z is None else np.asarray(z, dtype=np.float64)
    m = mix(zb, R, bias, task)
    s, a, g, u = m["s"], m["a"], m["g"], m["u"]
    res.update(m)
    da = a * (1 - a) if task == "binary" else np.ones_like(a)
    # d out / d z: what an error of z turns into (first order)
    pz = np.zeros((B, K))
    pz[:, :R] = g[:, None] * s * (a - u[:, None])
    pz[:, R:2 * R] = g[:, None] * s * da
    if bias:
        pz[:, 2 * R] = u * g * (1 - g)
    res["dout_dz"] = pz
    res["sum_terms"] = (s * np.abs(a)).sum(axis=1) * g          # the magnitude the R products were summed at
    if d_out is None:
        return res
    d = np.asarray(d_out, dtype=np.float64).reshape(B)
    dz = d[:, None] * pz
    dzt = np.abs(dz)
    sa = (s * np.abs(a)).sum(axis=1)                              # the magnitude u was summed at (regression learners: a = z has a sign)
    dzt[:, :R] = np.abs(d)[:, None] * g[:, None] * s * (np.abs(a) + sa[:, None])   # (a - u cancels)
    if bias:
        dzt[:, 2 * R] = np.abs(d) * sa * g * (1 - g)
    grads, gterms = [], []
    for f, (idx, ok) in zip(fields, picked):
        rows = np.asarray(f["rows"])
        sl = slice(f["col0"], f["col0"] + f["width"])
        gr = np.zeros((rows.shape[0], f["width"]))
        gt = np.zeros_like(gr)
        np.add.at(gr, idx[ok], dz[ok][:, sl])
        np.add.at(gt, idx[ok], dzt[ok][:, sl])
        grads.append(gr)
        gterms.append(gt)
    res.update(dz=dz, dz_terms=dzt, grads=grads, grad_terms=gterms)
    return res


def op_case(F, R, bias, B, n_dense, i64, seed, vocab=37):
    """Random operands of one op call over F features (read-only arrays): feature j is, in turn,
        0: a table over every column 0 .. K-1 (region + base (+ bias): one contiguous run);
        1: a pre-pooled field over the columns 0 .. 2R-1, in a buffer whose pitch is 5 floats wider than its row;
        2: a table field with a PARTIAL column range — R columns from column 1, read from column 1 of a master that starts at column 0;
        3: with a bias part the two-entry feature (region columns 0 .. R-1 in one master, the bias column in another, ONE id vector),
           else a table over the learner columns R .. 2R-1.
    Returns dict(fields (for mlr_op / ops.mlr: rows, ids, col0, width), masters (per field the array its rows are a view of, the
    first master column of the field), dense, dense_w)."""
    rng = np.random.RandomState(seed)
    K = 2 * R + int(bool(bias))
    idt = np.int64 if i64 else np.int32
    fields, owners = [], []

    def table(V, cols):
        return rng.standard_normal((V, (cols + 3) // 4 * 4)).astype(np.float32)

    for j in range(F):
        V = vocab + 3 * j
        ids = rng.randint(0, V, B).astype(idt)
        kind = j % 4
        if kind == 0:
            m = table(V, K)
            fields.append(dict(rows=m, ids=ids, col0=0, width=K))
            owners.append((m, 0))
        elif kind == 1:
            m = rng.standard_normal((B, 2 * R + 5)).astype(np.float32)
            fields.append(dict(rows=m, ids=None, col0=0, width=2 * R))
            owners.append((m, 0))
        elif kind == 2:
            m = table(V, R + 1)
            fields.append(dict(rows=m[:, 1:], ids=ids, col0=1, width=R))
            owners.append((m, 1))
        elif bias:
            m1, m2 = table(V, R), table(V, 1)
            fields.append(dict(rows=m1, ids=ids, col0=0, width=R))
            fields.append(dict(rows=m2, ids=ids, col0=2 * R, width=1))
            owners += [(m1, 0), (m2, 0)]
        else:
            m = table(V, R)
            fields.append(dict(rows=m, ids=ids, col0=R, width=R))
            owners.append((m, 0))
    dense = dense_w = None
    if n_dense:
        dense = rng.standard_normal((B, n_dense)).astype(np.float32)
        dense_w = rng.standard_normal((n_dense, K)).astype(np.float32)
        dense_w[0, ::2] = 0.0                      # a logit that does not use a dense column: a zero of the packed matrix
    for a in [o[0] for o in owners] + [f["ids"] for f in fields if f["ids"] is not None] + [x for x in (dense, dense_w) if x is not None]:
        a.setflags(write=False)
    return dict(fields=fields, owners=owners, dense=dense, dense_w=dense_w, K=K)


def out_bar(res, task, rtol=1e-4, rtol_terms=2e-6):
    """The bar of out: 1e-4 of it, plus what z's allowance of 2e-6 of its summed magnitude turns into at first order (sum_c
    |d out / d z_c| * 2e-6 * terms_c), plus — regression learners, whose R products may cancel — 2e-6 of the magnitude they were summed
    at.  All from the float64 oracle."""
    bar = rtol * np.abs(res["out"]) + (np.abs(res["dout_dz"]) * rtol_terms * res["z_terms"]).sum(axis=1) + 1e-30
    if task != "binary":
        bar = bar + rtol_terms * res["sum_terms"]
    return bar
