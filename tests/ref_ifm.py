"""NumPy oracle of IFM and DIFM (reference deepctr/models/ifm.py:21-74, difm.py:20-82), float64 or float32, on the shared oracle helpers
(embedding groups, DNN, sequence pooling, Hash) and tests.ref_autoint.interacting_layer, plus ``ifm_op``: the function of the fused
kernel the op tests use.

``absolute=True`` runs ``ifm_op`` on absolute values (and adds where the graph subtracts): an upper bound of the magnitude every output
was summed at, the ``terms`` of tests.util.assert_close_terms."""
import numpy as np

from oracle import ref_numpy as R
from oracle.ref_models import _dnn, _embed_groups, _is_dense

from tests.ref_autoint import interacting_layer


def ifm_op(x, fields, dim, sources=(), mprime=None, softmax=False, lin=None, add=(), bias=0.0, sigmoid=False, dtype=np.float64,
           absolute=False):
    """x [B, >= fields*dim]; sources: (act [B, K], kernel [K, fields]) pairs; mprime [B, fields] or None; lin [B, fields] first-order
    terms or None; add: [B] vectors -> (out [B], m [B, fields]).  With ``absolute`` everything enters by magnitude and the output is
    the bound T of the pre-activation sum.  The softmax factor is positive whatever the signs, so it enters as its true value; its own
    rounding comes from m', a cancelling sum of magnitude A = max_f sum_k |act| |kernel|: an error e A in m' is a relative error e A in
    every m[f], and the output — at most quadratic in m — moves by at most 4 e A T.  The bound returned with softmax is T (1 + 4 A)."""
    dt = np.dtype(dtype).type
    ab = np.abs if absolute else (lambda v: v)
    F, d = int(fields), int(dim)
    x = np.asarray(x)
    B = x.shape[0]

    def factor(a):
        mp = np.zeros((B, F), dt) if mprime is None else a(np.asarray(mprime).astype(dt)[:, :F])
        for act, kernel in sources:
            mp = mp + a(np.asarray(act).astype(dt)) @ a(np.asarray(kernel).astype(dt))
        return mp
    mp = factor(ab)
    if softmax:
        t = factor(lambda v: v)
        e = np.exp(t - t.max(axis=1, keepdims=True))
        m = dt(F) * (e / e.sum(axis=1, keepdims=True))
    else:
        m = mp
    r = ab(x[:, :F * d].astype(dt)).reshape(B, F, d) * m[:, :, None]
    sq, ss = r.sum(1) ** 2, (r * r).sum(1)
    out = dt(0.5) * ((sq + ss) if absolute else (sq - ss)).sum(-1)
    if lin is not None:
        out = out + (ab(np.asarray(lin).astype(dt)) * m).sum(-1)
    for v in add:
        out = out + ab(np.asarray(v).astype(dt)).reshape(-1)
    out = out + ab(dt(bias))
    if absolute and softmax:
        out = out * (1 + 4 * mp.max(axis=1))
    if sigmoid and not absolute:
        out = dt(1) / (dt(1) + np.exp(-out))
    return out, m


class _One(object):
    """fc._replace(embedding_dim=1): only the table width changes (feature_column.py:171-181)."""

    def __init__(self, fc):
        self.__dict__["_fc"] = fc

    def __getattr__(self, k):
        return getattr(self._fc, k)


def linear_terms(linear_cols, feed, weights, dt):
    """get_linear_logit's operands: ([B, F_lin] first-order terms in the order the reference concatenates them, or None;
    dense . linear_kernel [B] or None)."""
    groups, dense = _embed_groups([_One(fc) for fc in linear_cols], feed, weights, "linear0", dt)
    sparse = [e.reshape(e.shape[0], -1) for g in groups.values() for e in g]
    terms = np.concatenate(sparse, axis=-1) if sparse else None
    dlin = None
    if dense:
        dlin = (np.concatenate([v.reshape(v.shape[0], -1) for v in dense], axis=-1) @ weights["linear/linear_kernel"].astype(dt)).reshape(-1)
    return terms, dlin


def attention_bound(x, wq, wk, wv, wres, d, H, use_res):
    """Magnitude bound of InteractingLayer(scaling=True) on |x|, |weights|: every output row is a convex combination of the value rows,
    so max_j |x_j| |W_v| (+ |x_f| |W_res|) bounds it; the scores' own rounding — a cancelling sum of magnitude S = max |q| |k| / sqrt(d) —
    moves the softmax weights by a relative e S each, the output by at most 2 e S of that bound: the bound returned carries (1 + 4 S),
    the same allowance ifm_op makes for IFM's softmax."""
    B, F = x.shape[0], x.shape[1]
    q, k, v = (np.tensordot(x, w, axes=(-1, 0)) for w in (wq, wk, wv))                      # [B,F,dH]
    S = 0.0
    for h in range(H):
        sl = slice(h * d, (h + 1) * d)
        S = max(S, float((q[:, :, sl] @ k[:, :, sl].transpose(0, 2, 1)).max()) / d ** 0.5)
    out = np.broadcast_to(v.max(axis=1, keepdims=True), v.shape) * (1 + 4 * S)
    if use_res:
        out = out + np.tensordot(x, wres, axes=(-1, 0))
    return out


def input_aware(kind, linear_cols, dnn_cols, weights, feed, att_embedding_size=8, att_head_num=8, att_res=True,
                dnn_hidden_units=(256, 128, 64), dnn_activation="relu", dnn_use_bn=False, task="binary", dtype=np.float32,
                absolute=False, **_):
    """``absolute``: the bound of the magnitude the logit was summed at (the `terms` of assert_close_terms), for models without
    BatchNormalization, weighted sequences or a DNN activation other than relu / linear: weights and dense inputs by magnitude, the
    attention through attention_bound, the factor and the logit through ifm_op(absolute=True)."""
    dt = np.dtype(dtype).type
    if absolute:
        assert not dnn_use_bn and dnn_activation in ("relu", "linear")
        weights = {k: np.abs(v) for k, v in weights.items()}
        feed = {k: (np.abs(v) if np.asarray(v).dtype.kind == "f" else v) for k, v in feed.items()}
    groups, _dense = _embed_groups([fc for fc in dnn_cols if not _is_dense(fc)], feed, weights, "", dt)
    embs = [e for g in groups.values() for e in g]
    x = np.concatenate(embs, axis=1)                                      # [B,F,d]
    B, F, d = x.shape
    flat = x.reshape(B, -1)                                               # combined_dnn_input(sparse_embedding_list, [])
    hidden = _dnn("dnn", flat, weights, dt, dnn_activation, dnn_use_bn)
    if kind == "IFM":
        sources = [(hidden, weights["dense/kernel"])]
    else:
        n = "interacting_layer"
        qkvr = (weights[n + "/query"], weights[n + "/key"], weights[n + "/value"], weights.get(n + "/res"))
        if absolute:
            att = attention_bound(x, *(None if w is None else w.astype(dt) for w in qkvr), att_embedding_size, att_head_num, att_res)
        else:
            att = interacting_layer(x, *qkvr, att_embedding_size, att_head_num, att_res, scaling=True, dtype=dt)
        sources = [(att.reshape(B, -1), weights["dense/kernel"]), (hidden, weights["dense_1/kernel"])]
    terms, dlin = linear_terms(linear_cols, feed, weights, dt)
    if terms is not None and terms.shape[1] != F:
        raise ValueError("operands could not be broadcast: %d first-order terms, %d fields" % (terms.shape[1], F))
    bias = weights["prediction_layer/global_bias"].astype(dt)
    if absolute:
        out, _m = ifm_op(flat, F, d, sources=sources, softmax=kind == "IFM", lin=terms, add=[] if dlin is None else [dlin],
                         bias=float(bias.reshape(-1)[0]), dtype=dt, absolute=True)
        return out.reshape(-1, 1)
    logit, m = ifm_op(flat, F, d, sources=sources, softmax=kind == "IFM", lin=terms, add=[] if dlin is None else [dlin], dtype=dt)
    return R.prediction_layer(logit.reshape(-1, 1), bias, task)


def run_fixture(g, dtype=np.float32, task=None, weights=None, absolute=False):
    """The oracle over a tests/golden/model_ifm*.npz / model_difm*.npz fixture (task='regression': the logit; `weights` overrides the
    fixture's)."""
    import json
    from tests.spec import columns_from_spec
    meta = json.loads(bytes(g["meta"]).decode())
    feed = {k[5:]: v for k, v in g.items() if k.startswith("feed/")}
    if weights is None:
        weights = {k[2:]: v for k, v in g.items() if k.startswith("w/")}
    kw = dict(meta["kwargs"])
    if task is not None:
        kw["task"] = task
    return input_aware(meta["model"], columns_from_spec(meta["linear"]), columns_from_spec(meta["dnn"]), weights, feed, dtype=dtype,
                       absolute=absolute, **kw)
