"""NumPy oracle of FLEN (reference deepctr/models/flen.py:22-81) and FieldWiseBiInteraction (layers/interaction.py:1224-1348), float64
or float32, on the shared oracle helpers (embedding groups, linear logit, DNN, keras Add).

``absolute=True`` is the magnitude mode for tests.util.assert_close_terms: sum |w| |s_i| |s_j| + sum |k| (s^2 + q) + |b| over absolute
inputs.  (The plain formula on absolute values would keep the subtraction s^2 - q and under-estimate the magnitude.)"""
import itertools

import numpy as np

from oracle import ref_numpy as R
from oracle.ref_models import _add, _dnn, _embed_groups, linear_logit


def pairs(G):
    """The group pairs in the order kernel_mf's rows meet them (interaction.py:1301)."""
    return list(itertools.combinations(range(G), 2))


def fieldwise_layer(xs, kernel_mf, kernel_fm, bias_mf=None, bias_fm=None, dtype=np.float64, absolute=False):
    """xs: G arrays [B, n_g, d]; kernel_mf [G(G-1)/2(, 1)], kernel_fm [G(, 1)], the biases [d] or None -> [B, d]."""
    dt = np.dtype(dtype).type
    ab = np.abs if absolute else (lambda v: v)
    xs = [ab(np.asarray(x).astype(dt)) for x in xs]
    w, k = ab(np.asarray(kernel_mf).astype(dt)).reshape(-1), ab(np.asarray(kernel_fm).astype(dt)).reshape(-1)
    G = len(xs)
    assert w.shape == (G * (G - 1) // 2,) and k.shape == (G,)
    s = [x.sum(1) for x in xs]
    q = [(x * x).sum(1) for x in xs]
    h_mf = np.zeros_like(s[0])
    for p, (i, j) in enumerate(pairs(G)):
        h_mf = h_mf + w[p] * s[i] * s[j]
    h_fm = np.zeros_like(s[0])
    for g in range(G):
        h_fm = h_fm + k[g] * ((s[g] * s[g] + q[g]) if absolute else (s[g] * s[g] - q[g]))
    if bias_mf is not None:
        h_mf = h_mf + ab(np.asarray(bias_mf).astype(dt))
        h_fm = h_fm + ab(np.asarray(bias_fm).astype(dt))
    return h_mf + h_fm


def fieldwise_op(xbuf, groups, dim, kernel_mf, kernel_fm, bias_mf=None, bias_fm=None, x_offset=0, head_w=None, add=None,
                 dtype=np.float64, absolute=False):
    """What dctr_fieldwise_fwd computes from a [B, stride] buffer and a (first column, n fields) table -> (y [B, d], logit [B] or None)."""
    dt = np.dtype(dtype).type
    ab = np.abs if absolute else (lambda v: v)
    xbuf = np.asarray(xbuf)
    B = xbuf.shape[0]
    xs = [xbuf[:, x_offset + f:x_offset + f + n * dim].reshape(B, n, dim) for f, n in groups]
    y = fieldwise_layer(xs, kernel_mf, kernel_fm, bias_mf, bias_fm, dtype=dt, absolute=absolute)
    logit = None
    if head_w is not None:
        logit = y @ ab(np.asarray(head_w).astype(dt)).reshape(-1)
        if add is not None:
            logit = logit + ab(np.asarray(add).astype(dt)).reshape(-1)
    return y, logit


def flen(linear_cols, dnn_cols, weights, feed, dnn_hidden_units=(256, 128, 64), dnn_activation="relu", dnn_use_bn=False, task="binary",
         dtype=np.float32, absolute=False, **_):
    """``absolute``: the bound of the magnitude the logit was summed at, for models without BatchNormalization, weighted sequences or a
    DNN activation other than relu / linear: weights and dense inputs by magnitude, the layer through its magnitude mode."""
    dt = np.dtype(dtype).type
    if absolute:
        assert not dnn_use_bn and dnn_activation in ("relu", "linear")
        weights = {k: np.abs(v) for k, v in weights.items()}
        feed = {k: (np.abs(v) if np.asarray(v).dtype.kind == "f" else v) for k, v in feed.items()}
    lin = linear_logit(linear_cols, feed, weights, dt)
    groups, dense = _embed_groups(dnn_cols, feed, weights, "", dt)
    n = "field_wise_bi_interaction"
    xs = [np.concatenate(v, axis=1) for v in groups.values()]
    B = xs[0].shape[0]
    fw = fieldwise_layer(xs, weights[n + "/kernel_mf"], weights[n + "/kernel_fm"], weights.get(n + "/bias_mf"), weights.get(n + "/bias_fm"),
                         dtype=dt, absolute=absolute)
    h = np.concatenate([np.asarray(e).reshape(B, -1) for g in groups.values() for e in g] +
                       [np.asarray(d).reshape(B, -1) for d in dense], axis=-1)
    h = _dnn("dnn", h, weights, dt, dnn_activation, use_bn=dnn_use_bn)
    logit = np.concatenate([fw, h], axis=-1) @ weights["dense/kernel"].astype(dt)
    bias = weights["prediction_layer/global_bias"].astype(dt)
    if absolute:
        return _add(lin, logit) + np.abs(bias)
    return R.prediction_layer(_add(lin, logit), bias, task)


def run_fixture(g, dtype=np.float32, task=None, weights=None, absolute=False):
    """The oracle over a tests/golden/model_flen*.npz fixture (task='regression': the logit; `weights` overrides the fixture's)."""
    import json
    from tests.spec import columns_from_spec
    meta = json.loads(bytes(g["meta"]).decode())
    feed = {k[5:]: v for k, v in g.items() if k.startswith("feed/")}
    if weights is None:
        weights = {k[2:]: v for k, v in g.items() if k.startswith("w/")}
    kw = dict(meta["kwargs"])
    if task is not None:
        kw["task"] = task
    return flen(columns_from_spec(meta["linear"]), columns_from_spec(meta["dnn"]), weights, feed, dtype=dtype, absolute=absolute, **kw)
