"""NumPy oracle of AutoInt (reference deepctr/models/autoint.py:21-84) and InteractingLayer (layers/interaction.py:749-779), float64
or float32, on the shared oracle helpers (embedding groups, linear logit, DNN input, DNN, keras Add)."""
import numpy as np

from oracle import ref_numpy as R
from oracle.ref_models import _add, _combined_dnn_input, _dnn, _embed_groups, linear_logit


def _softmax(x):
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def interacting_layer(x, query, key, value, res, d, H, use_res=True, scaling=False, dtype=np.float64):
    """x [B,F,E] -> [B,F,d*H]."""
    dt = np.dtype(dtype).type
    x = np.asarray(x).astype(dt)
    B, F = x.shape[0], x.shape[1]

    def heads(w):
        return np.tensordot(x, np.asarray(w).astype(dt), axes=(-1, 0)).reshape(B, F, H, d).transpose(2, 0, 1, 3)    # [H,B,F,d]
    q, k, v = heads(query), heads(key), heads(value)
    s = q @ k.transpose(0, 1, 3, 2)
    if scaling:
        s = s / dt(d ** 0.5)
    o = (_softmax(s) @ v).transpose(1, 2, 0, 3).reshape(B, F, H * d)
    if use_res:
        o = o + np.tensordot(x, np.asarray(res).astype(dt), axes=(-1, 0))
    return np.maximum(o, 0)


def layer_name(i):
    return "interacting_layer" if i == 0 else "interacting_layer_%d" % i


def autoint(linear_cols, dnn_cols, weights, feed, att_layer_num=3, att_embedding_size=8, att_head_num=2, att_res=True,
            dnn_hidden_units=(256, 128, 64), dnn_activation="relu", dnn_use_bn=False, task="binary", dtype=np.float32, **_):
    dt = np.dtype(dtype).type
    lin = linear_logit(linear_cols, feed, weights, dt)
    groups, dense = _embed_groups(dnn_cols, feed, weights, "", dt)
    embs = [e for g in groups.values() for e in g]
    outs = []
    if att_layer_num > 0:
        h = np.concatenate(embs, axis=1)                                  # [B,F,E]
        for i in range(att_layer_num):
            n = layer_name(i)
            h = interacting_layer(h, weights[n + "/query"], weights[n + "/key"], weights[n + "/value"],
                                  weights.get(n + "/res"), att_embedding_size, att_head_num, att_res, dtype=dt)
        outs.append(h.reshape(h.shape[0], -1))
    if len(dnn_hidden_units) > 0:
        outs.append(_dnn("dnn", _combined_dnn_input(embs, dense), weights, dt, dnn_activation, dnn_use_bn))
    final = _add(np.concatenate(outs, axis=-1) @ weights["dense/kernel"].astype(dt), lin)
    return R.prediction_layer(final, weights["prediction_layer/global_bias"].astype(dt), task)


def run_fixture(g, dtype=np.float32, task=None):
    """The oracle over a tests/golden/model_autoint_*.npz fixture (task='regression': the logit)."""
    import json
    from tests.spec import columns_from_spec
    meta = json.loads(bytes(g["meta"]).decode())
    feed = {k[5:]: v for k, v in g.items() if k.startswith("feed/")}
    weights = {k[2:]: v for k, v in g.items() if k.startswith("w/")}
    kw = dict(meta["kwargs"])
    if task is not None:
        kw["task"] = task
    return autoint(columns_from_spec(meta["linear"]), columns_from_spec(meta["dnn"]), weights, feed, dtype=dtype, **kw)
