"""NumPy oracle of FiBiNET (reference deepctr/models/fibinet.py:19-66), SENETLayer (layers/interaction.py:1067-1139) and
BilinearInteraction (:1142-1221), float64 or float32, on the shared oracle helpers (embedding groups, linear logit, DNN, keras Add)."""
import itertools

import numpy as np

from oracle import ref_numpy as R
from oracle.ref_models import _add, _dnn, _embed_groups, linear_logit


def senet(x, W_1, W_2, dtype=np.float64):
    """x [B,F,E] -> [B,F,E]."""
    dt = np.dtype(dtype).type
    x = np.asarray(x).astype(dt)
    a1 = np.maximum(x.mean(axis=-1) @ np.asarray(W_1).astype(dt), 0)
    a2 = np.maximum(a1 @ np.asarray(W_2).astype(dt), 0)
    return x * a2[:, :, None]


def bilinear(x, weights, bilinear_type, dtype=np.float64):
    """x [B,F,E]; weights: the layer's matrices in creation order -> [B, F(F-1)/2, E]."""
    dt = np.dtype(dtype).type
    x = np.asarray(x).astype(dt)
    ws = np.stack([np.asarray(w).astype(dt) for w in weights])
    F = x.shape[1]
    ii, jj = (np.array(v, dtype=np.int64).reshape(-1) for v in zip(*itertools.combinations(range(F), 2)))
    if bilinear_type == "all":
        return (x[:, :F - 1] @ ws[0])[:, ii] * x[:, jj]
    if bilinear_type == "each":
        return np.einsum("bfe,fed->bfd", x[:, :F - 1], ws)[:, ii] * x[:, jj]
    return np.einsum("bpe,ped->bpd", x[:, ii], ws) * x[:, jj]


def layer_weights(weights, name, bilinear_type, F):
    if bilinear_type == "all":
        return [weights[name + "/bilinear_weight"]]
    if bilinear_type == "each":
        return [weights["%s/bilinear_weight%d" % (name, i)] for i in range(F - 1)]
    return [weights["%s/bilinear_weight%d_%d" % (name, i, j)] for i, j in itertools.combinations(range(F), 2)]


def fibinet(linear_cols, dnn_cols, weights, feed, bilinear_type="interaction", dnn_hidden_units=(256, 128, 64),
            dnn_activation="relu", task="binary", dtype=np.float32, **_):
    dt = np.dtype(dtype).type
    lin = linear_logit(linear_cols, feed, weights, dt)
    groups, dense = _embed_groups(dnn_cols, feed, weights, "", dt)
    x = np.concatenate([e for g in groups.values() for e in g], axis=1)       # [B,F,E]
    B, F = x.shape[0], x.shape[1]
    v = senet(x, weights["senet_layer/W_1"], weights["senet_layer/W_2"], dt)
    # concat_func([senet_bilinear_out, bilinear_out]) joins on the LAST axis (layers/utils.py:236), then Flatten
    both = np.concatenate([bilinear(v, layer_weights(weights, "bilinear_interaction", bilinear_type, F), bilinear_type, dt),
                           bilinear(x, layer_weights(weights, "bilinear_interaction_1", bilinear_type, F), bilinear_type, dt)], axis=-1)
    parts = [both.reshape(B, -1)] + [np.asarray(d).reshape(B, -1) for d in dense]
    h = np.concatenate(parts, axis=-1)
    if len(dnn_hidden_units) > 0:
        h = _dnn("dnn", h, weights, dt, dnn_activation)
    final = _add(h @ weights["dense/kernel"].astype(dt), lin)
    return R.prediction_layer(final, weights["prediction_layer/global_bias"].astype(dt), task)


def run_fixture(g, dtype=np.float32, task=None, weights=None):
    """The oracle over a tests/golden/model_fibinet_*.npz fixture (task='regression': the logit; `weights` overrides the fixture's)."""
    import json
    from tests.spec import columns_from_spec
    meta = json.loads(bytes(g["meta"]).decode())
    feed = {k[5:]: v for k, v in g.items() if k.startswith("feed/")}
    if weights is None:
        weights = {k[2:]: v for k, v in g.items() if k.startswith("w/")}
    kw = dict(meta["kwargs"])
    if task is not None:
        kw["task"] = task
    return fibinet(columns_from_spec(meta["linear"]), columns_from_spec(meta["dnn"]), weights, feed, dtype=dtype, **kw)
