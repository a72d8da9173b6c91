"""NumPy oracle of FwFM (reference deepctr/models/fwfm.py:21-71), DeepFEFM (deepctr/models/deepfefm.py:23-108), FwFMLayer
(layers/interaction.py:1351-1425) and FEFMLayer (:1428-1499), float64 or float32, on the shared oracle helpers (embedding groups,
linear logit, DNN, keras Add)."""
import itertools

import numpy as np

from oracle import ref_numpy as R
from oracle.ref_models import _add, _dnn, _embed_groups, linear_logit


def _pairs(F):
    ii, jj = (np.array(v, dtype=np.int64).reshape(-1) for v in zip(*itertools.combinations(range(F), 2)))
    return ii, jj


def fwfm_layer(x, r, dtype=np.float64):
    """x [B,F,E], r [F,F] -> [B,1] = sum_{i<j} r[i][j] <x_i, x_j>."""
    dt = np.dtype(dtype).type
    x, r = np.asarray(x).astype(dt), np.asarray(r).astype(dt)
    ii, jj = _pairs(x.shape[1])
    return ((x[:, ii] * x[:, jj]).sum(-1) * r[ii, jj]).sum(-1, keepdims=True)


def fefm_layer(x, weights, dtype=np.float64):
    """x [B,F,E]; weights: the P pair matrices in itertools.combinations order -> [B,P] = x_i^T (W + W^T) x_j."""
    dt = np.dtype(dtype).type
    x = np.asarray(x).astype(dt)
    w = np.stack([np.asarray(m).astype(dt) for m in weights])
    ii, jj = _pairs(x.shape[1])
    return (np.einsum("bpe,ped->bpd", x[:, ii], w + w.transpose(0, 2, 1)) * x[:, jj]).sum(-1)


def fefm_weights(weights, name, F):
    return [weights["%s/field_embeddings%d-%d" % (name, i, j)] for i, j in itertools.combinations(range(F), 2)]


def _flat_dnn_input(groups, dense, B):
    return np.concatenate([np.asarray(e).reshape(B, -1) for g in groups.values() for e in g] +
                          [np.asarray(d).reshape(B, -1) for d in dense], axis=-1)


def fwfm(linear_cols, dnn_cols, weights, feed, fm_group=("default_group",), dnn_hidden_units=(256, 128, 64), dnn_activation="relu",
         dnn_use_bn=False, task="binary", dtype=np.float32, **_):
    dt = np.dtype(dtype).type
    lin = linear_logit(linear_cols, feed, weights, dt)
    groups, dense = _embed_groups(dnn_cols, feed, weights, "", dt)
    logits = []
    i = 0
    for k, v in groups.items():
        if k not in fm_group:
            continue
        pre = "fw_fm_layer" if i == 0 else "fw_fm_layer_%d" % i
        logits.append(fwfm_layer(np.concatenate(v, axis=1), weights[pre + "/field_pair_strengths"], dt))
        i += 1
    if len(dnn_hidden_units) > 0:
        h = _flat_dnn_input(groups, dense, logits[0].shape[0])
        h = _dnn("dnn", h, weights, dt, dnn_activation, use_bn=dnn_use_bn)
        logits.append(h @ weights["dense/kernel"].astype(dt))
    return R.prediction_layer(_add(lin, *logits), weights["prediction_layer/global_bias"].astype(dt), task)


def deepfefm(linear_cols, dnn_cols, weights, feed, use_fefm=True, dnn_hidden_units=(256, 128, 64), exclude_feature_embed_in_dnn=False,
             use_linear=True, use_fefm_embed_in_dnn=True, dnn_activation="relu", dnn_use_bn=False, task="binary", dtype=np.float32, **_):
    dt = np.dtype(dtype).type
    lin = linear_logit(linear_cols, feed, weights, dt)
    groups, dense = _embed_groups(dnn_cols, feed, weights, "", dt)
    x = np.concatenate(groups["default_group"], axis=1)             # [B,F,E]
    B, F = x.shape[0], x.shape[1]
    pairs = fefm_layer(x, fefm_weights(weights, "fefm_layer", F), dt)
    logits = []
    if use_linear:
        logits.append(lin)
    if use_fefm:
        logits.append(pairs.sum(-1, keepdims=True))
    if len(dnn_hidden_units) > 0:
        h = _flat_dnn_input(groups, dense, B)
        if use_fefm_embed_in_dnn:
            h = pairs if exclude_feature_embed_in_dnn else np.concatenate([h, pairs], axis=-1)
        h = _dnn("dnn", h, weights, dt, dnn_activation, use_bn=dnn_use_bn)
        logits.append(h @ weights["dense/kernel"].astype(dt))
    if not logits:
        raise NotImplementedError
    return R.prediction_layer(_add(*logits), weights["prediction_layer/global_bias"].astype(dt), task)


def run_fixture(g, dtype=np.float32, task=None, weights=None):
    """The oracle over a tests/golden/model_fwfm*.npz / model_fefm*.npz fixture (task='regression': the logit; `weights` overrides
    the fixture's)."""
    import json
    from tests.spec import columns_from_spec
    meta = json.loads(bytes(g["meta"]).decode())
    feed = {k[5:]: v for k, v in g.items() if k.startswith("feed/")}
    if weights is None:
        weights = {k[2:]: v for k, v in g.items() if k.startswith("w/")}
    kw = dict(meta["kwargs"])
    if task is not None:
        kw["task"] = task
    fn = fwfm if meta["model"] == "FwFM" else deepfefm
    return fn(columns_from_spec(meta["linear"]), columns_from_spec(meta["dnn"]), weights, feed, dtype=dtype, **kw)
