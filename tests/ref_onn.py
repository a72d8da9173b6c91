"""NumPy oracle of ONN (reference deepctr/models/onn.py:32-116), float64 or float32, on the shared oracle helpers (linear logit, DNN,
sequence pooling, Hash), plus ``ffm_pairs``: the layer-level function of the fused field-aware tables the op tests use.

``absolute=True`` runs the same graph on absolute values (weights, dense inputs, and the BatchNormalization as |x| |inv| + |beta| +
|mean| |inv|): an upper bound of the magnitude every output was summed at, the ``terms`` of tests.util.assert_close_terms."""
import itertools

import numpy as np

from oracle import ref_numpy as R
from oracle.ref_models import _add, _dnn, _feed, _is_dense, _is_sparse, _is_varlen, linear_logit

BN_EPS = 1e-3       # keras BatchNormalization default


def slot(j, i):
    """Slot of partner i inside feature j's fused row: field order with j itself skipped."""
    return i if i < j else i - 1


def ffm_pairs(ids, masters, reduce_sum=False, scale=None, shift=None, dense=None, pooled=None, dtype=np.float64, absolute=False):
    """ids [F, B]; masters[j]: the fused table [V_j, F-1, d]; ``pooled`` {j: [B, (F-1)*d]}: fields that arrive pre-pooled (their ids
    unused) -> [B, P*d (+ n_dense)] ([B, P (+ n_dense)] with reduce_sum): per pair (i < j, itertools.combinations order)
    master_i[id_i, slot(j)] * master_j[id_j, slot(i)], then * scale + shift over the pair columns, then the dense values."""
    dt = np.dtype(dtype).type
    ab = np.abs if absolute else (lambda v: v)
    F = len(masters)
    B = np.asarray(ids).shape[1]
    pooled = pooled or {}
    rows = []
    for j in range(F):
        if j in pooled:
            d = np.asarray(pooled[j]).shape[1] // (F - 1)
            rows.append(ab(np.asarray(pooled[j]).astype(dt))[:B, :(F - 1) * d].reshape(B, F - 1, d))
        else:
            m = np.asarray(masters[j])
            idx = np.asarray(ids[j]).astype(np.int64)
            if idx.size and (idx.min() < 0 or idx.max() >= m.shape[0]):
                raise IndexError("embedding index out of range")
            rows.append(ab(m.astype(dt))[idx])
    outs = []
    for i, j in itertools.combinations(range(F), 2):
        pr = rows[i][:, slot(i, j)] * rows[j][:, slot(j, i)]
        outs.append(pr.sum(-1, keepdims=True) if reduce_sum else pr)
    x = np.concatenate(outs, axis=-1)
    if scale is not None:
        x = x * ab(np.asarray(scale).astype(dt)) + ab(np.asarray(shift).astype(dt))
    if dense is not None:
        x = np.concatenate([x, ab(np.asarray(dense).astype(dt))], axis=-1)
    return x


def _field_order(dnn_cols):
    return [fc for fc in dnn_cols if _is_sparse(fc)] + [fc for fc in dnn_cols if _is_varlen(fc)]


def onn(linear_cols, dnn_cols, weights, feed, dnn_hidden_units=(256, 128, 64), use_bn=True, reduce_sum=False, task="binary",
        dtype=np.float32, absolute=False, **_):
    dt = np.dtype(dtype).type
    if absolute:
        weights = {k: np.abs(v) for k, v in weights.items()}
        feed = {k: (np.abs(v) if np.asarray(v).dtype.kind == "f" else v) for k, v in feed.items()}
    lin = linear_logit(linear_cols, feed, weights, dt)
    deep = _field_order(dnn_cols)
    idx = {}
    for fc in deep:                                 # hashed once per feature, plain Hash(vocabulary_size) (onn.py:80-85)
        x = _feed(feed, fc.name)
        idx[fc.name] = (R.hash_layer(x, fc.vocabulary_size, mask_zero=False, vocabulary_path=fc.vocabulary_path) if fc.use_hash
                        else x.astype(np.int64))

    def emb(fc_i, fc_j):                            # feature_embedding (onn.py:111-116): fc_i's embedding towards fc_j, [B, d]
        table = weights["sparse_emb_%s_%s/embeddings" % (fc_i.embedding_name, fc_j.embedding_name)].astype(dt)
        e = R.embedding(table, idx[fc_i.name])
        if _is_sparse(fc_i):
            return e.reshape(e.shape[0], -1)
        # SequencePoolingLayer(combiner, supports_masking=True) on the Embedding's mask_zero mask of the (hashed) id
        return R.sequence_pooling(e, fc_i.combiner, mask=idx[fc_i.name] != 0).reshape(e.shape[0], -1)

    outs = []
    for fc_i, fc_j in itertools.combinations(deep, 2):
        pr = emb(fc_i, fc_j) * emb(fc_j, fc_i)
        outs.append(pr.sum(-1, keepdims=True) if reduce_sum else pr)
    x = np.concatenate(outs, axis=-1)
    if use_bn:
        g, b, m, v = (weights["batch_normalization/" + n].astype(dt) for n in ("gamma", "beta", "moving_mean", "moving_variance"))
        inv = g / np.sqrt(v + dt(BN_EPS))
        x = x * inv + (b + m * inv if absolute else b - m * inv)
    dense = [_feed(feed, fc.name).astype(dt) for fc in dnn_cols if _is_dense(fc)]
    if dense:
        x = np.concatenate([x] + [d.reshape(d.shape[0], -1) for d in dense], axis=-1)
    h = _dnn("dnn", x, weights, dt, "relu")
    logit = h @ weights["dense/kernel"].astype(dt)
    return R.prediction_layer(_add(logit, lin), weights["prediction_layer/global_bias"].astype(dt), task)


def run_fixture(g, dtype=np.float32, task=None, weights=None, absolute=False):
    """The oracle over a tests/golden/model_onn*.npz fixture (task='regression': the logit; `weights` overrides the fixture's)."""
    import json
    from tests.spec import columns_from_spec
    meta = json.loads(bytes(g["meta"]).decode())
    feed = {k[5:]: v for k, v in g.items() if k.startswith("feed/")}
    if weights is None:
        weights = {k[2:]: v for k, v in g.items() if k.startswith("w/")}
    kw = dict(meta["kwargs"])
    if task is not None:
        kw["task"] = task
    return onn(columns_from_spec(meta["linear"]), columns_from_spec(meta["dnn"]), weights, feed, dtype=dtype, absolute=absolute, **kw)
