"""NumPy oracle of BST (reference deepctr/models/sequence/bst.py:21-107), Transformer (layers/sequence.py:523-635), PositionEncoding
(:683-689) and LayerNormalization (layers/normalization.py:34-43), float64 or float32, written from the math on the shared oracle
helpers (embedding tables, hashing, sequence pooling, the attention pooling layer, DNN)."""
import numpy as np

from oracle import ref_numpy as R
from oracle.ref_models import (_combined_dnn_input, _dnn, _feed, _is_dense, _is_sparse, _is_varlen, _lookup_idx, _table_names)

NEG = float(-2 ** 32 + 1)


def layer_norm(x, gamma, beta, eps=1e-9):
    """(x - mean) / sqrt(var + eps) * gamma + beta over the last axis, var the biased variance."""
    mean = x.mean(axis=-1, keepdims=True)
    var = np.square(x - mean).mean(axis=-1, keepdims=True)
    return (x - mean) / np.sqrt(var + x.dtype.type(eps)) * gamma + beta


def sequence_mask(lengths, T):
    return np.arange(T)[None, :] < np.asarray(lengths).reshape(-1, 1)


def transformer(queries, keys, w, head_num, query_mask=None, key_mask=None, use_positional_encoding=True, use_res=True,
                use_feed_forward=True, use_layer_norm=False, blinding=True, output_type="mean", dtype=np.float64, stats=None):
    """One Transformer layer.  queries, keys [B,T,E]; masks bool [B,T] (None: all ones); ``w``: query, key, value [E,E], fw1 [E,4E],
    fw2 [4E,E], ln_gamma, ln_beta [E], pe_q, pe_k [T,E] (the UNSCALED lookup tables).  ``stats``: a list that receives, per row that
    enters a LayerNorm, var / mean-square (inf for an all-zero row)."""
    dt = np.dtype(dtype).type
    g = lambda k: np.asarray(w[k]).astype(dt)   # noqa: E731
    q_in, k_in = np.asarray(queries).astype(dt), np.asarray(keys).astype(dt)
    B, T, E = q_in.shape
    H = int(head_num)
    d = E // H
    qm = np.ones((B, T), bool) if query_mask is None else np.asarray(query_mask).astype(bool)
    km = np.ones((B, T), bool) if key_mask is None else np.asarray(key_mask).astype(bool)
    if use_positional_encoding:
        scale = dt(E ** 0.5)
        q_in = q_in + g("pe_q") * scale
        k_in = k_in + g("pe_k") * scale

    def heads(x, name):
        return (x @ g(name)).reshape(B, T, H, d).transpose(0, 2, 1, 3)       # [B,H,T,d]
    Q, K, V = heads(q_in, "query"), heads(k_in, "key"), heads(k_in, "value")
    s = Q @ K.transpose(0, 1, 3, 2) / dt(d ** 0.5)                            # [B,H,Tq,Tk]
    s = np.where(km[:, None, None, :], s, dt(NEG))
    if blinding:
        s = np.where(np.eye(T, dtype=bool)[None, None], dt(NEG), s)
    s = s - s.max(axis=-1, keepdims=True)
    p = np.exp(s)
    p = p / p.sum(axis=-1, keepdims=True)
    p = p * qm[:, None, :, None].astype(dt)
    r = (p @ V).transpose(0, 2, 1, 3).reshape(B, T, E)
    if use_res:
        r = r + q_in

    def ln(x):
        if stats is not None:
            m = x.mean(axis=-1, keepdims=True)
            var, ms = np.square(x - m).mean(axis=-1).reshape(-1), np.square(x).mean(axis=-1).reshape(-1)
            # (an all-zero row — no residual, query mask 0 — meets var >= c * ms for every c and normalises to beta whatever eps is)
            stats.extend(np.where(ms > 0, var / np.where(ms > 0, ms, 1), np.inf))
        return layer_norm(x, g("ln_gamma"), g("ln_beta"))
    if use_layer_norm:
        r = ln(r)
    if use_feed_forward:
        if use_res:
            r = r + np.maximum(r @ g("fw1"), 0) @ g("fw2")
        if use_layer_norm:
            r = ln(r)
    if output_type == "mean":
        return r.mean(axis=1, keepdims=True)
    if output_type == "sum":
        return r.sum(axis=1, keepdims=True)
    return r


def transformer_name(i):
    return "transformer" if i == 0 else "transformer_%d" % i


def layer_weights(weights, i, use_positional_encoding=True):
    """The weights of the i-th Transformer of a model out of the fixture's name -> array dict: its own query .. fw2, the i-th
    LayerNormalization and the (2i)-th / (2i+1)-th PositionEncoding (query_pe is built first, sequence.py:518-519)."""
    n = transformer_name(i)
    sfx = lambda base, k: base if k == 0 else "%s_%d" % (base, k)    # noqa: E731
    w = {k: weights["%s/%s" % (n, k)] for k in ("query", "key", "value", "fw1", "fw2") if "%s/%s" % (n, k) in weights}
    w["ln_gamma"] = weights[sfx("layer_normalization", i) + "/gamma"]
    w["ln_beta"] = weights[sfx("layer_normalization", i) + "/beta"]
    if use_positional_encoding:
        w["pe_q"] = weights[sfx("position_encoding", 2 * i) + "/lookup_table"]
        w["pe_k"] = weights[sfx("position_encoding", 2 * i + 1) + "/lookup_table"]
    return w


def bst(dnn_cols, history_feature_list, weights, feed, transformer_num=1, att_head_num=8, use_bn=False, dnn_hidden_units=(256, 128, 64),
        dnn_activation="relu", task="binary", dtype=np.float64, stats=None, **_):
    dt = np.dtype(dtype).type
    tables = _table_names(dnn_cols, "")
    sparse = [fc for fc in dnn_cols if _is_sparse(fc)]
    varlen = [fc for fc in dnn_cols if _is_varlen(fc)]
    hist_names = ["hist_" + n for n in history_feature_list]
    hist_cols = [fc for fc in varlen if fc.name in hist_names]
    other_varlen = [fc for fc in varlen if fc.name not in hist_names]
    lengths = np.asarray(feed["seq_length"]).reshape(-1)                                        # bst.py:45

    def emb_of(fc, mask_zero_hash):
        idx = _lookup_idx(fc, feed, mask_zero=mask_zero_hash)
        tname, _ = tables[fc.embedding_name]
        return R.embedding(weights[tname + "/embeddings"].astype(dt), idx)

    query = [emb_of(fc, False) for fc in sparse if fc.name in history_feature_list]             # bst.py:68-69 (no mask_feat_list)
    hist = [emb_of(fc, False) for fc in hist_cols]                                              # bst.py:70-71
    dnn_emb = [emb_of(fc, fc.name in history_feature_list) for fc in sparse]                    # bst.py:72-73
    dense = [_feed(feed, fc.name).astype(dt) for fc in dnn_cols if _is_dense(fc)]
    for fc in other_varlen:                                                                     # bst.py:75-79
        idx = _lookup_idx(fc, feed, mask_zero=True)
        tname, mz = tables[fc.embedding_name]
        seq = R.embedding(weights[tname + "/embeddings"].astype(dt), idx)
        mask = (idx != 0) if mz else None
        kw = dict(lengths=_feed(feed, fc.length_name)) if fc.length_name is not None else dict(mask=mask)
        if fc.weight_name is not None:
            seq = R.weighted_sequence(seq, np.asarray(feed[fc.weight_name]).astype(dt), weight_normalization=fc.weight_norm, **kw)
        dnn_emb.append(R.sequence_pooling(seq, fc.combiner, **kw))
    h = np.concatenate(hist, axis=-1)                                                           # bst.py:82
    T = h.shape[1]
    m = sequence_mask(lengths, T)
    for i in range(transformer_num):                                                            # bst.py:84-92
        h = transformer(h, h, layer_weights(weights, i), att_head_num, m, m, True, True, True, True, False, None, dtype=dt, stats=stats)
    ks, bs, i = [], [], 0
    while "dnn/kernel%d" % i in weights:                # the attention unit's DNN is built before the model's ("dnn", then "dnn_1")
        ks.append(weights["dnn/kernel%d" % i].astype(dt))
        bs.append(weights["dnn/bias%d" % i].astype(dt))
        i += 1
    att = R.attention_sequence_pooling(np.concatenate(query, axis=-1), h, m, ks, bs, weights["local_activation_unit/kernel"].astype(dt),
                                       weights["local_activation_unit/bias"].astype(dt), "sigmoid", None, True)      # bst.py:94-96
    deep = np.concatenate([np.concatenate(dnn_emb, axis=-1), att], axis=-1)                     # bst.py:97
    dnn_in = _combined_dnn_input([deep.reshape(deep.shape[0], 1, -1)], dense)
    out = _dnn("dnn_1", dnn_in, weights, dt, dnn_activation, use_bn)
    logit = out @ weights["dense/kernel"].astype(dt)
    return R.prediction_layer(logit, weights["prediction_layer/global_bias"].astype(dt), task)


def run_fixture(g, dtype=np.float64, task=None, stats=None):
    """The oracle over a tests/golden/model_bst_*.npz fixture (task='regression': the logit)."""
    import json
    from tests.spec import columns_from_spec
    meta = json.loads(bytes(g["meta"]).decode())
    feed = {k[5:]: v for k, v in g.items() if k.startswith("feed/")}
    weights = {k[2:]: v for k, v in g.items() if k.startswith("w/")}
    kw = dict(meta["kwargs"])
    if task is not None:
        kw["task"] = task
    return bst(columns_from_spec(meta["dnn"]), meta["extra_args"][0], weights, feed, dtype=dtype, stats=stats, **kw)
