"""NumPy oracle of DIEN (reference deepctr/models/sequence/dien.py:22-219), DynamicGRU (layers/sequence.py:760-815), tf's GRUCell and the
attention-gated cells (contrib/utils.py:208-261 AGRU, :327-378 AUGRU) under dynamic_rnn's sequence_length rule (contrib/rnn_v2.py:1324-1401),
float64 or float32.  Written from the equations, independently of the torch restatement and of the kernel:
    [r | u] = sigmoid([x_t | h] Wg + bg);  c = tanh([x_t | r * h] Wc + bc)
    GRU  h' = u h + (1 - u) c;   AGRU  h' = (1 - a) h + a c;   AUGRU  u <- (1 - a) u, then the GRU form
    t >= length: the state is copied through and the emitted row is zero; the final state is the state at min(length, T).
The model stands on the shared oracle helpers (embedding tables, hashing, sequence pooling, the attention pooling layer, DNN)."""
import numpy as np

from oracle import ref_numpy as R
from oracle.ref_models import _combined_dnn_input, _dnn, _feed, _is_dense, _is_sparse, _is_varlen, _lookup_idx, _table_names

CELLS = ("GRU", "AGRU", "AUGRU")


def sigmoid(x):
    """1 / (1 + e^-x) without overflow: e^-|x| only."""
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1 / (1 + e), e / (1 + e)).astype(x.dtype)


def sequence_mask(lengths, T):
    return np.arange(T)[None, :] < np.asarray(lengths).reshape(-1, 1)


def gru_step(x, h, wg, bg, wc, bc, cell="GRU", a=None):
    """One step of a cell: x, h [B,E], a [B,1] -> h' [B,E]."""
    E = h.shape[1]
    ru = sigmoid(np.concatenate([x, h], axis=1) @ wg + bg)
    r, u = ru[:, :E], ru[:, E:]
    c = np.tanh(np.concatenate([x, r * h], axis=1) @ wc + bc)
    if cell == "AGRU":
        return (1 - a) * h + a * c
    if cell == "AUGRU":
        u = (1 - a) * u
    return u * h + (1 - u) * c


def dynamic_gru(x, lengths, layers, cell="GRU", att_scores=None, scale_input=False, return_sequence=True, dtype=np.float64,
                ignore_length=False):
    """x [B,T,E], lengths [B], layers [(Wg [2E,2E], bg [2E], Wc [2E,E], bc [E])] stacked, att_scores [B,T] -> [B,T,E] or the final state
    [B,E].  ``ignore_length``: every step runs (what the length rule is compared against)."""
    dt = np.dtype(dtype).type
    x = np.asarray(x).astype(dt)
    B, T, E = x.shape
    lengths = np.full(B, T) if ignore_length else np.asarray(lengths).reshape(-1)
    a = None if att_scores is None else np.asarray(att_scores).astype(dt).reshape(B, T)
    if scale_input:
        x = x * a[:, :, None]
    h = np.zeros((B, E), dt)
    for wg, bg, wc, bc in layers:
        wg, bg, wc, bc = (np.asarray(v).astype(dt) for v in (wg, bg, wc, bc))
        h = np.zeros((B, E), dt)
        out = np.zeros((B, T, E), dt)
        for t in range(T):
            hn = gru_step(x[:, t], h, wg, bg, wc, bc, cell, None if a is None else a[:, t:t + 1])
            live = (t < lengths)[:, None]
            h = np.where(live, hn, h)
            out[:, t] = np.where(live, hn, 0)
        x = out
    return x if return_sequence else h


def auxiliary_loss(h_states, click_seq, noclick_seq, lengths, kernels, biases):
    """dien.py:22-63.  h_states, click_seq, noclick_seq [B,T-1,E]; lengths [B] (= seq_length - 1); the DNN [100, 50, 1] with sigmoid on
    every layer; the mean over ALL B (T - 1) entries of (-log p_click - log(1 - p_noclick)) * mask."""
    dt = h_states.dtype
    mask = sequence_mask(lengths, click_seq.shape[1]).astype(dt)
    click = R.dnn(np.concatenate([h_states, click_seq], axis=-1), kernels, biases, "sigmoid")[:, :, 0]
    noclick = R.dnn(np.concatenate([h_states, noclick_seq], axis=-1), kernels, biases, "sigmoid")[:, :, 0]
    return float(np.mean(-np.log(click) * mask - np.log(1 - noclick) * mask))


def _gru_weights(weights, name, dt):
    scope = name + "/gru_cell/" if name + "/gru_cell/gates/kernel" in weights else name + "/"
    return tuple(weights[scope + k].astype(dt) for k in ("gates/kernel", "gates/bias", "candidate/kernel", "candidate/bias"))


def _sfx(base, k):
    return base if k == 0 else "%s_%d" % (base, k)


def dien(dnn_cols, history_feature_list, weights, feed, gru_type="GRU", use_negsampling=False, alpha=1.0, use_bn=False,
         dnn_hidden_units=(256, 128, 64), dnn_activation="relu", att_hidden_units=(64, 16), att_activation="dice",
         att_weight_normalization=True, task="binary", dtype=np.float64, cell=None, ignore_length=False, want_aux=False, stats=None, **_):
    """The model.  ``cell``: run the evolution GRU with another cell kind; ``ignore_length``: run every step of both GRUs (the two
    perturbations the fixture conditions measure); ``want_aux``: returns (prediction, alpha x auxiliary loss); ``stats``: a list that
    receives the |final state| entries of the evolution GRU."""
    dt = np.dtype(dtype).type
    tables = _table_names(dnn_cols, "")
    sparse = [fc for fc in dnn_cols if _is_sparse(fc)]
    varlen = [fc for fc in dnn_cols if _is_varlen(fc)]
    hist_names = ["hist_" + n for n in history_feature_list]
    neg_names = ["neg_" + n for n in hist_names]
    hist_cols = [fc for fc in varlen if fc.name in hist_names]
    neg_cols = [fc for fc in varlen if fc.name in neg_names]
    other_varlen = [fc for fc in varlen if fc.name not in hist_names and fc.name not in neg_names]
    lengths = np.asarray(feed["seq_length"]).reshape(-1)                                        # dien.py:141

    def emb_of(fc, mask_zero_hash):
        idx = _lookup_idx(fc, feed, mask_zero=mask_zero_hash)
        tname, _ = tables[fc.embedding_name]
        return R.embedding(weights[tname + "/embeddings"].astype(dt), idx)

    query = np.concatenate([emb_of(fc, False) for fc in sparse if fc.name in history_feature_list], axis=-1)     # dien.py:169-170
    keys = np.concatenate([emb_of(fc, False) for fc in hist_cols], axis=-1)                                      # :172-173
    dnn_emb = [emb_of(fc, fc.name in history_feature_list) for fc in sparse]                                     # :174-175
    dense = [_feed(feed, fc.name).astype(dt) for fc in dnn_cols if _is_dense(fc)]
    for fc in other_varlen:                                                                                      # :178-180
        idx = _lookup_idx(fc, feed, mask_zero=True)
        tname, mz = tables[fc.embedding_name]
        seq = R.embedding(weights[tname + "/embeddings"].astype(dt), idx)
        mask = (idx != 0) if mz else None
        kw = dict(lengths=_feed(feed, fc.length_name)) if fc.length_name is not None else dict(mask=mask)
        if fc.weight_name is not None:
            seq = R.weighted_sequence(seq, np.asarray(feed[fc.weight_name]).astype(dt), weight_normalization=fc.weight_norm, **kw)
        dnn_emb.append(R.sequence_pooling(seq, fc.combiner, **kw))
    T = keys.shape[1]
    m = sequence_mask(lengths, T)
    # the DNNs in creation order: the auxiliary DNN (use_negsampling), the attention unit's, the model's
    n_aux = 1 if use_negsampling else 0
    att_dnn, main_dnn = _sfx("dnn", n_aux), _sfx("dnn", n_aux + 1)
    ks, bs, i = [], [], 0
    while "%s/kernel%d" % (att_dnn, i) in weights:
        ks.append(weights["%s/kernel%d" % (att_dnn, i)].astype(dt))
        bs.append(weights["%s/bias%d" % (att_dnn, i)].astype(dt))
        i += 1
    dice = None
    if att_activation in ("dice", "Dice"):
        dice = [(weights[_sfx("dice", j) + "/dice_alpha"].astype(dt), weights[_sfx("batch_normalization", j) + "/moving_mean"].astype(dt),
                 weights[_sfx("batch_normalization", j) + "/moving_variance"].astype(dt)) for j in range(i)]

    def attention(h, return_score):
        return R.attention_sequence_pooling(query, h, m, ks, bs, weights["local_activation_unit/kernel"].astype(dt),
                                            weights["local_activation_unit/bias"].astype(dt), att_activation, dice,
                                            att_weight_normalization, return_score=return_score)

    g1, g2 = _gru_weights(weights, "gru1", dt), _gru_weights(weights, "gru2", dt)
    h1 = dynamic_gru(keys, lengths, [g1], dtype=dt, ignore_length=ignore_length)                                 # dien.py:73-74
    aux = None
    if use_negsampling and want_aux:                                                                             # :76-81
        neg = np.concatenate([emb_of(fc, False) for fc in neg_cols], axis=-1)
        aks = [weights["dnn/kernel%d" % j].astype(dt) for j in range(3)]
        abs_ = [weights["dnn/bias%d" % j].astype(dt) for j in range(3)]
        aux = alpha * auxiliary_loss(h1[:, :-1], keys[:, 1:], neg[:, 1:], lengths - 1, aks, abs_)
    if gru_type == "GRU" and cell is None:                                                                       # :83-93
        h2 = dynamic_gru(h1, lengths, [g2], dtype=dt, ignore_length=ignore_length)
        hist = attention(h2, False)
        final = h2[np.arange(len(lengths)), np.clip(lengths, 1, T) - 1]
    else:                                                                                                        # :95-108
        scores = attention(h1, True)[:, 0, :]
        kind = cell or ("GRU" if gru_type == "AIGRU" else gru_type)
        final = dynamic_gru(h1, lengths, [g2], cell=kind, att_scores=scores, scale_input=gru_type == "AIGRU" and cell is None,
                            return_sequence=False, dtype=dt, ignore_length=ignore_length)
        hist = final[:, None, :]
    if stats is not None:
        stats.extend(np.abs(final[lengths > 0]).reshape(-1))
    deep = np.concatenate([np.concatenate(dnn_emb, axis=-1), hist], axis=-1)                                     # :201-203
    dnn_in = _combined_dnn_input([deep.reshape(deep.shape[0], 1, -1)], dense)
    out = _dnn(main_dnn, dnn_in, weights, dt, dnn_activation, use_bn, bn_first=len(dice) if dice else 0)
    logit = out @ weights["dense/kernel"].astype(dt)
    pred = R.prediction_layer(logit, weights["prediction_layer/global_bias"].astype(dt), task)
    return (pred, aux) if want_aux else pred


def run_fixture(g, dtype=np.float64, task=None, **kw):
    """The oracle over a tests/golden/model_dien_*.npz fixture (task='regression': the logit)."""
    import json
    from tests.spec import columns_from_spec
    meta = json.loads(bytes(g["meta"]).decode())
    feed = {k[5:]: v for k, v in g.items() if k.startswith("feed/")}
    weights = {k[2:]: v for k, v in g.items() if k.startswith("w/")}
    args = dict(meta["kwargs"])
    if task is not None:
        args["task"] = task
    args.update(kw)
    return dien(columns_from_spec(meta["dnn"]), meta["extra_args"][0], weights, feed, dtype=dtype, **args)
