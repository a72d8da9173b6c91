"""NumPy oracle of DSIN (reference deepctr/models/sequence/dsin.py:26-167), BiLSTM (layers/sequence.py:318-428) over keras' LSTM as
documented, and BiasEncoding (:706-757), float64 or float32.  Written from the equations, independently of the torch restatement, of
the fixture script and of the kernel:
    z = x_t W + h U + b, gate order i | f | c~ | o;  i, f, o = sigma(.), g = tanh(.);  c' = f c + i g;  h' = o tanh(c');  h_0 = c_0 = 0
    two independent stacks: forward t = 0 .. T-1, backward t = T-1 .. 0 with each layer's output back in time order before the next;
    layer l >= layers - res_layers adds its input; the stacks meet in the merge only.  No mask: every step runs.
The model stands on the shared oracle helpers (embedding tables, hashing, the attention pooling layer, DNN) and on the Transformer of
tests/ref_bst.py."""
import numpy as np

from oracle import ref_numpy as R
from oracle.ref_models import _combined_dnn_input, _dnn, _feed, _is_dense, _is_sparse, _lookup_idx
from tests.ref_bst import transformer
from tests.ref_dien import sequence_mask, sigmoid

MERGE_MODES = ("fw", "bw", "sum", "mul", "ave", "concat", None)


def hard_sigmoid(x):
    return np.clip(0.2 * x + 0.5, 0, 1)


def lstm(x, w, u, b, go_backwards=False, recurrent_activation="sigmoid", gate_order=(0, 1, 2, 3), stats=None):
    """One LSTM with return_sequences: x [B,T,D] -> [B,T,n] in TIME order (a backward layer's rows are put back).  ``gate_order``: the
    quarters read as (i, f, c~, o) — a permutation is what the fixture conditions compare against; ``stats``: a list that receives
    the |pre-activation| entries."""
    B, T, _ = x.shape
    n = u.shape[0]
    sig = sigmoid if recurrent_activation == "sigmoid" else hard_sigmoid
    h, c = np.zeros((B, n), x.dtype), np.zeros((B, n), x.dtype)
    out = np.zeros((B, T, n), x.dtype)
    qi, qf, qc, qo = gate_order
    for t in (range(T - 1, -1, -1) if go_backwards else range(T)):
        z = x[:, t] @ w + h @ u + b
        if stats is not None:
            stats.extend(np.abs(z).reshape(-1))
        i, f, o = sig(z[:, qi * n:(qi + 1) * n]), sig(z[:, qf * n:(qf + 1) * n]), sig(z[:, qo * n:(qo + 1) * n])
        c = f * c + i * np.tanh(z[:, qc * n:(qc + 1) * n])
        h = o * np.tanh(c)
        out[:, t] = h
    return out


def bilstm(x, layers, res_layers=0, merge_mode="ave", recurrent_activation="sigmoid", dtype=np.float64, gate_order=(0, 1, 2, 3),
           reverse_back=True, stats=None):
    """x [B,T,Din]; layers [(fw W, fw U, fw b, bw W, bw U, bw b)].  ``reverse_back`` False leaves every backward layer's output in
    the order it was produced (the dropped reversal the fixture conditions compare against)."""
    dt = np.dtype(dtype).type
    fw = bw = np.asarray(x).astype(dt)
    L = len(layers)
    for li, layer in enumerate(layers):
        wf, uf, bf, wb, ub, bb = (np.asarray(v).astype(dt) for v in layer)
        of = lstm(fw, wf, uf, bf, False, recurrent_activation, gate_order, stats)
        ob = lstm(bw, wb, ub, bb, True, recurrent_activation, gate_order, stats)
        if not reverse_back:
            ob = ob[:, ::-1]
        if li >= L - res_layers:
            of, ob = of + fw, ob + bw
        fw, bw = of, ob
    if merge_mode == "fw":
        return fw
    if merge_mode == "bw":
        return bw
    if merge_mode == "concat":
        return np.concatenate([fw, bw], axis=-1)
    if merge_mode == "sum":
        return fw + bw
    if merge_mode == "ave":
        return (fw + bw) / 2
    if merge_mode == "mul":
        return fw * bw
    assert merge_mode is None
    return fw, bw


def bias_encoding(x, sess_bias, seq_bias, item_bias):
    """x [B,S,T,E] + item_bias[e] + seq_bias[t] + sess_bias[s]."""
    x = np.asarray(x)
    S, T, E = x.shape[1:]
    dt = x.dtype
    return (x + np.asarray(item_bias).astype(dt).reshape(1, 1, 1, E) + np.asarray(seq_bias).astype(dt).reshape(1, 1, T, 1)
            + np.asarray(sess_bias).astype(dt).reshape(1, S, 1, 1))


def _sfx(base, k):
    return base if k == 0 else "%s_%d" % (base, k)


def lstm_layers(weights, n_layers, dt, first=0):
    """keras builds fw then bw per layer (sequence.py:364-370): lstm, lstm_1 the first layer's pair, lstm_2, lstm_3 the second's."""
    out = []
    for i in range(n_layers):
        f, b = _sfx("lstm", first + 2 * i), _sfx("lstm", first + 2 * i + 1)
        out.append(tuple(weights["%s/%s" % (n, k)].astype(dt) for n in (f, b) for k in ("kernel", "recurrent_kernel", "bias")))
    return out


def dsin(dnn_cols, sess_feature_list, weights, feed, sess_max_count=5, bias_encoding=False, att_embedding_size=1, att_head_num=8,
         dnn_hidden_units=(256, 128, 64), dnn_activation="relu", dnn_use_bn=False, task="binary", dtype=np.float64,
         gate_order=(0, 1, 2, 3), reverse_back=True, ignore_sess_length=False, empty_session_zero=False, stats=None, **_):
    """The model.  The last four switches are the perturbations the fixture conditions measure."""
    dt = np.dtype(dtype).type
    S = int(sess_max_count)
    sparse = [fc for fc in dnn_cols if _is_sparse(fc)]
    table = {fc.embedding_name: "sparse_emb_%d-%s" % (i, fc.name) for i, fc in enumerate(sparse)}                  # dsin.py:89-96
    sess_cols = [fc for fc in sparse if fc.name in sess_feature_list]

    def emb_of(fc, name=None):
        idx = _lookup_idx(fc if name is None else fc._replace(name=name), feed, mask_zero=fc.name in sess_feature_list)
        return R.embedding(weights[table[fc.embedding_name] + "/embeddings"].astype(dt), idx), idx

    query = np.concatenate([emb_of(fc)[0] for fc in sess_cols], axis=-1)                                            # dsin.py:98-99
    dnn_emb = [emb_of(fc)[0] for fc in sparse]                                                                     # :100-101
    dense = [_feed(feed, fc.name).astype(dt) for fc in dnn_cols if _is_dense(fc)]
    sessions, masks = [], []
    for i in range(S):                                                                                             # :149-155
        embs, m = [], None
        for fc in sess_cols:
            e, idx = emb_of(fc, "sess_%d_%s" % (i, fc.name))
            embs.append(e)
            m = (idx != 0) if m is None else (m & (idx != 0))                                                      # Concat.compute_mask: all
        sessions.append(np.concatenate(embs, axis=-1))
        masks.append(m)
    k = np.stack(sessions, axis=1)                                                                                 # [B,S,T,E]
    m = np.stack(masks, axis=1)
    B, _, T, E = k.shape
    if bias_encoding:                                                                                              # :156-157
        k = globals()["bias_encoding"](k, weights["bias_encoding/sess_bias_embedding"], weights["bias_encoding/seq_bias_embedding"],
                                       weights["bias_encoding/item_bias_embedding"])
    tw = {n: weights["transformer/" + n] for n in ("query", "key", "value", "fw1", "fw2")}
    if not bias_encoding:
        tw["pe_q"], tw["pe_k"] = weights["position_encoding/lookup_table"], weights["position_encoding_1/lookup_table"]
    kf, mf = k.reshape(B * S, T, E), m.reshape(B * S, T)
    sess_fea = transformer(kf, kf, tw, att_head_num, mf, mf, not bias_encoding, True, True, False, True, "mean", dtype=dt)   # :111-115
    sess_fea = sess_fea.reshape(B, S, E)
    if empty_session_zero:
        sess_fea = np.where(m.any(axis=2)[:, :, None], sess_fea, 0)
    lens = np.full(B, S) if ignore_sess_length else np.ceil(np.asarray(feed["sess_length"], dtype=np.float64).reshape(-1))
    sm = sequence_mask(lens, S)

    def pool(keys, dnn_name, lau_name):                                                                            # :117-124
        ks, bs, i = [], [], 0
        while "%s/kernel%d" % (dnn_name, i) in weights:
            ks.append(weights["%s/kernel%d" % (dnn_name, i)].astype(dt))
            bs.append(weights["%s/bias%d" % (dnn_name, i)].astype(dt))
            i += 1
        return R.attention_sequence_pooling(query, keys, sm, ks, bs, weights[lau_name + "/kernel"].astype(dt),
                                            weights[lau_name + "/bias"].astype(dt), "sigmoid", None, True)
    interest = pool(sess_fea, "dnn", "local_activation_unit")
    lstm_out = bilstm(sess_fea, lstm_layers(weights, 2, dt), 0, "ave", dtype=dt, gate_order=gate_order, reverse_back=reverse_back,
                      stats=stats)
    lstm_att = pool(lstm_out, "dnn_1", "local_activation_unit_1")
    deep = np.concatenate([np.concatenate(dnn_emb, axis=-1), interest, lstm_att], axis=-1)                         # :126-129
    dnn_in = _combined_dnn_input([deep.reshape(B, 1, -1)], dense)
    out = _dnn("dnn_2", dnn_in, weights, dt, dnn_activation, dnn_use_bn)
    logit = out @ weights["dense/kernel"].astype(dt)
    return R.prediction_layer(logit, weights["prediction_layer/global_bias"].astype(dt), task)


def run_fixture(g, dtype=np.float64, task=None, **kw):
    """The oracle over a tests/golden/model_dsin_*.npz fixture (task='regression': the logit)."""
    import json
    from tests.spec import columns_from_spec
    meta = json.loads(bytes(g["meta"]).decode())
    feed = {k[5:]: v for k, v in g.items() if k.startswith("feed/")}
    weights = {k[2:]: v for k, v in g.items() if k.startswith("w/")}
    args = dict(meta["kwargs"])
    if task is not None:
        args["task"] = task
    args.update(kw)
    return dsin(columns_from_spec(meta["dnn"]), meta["extra_args"][0], weights, feed, dtype=dtype, **args)
