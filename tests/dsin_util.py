"""What the DSIN tests share: fixture names and readers, weight and problem generators, the oracle in the op tests' output form."""
import numpy as np
import torch

from tests import ref_dsin as RS
from tests.spec import columns_from_spec

DSIN_FIXTURES = ["model_dsin_pe", "model_dsin_bias", "model_dsin_hash", "model_dsin_bn", "model_dsin_regression", "model_dsin_one",
                 "model_dsin_extra", "model_dsin_head1"]
BILSTM_TAGS = ["ave", "fw", "bw", "sum", "mul", "concat", "none", "l1_res1", "l2_res1", "l3_res3", "l3_res0", "din"]


def make_layers(rng, Din, u, L):
    """Kernels at a scale that keeps the gates off saturation, biases away from their initial ones."""
    out = []
    for li in range(L):
        D = Din if li == 0 else u
        layer = ()
        for _ in range(2):
            layer += ((rng.standard_normal((D, 4 * u)) * 0.7 / np.sqrt(D)).astype(np.float32),
                      (rng.standard_normal((u, 4 * u)) * 0.7 / np.sqrt(u)).astype(np.float32),
                      (1 + 0.5 * rng.standard_normal(4 * u)).astype(np.float32))
        out.append(layer)
    return out


def to_dev(layers, device):
    return [tuple(torch.from_numpy(w).to(device) for w in layer) for layer in layers]


def oracle(x, layers, res, mm, act):
    ref = RS.bilstm(x, layers, res, mm, act)
    return np.stack(ref, axis=1) if mm is None else ref


def build_dsin(meta, device):
    from deepctr_amd.models import DSIN
    return DSIN(columns_from_spec(meta["dnn"]), meta["extra_args"][0], device=device, **meta["kwargs"])


def fixture_feed(g):
    return {k[5:]: v for k, v in g.items() if k.startswith("feed/")}


def fixture_weights(g):
    return {k[2:]: v for k, v in g.items() if k.startswith("w/")}


def bilstm_case(g, tag):
    """(cfg, x, per layer (fw W, fw U, fw b, bw W, bw U, bw b), y) of a bilstm_layer.npz case; y of merge_mode None is stacked on axis 1."""
    import json
    cfg = json.loads(bytes(g[tag + "/cfg"]).decode())
    prefix = "w%d/" % cfg["in_dim"]                 # the cases of one input width share their weights
    named = {n[len(prefix):]: v for n, v in g.items() if n.startswith(prefix)}
    return cfg, g[tag + "/x"], RS.lstm_layers(named, cfg["layers"], np.float32), g[tag + "/y"]


def bias_encoding_case(g, tag):
    """(S, the S inputs [B,T,E], (sess, seq, item) biases, the S outputs) of a bias_encoding_layer.npz case."""
    x, y = g[tag + "/x"], g[tag + "/y"]
    ws = tuple(g["%s/w/bias_encoding/%s_bias_embedding" % (tag, k)] for k in ("sess", "seq", "item"))
    return x.shape[1], [x[:, i] for i in range(x.shape[1])], ws, [y[:, i] for i in range(y.shape[1])]


def dsin_problem(rng, n, feats=(("item", 8), ("cate", 4)), S=3, T=4, hash_=False, extra=False, vocab=30):
    """Columns, the session feature list and a feed with a sample whose sessions are all full (row 0), a sample of sess_length 0
    (row 1) and, from four rows on, a sample of full sess_length whose sessions are all empty (row 3); the other rows draw both."""
    from deepctr_amd.feature_column import DenseFeat, SparseFeat, VarLenSparseFeat
    cols = [SparseFeat("user", 7, 4, use_hash=hash_)] + [SparseFeat(nm, vocab, w, use_hash=hash_) for nm, w in feats]
    hi = 10 ** 6 if hash_ else vocab
    feed = {"user": rng.randint(0, 10 ** 6 if hash_ else 7, n).astype(np.int32)}
    sess_len = rng.randint(0, S + 1, n).astype(np.int32)
    sess_len[:min(n, 4)] = np.array([S, 0, 1, S])[:min(n, 4)]
    feed["sess_length"] = sess_len
    fill = rng.randint(0, T + 1, (n, S))
    fill[0] = T                                     # every session full
    if n > 3:
        fill[3] = 0                                 # every session empty
    fill[np.arange(S)[None, :] >= sess_len[:, None]] = 0
    for nm, w in feats:
        feed[nm] = rng.randint(1, hi, n).astype(np.int32)
        for i in range(S):
            ids = rng.randint(1, hi, (n, T)).astype(np.int32)
            ids[np.arange(T)[None, :] >= fill[:, i:i + 1]] = 0
            if nm != feats[0][0]:
                ids[rng.rand(n, T) < 0.1] = 0       # one feature's id missing: the position is masked (Concat.compute_mask: all)
            feed["sess_%d_%s" % (i, nm)] = ids
            cols.append(VarLenSparseFeat(SparseFeat("sess_%d_%s" % (i, nm), vocab, w, embedding_name=nm, use_hash=hash_), T))
    if extra:
        cols.append(VarLenSparseFeat(SparseFeat("other_seq", 11, 6), 4, combiner="mean"))
        feed["other_seq"] = rng.randint(0, 11, (n, 4)).astype(np.int32)
        cols.append(DenseFeat("pay_score", 1))
        feed["pay_score"] = rng.rand(n).astype(np.float32)
    return cols, [nm for nm, _ in feats], feed


def randomise(model, rng):
    """Trained-like weights: embeddings of order 0.3 so that the gates move, LSTM biases away from one, bias encodings of order 0.1."""
    new = {}
    for k, v in model.get_weights_by_name().items():
        draw = rng.standard_normal(v.shape)
        if k.endswith("embeddings"):
            a = 0.3 * draw
        elif k.startswith("lstm") and k.endswith("bias"):
            a = 1.0 + 0.5 * draw
        elif k.endswith("moving_variance"):
            a = rng.uniform(0.5, 1.5, v.shape)
        elif k.endswith("lookup_table"):
            a = v + 0.05 * draw
        elif "bias" in k or k.endswith("beta") or k.endswith("moving_mean"):
            a = 0.1 * draw
        elif k.endswith("gamma"):
            a = 1.0 + 0.2 * draw
        else:
            a = draw * (v.std() if v.std() > 0 else 0.1)
        new[k] = a.astype(np.float32)
    model.set_weights_by_name(new)
    return new
