"""Generates the DSIN fixtures tests/golden/model_dsin_*.npz, bilstm_layer.npz and bias_encoding_layer.npz on the oracle's TensorFlow shim,
with the oracle's deterministic weights (oracle/make_golden.py).  CPU only; needs the reference checkout, so it is not part of the suite:

    python scripts/make_golden_dsin.py [--out DIR]

Run it into a scratch directory and compare with the committed files to check that the recipe has not rotted (a second run gives the
same bytes).

WHAT IS THE REFERENCE'S CODE HERE, imported in place from the checkout and never copied: ``DSIN``, ``sess_interest_division`` and
``sess_interest_extractor`` (deepctr/models/sequence/dsin.py), ``BiLSTM``, ``BiasEncoding``, ``Transformer``, ``PositionEncoding`` and
``AttentionSequencePoolingLayer`` (layers/sequence.py), ``DNN``, ``LocalActivationUnit``, the embedding plumbing and ``Concat`` with its
mask rule.

WHAT IS RESTATED, from the TensorFlow / keras documentation and not from their code, installed after the shim:
  * the symbols the Transformer touches, as scripts/make_golden_bst.py installs them;
  * ``tf.keras.layers.LSTM`` as documented: ``kernel`` [D, 4u], ``recurrent_kernel`` [u, 4u], ``bias`` [4u] in the gate order
    i | f | c~ | o; z = x_t W + h U + b, i, f, o = sigmoid, g = tanh, c' = f c + i g, h' = o tanh(c'), h_0 = c_0 = 0;
    ``go_backwards`` walks the steps from the last to the first and, with ``return_sequences``, hands the rows back in the order they
    were produced; ``bias_initializer`` ('ones' here; with 'zeros', ``unit_forget_bias`` sets the f quarter to one); kernel
    glorot_uniform, recurrent kernel orthogonal; ``dropout`` is inactive at inference; no mask reaches the layer in DSIN;
  * ``keras.backend.reverse(x, axes)``;
  * keras' mask propagation for a layer that returns a list: element i of the output carries element i of ``compute_mask``'s list
    (the shim attaches masks to single tensors only; BiasEncoding returns one tensor per session).
So the stacking, the reversal, the residuals, the merge, the bias encoding, the session wiring and the masks carry the reference's
authority; the cell carries the documentation's, and tests/ref_dsin.py, written from the equations, is its independent check: this
script asserts agreement with it to 1e-5 before it writes anything.

Weights: the oracle's hook, except the LSTMs (kernels 0.4 N, those over the Transformer's outputs 0.2 N, biases 1 + 1.5 N: a wrong gate order or a dropped bias is visible), the BiasEncoding
weights (0.1 N instead of the 1e-4 N of their initialiser) and the PositionEncoding tables (0.1 x sinusoid + 0.05 N per layer name: at the initial
scale, sqrt(E) x the sinusoid against embeddings of 0.3 N, every session interest is nearly the same vector and nothing behind the
Transformer moves the logits).

Model fixtures (B = 32, S = 3, T = 4; item width 8, cate width 4 -> E = 12 = 2 heads x 6): position encoding, bias_encoding, hashed
columns, dnn_use_bn, regression, sess_max_count = 1 (one feature, E = 8), an extra SparseFeat, an unused sequence column and a
DenseFeat, and att_head_num = 1.  Every feed has a sample with every session full (row 0), a sample with sess_length 0 (row 1), an
empty session inside sess_length (row 2) and a sample whose sessions are all empty (row 3).
Layer fixtures: bilstm_layer.npz (B = 6, T = 5, u = 4): every merge_mode, res_layers 0 / 1 / layers, layers 1 - 3, Din = 7 != u (the
weights of an input width stored once for all its cases);
bias_encoding_layer.npz: three sessions and two.

Conditions, asserted by this script and by tests/test_dsin_cpu.py from the float64 oracle alone: swapping any two gate quarters,
dropping the reversal of the backward stack, ignoring sess_length (both where S > 1: one session has nothing to reverse and pools to
itself at any length) and treating an empty session as zeros each move the logits
by >= 100 x 1e-4 of their largest; >= 90 % of the LSTM gate pre-activations have |z| < 4 (sigmoid(4) = 0.982).  The figures of the
committed files are in REPORT below; a run that gives others says so."""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import make_golden as G  # noqa: E402
from oracle import tf_shim as S  # noqa: E402

SEED = 81
S_MAX, T = 3, 4
SWAPS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
REPORT = """    model_dsin_pe              0.315 .. 0.592   moved x tol: gates 673  reversal 427  sess_length 1043  empty 1420   |z| < 4: 0.982
    model_dsin_bias            0.250 .. 0.569   moved x tol: gates 364  reversal 304  sess_length 1056  empty 2809   |z| < 4: 0.981
    model_dsin_hash            0.308 .. 0.568   moved x tol: gates 557  reversal 590  sess_length 1768  empty 1905   |z| < 4: 0.982
    model_dsin_bn              0.263 .. 0.552   moved x tol: gates 414  reversal 363  sess_length 1164  empty 3216   |z| < 4: 0.981
    model_dsin_regression      (logits)         moved x tol: gates 673  reversal 427  sess_length 1043  empty 1420   |z| < 4: 0.982
    model_dsin_one             0.344 .. 0.571   moved x tol: gates 400  reversal   -  sess_length    -  empty 3100   |z| < 4: 0.974
    model_dsin_extra           0.357 .. 0.564   moved x tol: gates 336  reversal 619  sess_length 1378  empty 4267   |z| < 4: 0.981
    model_dsin_head1           0.315 .. 0.592   moved x tol: gates 673  reversal 427  sess_length 1043  empty 1420   |z| < 4: 0.982
"""


def arr(x):
    return np.asarray(S._arr(x))


class Orthogonal(object):
    """keras' Orthogonal initialiser as documented: Q of the QR decomposition of a normal matrix (replaced by the weight hook)."""

    def __call__(self, shape, dtype=None):
        rng = np.random.RandomState(SEED)
        a = rng.standard_normal((max(shape), min(shape)))
        q, r = np.linalg.qr(a)
        q = q * np.sign(np.diag(r))
        return (q if shape[0] >= shape[1] else q.T).astype(np.float32)


class LSTM(S.Layer):
    """tf.keras.layers.LSTM as documented (see the module docstring)."""

    def __init__(self, units, dropout=0.0, bias_initializer="zeros", unit_forget_bias=True, return_sequences=False, go_backwards=False,
                 unroll=False, **kw):
        super(LSTM, self).__init__(**kw)
        self.units, self.bias_initializer, self.unit_forget_bias = int(units), bias_initializer, unit_forget_bias
        self.return_sequences, self.go_backwards = return_sequences, go_backwards

    def build(self, input_shape):
        n = self.units
        self.kernel = self.add_weight("kernel", (int(input_shape[-1]), 4 * n), initializer=S.glorot_uniform())
        self.recurrent_kernel = self.add_weight("recurrent_kernel", (n, 4 * n), initializer=Orthogonal())
        bias = np.ones(4 * n) if self.bias_initializer == "ones" else np.zeros(4 * n)
        if self.bias_initializer == "zeros" and self.unit_forget_bias:
            bias[n:2 * n] = 1.0
        self.bias = self.add_weight("bias", (4 * n,), initializer=S.Constant(bias))

    def call(self, inputs, **kw):
        x = arr(inputs).astype(np.float32)
        w, u, b = arr(self.kernel), arr(self.recurrent_kernel), arr(self.bias)
        B, steps, _ = x.shape
        n = self.units
        h, c = np.zeros((B, n), np.float32), np.zeros((B, n), np.float32)
        rows = []
        for t in (range(steps - 1, -1, -1) if self.go_backwards else range(steps)):
            z = x[:, t] @ w + h @ u + b
            i, f, o = (arr(S.sigmoid(S.Tensor(z[:, q * n:(q + 1) * n]))) for q in (0, 1, 3))
            c = (f * c + i * np.tanh(z[:, 2 * n:3 * n])).astype(np.float32)
            h = (o * np.tanh(c)).astype(np.float32)
            rows.append(h)
        return S.Tensor(np.stack(rows, axis=1) if self.return_sequences else h)


def install_restated_symbols():
    import make_golden_bst as GB
    GB.install_restated_symbols()
    K = sys.modules["tensorflow.keras.backend"]
    K.reverse = lambda x, axes: S.Tensor(np.flip(arr(x), axis=axes).copy())
    sys.modules["tensorflow.keras.layers"].LSTM = LSTM
    seq = importlib.import_module("deepctr.layers.sequence")
    seq.LSTM = LSTM

    def call_with_list_masks(self, inputs, *a, **kw):
        out = S.Layer.__call__(self, inputs, *a, **kw)
        masks = self.compute_mask(inputs, S._mask_of(inputs))
        if isinstance(out, list) and isinstance(masks, list):
            for o, m in zip(out, masks):
                if m is not None:
                    o._keras_mask = m
        return out
    seq.BiasEncoding.__call__ = call_with_list_masks


def weight_hook(layer, wname, default):
    w = str(wname)
    rng = np.random.RandomState(G._seed(layer.name, w, "dsin"))
    if isinstance(layer, LSTM):
        if w == "bias":
            return default + 1.5 * rng.standard_normal(default.shape)
        first = layer.name in ("lstm", "lstm_1") and w == "kernel"        # the kernels that meet the Transformer's (larger) outputs
        return (0.2 if first else 0.4) * rng.standard_normal(default.shape)
    if type(layer).__name__ == "BiasEncoding":
        return 0.1 * rng.standard_normal(default.shape)
    if w == "lookup_table":
        return 0.1 * default + 0.05 * rng.standard_normal(default.shape)
    return G.weight_hook(layer, wname, default)


def dsin_spec(hash_flag=False, one=False, extra=False, sess=S_MAX, item_v=40, cate_v=9, Eu=6, Ei=8, Ec=4):
    sp = lambda n, v, e, **kw: dict(type="sparse", name=n, vocabulary_size=v, embedding_dim=e, use_hash=hash_flag, **kw)   # noqa: E731
    feats = [("item", item_v, Ei)] + ([] if one else [("cate", cate_v, Ec)])
    spec = [sp("user", 5, Eu)] + [sp(n, v, e) for n, v, e in feats]
    if extra:
        spec.append(sp("gender", 3, 4))
    for i in range(sess):
        for n, v, e in feats:
            spec.append(dict(type="varlen", sparsefeat=sp("sess_%d_%s" % (i, n), v, e, embedding_name=n), maxlen=T))
    if extra:
        spec.append(dict(type="varlen", sparsefeat=sp("other_seq", 11, 6), maxlen=4, combiner="mean"))
        spec.append(dict(type="dense", name="pay_score", dimension=1))
    return spec, [n for n, _, _ in feats]


def feed_for(spec, names, sess, B, rng):
    feed = G._feed_for(spec, B, rng)
    sl = rng.randint(0, sess + 1, size=B).astype(np.int32)
    sl[:4] = (sess, 0, sess, min(2, sess))
    feed["sess_length"] = sl
    fill = rng.randint(0, T + 1, size=(B, sess))
    fill[0] = T                                 # every session full
    fill[2, 0] = 0                              # an empty session inside sess_length
    fill[3] = 0                                 # every session empty
    fill[np.arange(sess)[None, :] >= sl[:, None]] = 0
    fill[1] = rng.randint(0, T + 1, size=sess)  # sess_length 0 over sessions that hold ids: the length decides, not the ids
    for d in spec:
        if d["type"] == "varlen" and d["sparsefeat"]["name"].startswith("sess_"):
            sf = d["sparsefeat"]
            i = int(sf["name"].split("_")[1])
            hi = 10 ** 6 if sf.get("use_hash") else sf["vocabulary_size"]
            ids = rng.randint(1, hi, size=(B, T)).astype(np.int32)
            ids[np.arange(T)[None, :] >= fill[:, i:i + 1]] = 0
            if sf["embedding_name"] != names[0]:
                drop = rng.rand(B, T) < 0.1     # one feature's id missing: the position is masked (Concat.compute_mask: all)
                drop[0] = False
                ids[drop] = 0
            feed[sf["name"]] = ids
    for name in names:
        d = next(d for d in spec if d.get("name") == name)
        feed[name] = rng.randint(1, 10 ** 6 if d.get("use_hash") else d["vocabulary_size"], size=B).astype(np.int32)
    return feed


def run_model(name, spec, names, feed, kwargs):
    from deepctr.models.sequence.dsin import DSIN
    from tests import ref_dsin as RS
    S.reset()
    S.set_feed(feed)
    model = DSIN(G.build_ref_columns(spec), names, **kwargs)
    y = model.predict()
    arrays = {"y": y.astype(np.float32)}
    for k, v in feed.items():
        arrays["feed/" + k] = v
    for k, v in G._weights_dict().items():
        arrays["w/" + k] = v
    meta = {"model": "DSIN", "linear": [], "dnn": spec, "kwargs": kwargs, "extra_args": [list(names)]}
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    ref = RS.run_fixture(arrays, np.float64)
    assert np.abs(ref.reshape(-1) - arrays["y"].reshape(-1)).max() < 1e-5, (name, np.abs(ref.reshape(-1) - arrays["y"].reshape(-1)).max())
    line = conditions(name, arrays)
    G._save(name, **arrays)
    return line


def conditions(name, g):
    """The fixture conditions from the float64 oracle alone; returns the report line."""
    from tests import ref_dsin as RS
    meta = json.loads(bytes(g["meta"]).decode())
    stats = []
    base = RS.run_fixture(g, np.float64, task="regression", stats=stats).reshape(-1)
    tol = 1e-4 * np.abs(base).max()

    def moved(**kw):
        return np.abs(RS.run_fixture(g, np.float64, task="regression", **kw).reshape(-1) - base).max() / tol
    gates = min(moved(gate_order=tuple(np.array([0, 1, 2, 3])[[b if q == a else a if q == b else q for q in range(4)]])) for a, b in SWAPS)
    many = meta["kwargs"].get("sess_max_count", 5) > 1
    rev = moved(reverse_back=False) if many else None
    lens, empty = moved(ignore_sess_length=True) if many else None, moved(empty_session_zero=True)
    share = float((np.asarray(stats) < 4).mean())
    for what, v in (("gates", gates), ("reversal", rev), ("sess_length", lens), ("empty", empty)):
        assert v is None or v >= 100, (name, what, v)
    assert share >= 0.9, (name, share)
    y = g["y"].reshape(-1)
    rng = "(logits)      " if meta["kwargs"].get("task") == "regression" else "%.3f .. %.3f" % (y.min(), y.max())
    line = "    %-26s %s   moved x tol: gates %3.0f  reversal %s  sess_length %s  empty %4.0f   |z| < 4: %.3f" % (
        name, rng, gates, "%3.0f" % rev if many else "  -", "%4.0f" % lens if many else "   -", empty, share)
    print(line)
    return line


def gen_models():
    rng = np.random.RandomState(SEED)
    B = 32
    spec, both = dsin_spec()
    feed = feed_for(spec, both, S_MAX, B, rng)
    spec_h, _ = dsin_spec(hash_flag=True)
    feed_h = feed_for(spec_h, both, S_MAX, B, rng)
    spec_1, one = dsin_spec(one=True, sess=1)
    feed_1 = feed_for(spec_1, one, 1, B, rng)
    spec_x, _ = dsin_spec(extra=True)
    feed_x = feed_for(spec_x, both, S_MAX, B, rng)
    base = {"sess_max_count": S_MAX, "att_embedding_size": 6, "att_head_num": 2, "dnn_hidden_units": [16, 8]}
    runs = [("pe", spec, both, feed, {}), ("bias", spec, both, feed, {"bias_encoding": True}), ("hash", spec_h, both, feed_h, {}),
            ("bn", spec, both, feed, {"dnn_use_bn": True, "bias_encoding": True}), ("regression", spec, both, feed, {"task": "regression"}),
            ("one", spec_1, one, feed_1, {"sess_max_count": 1, "att_embedding_size": 4}),
            ("extra", spec_x, both, feed_x, {"bias_encoding": True}), ("head1", spec, both, feed, {"att_embedding_size": 12, "att_head_num": 1})]
    return [run_model("model_dsin_" + suffix, sp, names, fd, dict(base, **kw)) for suffix, sp, names, fd, kw in runs]


BILSTM_CASES = [  # tag, layers, res_layers, merge_mode, Din
    ("ave", 2, 0, "ave", 4), ("fw", 2, 0, "fw", 4), ("bw", 2, 0, "bw", 4), ("sum", 2, 0, "sum", 4), ("mul", 2, 0, "mul", 4),
    ("concat", 2, 0, "concat", 4), ("none", 2, 0, None, 4), ("l1_res1", 1, 1, "ave", 4), ("l2_res1", 2, 1, "ave", 4),
    ("l3_res3", 3, 3, "sum", 4), ("l3_res0", 3, 0, "ave", 4), ("din", 2, 1, "concat", 7),
]


def gen_layers():
    from deepctr.layers.sequence import BiasEncoding, BiLSTM
    from tests import ref_dsin as RS
    rng = np.random.RandomState(SEED + 1)
    B, Tl, u = 6, 5, 4
    arrays = {}
    for tag, L, res, mm, Din in BILSTM_CASES:
        S.reset()
        x = rng.standard_normal((B, Tl, Din)).astype(np.float32)
        y = BiLSTM(u, layers=L, res_layers=res, merge_mode=mm, name="bilstm")(G.T(x))
        y = np.stack([arr(v) for v in y], axis=1) if mm is None else arr(y)
        cfg = dict(units=u, layers=L, res_layers=res, merge_mode=mm, in_dim=Din)
        w = G._weights_dict()
        ref = RS.bilstm(x, RS.lstm_layers(w, L, np.float64), res, mm)
        ref = np.stack(ref, axis=1) if mm is None else ref
        assert np.abs(ref - y).max() < 1e-5, (tag, np.abs(ref - y).max())
        arrays.update({tag + "/x": x, tag + "/y": np.asarray(y, dtype=np.float32),
                       tag + "/cfg": np.frombuffer(json.dumps(cfg).encode(), dtype=np.uint8)})
        # the hook draws a weight from its layer's name and shape: the cases of one input width share theirs, stored once
        for name, v in w.items():
            key = "w%d/%s" % (Din, name)
            assert key not in arrays or np.array_equal(arrays[key], v), key
            arrays[key] = v
    G._save("bilstm_layer", **arrays)
    arrays = {}
    for tag, n in (("sess3", 3), ("sess2", 2)):
        S.reset()
        xs = [rng.standard_normal((B, Tl, u)).astype(np.float32) for _ in range(n)]
        ys = BiasEncoding(n, name="bias_encoding")([G.T(x) for x in xs])
        w = G._weights_dict()
        ref = RS.bias_encoding(np.stack(xs, axis=1).astype(np.float64), w["bias_encoding/sess_bias_embedding"],
                               w["bias_encoding/seq_bias_embedding"], w["bias_encoding/item_bias_embedding"])
        y = np.stack([arr(v) for v in ys], axis=1)
        assert np.abs(ref - y).max() < 1e-5, tag
        arrays.update({tag + "/x": np.stack(xs, axis=1), tag + "/y": y.astype(np.float32)})
        for name, v in w.items():
            arrays["%s/w/%s" % (tag, name)] = v
    G._save("bias_encoding_layer", **arrays)


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if "--out" in argv:
        i = argv.index("--out")
        G.OUT = os.path.abspath(argv[i + 1])
        del argv[i:i + 2]
    S.install(G.REF)
    S.WEIGHT_HOOK = weight_hook
    install_restated_symbols()
    lines = gen_models()
    gen_layers()
    if "\n".join(lines) + "\n" != REPORT:
        print("the report differs from the one in the module docstring")


if __name__ == "__main__":
    sys.exit(main())
