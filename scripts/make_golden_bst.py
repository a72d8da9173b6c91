"""Generates the BST fixtures tests/golden/model_bst_*.npz and transformer_layer.npz by running the reference's own BST and Transformer
(deepctr/models/sequence/bst.py, layers/sequence.py:431-703, layers/normalization.py) on the oracle's TensorFlow shim, with the oracle's
deterministic weights (oracle/make_golden.py).  CPU only; needs the reference checkout, so it is not part of the suite:

    python scripts/make_golden_bst.py [--out DIR]

Run it into a scratch directory and compare with the committed files to check that the recipe has not rotted (a second run gives the
same bytes).

The shim lacks a few symbols this code path touches.  Installed here, after the shim, RESTATED FROM THE TENSORFLOW / KERAS DOCUMENTATION
and not taken from their code (the precedent of ``install_restated_symbols`` in scripts/make_golden_edcn.py):
``tf.equal`` (elementwise ==), ``tf.shape`` (the dimensions of a tensor), ``tf.range(n)`` (0 .. n-1, int32), ``tf.nn.embedding_lookup``
(rows of ``params`` at ``ids``), ``tf.matrix_set_diag`` (a copy of the input whose main diagonal of the last two axes is replaced),
and the ``keras.backend`` forms ``mean(x, axis, keepdims)``, ``square`` and ``sqrt``.

Weights: the oracle's hook, except that a PositionEncoding table is its sinusoid initial value plus N(0, 0.1) noise drawn per layer
name: query_pe != key_pe (at the initial values, swapping the two tables is invisible).  The hook already draws gamma = 1 + 0.2 N and
beta = 0.1 N for the LayerNormalization, so dropping the affine is visible too.

Model fixtures (B = 32, T = 6; item width 8, cate width 4 -> E = 12): base (two history features, transformer_num 1, att_head_num 2),
transformer_num 2, att_head_num 1, hashed columns, use_bn, regression, one history feature only (E = 8), and a spec with an extra
mean-pooled sequence and a DenseFeat.  seq_length holds 0, 1, T and T + 3 in its first four rows.
Layer fixtures (transformer_layer.npz; B = 6, T = 5, E = 8, H = 2): all flags on, each flag off in turn, blinding, output_type mean and
sum, supports_masking=True with explicit masks, and a cross form (queries != keys, their own lengths).

Conditions, printed by this script and asserted by tests/test_bst_cpu.py: binary probabilities inside (1e-3, 1 - 1e-3); rows kept
under tests.test_autoint_cpu.att_rows >= half (these specs have no max-pooled sequence: all rows); every row that enters a
LayerNormalization has variance >= 1e-3 x its mean square (the float64 oracle's statistics over the same inputs):

    model_bst_base             32/32  0.253 .. 0.567   min var/ms 0.297
    model_bst_t2               32/32  0.353 .. 0.530   min var/ms 0.297
    model_bst_h1               32/32  0.253 .. 0.567   min var/ms 0.298
    model_bst_hash             32/32  0.267 .. 0.557   min var/ms 0.327
    model_bst_bn               32/32  0.307 .. 0.532   min var/ms 0.297
    model_bst_regression       32/32  (logits)         min var/ms 0.297
    model_bst_one              32/32  0.380 .. 0.569   min var/ms 0.283
    model_bst_extra            32/32  0.297 .. 0.568   min var/ms 0.315
    transformer_layer          10 cases        min var/ms 0.196

(an all-zero row — no residual and a zero query mask — normalises to beta whatever eps is and is left out of the minimum)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import make_golden as G  # noqa: E402
from oracle import tf_shim as S  # noqa: E402

SEED = 61
T = 6


def install_restated_symbols():
    tf = sys.modules["tensorflow"]
    arr = lambda x: np.asarray(S._arr(x))   # noqa: E731

    def matrix_set_diag(x, diagonal, name=None):
        out = arr(x).copy()
        i = np.arange(min(out.shape[-2:]))
        out[..., i, i] = arr(diagonal)[..., :i.size]
        return S.Tensor(out)

    tf.equal = lambda x, y: S.Tensor(np.equal(arr(x), arr(y)))
    tf.shape = lambda x: tuple(int(v) for v in arr(x).shape)
    tf.range = lambda n: S.Tensor(np.arange(int(n), dtype=np.int32))
    tf.matrix_set_diag = matrix_set_diag
    sys.modules["tensorflow.nn"].embedding_lookup = lambda params, ids: S.Tensor(arr(params)[arr(ids)])
    K = sys.modules["tensorflow.keras.backend"]
    K.mean = lambda x, axis=None, keepdims=False: S.Tensor(np.mean(arr(x), axis=axis, keepdims=keepdims))
    K.square = lambda x: S.Tensor(np.square(arr(x)))
    K.sqrt = lambda x: S.Tensor(np.sqrt(arr(x)))


def weight_hook(layer, wname, default):
    if str(wname) == "lookup_table":
        rng = np.random.RandomState(G._seed(layer.name, str(wname), "bst"))
        return default + 0.1 * rng.standard_normal(default.shape)
    return G.weight_hook(layer, wname, default)


def bst_spec(hash_flag=False, one=False, extra=False, item_v=40, cate_v=9, Eu=6, Ei=8, Ec=4):
    sp = lambda n, v, e, **kw: dict(type="sparse", name=n, vocabulary_size=v, embedding_dim=e, use_hash=hash_flag, **kw)   # noqa: E731
    spec = [sp("user", 5, Eu), sp("item_id", item_v, Ei), sp("cate_id", cate_v, Ec),
            dict(type="varlen", sparsefeat=sp("hist_item_id", item_v, Ei, embedding_name="item_id"), maxlen=T, length_name="seq_length")]
    if not one:
        spec.append(dict(type="varlen", sparsefeat=sp("hist_cate_id", cate_v, Ec, embedding_name="cate_id"), maxlen=T,
                         length_name="seq_length"))
    if extra:
        spec.append(dict(type="varlen", sparsefeat=sp("other_seq", 11, 6), maxlen=4, combiner="mean"))
        spec.append(dict(type="dense", name="pay_score", dimension=1))
    return spec


def feed_for(spec, B, rng):
    feed = G._feed_for(spec, B, rng)
    lens = rng.randint(0, T + 1, size=B).astype(np.int32)
    lens[:4] = (T, 0, 1, T + 3)
    feed["seq_length"] = lens
    for d in spec:
        if d["type"] == "varlen" and d.get("length_name") == "seq_length":
            name = d["sparsefeat"]["name"]
            hi = 10 ** 6 if d["sparsefeat"].get("use_hash") else d["sparsefeat"]["vocabulary_size"]
            ids = rng.randint(1, hi, size=(B, T)).astype(np.int32)
            ids[np.arange(T)[None, :] >= lens[:, None]] = 0          # zero-padded tail: still looked up (row 0), still in the block
            feed[name] = ids
    for name in ("item_id", "cate_id"):                             # candidate ids >= 1, like the reference's fixture
        hi = 10 ** 6 if spec[1].get("use_hash") else next(d for d in spec if d.get("name") == name)["vocabulary_size"]
        feed[name] = rng.randint(1, hi, size=B).astype(np.int32)
    return feed


def run_model(name, spec, hist, feed, kwargs):
    from deepctr.models.sequence.bst import BST
    S.reset()
    S.set_feed(feed)
    model = BST(G.build_ref_columns(spec), hist, **kwargs)
    y = model.predict()
    arrays = {"y": y.astype(np.float32)}
    for k, v in feed.items():
        arrays["feed/" + k] = v
    for k, v in G._weights_dict().items():
        arrays["w/" + k] = v
    meta = {"model": "BST", "linear": [], "dnn": spec, "kwargs": kwargs, "extra_args": [list(hist)]}
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    G._save(name, **arrays)


def gen_models():
    rng = np.random.RandomState(SEED)
    B = 32
    spec = bst_spec()
    feed = feed_for(spec, B, rng)
    spec_h = bst_spec(hash_flag=True)
    feed_h = feed_for(spec_h, B, rng)
    spec_1 = bst_spec(one=True)
    feed_1 = feed_for(spec_1, B, rng)
    spec_x = bst_spec(extra=True)
    feed_x = feed_for(spec_x, B, rng)
    both = ["item_id", "cate_id"]
    base = {"transformer_num": 1, "att_head_num": 2, "dnn_hidden_units": [16, 8]}
    runs = [("base", spec, both, feed, {}), ("t2", spec, both, feed, {"transformer_num": 2}), ("h1", spec, both, feed, {"att_head_num": 1}),
            ("hash", spec_h, both, feed_h, {}), ("bn", spec, both, feed, {"use_bn": True}),
            ("regression", spec, both, feed, {"task": "regression"}), ("one", spec_1, ["item_id"], feed_1, {}),
            ("extra", spec_x, both, feed_x, {})]
    names = []
    for suffix, sp, hist, fd, kw in runs:
        run_model("model_bst_" + suffix, sp, hist, fd, dict(base, **kw))
        names.append("model_bst_" + suffix)
    return names


LAYER_CASES = [  # tag, constructor kwargs on top of the all-on configuration, form
    ("all", {}, "lengths"), ("nope", {"use_positional_encoding": False}, "lengths"), ("nores", {"use_res": False}, "lengths"),
    ("noffn", {"use_feed_forward": False}, "lengths"), ("noln", {"use_layer_norm": False}, "lengths"),
    ("blind", {"blinding": True}, "lengths"), ("mean", {"output_type": "mean"}, "lengths"), ("sum", {"output_type": "sum"}, "lengths"),
    ("masking", {"supports_masking": True}, "masks"), ("cross", {}, "cross"),
]


def gen_layers():
    from deepctr.layers.sequence import Transformer
    rng = np.random.RandomState(SEED + 1)
    B, Tl, E, H = 6, 5, 8, 2
    arrays = {}
    for tag, kw, form in LAYER_CASES:
        S.reset()
        cfg = dict(att_embedding_size=E // H, head_num=H, dropout_rate=0.0, use_positional_encoding=True, use_res=True,
                   use_feed_forward=True, use_layer_norm=True, blinding=False, seed=1024, supports_masking=False, output_type=None)
        cfg.update(kw)
        q = rng.standard_normal((B, Tl, E)).astype(np.float32)
        k = rng.standard_normal((B, Tl, E)).astype(np.float32) if form == "cross" else q
        ql = np.array([0, 1, Tl, Tl + 3, 2, 4], dtype=np.int32)
        kl = np.array([Tl, 0, 3, 1, Tl + 3, 2], dtype=np.int32) if form == "cross" else ql
        layer = Transformer(**cfg)
        if form == "masks":
            qm = rng.rand(B, Tl) < 0.6
            km = rng.rand(B, Tl) < 0.6
            qm[0], km[1] = False, False           # a sample without queries, one without keys
            y = layer([G.T(q), G.T(k)], mask=[G.T(qm), G.T(km)])
            arrays.update({tag + "/query_mask": qm, tag + "/key_mask": km})
        else:
            y = layer([G.T(q), G.T(k), G.T(ql[:, None]), G.T(kl[:, None])])
            arrays.update({tag + "/query_lengths": ql, tag + "/key_lengths": kl})
        arrays.update({tag + "/queries": q, tag + "/keys": k, tag + "/y": np.asarray(y.a, dtype=np.float32),
                       tag + "/cfg": np.frombuffer(json.dumps(cfg).encode(), dtype=np.uint8)})
        for name, v in G._weights_dict().items():
            arrays["%s/w/%s" % (tag, name)] = v
    G._save("transformer_layer", **arrays)


def report(name):
    """Rows kept, probability range and the smallest LayerNorm variance / mean-square of a written fixture, by the tests' rules."""
    from tests import ref_bst as RB
    from tests.test_autoint_cpu import att_rows
    g = dict(np.load(os.path.join(G.OUT, name + ".npz")))
    meta = json.loads(bytes(g["meta"]).decode())
    feed = {k[5:]: v for k, v in g.items() if k.startswith("feed/")}
    keep = att_rows(meta, feed, g["y"].shape[0])
    stats = []
    ref = RB.run_fixture(g, np.float64, stats=stats)
    y = g["y"].reshape(-1)[keep]
    assert np.abs(ref.reshape(-1) - g["y"].reshape(-1)).max() < 1e-5
    rng = "(logits)      " if meta["kwargs"].get("task") == "regression" else "%.3f .. %.3f" % (y.min(), y.max())
    print("    %-26s %d/%d  %s   min var/ms %.3f" % (name, keep.sum(), keep.size, rng, min(stats)))


def report_layers():
    """The smallest LayerNorm variance / mean-square over the layer fixtures (all-zero rows, which normalise to beta, aside)."""
    from tests import ref_bst as RB
    from tests.test_bst_cpu import layer_case, layer_flags
    g = dict(np.load(os.path.join(G.OUT, "transformer_layer.npz")))
    stats = []
    for tag, _, _ in LAYER_CASES:
        cfg, q, k, qm, km, w, _, _ = layer_case(g, tag)
        RB.transformer(q, k, w, cfg["head_num"], qm, km, stats=stats, **layer_flags(cfg))
    print("    %-26s %d cases        min var/ms %.3f" % ("transformer_layer", len(LAYER_CASES), min(stats)))


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if "--out" in argv:
        i = argv.index("--out")
        G.OUT = os.path.abspath(argv[i + 1])
        del argv[i:i + 2]
    S.install(G.REF)
    S.WEIGHT_HOOK = weight_hook
    install_restated_symbols()
    names = gen_models()
    gen_layers()
    for name in names:
        report(name)
    report_layers()


if __name__ == "__main__":
    sys.exit(main())
