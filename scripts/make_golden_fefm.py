"""Generates the FwFM / DeepFEFM fixtures tests/golden/model_fwfm*.npz, model_fefm*.npz and tests/golden/fwfm_fefm_layer.npz by running
the reference's own FwFM / DeepFEFM / FwFMLayer / FEFMLayer (deepctr/models/fwfm.py, deepfefm.py, layers/interaction.py:1351-1499) on
the oracle's TensorFlow shim, with the oracle's deterministic weights (oracle/make_golden.py).  CPU only; needs the reference checkout,
so it is not part of the suite:

    python scripts/make_golden_fefm.py [--out DIR]

Run it into a scratch directory and compare with the committed files to check that the recipe has not rotted (a second run gives the
same bytes).

The shim lacks three symbols these two layers use.  They are installed here, after the shim and before the first import of
deepctr.layers.interaction, RESTATED FROM TENSORFLOW'S DOCUMENTATION, not taken from TensorFlow's code (the "unpinned
one level down" class):
  * tensorflow.keras.backend.batch_dot(x, y, axes=1) for two 2-D operands: sum(x * y, axis=1, keepdims=True);
  * tf.scalar_mul(scalar, x): scalar * x;
  * tf.add_n(inputs): the elementwise sum, taken left to right in float32.

Feeds: RandomState(31).  With G.mixed_spec(4, False) and B = 16 nine of the sixteen rows carry no all-padding max-pooled sequence
(tests.test_autoint_cpu.att_rows), and the hashed and two-group feeds drawn behind it keep at least half of their rows too (the
tests assert it)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import make_golden as G  # noqa: E402
from oracle import tf_shim as S  # noqa: E402

SEED = 31


def install_restated_symbols():
    import tensorflow as tf
    K = sys.modules["tensorflow.keras.backend"]

    def batch_dot(x, y, axes=None):
        a, b = np.asarray(S._arr(x)), np.asarray(S._arr(y))
        assert axes == 1 and a.ndim == 2 and b.ndim == 2 and a.shape == b.shape, "batch_dot: only two [B, E] operands with axes=1"
        return S.Tensor(np.sum(a * b, axis=1, keepdims=True))

    def scalar_mul(scalar, x, name=None):
        return S.Tensor(np.asarray(S._arr(scalar)) * np.asarray(S._arr(x)))

    def add_n(inputs, name=None):
        arrs = [np.asarray(S._arr(v), dtype=np.float32) for v in inputs]
        assert len(arrs) > 0, "add_n: needs at least one input"
        out = arrs[0]
        for a in arrs[1:]:
            out = out + a
        return S.Tensor(out)

    K.batch_dot = batch_dot
    tf.scalar_mul = scalar_mul
    tf.add_n = add_n


LAYER_SHAPES = [("a", (5, 4, 3)), ("two", (3, 2, 6)), ("odd", (4, 6, 5)), ("c", (3, 26, 16)), ("wide", (2, 3, 20))]


def gen_layer():
    import itertools
    from deepctr.layers.interaction import FEFMLayer, FwFMLayer
    rng = np.random.RandomState(SEED + 1)
    out = {}
    for tag, (B, F, E) in LAYER_SHAPES:
        x = rng.standard_normal((B, F, E)).astype(np.float32)
        S.reset()
        layer = FwFMLayer(num_fields=F, regularizer=1e-6)
        y = layer(G.T(x))
        out["fwfm_%s_x" % tag], out["fwfm_%s_y" % tag] = x, np.asarray(y.a, dtype=np.float32)
        out["fwfm_%s_r" % tag] = np.asarray(layer.field_strengths.a, dtype=np.float32)
        S.reset()
        layer = FEFMLayer(regularizer=1e-5)
        if F * F * E * E > 50000:
            # the Criteo shape has 325 matrices: eighths in [-1/4, 1/4] instead of the hook's normal draws keep the file small
            layer.build((None, F, E))
            layer.built = True
            for v in layer.field_embeddings.values():
                v.a[...] = rng.randint(-2, 3, size=v.a.shape).astype(np.float32) / 8
        y = layer(G.T(x))
        out["fefm_%s_x" % tag], out["fefm_%s_y" % tag] = x, np.asarray(y.a, dtype=np.float32)
        out["fefm_%s_w" % tag] = np.stack([np.asarray(layer.field_embeddings["%d-%d" % p].a, dtype=np.float32)
                                           for p in itertools.combinations(range(F), 2)])
    G._save("fwfm_fefm_layer", **out)


def fixed_spec(E=8):
    return ([dict(type="sparse", name="C%d" % i, vocabulary_size=11 + 3 * i, embedding_dim=E) for i in range(6)] +
            [dict(type="dense", name="I%d" % i, dimension=1) for i in range(3)])


def gen_models():
    rng = np.random.RandomState(SEED)
    B = 16
    spec = G.mixed_spec(4, False)
    feed = G._feed_for(spec, B, rng)
    spec_h = G.mixed_spec(4, True)
    feed_h = G._feed_for(spec_h, B, rng)
    two = json.loads(json.dumps(spec))
    for d in two:
        if d.get("name") == "sparse_feature_2":
            d["group_name"] = "g1"                      # a group of one field has no pair: tf.add_n([]) fails in the reference
    fw = lambda name, sp, fd, kw: G._run_model(name, "deepctr.models.fwfm", "FwFM", sp, sp, fd, kw)  # noqa: E731
    fw("model_fwfm", spec, feed, {"dnn_hidden_units": [16, 8]})
    fw("model_fwfm_two_groups", two, feed, {"dnn_hidden_units": [8], "fm_group": ["default_group", "g1"]})
    fw("model_fwfm_nodnn", spec, feed, {"dnn_hidden_units": []})
    fw("model_fwfm_hash", spec_h, feed_h, {"dnn_hidden_units": [8]})
    fw("model_fwfm_regression", spec, feed, {"dnn_hidden_units": [8, 4], "task": "regression"})
    fw("model_fwfm_bn", spec, feed, {"dnn_hidden_units": [8, 4], "dnn_use_bn": True})
    fe = lambda name, sp, fd, kw: G._run_model(name, "deepctr.models.deepfefm", "DeepFEFM", sp, sp, fd, kw)  # noqa: E731
    fe("model_fefm", spec, feed, {"dnn_hidden_units": [16, 8]})
    fe("model_fefm_nofefm", spec, feed, {"dnn_hidden_units": [8], "use_fefm": False})
    fe("model_fefm_exclude", spec, feed, {"dnn_hidden_units": [8], "exclude_feature_embed_in_dnn": True})
    fe("model_fefm_nolinear", spec, feed, {"dnn_hidden_units": [8], "use_linear": False})
    fe("model_fefm_noembed", spec, feed, {"dnn_hidden_units": [8], "use_fefm_embed_in_dnn": False})
    fe("model_fefm_deep_only", spec, feed, {"dnn_hidden_units": [8], "use_fefm": False, "use_linear": False})
    fe("model_fefm_nodnn", spec, feed, {"dnn_hidden_units": []})
    fe("model_fefm_shallow", spec, feed, {"dnn_hidden_units": [], "use_linear": False})
    fe("model_fefm_linear_only", spec, feed, {"dnn_hidden_units": [], "use_fefm": False})
    fe("model_fefm_hash", spec_h, feed_h, {"dnn_hidden_units": [8]})
    fe("model_fefm_bn", spec, feed, {"dnn_hidden_units": [8, 4], "dnn_use_bn": True, "task": "regression"})
    spec_f = fixed_spec(8)
    feed_f = G._feed_for(spec_f, 24, rng)
    fe("model_fefm_fixed", spec_f, feed_f, {"dnn_hidden_units": [32, 16]})
    fw("model_fwfm_fixed", spec_f, feed_f, {"dnn_hidden_units": [32, 16]})


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if "--out" in argv:
        i = argv.index("--out")
        G.OUT = os.path.abspath(argv[i + 1])
        del argv[i:i + 2]
    S.install(G.REF)
    S.WEIGHT_HOOK = G.weight_hook
    install_restated_symbols()
    gen_layer()
    gen_models()


if __name__ == "__main__":
    sys.exit(main())
