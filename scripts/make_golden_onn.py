"""Generates the ONN fixtures tests/golden/model_onn*.npz by running the reference's own ONN (deepctr/models/onn.py) on the oracle's
TensorFlow shim, with the oracle's deterministic weights (oracle/make_golden.py).  CPU only; needs the reference checkout, so it is not
part of the suite:

    python scripts/make_golden_onn.py [--out DIR]

Run it into a scratch directory and compare with the committed files to check that the recipe has not rotted (a second run gives the
same bytes).

The shim lacks two symbols ONN uses.  They are installed here, after the shim and before the first import of deepctr.models.onn,
RESTATED FROM THE KERAS DOCUMENTATION, not taken from Keras' code (the "unpinned one level down" class):
  * tensorflow.keras.layers.multiply(inputs): the elementwise product of a list of tensors, taken left to right;
  * tensorflow.keras.backend.sum(x, axis=None, keepdims=False): the sum of a tensor's values along an axis.

Specs: oracle.make_golden.mixed_spec with the ``embedding_name`` of ``sequence_len_max`` removed (the reference keys its field-aware
tables by embedding_name and looks them up by name: a shared table is a KeyError there); a fixed-length spec; a two-field spec.  Every
spec carries a DenseFeat in both lists: without one the shim's linear part broadcasts y to [n^2, 1], which is not reference behaviour.

Feeds: RandomState(41), B = 32 (24 for the fixed-length and two-field specs), drawn in the order plain / hashed / fixed / two-field.
Rows whose max-pooled sequence is all padding are excluded by the tests (tests.test_autoint_cpu.att_rows); 20/32, 21/32, 24/24 and
24/24 rows remain and the compared probabilities lie in 0.28 .. 0.71 (the tests assert >= half and (1e-3, 1 - 1e-3))."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import make_golden as G  # noqa: E402
from oracle import tf_shim as S  # noqa: E402

SEED = 41


def install_restated_symbols():
    layers = sys.modules["tensorflow.keras.layers"]
    K = sys.modules["tensorflow.keras.backend"]

    def multiply(inputs, **kwargs):
        arrs = [np.asarray(S._arr(v)) for v in inputs]
        assert len(arrs) >= 2, "multiply: a list of at least two tensors"
        out = arrs[0]
        for a in arrs[1:]:
            out = out * a
        return S.Tensor(out)

    def k_sum(x, axis=None, keepdims=False):
        return S.Tensor(np.sum(np.asarray(S._arr(x)), axis=axis, keepdims=keepdims))

    layers.multiply = multiply
    K.sum = k_sum


def onn_spec(hash_flag):
    spec = json.loads(json.dumps(G.mixed_spec(4, hash_flag)))
    for d in spec:
        if d["type"] == "varlen":
            d["sparsefeat"].pop("embedding_name", None)
    return spec


def fixed_spec(E=8):
    return ([dict(type="sparse", name="C%d" % i, vocabulary_size=11 + 3 * i, embedding_dim=E) for i in range(6)] +
            [dict(type="dense", name="I%d" % i, dimension=1) for i in range(3)])


def two_spec(E=4):
    return [dict(type="sparse", name="A", vocabulary_size=13, embedding_dim=E), dict(type="sparse", name="B", vocabulary_size=7, embedding_dim=E),
            dict(type="dense", name="I0", dimension=1)]


def gen_models():
    rng = np.random.RandomState(SEED)
    B = 32
    spec = onn_spec(False)
    feed = G._feed_for(spec, B, rng)
    spec_h = onn_spec(True)
    feed_h = G._feed_for(spec_h, B, rng)
    spec_f = fixed_spec(8)
    feed_f = G._feed_for(spec_f, 24, rng)
    spec_2 = two_spec(4)
    feed_2 = G._feed_for(spec_2, 24, rng)
    run = lambda name, lin, dnn, fd, kw: G._run_model(name, "deepctr.models.onn", "ONN", lin, dnn, fd, kw)  # noqa: E731
    run("model_onn", spec, spec, feed, {"dnn_hidden_units": [16, 8]})
    run("model_onn_reduce", spec, spec, feed, {"dnn_hidden_units": [16, 8], "reduce_sum": True})
    run("model_onn_nobn", spec, spec, feed, {"dnn_hidden_units": [16, 8], "use_bn": False})
    run("model_onn_hash", spec_h, spec_h, feed_h, {"dnn_hidden_units": [8]})
    run("model_onn_regression", spec, spec, feed, {"dnn_hidden_units": [8, 4], "task": "regression"})
    run("model_onn_nodnn", spec, spec, feed, {"dnn_hidden_units": []})
    run("model_onn_fixed", spec_f, spec_f, feed_f, {"dnn_hidden_units": [32, 16]})
    run("model_onn_two", spec_2, spec_2, feed_2, {"dnn_hidden_units": [8], "reduce_sum": True})
    # linear columns that are a strict subset of the deep columns
    drop = ("sparse_feature_1", "sequence_mean", "dense_vec")
    sub = [d for d in spec if (d.get("name") or d["sparsefeat"]["name"]) not in drop]
    run("model_onn_linear_subset", sub, spec, feed, {"dnn_hidden_units": [8]})


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if "--out" in argv:
        i = argv.index("--out")
        G.OUT = os.path.abspath(argv[i + 1])
        del argv[i:i + 2]
    S.install(G.REF)
    S.WEIGHT_HOOK = G.weight_hook
    install_restated_symbols()
    gen_models()


if __name__ == "__main__":
    sys.exit(main())
