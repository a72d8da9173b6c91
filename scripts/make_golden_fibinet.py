"""Generates the FiBiNET fixtures tests/golden/model_fibinet_*.npz and tests/golden/senet_bilinear_layer.npz by running the
reference's own FiBiNET / SENETLayer / BilinearInteraction (deepctr/models/fibinet.py, layers/interaction.py:1067-1221) on the
oracle's TensorFlow shim, with the oracle's deterministic weights (oracle/make_golden.py).  CPU only; needs the reference checkout, so
it is not part of the suite:

    python scripts/make_golden_fibinet.py [--out DIR]

Run it into a scratch directory and compare with the committed files to check that the recipe has not rotted."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import make_golden as G  # noqa: E402
from oracle import tf_shim as S  # noqa: E402


def gen_layer():
    from deepctr.layers.interaction import BilinearInteraction, SENETLayer
    rng = np.random.RandomState(12)
    out = {}
    # SENET: (tag, (B, F, E), reduction_ratio)
    for tag, (B, F, E), ratio in [("s", (5, 4, 3), 3), ("s_c", (3, 26, 16), 3), ("s_r1", (4, 6, 5), 1), ("s_big", (2, 3, 4), 7)]:
        x = rng.standard_normal((B, F, E)).astype(np.float32)
        S.reset()
        layer = SENETLayer(ratio, seed=1024)
        ys = layer([G.T(x[:, f:f + 1]) for f in range(F)])
        out[tag + "_x"] = x
        out[tag + "_y"] = np.concatenate([np.asarray(y.a, dtype=np.float32) for y in ys], axis=1)
        out[tag + "_W_1"], out[tag + "_W_2"] = layer.W_1.a, layer.W_2.a
        out[tag + "_cfg"] = np.array([ratio], dtype=np.int32)
    # bilinear: (tag, (B, F, E), type)
    for tag, (B, F, E), btype in [("b_all", (5, 4, 3), "all"), ("b_each", (5, 4, 3), "each"), ("b_int", (5, 4, 3), "interaction"),
                                  ("b_two", (3, 2, 6), "interaction"), ("b_wide", (2, 7, 17), "each")]:
        x = rng.standard_normal((B, F, E)).astype(np.float32)
        S.reset()
        layer = BilinearInteraction(btype, seed=1024)
        y = layer([G.T(x[:, f:f + 1]) for f in range(F)])
        out[tag + "_x"], out[tag + "_y"] = x, np.asarray(y.a, dtype=np.float32)
        ws = [layer.W] if btype == "all" else layer.W_list
        out[tag + "_w"] = np.stack([np.asarray(w.a, dtype=np.float32) for w in ws])
        out[tag + "_type"] = np.frombuffer(btype.encode(), dtype=np.uint8)
    G._save("senet_bilinear_layer", **out)


def fixed_spec(E=8):
    return ([dict(type="sparse", name="C%d" % i, vocabulary_size=11 + 3 * i, embedding_dim=E) for i in range(6)] +
            [dict(type="dense", name="I%d" % i, dimension=1) for i in range(3)])


def gen_models():
    rng = np.random.RandomState(22)
    B = 16
    spec = G.mixed_spec(4, False)
    feed = G._feed_for(spec, B, rng)
    spec_h = G.mixed_spec(4, True)
    feed_h = G._feed_for(spec_h, B, rng)
    run = lambda name, sp, fd, kw: G._run_model(name, "deepctr.models.fibinet", "FiBiNET", sp, sp, fd, kw)  # noqa: E731
    for btype in ("interaction", "all", "each"):
        run("model_fibinet_" + btype, spec, feed, {"bilinear_type": btype, "dnn_hidden_units": [16, 8]})
    run("model_fibinet_hash", spec_h, feed_h, {"bilinear_type": "each", "dnn_hidden_units": [8]})
    run("model_fibinet_nodnn", spec, feed, {"bilinear_type": "interaction", "dnn_hidden_units": []})
    run("model_fibinet_r1", spec, feed, {"bilinear_type": "all", "reduction_ratio": 1, "dnn_hidden_units": [8]})
    run("model_fibinet_rbig", spec, feed, {"bilinear_type": "interaction", "reduction_ratio": 20, "dnn_hidden_units": [8]})
    run("model_fibinet_regression", spec, feed, {"bilinear_type": "each", "task": "regression", "dnn_hidden_units": [8, 4]})
    spec_f = fixed_spec(8)
    feed_f = G._feed_for(spec_f, 24, rng)
    run("model_fibinet_fixed", spec_f, feed_f, {"dnn_hidden_units": [32, 16]})


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if "--out" in argv:
        i = argv.index("--out")
        G.OUT = os.path.abspath(argv[i + 1])
        del argv[i:i + 2]
    S.install(G.REF)
    S.WEIGHT_HOOK = G.weight_hook
    gen_layer()
    gen_models()


if __name__ == "__main__":
    sys.exit(main())
