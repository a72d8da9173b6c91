"""Generates the AutoInt fixtures tests/golden/model_autoint_*.npz and tests/golden/interacting_layer.npz by running the reference's
own AutoInt / InteractingLayer (deepctr/models/autoint.py, layers/interaction.py:697-790) on the oracle's TensorFlow shim, with the
oracle's deterministic weights (oracle/make_golden.py).  CPU only; needs the reference checkout, so it is not part of the suite:

    python scripts/make_golden_autoint.py [--out DIR]

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
    from deepctr.layers.interaction import InteractingLayer
    rng = np.random.RandomState(11)
    out = {}
    # the reference test's shape (tests/layers/interaction_test.py:122: B=5, F=4, E=3) + a few others
    cfgs = [("t", (5, 4, 3), 8, 2, True, False), ("t_scale", (5, 4, 3), 8, 2, True, True),
            ("t_nores", (5, 4, 3), 8, 2, False, False), ("t_both", (5, 4, 3), 4, 3, False, True),
            ("c", (3, 26, 16), 8, 2, True, False), ("one", (4, 1, 5), 3, 1, True, True),
            ("wide", (2, 7, 6), 5, 4, True, False)]
    for tag, shp, d, H, res, scaling in cfgs:
        x = rng.standard_normal(shp).astype(np.float32)
        S.reset()
        layer = InteractingLayer(d, H, res, scaling, seed=1024)
        y = layer(G.T(x)).a
        out["%s_x" % tag], out["%s_y" % tag] = x, np.asarray(y, dtype=np.float32)
        out["%s_query" % tag], out["%s_key" % tag], out["%s_value" % tag] = layer.W_Query.a, layer.W_key.a, layer.W_Value.a
        if res:
            out["%s_res" % tag] = layer.W_Res.a
        out["%s_cfg" % tag] = np.array([d, H, int(res), int(scaling)], dtype=np.int32)
    G._save("interacting_layer", **out)


def fixed_spec(E=8):
    return ([dict(type="sparse", name="C%d" % i, vocabulary_size=11 + 3 * i, embedding_dim=E) for i in range(6)] +
            [dict(type="dense", name="I%d" % i, dimension=1) for i in range(3)])


def gen_models():
    rng = np.random.RandomState(21)
    B = 16
    spec = G.mixed_spec(4, False)
    feed = G._feed_for(spec, B, rng)
    spec_h = G.mixed_spec(4, True)
    feed_h = G._feed_for(spec_h, B, rng)
    run = lambda name, sp, fd, kw, lin=None: G._run_model(  # noqa: E731
        name, "deepctr.models.autoint", "AutoInt", sp if lin is None else lin, sp, fd, kw)
    run("model_autoint_mixed", spec, feed, {"att_layer_num": 2, "att_embedding_size": 4, "att_head_num": 2, "dnn_hidden_units": [16, 8]})
    run("model_autoint_hash", spec_h, feed_h, {"att_layer_num": 1, "att_embedding_size": 3, "att_head_num": 2, "dnn_hidden_units": [8]})
    run("model_autoint_attonly", spec, feed, {"att_layer_num": 3, "att_embedding_size": 4, "att_head_num": 2, "dnn_hidden_units": []})
    run("model_autoint_deeponly", spec, feed, {"att_layer_num": 0, "dnn_hidden_units": [16, 8]})
    run("model_autoint_nores", spec, feed, {"att_layer_num": 2, "att_embedding_size": 4, "att_head_num": 2, "att_res": False,
                                            "dnn_hidden_units": [8]})
    run("model_autoint_h3", spec, feed, {"att_layer_num": 2, "att_embedding_size": 5, "att_head_num": 3, "dnn_hidden_units": [8, 4]})
    spec_f = fixed_spec(8)
    feed_f = G._feed_for(spec_f, 24, rng)
    run("model_autoint_fixed", spec_f, feed_f, {"dnn_hidden_units": [32, 16]})


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
