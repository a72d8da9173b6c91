"""Generates the IFM / DIFM fixtures tests/golden/model_ifm*.npz and model_difm*.npz by running the reference's own IFM and DIFM
(deepctr/models/ifm.py, difm.py) on the oracle's TensorFlow shim, with the oracle's deterministic weights (oracle/make_golden.py).
CPU only; needs the reference checkout, so it is not part of the suite:

    python scripts/make_golden_ifm.py [--out DIR]

Run it into a scratch directory and compare with the committed files to check that the recipe has not rotted (a second run gives the
same bytes).

The shim lacks one symbol IFM uses.  It is installed here, after the shim and before the first import of deepctr.models.ifm, RESTATED
FROM THE TENSORFLOW DOCUMENTATION, not taken from TensorFlow's code (the "unpinned one level down" class):
  * tensorflow.shape(input): the shape of a tensor as a 1-D integer tensor.

Specs: oracle.make_golden.mixed_spec(4), plain and hashed (its ``g1`` group puts sparse_feature_1 BEHIND the sequences in field order);
the same without the max-combiner sequences; a fixed-length spec (SparseFeat and DenseFeat only).  Every spec carries a DenseFeat in
its linear list: without one the shim's linear part broadcasts y to [n^2, 1], which is not reference behaviour.
Linear variants: the deep list reversed (pins the pairing of factor and first-order term by position), and the DenseFeat alone (no
sparse feature in the linear part).

Feeds: RandomState(43), B = 32 (24 for the fixed-length spec), drawn in the order plain / hashed / no-max / fixed.  Rows whose
max-pooled sequence is all padding are excluded by the tests (tests.test_autoint_cpu.att_rows: the reference's -1e9 embedding goes
straight into the FM term).  Rows kept and the range of the compared probabilities (binary fixtures), as the tests assert them
(>= half the rows, (1e-3, 1 - 1e-3)), are printed by this script and recorded here:

    model_ifm              18/32  0.035 .. 0.698     model_difm              18/32  0.424 .. 0.612
    model_ifm_hash         23/32  0.130 .. 0.790     model_difm_hash         23/32  0.375 .. 0.593
    model_ifm_nomax        32/32  0.232 .. 0.923     model_difm_nomax        32/32  0.413 .. 0.628
    model_ifm_fixed        24/24  0.108 .. 0.890     model_difm_fixed        24/24  0.390 .. 0.546
    model_ifm_regression   18/32  (logits)           model_difm_regression   18/32  (logits)
    model_ifm_bn           18/32  0.063 .. 0.764     model_difm_bn           18/32  0.423 .. 0.616
    model_ifm_reorder      18/32  0.107 .. 0.847     model_difm_reorder      18/32  0.368 .. 0.592
    model_ifm_denselin     18/32  0.166 .. 0.749     model_difm_denselin     18/32  0.367 .. 0.717
                                                     model_difm_nores        18/32  0.373 .. 0.739
                                                     model_difm_h3           18/32  0.387 .. 0.813
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

SEED = 43


def install_restated_symbols():
    tf = sys.modules["tensorflow"]

    def shape(input, name=None, out_type=None):  # noqa: A002
        return S.Tensor(np.array(np.asarray(S._arr(input)).shape, dtype=np.int32))

    tf.shape = shape


def _name(d):
    return d.get("name") or d["sparsefeat"]["name"]


def nomax_spec(spec):
    return [d for d in json.loads(json.dumps(spec)) if not (d["type"] == "varlen" and d["combiner"] == "max")]


def fixed_spec(E=8):
    return ([dict(type="sparse", name="C%d" % i, vocabulary_size=11 + 3 * i, embedding_dim=E) for i in range(6)] +
            [dict(type="dense", name="I%d" % i, dimension=1) for i in range(3)])


def report(name):
    """Rows kept and probability range of a written fixture, by the rule the tests apply."""
    g = dict(np.load(os.path.join(G.OUT, name + ".npz")))
    meta = json.loads(bytes(g["meta"]).decode())
    keep = np.ones(g["y"].shape[0], dtype=bool)
    for d in meta["dnn"]:
        if d["type"] == "varlen" and d["combiner"] == "max":
            ids = g["feed/" + d["sparsefeat"]["name"]]
            if d.get("length_name"):
                keep &= g["feed/" + d["length_name"]].reshape(-1) > 0
            else:
                keep &= (ids != 0).any(axis=1)
    y = g["y"].reshape(-1)[keep]
    rng = "(logits)" if meta["kwargs"].get("task") == "regression" else "%.3f .. %.3f" % (y.min(), y.max())
    print("    %-24s %d/%d  %s" % (name, keep.sum(), keep.size, rng))


def gen_models():
    rng = np.random.RandomState(SEED)
    B = 32
    spec = G.mixed_spec(4, False)
    feed = G._feed_for(spec, B, rng)
    spec_h = G.mixed_spec(4, True)
    feed_h = G._feed_for(spec_h, B, rng)
    spec_n = nomax_spec(spec)
    feed_n = {k: v for k, v in feed.items()}
    spec_f = fixed_spec(8)
    feed_f = G._feed_for(spec_f, 24, rng)
    # a linear list in another order than the deep list: the factor meets the first-order terms by position
    reorder = list(reversed(json.loads(json.dumps(spec))))
    dense_only = [d for d in spec if d["type"] == "dense"]
    names = []
    for tag, path, ctor, base in (("ifm", "deepctr.models.ifm", "IFM", {}),
                                  ("difm", "deepctr.models.difm", "DIFM", {"att_embedding_size": 4, "att_head_num": 2})):
        def run(suffix, lin, dnn, fd, kw):
            name = "model_%s%s" % (tag, suffix)
            G._run_model(name, path, ctor, lin, dnn, fd, dict(base, **kw))
            names.append(name)
        run("", spec, spec, feed, {"dnn_hidden_units": [16, 8]})
        run("_hash", spec_h, spec_h, feed_h, {"dnn_hidden_units": [8]})
        run("_nomax", spec_n, spec_n, feed_n, {"dnn_hidden_units": [16, 8]})
        run("_fixed", spec_f, spec_f, feed_f, {"dnn_hidden_units": [32, 16]})
        run("_regression", spec, spec, feed, {"dnn_hidden_units": [8, 4], "task": "regression"})
        run("_bn", spec, spec, feed, {"dnn_hidden_units": [16, 8], "dnn_use_bn": True})
        run("_reorder", reorder, spec, feed, {"dnn_hidden_units": [8]})
        run("_denselin", dense_only, spec, feed, {"dnn_hidden_units": [8]})
        if tag == "difm":
            run("_nores", spec, spec, feed, {"dnn_hidden_units": [8], "att_res": False})
            run("_h3", spec, spec, feed, {"dnn_hidden_units": [8, 4], "att_embedding_size": 5, "att_head_num": 3})
    for name in names:
        report(name)


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
