"""Generates the MLR fixtures tests/golden/model_mlr*.npz by running the reference's own MLR (deepctr/models/mlr.py) on the oracle's
TensorFlow shim, with the oracle's deterministic weights (oracle/make_golden.py).  CPU only; needs the reference checkout, so it is not
part of the suite:

    python scripts/make_golden_mlr.py [--out DIR]

Run it into a scratch directory and compare with the committed files to check that the recipe has not rotted (a second run gives the
same bytes).

MLR takes three column lists, so it has its own runner (oracle.make_golden._run_model builds (linear, dnn) models).  The meta record
holds ``region`` / ``base`` / ``bias`` (the specs, null where the argument is left out) and, for tests.test_autoint_cpu.att_rows, the
union of the three under ``dnn`` and the reference's input order (build_input_features over region + base + bias) under ``inputs``.

The shim lacks one symbol MLR uses.  It is installed here, after the shim and before the first import of deepctr.models.mlr, RESTATED
FROM THE KERAS DOCUMENTATION, not taken from Keras' code (the "unpinned one level down" class):
  * tensorflow.keras.layers.dot(inputs, axes): the batch-wise dot product of two tensors along ``axes``; for two [B, n] tensors and
    axes = -1 the [B, 1] tensor of sum_k a[b, k] * b[b, k].

Every column list of every fixture carries a DenseFeat: without one the shim's linear part broadcasts y to [n^2, 1], which is not
reference behaviour (scripts/make_golden_onn.py); the no-dense case is tested against the float64 oracle instead.

Weights: oracle.make_golden.weight_hook, with the one-wide tables drawn at WEIGHT_SCALE times its standard deviation and the
linear_kernels likewise (at the hook's 0.1 every logit is ~0.3: softmax ~ 1/R, sigmoid ~ 1/2, and no mutation of the graph would show).
The recipe checks, from the float64 oracle ALONE (tests/ref_mlr.py), that on at least half of the compared rows of every fixture each
applicable mutation moves the output by >= 100 x (1e-4 of it) — learners without their sigmoid (binary), region and learner tables
swapped (base = region), the bias factor dropped (bias part), softmax replaced by 1 / R — and that binary outputs lie in
(1e-3, 1 - 1e-3).  Rows whose max-pooled sequence is all padding are excluded (tests.test_autoint_cpu.att_rows); at least half must
remain.  If a condition fails, raise WEIGHT_SCALE, not the bar.

Feeds: RandomState(43), B = 32 (24 for the fixed-length spec), drawn in the order plain / hashed / fixed."""
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
WEIGHT_SCALE = 3.0


def install_restated_symbols():
    layers = sys.modules["tensorflow.keras.layers"]

    def dot(inputs, axes, normalize=False, **kwargs):
        assert len(inputs) == 2 and not normalize, "dot: two tensors, no normalisation"
        a, b = (np.asarray(S._arr(v)) for v in inputs)
        assert a.ndim == 2 and b.ndim == 2 and axes in (-1, 1), "dot: restated for two [B, n] tensors along the last axis"
        return S.Tensor((a * b).sum(axis=1, keepdims=True))

    layers.dot = dot


def weight_hook(layer, wname, default):
    w = G.weight_hook(layer, wname, default)
    if wname in ("embeddings", "linear_kernel"):
        w = w * WEIGHT_SCALE
    return w


def _name(d):
    return d.get("name") or d["sparsefeat"]["name"]


def pick(spec, names):
    return [d for d in spec if _name(d) in names]


def union(*specs):
    out, seen = [], set()
    for spec in specs:
        for d in spec or []:
            if _name(d) not in seen:
                seen.add(_name(d))
                out.append(d)
    return out


def fixed_spec():
    return ([dict(type="sparse", name="C%d" % i, vocabulary_size=11 + 3 * i, embedding_dim=4) for i in range(6)] +
            [dict(type="dense", name="I%d" % i, dimension=1) for i in range(3)])


def check_fixture(name, arrays):
    """The conditions of the module docstring, from tests/ref_mlr.py's float64 oracle alone."""
    from tests import ref_mlr as RM
    from tests.test_autoint_cpu import att_rows
    meta = json.loads(bytes(arrays["meta"]).decode())
    feed = {k[5:]: v for k, v in arrays.items() if k.startswith("feed/")}
    n = arrays["y"].shape[0]
    rows = att_rows(meta, feed, n)
    assert rows.sum() * 2 >= n, "%s: %d of %d rows remain" % (name, rows.sum(), n)
    y = RM.run_fixture(arrays).reshape(-1)[rows]
    binary = meta["kwargs"].get("task", "binary") == "binary"
    if binary:
        assert ((y > 1e-3) & (y < 1 - 1e-3)).all(), "%s: outputs in [%g, %g]" % (name, y.min(), y.max())
    for mutate in RM.mutations(meta):
        ym = RM.run_fixture(arrays, mutate=mutate).reshape(-1)[rows]
        moved = np.abs(ym - y) >= 100 * 1e-4 * np.abs(y)
        assert moved.sum() * 2 >= moved.size, "%s: mutation %r moves %d of %d rows" % (name, mutate, moved.sum(), moved.size)
    return int(rows.sum()), float(y.min()), float(y.max())


def run(name, region, base, bias, feed, kwargs):
    S.reset()
    S.set_feed(feed)
    from deepctr.models.mlr import MLR
    cols = lambda spec: None if spec is None else G.build_ref_columns(spec)     # noqa: E731
    model = MLR(cols(region), cols(base), bias_feature_columns=cols(bias), **kwargs)
    from deepctr.feature_column import build_input_features
    inputs = list(build_input_features(cols(region) + (cols(base) or cols(region)) + (cols(bias) or [])).keys())     # mlr.py:41
    y = model.predict()
    arrays = {"y": y.astype(np.float32)}
    for k, v in feed.items():
        if any(_name(d) == k or d.get("length_name") == k or d.get("weight_name") == k for d in union(region, base, bias)):
            arrays["feed/" + k] = v
    for k, v in G._weights_dict().items():
        arrays["w/" + k] = v
    both = union(region, base, bias)
    meta = {"model": "MLR", "region": region, "base": base, "bias": bias, "kwargs": kwargs, "linear": both, "dnn": both, "inputs": inputs}
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    kept, lo, hi = check_fixture(name, arrays)
    G._save(name, **arrays)
    print("    %d/%d rows compared, outputs in %.3f .. %.3f" % (kept, y.shape[0], lo, hi))


def gen_models():
    rng = np.random.RandomState(SEED)
    spec = G.mixed_spec(4, False)
    feed = G._feed_for(spec, 32, rng)
    spec_h = G.mixed_spec(4, True)
    feed_h = G._feed_for(spec_h, 32, rng)
    spec_f = fixed_spec()
    feed_f = G._feed_for(spec_f, 24, rng)
    run("model_mlr", spec, None, None, feed, {})
    run("model_mlr_hash", spec_h, None, None, feed_h, {})
    run("model_mlr_r2", spec, None, None, feed, {"region_num": 2})
    run("model_mlr_r7", spec, None, None, feed, {"region_num": 7, "seed": 7})
    # base != region: overlapping (two features and the dense vector shared), then disjoint
    a = pick(spec, ("weighted_seq", "sparse_feature_0", "sparse_feature_1", "dense_feature_0", "sequence_sum", "dense_vec"))
    b = pick(spec, ("sparse_feature_1", "sparse_feature_2", "dense_vec", "sequence_sum", "sequence_mean", "sequence_wsum"))
    run("model_mlr_base_overlap", a, b, None, feed, {"region_num": 3})
    c = pick(spec, ("sparse_feature_0", "dense_feature_0", "sequence_mean", "sequence_len_max"))
    d = pick(spec, ("sparse_feature_1", "sparse_feature_2", "dense_vec", "sequence_wsum"))
    run("model_mlr_base_disjoint", c, d, None, feed, {})
    # a bias part over a subset of the columns; then one feature (sparse_feature_0) in region + bias only
    run("model_mlr_bias", spec, None, pick(spec, ("sparse_feature_0", "sequence_sum", "dense_feature_0")), feed, {})
    run("model_mlr_bias_split", a, b, pick(spec, ("sparse_feature_0", "sparse_feature_2", "dense_vec")), feed, {"region_num": 3})
    run("model_mlr_regression", spec, None, pick(spec, ("sparse_feature_1", "dense_feature_0")), feed, {"task": "regression"})
    run("model_mlr_fixed", spec_f, None, spec_f[2:8], feed_f, {})


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if "--out" in argv:
        i = argv.index("--out")
        G.OUT = os.path.abspath(argv[i + 1])
        del argv[i:i + 2]
    S.install(G.REF)
    S.WEIGHT_HOOK = weight_hook
    install_restated_symbols()
    gen_models()


if __name__ == "__main__":
    sys.exit(main())
