"""Generates the EDCN fixtures tests/golden/model_edcn_*.npz and edcn_layer.npz by running the reference's own EDCN, BridgeModule and
RegulationModule (deepctr/models/edcn.py, layers/interaction.py:1502-1565, layers/core.py:270-321) on the oracle's TensorFlow shim,
with the oracle's deterministic weights (oracle/make_golden.py).  CPU only; needs the reference checkout, so it is not part of the suite:

    python scripts/make_golden_edcn.py [--out DIR]

Run it into a scratch directory and compare with the committed files to check that the recipe has not rotted (a second run gives the
same bytes).

EDCN cannot carry a DenseFeat, so its linear part is always the [n, 1, 1] form, and the shim's ``Add`` is plain NumPy broadcasting:
unpatched, [n, 1] + [n, 1, 1] answers [n, n, 1] and the reference then predicts [n^2, 1] (1024 rows for 32).  Installed here, after
the shim, RESTATED FROM THE KERAS DOCUMENTATION and not taken from its code (the precedent of ``tf.gather`` in
scripts/make_golden_flen.py): the rank rule of the Keras merge layers — inputs of lower rank get axes inserted at position 1 until the
ranks agree.  With it the reference answers [32, 1] for every fixture.

Specs: oracle.make_golden.mixed_spec(4) without its DenseFeats (9 fields of width 4: D = 36), plain and hashed, and once without the
max-pooled sequences (7 fields).  Fixtures: every bridge type x {vector, matrix} at cross_num = 3 and tau = 0.5; cross_num = 1;
tau = 2.0; regression; BatchNormalization; an empty linear list; the hashed spec; the spec without max-pooled sequences.

Layer fixture edcn_layer.npz: ``reg_F_d`` — RegulationModule at (F, d, tau) = (3, 4, 0.5) and (9, 4, 2.0) with the field weights drawn
N(0, 1) (the oracle's hook draws 0.1 N(0, 1): gates too close to uniform to be seen): x, g, tau, y; ``bridge_<type>`` — BridgeModule of
all four types at D = 12 on standard-normal x and h: x, h, w/<name>, y.

Feeds: RandomState(53), B = 32, drawn in the order plain / hashed.  Rows whose max-pooled sequence is all padding are excluded by the
tests (tests.test_autoint_cpu.att_rows).  Rows kept and the range of the compared probabilities (binary fixtures), as the tests assert
them (>= half the rows, (1e-3, 1 - 1e-3)), are printed by this script and recorded here:

    model_edcn_add_vec         24/32  0.453 .. 0.705
    model_edcn_add_mat         24/32  0.432 .. 0.686
    model_edcn_had_vec         24/32  0.445 .. 0.698
    model_edcn_had_mat         24/32  0.436 .. 0.690
    model_edcn_cat_vec         24/32  0.467 .. 0.716
    model_edcn_cat_mat         24/32  0.444 .. 0.697
    model_edcn_att_vec         24/32  0.439 .. 0.692
    model_edcn_att_mat         24/32  0.430 .. 0.685
    model_edcn_c1              24/32  0.418 .. 0.670
    model_edcn_tau2            24/32  0.445 .. 0.698
    model_edcn_regression      24/32  (logits)
    model_edcn_bn              24/32  0.466 .. 0.714
    model_edcn_nolin           24/32  0.531 .. 0.536
    model_edcn_hash            16/32  0.440 .. 0.644
    model_edcn_nomax           32/32  0.377 .. 0.657
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

SEED = 53
BRIDGES = (("add", "pointwise_addition"), ("had", "hadamard_product"), ("cat", "concatenation"), ("att", "attention_pooling"))


def install_restated_symbols():
    def merge_add(self, inputs):
        arrs = [np.asarray(S._arr(v)) for v in inputs]
        rank = max(a.ndim for a in arrs)
        out = None
        for a in arrs:
            while a.ndim < rank:
                a = np.expand_dims(a, 1)
            out = a if out is None else out + a
        return S.Tensor(out)

    S.Add.call = merge_add


def sparse_only(spec, nomax=False):
    return [d for d in json.loads(json.dumps(spec))
            if d["type"] != "dense" and not (nomax and d["type"] == "varlen" and d["combiner"] == "max")]


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
    print("    %-26s %d/%d  %s" % (name, keep.sum(), keep.size, rng))


def gen_models():
    rng = np.random.RandomState(SEED)
    B = 32
    spec = sparse_only(G.mixed_spec(4, False))
    feed = G._feed_for(spec, B, rng)
    spec_h = sparse_only(G.mixed_spec(4, True))
    feed_h = G._feed_for(spec_h, B, rng)
    spec_n = sparse_only(G.mixed_spec(4, False), nomax=True)
    names = []

    def run(suffix, lin, dnn, fd, **kw):
        name = "model_edcn_%s" % suffix
        kwargs = dict(cross_num=3, cross_parameterization="vector", bridge_type="concatenation", tau=0.5)
        kwargs.update(kw)
        G._run_model(name, "deepctr.models.edcn", "EDCN", lin, dnn, fd, kwargs)
        names.append(name)

    for short, bridge in BRIDGES:
        for par in ("vector", "matrix"):
            run("%s_%s" % (short, par[:3]), spec, spec, feed, bridge_type=bridge, cross_parameterization=par)
    run("c1", spec, spec, feed, cross_num=1)
    run("tau2", spec, spec, feed, tau=2.0, bridge_type="hadamard_product")
    run("regression", spec, spec, feed, task="regression", cross_num=2)
    run("bn", spec, spec, feed, dnn_use_bn=True, cross_num=2)
    run("nolin", [], spec, feed, cross_num=2, bridge_type="pointwise_addition")
    run("hash", spec_h, spec_h, feed_h, cross_num=2, cross_parameterization="matrix")
    run("nomax", spec_n, spec_n, dict(feed), cross_num=2)
    return names


def gen_layers():
    from deepctr.layers.core import RegulationModule
    from deepctr.layers.interaction import BridgeModule
    rng = np.random.RandomState(SEED + 1)
    arrays = {}
    hook = S.WEIGHT_HOOK

    def normal_gates(layer, wname, default):
        if str(wname).endswith("_field_weight"):
            return rng.standard_normal(default.shape)
        return hook(layer, wname, default)

    S.WEIGHT_HOOK = normal_gates
    try:
        for F, d, tau in ((3, 4, 0.5), (9, 4, 2.0)):
            S.reset()
            x = rng.standard_normal((6, F, d)).astype(np.float32)
            layer = RegulationModule(tau)
            y = layer(G.T(x))
            tag = "reg_%d_%d" % (F, d)
            (g,) = G._weights_dict().values()
            arrays.update({tag + "/x": x, tag + "/g": g, tag + "/tau": np.array(tau, dtype=np.float64),
                           tag + "/y": np.asarray(y.a, dtype=np.float32)})
    finally:
        S.WEIGHT_HOOK = hook
    for _, bridge in BRIDGES:
        S.reset()
        x, h = (rng.standard_normal((6, 12)).astype(np.float32) for _ in range(2))
        y = BridgeModule(bridge)([G.T(x), G.T(h)])
        tag = "bridge_" + bridge
        arrays.update({tag + "/x": x, tag + "/h": h, tag + "/y": np.asarray(y.a, dtype=np.float32)})
        for k, v in G._weights_dict().items():
            arrays["%s/w/%s" % (tag, k)] = v
    G._save("edcn_layer", **arrays)


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if "--out" in argv:
        i = argv.index("--out")
        G.OUT = os.path.abspath(argv[i + 1])
        del argv[i:i + 2]
    S.install(G.REF)
    S.WEIGHT_HOOK = G.weight_hook
    install_restated_symbols()
    names = gen_models()
    gen_layers()
    for name in names:
        report(name)


if __name__ == "__main__":
    sys.exit(main())
