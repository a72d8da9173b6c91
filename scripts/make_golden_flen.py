"""Generates the FLEN fixtures tests/golden/model_flen*.npz and flen_layer.npz by running the reference's own FLEN and
FieldWiseBiInteraction (deepctr/models/flen.py, deepctr/layers/interaction.py:1224-1348) on the oracle's TensorFlow shim, with the
oracle's deterministic weights (oracle/make_golden.py).  CPU only; needs the reference checkout, so it is not part of the suite:

    python scripts/make_golden_flen.py [--out DIR]

Run it into a scratch directory and compare with the committed files to check that the recipe has not rotted (a second run gives the
same bytes).

The shim lacks two things FLEN uses.  They are installed here, after the shim and before the first import of deepctr.models.flen,
RESTATED FROM THE TENSORFLOW / KERAS DOCUMENTATION, not taken from their code (the "unpinned one level down" class):
  * tensorflow.gather(params, indices, axis): the slices of ``params`` along ``axis`` at ``indices``.
  * Layer.add_weight(shape=<int>): a bare integer is the shape of a 1-D weight (the reference passes ``shape=(embedding_size)``).

Specs: oracle.make_golden.mixed_spec(4), plain and hashed: two groups, the second (``g1``) holds one field, max-pooled sequences
present; the same without the max-combiner sequences; a fixed-length spec (SparseFeat and DenseFeat only) in three groups of 3, 2
and 2 fields; variants: regression, BatchNormalization, no hidden units, the DenseFeat alone in the linear list.  Every spec carries
a DenseFeat in its linear list: without one the shim's linear part broadcasts y to [n^2, 1], which is not reference behaviour
(scripts/make_golden_ifm.py).  That holds for the example's own columns too (examples/run_flen.py: 21 SparseFeat and nothing else;
checked here: the shim answers [n^2, 1] for them), so model_flen_avazu_sample is generated through the example's preprocessing and its
three ``field_info`` groups PLUS the ``day`` column the example derives from ``hour`` and then leaves unused, as a DenseFeat (day of
the month / 31) of the linear and the deep list.  The example's embedding_dim 16; a 32-16 DNN keeps the file below 90 KB.

Layer fixture flen_layer.npz: tags ``g2`` (2 groups of 1 field, d = 4: one field per group, the FM part vanishes), ``g3`` (groups of
3 / 1 / 2 fields, d = 5), ``g4nb`` (4 groups of 2 / 2 / 1 / 3 fields, d = 8, use_bias=False); per tag x<k> (the inputs), w/<name>, y.

Feeds: RandomState(47), B = 32 (24 for the fixed-length spec), drawn in the order plain / hashed / fixed.  Rows whose max-pooled
sequence is all padding are excluded by the tests (tests.test_autoint_cpu.att_rows: the reference's -1e9 embedding goes straight into
the group sums).  Rows kept and the range of the compared probabilities (binary fixtures), as the tests assert them (>= half the
rows, (1e-3, 1 - 1e-3)), are printed by this script and recorded here:

    model_flen               20/32  0.359 .. 0.841
    model_flen_hash          21/32  0.382 .. 0.777
    model_flen_nomax         32/32  0.335 .. 0.789
    model_flen_fixed         24/24  0.256 .. 0.600
    model_flen_regression    20/32  (logits)
    model_flen_bn            20/32  0.287 .. 0.819
    model_flen_nodnn         20/32  0.426 .. 0.867
    model_flen_denselin      20/32  0.298 .. 0.670
    model_flen_avazu_sample  100/100  0.485 .. 0.890
"""
import json
import os
import shutil
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import make_golden as G  # noqa: E402
from oracle import tf_shim as S  # noqa: E402

SEED = 47


def install_restated_symbols():
    tf = sys.modules["tensorflow"]

    def gather(params, indices, validate_indices=None, axis=0, batch_dims=0, name=None):
        return S.Tensor(np.take(np.asarray(S._arr(params)), np.asarray(S._arr(indices), dtype=np.int64), axis=axis))

    tf.gather = gather
    add_weight = S.Layer.add_weight

    def add_weight_int_shape(self, name=None, shape=None, *args, **kwargs):
        if isinstance(shape, (int, np.integer)):
            shape = (int(shape),)
        return add_weight(self, name, shape, *args, **kwargs)

    S.Layer.add_weight = add_weight_int_shape


def nomax_spec(spec):
    return [d for d in json.loads(json.dumps(spec)) if not (d["type"] == "varlen" and d["combiner"] == "max")]


def fixed_spec(E=8):
    grp = ["user", "context", "item", "user", "item", "context", "user"]
    return ([dict(type="sparse", name="C%d" % i, vocabulary_size=11 + 3 * i, embedding_dim=E, group_name=grp[i]) for i in range(7)] +
            [dict(type="dense", name="I%d" % i, dimension=1) for i in range(2)])


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
    spec_f = fixed_spec(8)
    feed_f = G._feed_for(spec_f, 24, rng)
    dense_only = [d for d in spec if d["type"] == "dense"]
    names = []

    def run(suffix, lin, dnn, fd, kw):
        name = "model_flen%s" % suffix
        G._run_model(name, "deepctr.models.flen", "FLEN", lin, dnn, fd, kw)
        names.append(name)

    run("", spec, spec, feed, {"dnn_hidden_units": [16, 8]})
    run("_hash", spec_h, spec_h, feed_h, {"dnn_hidden_units": [8]})
    run("_nomax", spec_n, spec_n, dict(feed), {"dnn_hidden_units": [16, 8]})
    run("_fixed", spec_f, spec_f, feed_f, {"dnn_hidden_units": [32, 16]})
    run("_regression", spec, spec, feed, {"dnn_hidden_units": [8, 4], "task": "regression"})
    run("_bn", spec, spec, feed, {"dnn_hidden_units": [16, 8], "dnn_use_bn": True})
    run("_nodnn", spec, spec, feed, {"dnn_hidden_units": []})
    run("_denselin", dense_only, spec, feed, {"dnn_hidden_units": [8]})
    return names


def gen_avazu_sample():
    """examples/avazu_sample.txt through the example's own preprocessing (examples/run_flen.py:10-42) and field_info groups."""
    import pandas as pd
    from sklearn.preprocessing import LabelEncoder
    src = os.path.join(G.REF, "examples", "avazu_sample.txt")
    data = pd.read_csv(src)
    data['day'] = data['hour'].apply(lambda x: str(x)[4:6])
    data['hour'] = data['hour'].apply(lambda x: str(x)[6:])
    sparse_features = ['hour', 'C1', 'banner_pos', 'site_id', 'site_domain', 'site_category', 'app_id', 'app_domain', 'app_category',
                       'device_id', 'device_model', 'device_type', 'device_conn_type', 'C14', 'C15', 'C16', 'C17', 'C18', 'C19', 'C20',
                       'C21']
    data[sparse_features] = data[sparse_features].fillna('-1', )
    for feat in sparse_features:
        data[feat] = LabelEncoder().fit_transform(data[feat])
    field_info = dict(C14='user', C15='user', C16='user', C17='user', C18='user', C19='user', C20='user', C21='user', C1='user',
                      banner_pos='context', site_id='context', site_domain='context', site_category='context', app_id='item',
                      app_domain='item', app_category='item', device_model='user', device_type='user', device_conn_type='context',
                      hour='context', device_id='user')
    spec = [dict(type="sparse", name=f, vocabulary_size=int(data[f].max()) + 1, embedding_dim=16, group_name=field_info[f])
            for f in sparse_features]
    feed = {f: data[f].values.astype(np.int32) for f in sparse_features}
    # the example's own columns: does the shim's DenseFeat-free linear part give [n, 1]?
    S.reset()
    S.set_feed(feed)
    from deepctr.models.flen import FLEN
    y = FLEN(G.build_ref_columns(spec), G.build_ref_columns(spec), dnn_hidden_units=[32, 16]).predict()
    print("    the example's DenseFeat-free columns on the shim: y %s for %d rows" % (tuple(np.asarray(y).shape), len(data)))
    spec.append(dict(type="dense", name="day", dimension=1))
    feed["day"] = (data["day"].astype(np.float32) / 31.0).values.astype(np.float32)
    G._run_model("model_flen_avazu_sample", "deepctr.models.flen", "FLEN", spec, spec, feed, {"dnn_hidden_units": [32, 16]})
    # the 100-row DATA file itself (not source code), so that the example flow can run from the CSV where the reference is absent
    shutil.copyfile(src, os.path.join(G.OUT, "avazu_sample.txt"))
    return ["model_flen_avazu_sample"]


def gen_layer():
    from deepctr.layers.interaction import FieldWiseBiInteraction
    rng = np.random.RandomState(SEED + 1)
    arrays = {}
    for tag, sizes, d, use_bias in (("g2", (1, 1), 4, True), ("g3", (3, 1, 2), 5, True), ("g4nb", (2, 2, 1, 3), 8, False)):
        S.reset()
        xs = [rng.standard_normal((6, n, d)).astype(np.float32) * 0.5 for n in sizes]
        layer = FieldWiseBiInteraction(use_bias=use_bias, seed=1024)
        y = layer([G.T(x) for x in xs])
        for k, x in enumerate(xs):
            arrays["%s/x%d" % (tag, k)] = x
        for k, v in G._weights_dict().items():
            arrays["%s/w/%s" % (tag, k)] = v
        arrays["%s/y" % tag] = np.asarray(y.a, dtype=np.float32)
        arrays["%s/use_bias" % tag] = np.array(int(use_bias), dtype=np.int32)
    G._save("flen_layer", **arrays)


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
    names += gen_avazu_sample()
    gen_layer()
    for name in names:
        report(name)


if __name__ == "__main__":
    sys.exit(main())
