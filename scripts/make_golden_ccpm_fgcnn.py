"""Generates the CCPM / FGCNN fixtures tests/golden/model_ccpm_*.npz, model_fgcnn_*.npz, kmax_layer.npz and fgcnn_layer.npz on the oracle's
TensorFlow shim, with the oracle's deterministic weights (oracle/make_golden.py).  CPU only; needs the reference checkout, so it is not
part of the suite:

    python scripts/make_golden_ccpm_fgcnn.py [--out DIR]

Run it into a scratch directory and compare with the committed files to check that the recipe has not rotted (a second run gives the
same bytes).

WHAT IS THE REFERENCE'S CODE HERE, imported in place from the checkout and never copied: ``CCPM`` (deepctr/models/ccpm.py), ``FGCNN``
and its ``unstack`` (deepctr/models/fgcnn.py), ``KMaxPooling`` (layers/sequence.py), ``FGCNNLayer`` and ``InnerProductLayer``
(layers/interaction.py), ``DNN``, the embedding plumbing, ``concat_func`` and the linear part.

WHAT IS RESTATED, from the TensorFlow / keras documentation and not from their code, installed after the shim:
  * ``tf.keras.layers.Conv2D`` as documented: ``kernel`` [kh, kw, C_in, filters] (glorot_uniform), ``bias`` [filters] (zeros), channels
    last, stride 1; a cross-correlation (the kernel is not flipped); padding 'same' pads each spatial axis with k - 1 zeros in all,
    (k - 1) // 2 of them in front; then the activation;
  * ``tf.keras.layers.MaxPooling2D(pool_size)``: strides = pool_size, padding 'valid': floor(n / p) windows, the tail dropped;
  * ``tf.nn.top_k(input, k, sorted=True)``: the k largest along the last axis in descending order, with their indices;
  * ``tf.unstack(value, num, axis)``;
  * ``conv_output_length(input_length, filter_size, padding, stride, dilation)`` of keras' conv utilities: 'same' -> n, 'valid' ->
    n - dilated filter + 1, then ceil-divided by the stride;
  * a ``Lambda`` that hands a list result through (the shim's wraps results into one tensor; FGCNN's unstack returns a list);
  * the rank rule of the Keras merge layers for ``Add``, as scripts/make_golden_edcn.py installs it (a linear part of sparse columns
    only is [n, 1, 1] against the DNN logit's [n, 1]).
So the wiring, the k schedule, the recombination reshape, the two embedding sets and the inner products carry the reference's authority;
the convolution and the poolings carry the documentation's, and tests/ref_fieldconv.py, written from the equations, is their independent
check: this script asserts agreement with it to 1e-5 before it writes anything.

Weights: the oracle's hook (embeddings 0.3 N), except the Conv2D kernels (N / sqrt(C_in)) and biases (0.2 N): at glorot scale a conv
stage's output is near zero and nothing behind it moves the logits.

Model fixtures (B = 32, E = 4), CCPM: default widths and filters over 7 fields; three layers over 5 fields, where min(k, rows) bites;
no conv layers; hashed columns; a sequence column; regression; no DNN.  FGCNN: the default lengths cut to 2 layers; pooling width 3 on
odd rows with an even conv width; new_maps differing per layer; no conv layers; hashed columns; a sequence column plus a DenseFeat
that is ignored; regression.
Layer fixtures: kmax_layer.npz (3-D and 4-D inputs, every axis >= 1, k in {1, 3, n}); fgcnn_layer.npz (odd and even F, an even width).

Conditions, asserted by this script and by tests/test_ccpm_fgcnn_cpu.py from the float64 oracle alone: each mutation of
tests/ref_fieldconv.MUTATIONS that applies to a fixture moves its logits by >= 100 x 1e-4 of their largest; >= 90 % of the tanh
pre-activations (conv stages and recombination) have |z| < 3.  The figures of the committed files are in REPORT below; a run that gives
others says so."""
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

SEED = 93
REPORT = """    model_ccpm_default       0.297 .. 0.626   moved x tol: pad_side  4549  keep_order 10603  flip  8281  channel_first 10878  pool_pad     -  recombine_ew     -  swap_fg     -   |z| < 3: 1.000
    model_ccpm_l3            0.460 .. 0.655   moved x tol: pad_side   840  keep_order  1100  flip   979  channel_first  1486  pool_pad     -  recombine_ew     -  swap_fg     -   |z| < 3: 1.000
    model_ccpm_noconv        0.327 .. 0.672   moved x tol: pad_side     -  keep_order     -  flip     -  channel_first     -  pool_pad     -  recombine_ew     -  swap_fg     -   |z| < 3: -
    model_ccpm_hash          0.327 .. 0.571   moved x tol: pad_side  6012  keep_order 11858  flip  8611  channel_first 11154  pool_pad     -  recombine_ew     -  swap_fg     -   |z| < 3: 1.000
    model_ccpm_seq           0.184 .. 0.505   moved x tol: pad_side  3412  keep_order  3310  flip  4750  channel_first  5982  pool_pad     -  recombine_ew     -  swap_fg     -   |z| < 3: 1.000
    model_ccpm_regression    (logits)         moved x tol: pad_side  4549  keep_order 10603  flip  8281  channel_first 10878  pool_pad     -  recombine_ew     -  swap_fg     -   |z| < 3: 1.000
    model_ccpm_nodnn         0.236 .. 0.709   moved x tol: pad_side  4874  keep_order  9724  flip  8364  channel_first 11651  pool_pad     -  recombine_ew     -  swap_fg     -   |z| < 3: 1.000
    model_fgcnn_l2           0.430 .. 0.722   moved x tol: pad_side     -  keep_order     -  flip  3322  channel_first  5672  pool_pad  5590  recombine_ew  3758  swap_fg  5195   |z| < 3: 0.999
    model_fgcnn_pool3        0.388 .. 0.702   moved x tol: pad_side  2772  keep_order     -  flip  2223  channel_first  4515  pool_pad  2514  recombine_ew  4191  swap_fg  5126   |z| < 3: 1.000
    model_fgcnn_maps         0.404 .. 0.648   moved x tol: pad_side  4736  keep_order     -  flip  4895  channel_first  5667  pool_pad  4910  recombine_ew  4489  swap_fg  6146   |z| < 3: 1.000
    model_fgcnn_noconv       0.367 .. 0.706   moved x tol: pad_side     -  keep_order     -  flip     -  channel_first     -  pool_pad     -  recombine_ew     -  swap_fg     -   |z| < 3: -
    model_fgcnn_hash         0.431 .. 0.648   moved x tol: pad_side     -  keep_order     -  flip  7021  channel_first  7595  pool_pad  5417  recombine_ew  5520  swap_fg  6088   |z| < 3: 1.000
    model_fgcnn_seq          0.396 .. 0.655   moved x tol: pad_side     -  keep_order     -  flip  6136  channel_first  8357  pool_pad 11843  recombine_ew  7927  swap_fg  9605   |z| < 3: 0.999
    model_fgcnn_regression   (logits)         moved x tol: pad_side     -  keep_order     -  flip  3322  channel_first  5672  pool_pad  5590  recombine_ew  3758  swap_fg  5195   |z| < 3: 0.999
"""


def arr(x):
    return np.asarray(S._arr(x))


def _pair(v):
    return (int(v), int(v)) if np.isscalar(v) else tuple(int(a) for a in v)


class Conv2D(S.Layer):
    """tf.keras.layers.Conv2D as documented (see the module docstring); stride 1, channels last."""

    def __init__(self, filters, kernel_size, strides=(1, 1), padding="valid", activation=None, use_bias=True, **kw):
        super(Conv2D, self).__init__(**kw)
        assert _pair(strides) == (1, 1) and padding in ("same", "valid")
        self.filters, self.kernel_size, self.padding = int(filters), _pair(kernel_size), padding
        self.activation, self.use_bias = activation, use_bias

    def build(self, input_shape):
        self.kernel = self.add_weight("kernel", self.kernel_size + (int(input_shape[-1]), self.filters), initializer=S.glorot_uniform())
        if self.use_bias:
            self.bias = self.add_weight("bias", (self.filters,), initializer=S.Zeros())

    def call(self, inputs, **kw):
        x = arr(inputs).astype(np.float32)
        k = arr(self.kernel)
        kh, kw_ = self.kernel_size
        if self.padding == "same":
            ph, pw = kh - 1, kw_ - 1
            x = np.pad(x, ((0, 0), (ph // 2, ph - ph // 2), (pw // 2, pw - pw // 2), (0, 0)))
        H, W = x.shape[1] - kh + 1, x.shape[2] - kw_ + 1
        y = np.zeros((x.shape[0], H, W, self.filters), np.float32)
        for i in range(kh):
            for j in range(kw_):
                y = y + x[:, i:i + H, j:j + W] @ k[i, j]
        if self.use_bias:
            y = y + arr(self.bias)
        y = S.Tensor(y.astype(np.float32))
        return S.Activation(self.activation).call(y) if self.activation is not None else y


class MaxPooling2D(S.Layer):
    """tf.keras.layers.MaxPooling2D as documented: strides default to pool_size, padding 'valid'."""

    def __init__(self, pool_size=(2, 2), strides=None, padding="valid", **kw):
        super(MaxPooling2D, self).__init__(**kw)
        assert strides is None and padding == "valid"
        self.pool_size = _pair(pool_size)

    def call(self, inputs, **kw):
        x = arr(inputs)
        ph, pw = self.pool_size
        nh, nw = x.shape[1] // ph, x.shape[2] // pw
        x = x[:, :nh * ph, :nw * pw].reshape(x.shape[0], nh, ph, nw, pw, x.shape[3])
        return S.Tensor(x.max(axis=(2, 4)))


class ListLambda(S.Lambda):
    def call(self, inputs, **kw):
        out = self.function(inputs)
        return out if isinstance(out, (list, S.Tensor)) else S._t(out)


def top_k(input, k=1, sorted=True, name=None):  # noqa: A002
    x = arr(input)
    idx = np.argsort(-x, axis=-1, kind="stable")[..., :k]
    return S.Tensor(np.take_along_axis(x, idx, axis=-1)), S.Tensor(idx.astype(np.int32))


def unstack(value, num=None, axis=0, name=None):
    x = arr(value)
    assert num is None or int(num) == x.shape[axis]
    return [S.Tensor(np.take(x, i, axis=axis)) for i in range(x.shape[axis])]


def conv_output_length(input_length, filter_size, padding, stride, dilation=1):
    if input_length is None:
        return None
    dilated = filter_size + (filter_size - 1) * (dilation - 1)
    out = {"same": input_length, "causal": input_length, "valid": input_length - dilated + 1, "full": input_length + dilated - 1}[padding]
    return (out + stride - 1) // stride


def install_restated_symbols():
    import make_golden_edcn as GE
    GE.install_restated_symbols()
    tf = sys.modules["tensorflow"]
    tf.nn.top_k, tf.unstack = top_k, unstack
    layers = sys.modules["tensorflow.keras.layers"]
    layers.Conv2D, layers.MaxPooling2D = Conv2D, MaxPooling2D
    S._mod("tensorflow.python.layers.utils").conv_output_length = conv_output_length
    inter = importlib.import_module("deepctr.layers.interaction")
    inter.Conv2D, inter.MaxPooling2D = Conv2D, MaxPooling2D
    inter.utils.conv_output_length = conv_output_length
    importlib.import_module("deepctr.models.ccpm").Conv2D = Conv2D
    importlib.import_module("deepctr.models.fgcnn").Lambda = ListLambda


def weight_hook(layer, wname, default):
    if isinstance(layer, Conv2D):
        rng = np.random.RandomState(G._seed(layer.name, str(wname), "fieldconv"))
        if str(wname) == "bias":
            return 0.2 * rng.standard_normal(default.shape)
        return rng.standard_normal(default.shape) / np.sqrt(default.shape[2])
    return G.weight_hook(layer, wname, default)


def spec_for(F, E=4, hash_flag=False, seq=False, dense=False):
    sp = lambda n, v, **kw: dict(type="sparse", name=n, vocabulary_size=v, embedding_dim=E, **kw)   # noqa: E731
    spec = [sp("C%d" % i, 7 + 2 * i, use_hash=hash_flag) for i in range(F - (1 if seq else 0))]
    if seq:
        spec.append(dict(type="varlen", sparsefeat=sp("hist", 9), maxlen=4, combiner="mean"))
    if dense:
        spec.append(dict(type="dense", name="price", dimension=1))
    return spec


def conditions(name, g):
    """The fixture conditions from the float64 oracle alone; returns the report line."""
    from tests import ref_fieldconv as RF
    meta = json.loads(bytes(g["meta"]).decode())
    stats = []
    base = RF.run_fixture(g, np.float64, task="regression", stats=stats).reshape(-1)
    tol = 1e-4 * np.abs(base).max()
    moved = {}
    for m in RF.applicable(meta):
        moved[m] = np.abs(RF.run_fixture(g, np.float64, task="regression", mutate=(m,)).reshape(-1) - base).max() / tol
        assert moved[m] >= 100, (name, m, moved[m])
    share = float((np.concatenate(stats) < 3).mean()) if stats else None
    assert share is None or share >= 0.9, (name, share)
    y = g["y"].reshape(-1)
    rng = "(logits)      " if meta["kwargs"].get("task") == "regression" else "%.3f .. %.3f" % (y.min(), y.max())
    line = "    %-24s %s   moved x tol: %s   |z| < 3: %s" % (
        name, rng, "  ".join("%s %s" % (m, "%5.0f" % moved[m] if m in moved else "    -") for m in RF.MUTATIONS),
        "%.3f" % share if share is not None else "-")
    print(line)
    return line


def run_model(name, ctor, spec, feed, kwargs):
    from tests import ref_fieldconv as RF
    S.reset()
    S.set_feed(feed)
    mod = importlib.import_module("deepctr.models." + ctor.lower())
    model = getattr(mod, ctor)(G.build_ref_columns(spec), G.build_ref_columns(spec), **kwargs)
    y = model.predict()
    arrays = {"y": y.astype(np.float32)}
    for k, v in feed.items():
        arrays["feed/" + k] = v
    for k, v in G._weights_dict().items():
        arrays["w/" + k] = v
    meta = {"model": ctor, "linear": spec, "dnn": spec, "kwargs": kwargs, "extra_args": []}
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    ref = RF.run_fixture(arrays, np.float64)
    err = np.abs(ref.reshape(-1) - arrays["y"].reshape(-1)).max()
    assert err < 1e-5, (name, err)
    line = conditions(name, arrays)
    G._save(name, **arrays)
    return line


def gen_models():
    rng = np.random.RandomState(SEED)
    B = 32
    feeds = {}

    def fd(key, **kw):
        if key not in feeds:
            spec = spec_for(**kw)
            feeds[key] = (spec, G._feed_for(spec, B, rng))
        return feeds[key]
    f7, f5, f6 = fd("f7", F=7), fd("f5", F=5), fd("f6", F=6)
    fh, fs, fsd = fd("hash", F=7, hash_flag=True), fd("seq", F=7, seq=True), fd("seqdense", F=7, seq=True, dense=True)
    dnn = {"dnn_hidden_units": [16, 8]}
    ccpm = [("default", f7, {}), ("l3", f5, {"conv_kernel_width": [6, 5, 3], "conv_filters": [4, 3, 2]}),
            ("noconv", f7, {"conv_kernel_width": [], "conv_filters": []}), ("hash", fh, {}), ("seq", fs, {}),
            ("regression", f7, {"task": "regression"}), ("nodnn", f7, {"dnn_hidden_units": []})]
    two = {"conv_kernel_width": [7, 7], "conv_filters": [14, 16], "new_maps": [3, 3], "pooling_width": [2, 2]}
    fgcnn = [("l2", f7, two),
             ("pool3", f7, {"conv_kernel_width": [4, 2], "conv_filters": [5, 6], "new_maps": [2, 2], "pooling_width": [3, 2]}),
             ("maps", f6, {"conv_kernel_width": [4, 3], "conv_filters": [3, 4], "new_maps": [1, 3], "pooling_width": [2, 2]}),
             ("noconv", f7, {"conv_kernel_width": [], "conv_filters": [], "new_maps": [], "pooling_width": []}),
             ("hash", fh, two), ("seq", fsd, two), ("regression", f7, dict(two, task="regression"))]
    lines = [run_model("model_ccpm_" + tag, "CCPM", sp, feed, dict(dnn, **kw)) for tag, (sp, feed), kw in ccpm]
    lines += [run_model("model_fgcnn_" + tag, "FGCNN", sp, feed, dict(dnn, **kw)) for tag, (sp, feed), kw in fgcnn]
    return lines


FGCNN_LAYER_CASES = [  # tag, (B, F, E), filters, kernel_width, new_maps, pooling_width
    ("odd", (32, 7, 4), (3, 4), (7, 3), (2, 1), (2, 2)),
    ("even", (32, 8, 3), (17, 2), (6, 4), (1, 2), (2, 3)),
    ("one", (32, 5, 5), (4,), (2,), (3,), (1,)),
]


def gen_layers():
    from deepctr.layers.interaction import FGCNNLayer
    from deepctr.layers.sequence import KMaxPooling
    from tests import ref_fieldconv as RF
    rng = np.random.RandomState(SEED + 1)
    arrays = {}
    for tag, shape in (("d3", (32, 7, 5)), ("d4", (32, 5, 3, 4))):
        x = rng.standard_normal(shape).astype(np.float32)
        x[0].reshape(-1)[:4] = x[0].reshape(-1)[4]              # repeated values
        arrays[tag + "/x"] = x
        for axis in range(1, len(shape)):
            for k in sorted(set((1, min(3, shape[axis]), shape[axis]))):
                S.reset()
                y = arr(KMaxPooling(k=k, axis=axis)(G.T(x)))
                assert np.array_equal(y, RF.kmax(x, k, axis)), (tag, axis, k)
                arrays["%s/axis%d/k%d" % (tag, axis, k)] = y.astype(np.float32)
    G._save("kmax_layer", **arrays)
    arrays = {}
    for tag, shape, filters, widths, new, pool in FGCNN_LAYER_CASES:
        S.reset()
        x = (0.5 * rng.standard_normal(shape)).astype(np.float32)
        y = arr(FGCNNLayer(filters, widths, new, pool)(G.T(x)))
        w = G._weights_dict()
        ref = RF.fgcnn_layer(x, w, filters, widths, new, pool)
        assert np.abs(ref - y).max() < 1e-5, (tag, np.abs(ref - y).max())
        cfg = dict(filters=filters, kernel_width=widths, new_maps=new, pooling_width=pool)
        arrays.update({tag + "/x": x, tag + "/y": y.astype(np.float32), tag + "/cfg": np.frombuffer(json.dumps(cfg).encode(), dtype=np.uint8)})
        for name, v in w.items():
            arrays["%s/w/%s" % (tag, name)] = v
    G._save("fgcnn_layer", **arrays)


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
