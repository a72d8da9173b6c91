"""Generates the DIEN fixtures tests/golden/model_dien_*.npz and gru_layer.npz on the oracle's TensorFlow shim, with the oracle's
deterministic weights (oracle/make_golden.py).  CPU only; needs the reference checkout, so it is not part of the suite:

    python scripts/make_golden_dien.py [--out DIR]

Run it into a scratch directory and compare with the committed files to check that the recipe has not rotted (a second run gives the
same bytes).

WHAT IS THE REFERENCE'S CODE HERE, imported in place from the checkout and never copied: ``DIEN``, ``interest_evolution`` and
``auxiliary_loss`` (deepctr/models/sequence/dien.py), ``DynamicGRU`` and ``AttentionSequencePoolingLayer`` (layers/sequence.py), ``DNN``,
``LocalActivationUnit``, ``Dice``, the embedding plumbing, and the attention-gated cells ``QAAttGRUCell`` (AGRU) and ``VecAttGRUCell``
(AUGRU) with their ``_Linear_`` of deepctr/contrib/utils.py: the shim's stub of that module is replaced by the real file.

WHAT IS RESTATED, from the TensorFlow documentation and not from its code (the precedent of
scripts/make_golden_bst.py), installed after the shim:
  * the ``tensorflow.python.ops`` symbols contrib/utils.py touches: ``math_ops.sigmoid / tanh / matmul``, ``array_ops.concat / split``,
    ``nn_ops.bias_add``, ``init_ops.constant_initializer``, ``variable_scope.variable_scope / get_variable_scope / get_variable`` (a stack
    of scope names; a variable is created once per full name, on the keras layer whose name opens the scope, with get_variable's documented
    default initialiser glorot_uniform), the ``RNNCell`` base (state_size / output_size, nothing else), ``util.nest.is_sequence``;
  * ``tf.nn.rnn_cell.GRUCell`` as documented: scope ``gru_cell``, ``gates/kernel`` [input + units, 2 units] with bias 1, gate order r then
    u, ``candidate/kernel`` [input + units, units] with bias 0, c = tanh([x | r * h] Wc + bc), h' = u h + (1 - u) c;
  * ``dynamic_rnn``: the vendored loop (contrib/rnn_v2.py, 1,450 lines of TF-private control flow; the shim stubs it to None) is replaced by
    the documented ``sequence_length`` semantics — h_0 = 0; at t >= length the state is copied through and the emitted row is zero; the
    returned state is the state at min(length, T); ``att_scores`` [B, T, 1] hands the cell its step's [B, 1] column;
  * ``TensorShape.ndims`` (the rank), ``tf.shape``, ``tf.subtract``, ``tf.log``, the keras layers ``Permute`` and ``multiply``, ``Model.add_loss`` (keeps the value), and
    ``tf.keras.backend.get_session`` raising AttributeError so that dien.py takes its ``tf.compat.v1`` branch, whose three calls do nothing.
So the cells' arithmetic, the attention, the auxiliary loss and the model wiring carry the reference's authority; the time loop's length
rule and tf's plain GRUCell carry the documentation's, and tests/ref_dien.py, written from the equations, is their independent check.

Weights: the oracle's hook, except the GRU biases: gate bias 1 + 0.3 N, candidate bias 0.3 N (dropping either is visible).

Model fixtures (B = 32, T = 6; item width 8, cate width 4 -> E = 12; seq_length holds T, 0, 1, T + 3 in its first four rows): each of
the four gru_types, AUGRU with att_weight_normalization=False, hashed columns, use_bn, regression, one history feature (E = 8), an extra
pooled sequence plus a DenseFeat, and use_negsampling=True (predictions and alpha x the auxiliary loss).
Layer fixture gru_layer.npz (B = 6, T = 5, E = 8, lengths 0, 1, T, T + 3, 2, 4): every cell kind with return_sequence on and off, and
the plain cell over an input scaled by the scores (AIGRU's multiply).

Conditions, printed by this script and asserted by tests/test_dien_cpu.py from the float64 oracle alone: binary probabilities inside
(1e-3, 1 - 1e-3); >= 90 % of the evolution GRU's final-state entries with |h| in (1e-3, 0.999); for every attention-gated fixture another
cell kind moves the logits by >= 100 x 1e-4 of their largest, and (AGRU aside: there the attention's own length mask makes a = 0, h' = h)
so does ignoring seq_length on the rows shorter than T."""
import contextlib
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import make_golden as G  # noqa: E402
from oracle import tf_shim as S  # noqa: E402

SEED = 71
T = 6


def arr(x):
    return np.asarray(S._arr(x))


# ---- variable scopes -------------------------------------------------------------------------------------------------------------
class _Scope(object):
    def __init__(self, name):
        self.name = name

    def set_partitioner(self, _):
        pass


_SCOPES = [_Scope("")]
_VARIABLES = {}


@contextlib.contextmanager
def variable_scope(name_or_scope, *a, **kw):
    if isinstance(name_or_scope, _Scope):
        scope = _Scope(name_or_scope.name)
    else:
        cur = _SCOPES[-1].name
        scope = _Scope(cur + "/" + str(name_or_scope) if cur else str(name_or_scope))
    _SCOPES.append(scope)
    try:
        yield scope
    finally:
        _SCOPES.pop()


def get_variable(name, shape=None, dtype=None, initializer=None, **kw):
    full = _SCOPES[-1].name + "/" + name
    if full not in _VARIABLES:
        owner, rest = full.split("/", 1)
        _VARIABLES[full] = S.layer_by_name(owner).add_weight(name=rest, shape=tuple(int(s) for s in shape), initializer=initializer)
    return _VARIABLES[full]


class RNNCell(object):
    def __init__(self, _reuse=None, **kw):
        pass


class GRUCell(RNNCell):
    """tf.nn.rnn_cell.GRUCell as documented (see the module docstring)."""

    def __init__(self, num_units, **kw):
        super(GRUCell, self).__init__()
        self._num_units = num_units

    @property
    def state_size(self):
        return self._num_units

    @property
    def output_size(self):
        return self._num_units

    def __call__(self, inputs, state):
        x, h = arr(inputs), arr(state)
        n, d = self._num_units, x.shape[1]
        with variable_scope("gru_cell"):
            with variable_scope("gates"):
                wg = arr(get_variable("kernel", [d + n, 2 * n]))
                bg = arr(get_variable("bias", [2 * n], initializer=S.Constant(1.0)))
            with variable_scope("candidate"):
                wc = arr(get_variable("kernel", [d + n, n]))
                bc = arr(get_variable("bias", [n], initializer=S.Constant(0.0)))
        ru = arr(S.sigmoid(S.Tensor(np.concatenate([x, h], axis=1) @ wg + bg)))
        r, u = ru[:, :n], ru[:, n:]
        c = np.tanh(np.concatenate([x, r * h], axis=1) @ wc + bc)
        new_h = S.Tensor((u * h + (1 - u) * c).astype(np.float32))
        return new_h, new_h


def dynamic_rnn(cell, inputs, att_scores=None, sequence_length=None, dtype=None, scope=None, **kw):
    """The documented sequence_length semantics (see the module docstring)."""
    x = arr(inputs)
    B, steps, _ = x.shape
    lens = arr(sequence_length).reshape(-1)
    att = None if att_scores is None else arr(att_scores).reshape(B, steps, 1)
    h = np.zeros((B, cell.state_size), np.float32)
    rows = []
    with variable_scope(scope):
        for t in range(steps):
            args = (S.Tensor(x[:, t]), S.Tensor(h)) + (() if att is None else (S.Tensor(att[:, t]),))
            out, new_h = cell(*args)
            live = (t < lens)[:, None]
            rows.append(np.where(live, arr(out), 0).astype(np.float32))
            h = np.where(live, arr(new_h), h).astype(np.float32)
    return S.Tensor(np.stack(rows, axis=1)), S.Tensor(h)


class Permute(S.Layer):
    def __init__(self, dims, **kw):
        super(Permute, self).__init__(**kw)
        self.dims = tuple(dims)

    def call(self, inputs, **kw):
        return S.Tensor(np.transpose(arr(inputs), (0,) + self.dims))


def install_restated_symbols():
    tf = sys.modules["tensorflow"]
    tf.shape = lambda x: tuple(int(v) for v in arr(x).shape)
    tf.subtract = lambda x, y: S.Tensor(arr(x) - arr(y))
    tf.log = lambda x: S.Tensor(np.log(arr(x)))
    layers = sys.modules["tensorflow.keras.layers"]
    layers.Permute = Permute
    layers.multiply = lambda inputs: S.Tensor(arr(inputs[0]) * arr(inputs[1]))
    S.Model.add_loss = lambda self, value: setattr(self, "added_loss", float(arr(value)))
    S.TensorShape.ndims = property(len)

    def no_session():
        raise AttributeError("get_session")
    sys.modules["tensorflow.keras.backend"].get_session = no_session

    class _Session(object):
        def run(self, *a, **kw):
            return None
    v1 = S._mod("tensorflow.compat.v1")
    S._mod("tensorflow.compat").v1 = v1
    tf.compat = sys.modules["tensorflow.compat"]
    S._mod("tensorflow.compat.v1.keras.backend").get_session = lambda: _Session()
    v1.keras = S._mod("tensorflow.compat.v1.keras")
    v1.keras.backend = sys.modules["tensorflow.compat.v1.keras.backend"]
    v1.global_variables_initializer = lambda: None
    S._mod("tensorflow.compat.v1.experimental").output_all_intermediates = lambda flag: None
    v1.experimental = sys.modules["tensorflow.compat.v1.experimental"]
    v1.log = tf.log

    m = S._mod("tensorflow.python.ops.math_ops")
    m.sigmoid, m.tanh, m.matmul = S.sigmoid, S._tanh, S.matmul
    m = S._mod("tensorflow.python.ops.array_ops")
    m.concat = S.concat
    m.split = lambda value, num_or_size_splits, axis=0: S.split(value, num_or_size_splits, axis)
    S._mod("tensorflow.python.ops.nn_ops").bias_add = S._bias_add
    S._mod("tensorflow.python.ops.init_ops").constant_initializer = lambda value=0, dtype=None: S.Constant(value)
    m = S._mod("tensorflow.python.ops.variable_scope")
    m.variable_scope, m.get_variable, m.get_variable_scope = variable_scope, get_variable, lambda: _SCOPES[-1]
    m = S._mod("tensorflow.python.ops.rnn_cell")
    m.RNNCell, m.GRUCell = RNNCell, GRUCell
    m.__all__ = ["RNNCell", "GRUCell"]
    S._mod("tensorflow.python.util.nest").is_sequence = lambda x: isinstance(x, (list, tuple))
    sys.modules["tensorflow.python.ops.rnn_cell_impl"] = None          # contrib/utils.py then takes its own _Linear_
    S._mod("tensorflow.nn.rnn_cell").GRUCell = GRUCell
    sys.modules["tensorflow.nn"].rnn_cell = sys.modules["tensorflow.nn.rnn_cell"]
    # the reference's cells from its own file, and the restated loop, where layers/sequence.py looks for them
    sys.modules.pop("deepctr.contrib.utils", None)
    utils = importlib.import_module("deepctr.contrib.utils")
    setattr(sys.modules["deepctr.contrib"], "utils", utils)
    for sub in ("rnn", "rnn_v2"):
        sys.modules["deepctr.contrib." + sub].dynamic_rnn = dynamic_rnn
    seq = importlib.import_module("deepctr.layers.sequence")
    seq.dynamic_rnn, seq.QAAttGRUCell, seq.VecAttGRUCell = dynamic_rnn, utils.QAAttGRUCell, utils.VecAttGRUCell


def weight_hook(layer, wname, default):
    w = str(wname)
    if w.endswith("gates/bias") or w.endswith("candidate/bias"):
        rng = np.random.RandomState(G._seed(layer.name, w, "dien"))
        return default + 0.3 * rng.standard_normal(default.shape)
    return G.weight_hook(layer, wname, default)


def reset():
    S.reset()
    _VARIABLES.clear()
    del _SCOPES[1:]


def dien_spec(hash_flag=False, one=False, extra=False, neg=False, item_v=40, cate_v=9, Eu=6, Ei=8, Ec=4):
    sp = lambda n, v, e, **kw: dict(type="sparse", name=n, vocabulary_size=v, embedding_dim=e, use_hash=hash_flag, **kw)   # noqa: E731
    vl = lambda n, v, e, emb: dict(type="varlen", sparsefeat=sp(n, v, e, embedding_name=emb), maxlen=T, length_name="seq_length")   # noqa: E731
    spec = [sp("user", 5, Eu), sp("item_id", item_v, Ei), sp("cate_id", cate_v, Ec), vl("hist_item_id", item_v, Ei, "item_id")]
    if not one:
        spec.append(vl("hist_cate_id", cate_v, Ec, "cate_id"))
    if neg:
        spec += [vl("neg_hist_item_id", item_v, Ei, "item_id"), vl("neg_hist_cate_id", cate_v, Ec, "cate_id")]
    if extra:
        # (with a length input: DIEN builds its embeddings with seq_mask_zero=False, so a pooled sequence has no mask to pool by)
        spec.append(dict(type="varlen", sparsefeat=sp("other_seq", 11, 6), maxlen=4, combiner="mean", length_name="other_len"))
        spec.append(dict(type="dense", name="pay_score", dimension=1))
    return spec


def feed_for(spec, B, rng):
    feed = G._feed_for(spec, B, rng)
    lens = rng.randint(0, T + 1, size=B).astype(np.int32)
    lens[:4] = (T, 0, 1, T + 3)
    feed["seq_length"] = lens
    if any(d.get("length_name") == "other_len" for d in spec):
        feed["other_len"] = rng.randint(1, 5, size=B).astype(np.int32)
    for d in spec:
        if d["type"] == "varlen" and d.get("length_name") == "seq_length":
            name = d["sparsefeat"]["name"]
            hi = 10 ** 6 if d["sparsefeat"].get("use_hash") else d["sparsefeat"]["vocabulary_size"]
            ids = rng.randint(1, hi, size=(B, T)).astype(np.int32)
            ids[np.arange(T)[None, :] >= lens[:, None]] = 0          # zero-padded tail: still looked up (row 0)
            feed[name] = ids
    for name in ("item_id", "cate_id"):
        hi = 10 ** 6 if spec[1].get("use_hash") else next(d for d in spec if d.get("name") == name)["vocabulary_size"]
        feed[name] = rng.randint(1, hi, size=B).astype(np.int32)
    return feed


def run_model(name, spec, hist, feed, kwargs):
    from deepctr.models.sequence.dien import DIEN
    reset()
    S.set_feed(feed)
    model = DIEN(G.build_ref_columns(spec), hist, **kwargs)
    y = model.predict()
    arrays = {"y": y.astype(np.float32)}
    if kwargs.get("use_negsampling"):
        arrays["aux_loss"] = np.float32(model.added_loss)
    for k, v in feed.items():
        arrays["feed/" + k] = v
    for k, v in G._weights_dict().items():
        arrays["w/" + k] = v
    meta = {"model": "DIEN", "linear": [], "dnn": spec, "kwargs": kwargs, "extra_args": [list(hist)]}
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    G._save(name, **arrays)


def gen_models():
    rng = np.random.RandomState(SEED)
    B = 32
    spec = dien_spec()
    feed = feed_for(spec, B, rng)
    spec_h = dien_spec(hash_flag=True)
    feed_h = feed_for(spec_h, B, rng)
    spec_1 = dien_spec(one=True)
    feed_1 = feed_for(spec_1, B, rng)
    spec_x = dien_spec(extra=True)
    feed_x = feed_for(spec_x, B, rng)
    spec_n = dien_spec(neg=True)
    feed_n = feed_for(spec_n, B, rng)
    both = ["item_id", "cate_id"]
    base = {"gru_type": "GRU", "dnn_hidden_units": [16, 8], "att_hidden_units": [16, 8]}
    runs = [("gru", spec, both, feed, {}), ("aigru", spec, both, feed, {"gru_type": "AIGRU"}), ("agru", spec, both, feed, {"gru_type": "AGRU"}),
            ("augru", spec, both, feed, {"gru_type": "AUGRU"}),
            ("augru_nonorm", spec, both, feed, {"gru_type": "AUGRU", "att_weight_normalization": False}),
            ("hash", spec_h, both, feed_h, {"gru_type": "AUGRU"}), ("bn", spec, both, feed, {"gru_type": "AGRU", "use_bn": True}),
            ("regression", spec, both, feed, {"gru_type": "AIGRU", "task": "regression"}), ("one", spec_1, ["item_id"], feed_1, {}),
            ("extra", spec_x, both, feed_x, {"gru_type": "AUGRU"}),
            ("neg", spec_n, both, feed_n, {"gru_type": "AUGRU", "use_negsampling": True, "alpha": 0.5})]
    names = []
    for suffix, sp, hist, fd, kw in runs:
        run_model("model_dien_" + suffix, sp, hist, fd, dict(base, **kw))
        names.append("model_dien_" + suffix)
    return names


LAYER_CASES = [  # tag, gru_type, return_sequence, input scaled by the scores
    ("gru_seq", "GRU", True, False), ("gru_last", "GRU", False, False), ("agru_seq", "AGRU", True, False), ("agru_last", "AGRU", False, False),
    ("augru_seq", "AUGRU", True, False), ("augru_last", "AUGRU", False, False), ("scaled_seq", "GRU", True, True),
    ("scaled_last", "GRU", False, True),
]


def gen_layers():
    from deepctr.layers.sequence import DynamicGRU
    rng = np.random.RandomState(SEED + 1)
    B, Tl, E = 6, 5, 8
    arrays = {}
    for tag, gru_type, rs, scaled in LAYER_CASES:
        reset()
        x = rng.standard_normal((B, Tl, E)).astype(np.float32)
        att = rng.rand(B, Tl, 1).astype(np.float32)
        lens = np.array([0, 1, Tl, Tl + 3, 2, 4], dtype=np.int32)
        layer = DynamicGRU(None, gru_type=gru_type, return_sequence=rs, name="gru")
        xin = x * att if scaled else x
        inputs = [G.T(xin), G.T(lens[:, None])] + ([G.T(att)] if gru_type in ("AGRU", "AUGRU") else [])
        y = layer(inputs)
        cfg = dict(gru_type=gru_type, return_sequence=rs, scale_input=scaled)
        arrays.update({tag + "/x": x, tag + "/att": att, tag + "/lengths": lens, tag + "/y": np.asarray(arr(y), dtype=np.float32),
                       tag + "/cfg": np.frombuffer(json.dumps(cfg).encode(), dtype=np.uint8)})
        for name, v in G._weights_dict().items():
            arrays["%s/w/%s" % (tag, name)] = v
    G._save("gru_layer", **arrays)


def report(name):
    from tests import ref_dien as RD
    g = dict(np.load(os.path.join(G.OUT, name + ".npz")))
    stats = []
    ref = RD.run_fixture(g, np.float64, stats=stats)
    assert np.abs(ref.reshape(-1) - g["y"].reshape(-1)).max() < 1e-5, name
    meta = json.loads(bytes(g["meta"]).decode())
    stats = np.asarray(stats)
    y = g["y"].reshape(-1)
    rng = "(logits)      " if meta["kwargs"].get("task") == "regression" else "%.3f .. %.3f" % (y.min(), y.max())
    print("    %-26s %s   |h| in (1e-3, 0.999): %.3f" % (name, rng, ((stats > 1e-3) & (stats < 0.999)).mean()))


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


if __name__ == "__main__":
    sys.exit(main())
