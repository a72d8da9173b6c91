"""Bits of the row-chained kernel's layer epilogues (csrc/chain_device.h: act_block, the bias quads of the accumulators, the head)
against the 32-row tile kernel, with pre-activations that are EXACT and sit on the awkward values: the DNN kernels are zero, so a
layer's pre-activation is its bias, and the biases cycle through -1, -0.0, +0.0, 1e-39, 1, -1e-39 (signed zeros, fp32 denormals of
both signs).  ReLU is one v_max_f32 against the constant 0 there and a linear DNN branches around the epilogue; the biases lie in LDS
in accumulator order.  None of that may move a bit.

Everything else of the model is chosen so that every sum is exact in fp32 in ANY order (the two kernels add in different orders):
embeddings, linear weights and dense values are small multiples of 1/8, the head weights are 1, 2, 4 — a partial sum is then
either an exact dyadic number (a denormal term added to it rounds away, whichever side comes first) or a sum of denormals alone (fixed
point, exact), and the head's total is non-zero, so the output does not depend on the order.  The `tiny` model keeps only the
denormal and zero biases in its last layer and is a regression model with every other term zero: its output IS the head's sum of
denormals, so a flushed denormal or a wrong zero is visible in the output itself.

Shapes: the forced 256-row shape on one ragged launch (main phase code), 64 rows per CU + 37 (tail phase only), 256 + 64 rows per CU + 5
(both phases of one launch).  F = 3 fields: an odd count (the last id pair is half empty); one dense column (a K tail in layer 0).
The two-layer instantiations (M2 = 0) are reached with units (256, 64) on the same three fields and with (128, 64) on 13 fields: a model
whose widest layer is 128 is only fused (models/_common.py: _init_fused — the gather's partial sums alias an LDS tile of that width)
from a DNN input of 193 columns on, and an unfused model never reaches the row-chained kernel."""
import numpy as np
import pytest
import torch

from oracle import ref_models as RM
from tests.test_gpu_models import _randomise, check_probs
from tests.util import assert_close

pytestmark = pytest.mark.gpu

ND, E, V = 1, 16, 50
MODELS = [((256, 128, 64), 3), ((256, 64), 3), ((128, 64), 13)]      # (DNN units, fields)
BIAS_CYCLE = np.array([-1.0, -0.0, 0.0, 1e-39, 1.0, -1e-39], dtype=np.float32)
TINY_CYCLE = np.array([-0.0, 1e-39, 0.0, -1e-39, 1e-39, 1e-39], dtype=np.float32)      # (more + than -: a linear head's sum is not 0)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _shapes():
    cus = _cus()
    return [("forced 256", 256 + 37, 256), ("tail only", 64 * cus + 37, 0), ("both phases", 256 * cus + 64 * cus + 5, 0)]


def _last_kernel():
    from deepctr_amd import _C
    return {0: "tile", 1: "stream", 2: "chain", -1: None}[_C.lib().dctr_embed_mlp_fwd_last_kernel()]


def _predict(model, feed, batch_size, **attrs):
    old = {k: getattr(model, k) for k in attrs}
    for k, v in attrs.items():
        setattr(model, k, v)
    try:
        return model.predict(feed, batch_size=batch_size)
    finally:
        for k, v in old.items():
            setattr(model, k, v)


def _cols_feed(rng, n, F):
    from deepctr_amd.feature_column import DenseFeat, SparseFeat
    cols = [SparseFeat("C%d" % i, V, E) for i in range(1, F + 1)] + [DenseFeat("I%d" % i, 1) for i in range(1, ND + 1)]
    feed = {"C%d" % i: rng.randint(0, V, n).astype(np.int32) for i in range(1, F + 1)}
    feed.update({"I%d" % i: (rng.randint(0, 9, n) / 8.0).astype(np.float32) for i in range(1, ND + 1)})
    return cols, feed


def _exact_weights(model, rng, tiny):
    """Zero DNN kernels, cycling biases, dyadic everything else (module docstring)."""
    w = {}
    unit = 0
    names = list(model.get_weights_by_name().items())
    last_bias = [k for k, _ in names if k.startswith("dnn/bias")][-1]
    for k, v in names:
        if k.startswith("dnn/kernel"):
            w[k] = np.zeros(v.shape, np.float32)
        elif k.startswith("dnn/bias"):
            cyc = TINY_CYCLE if (tiny and k == last_bias) else BIAS_CYCLE
            w[k] = cyc[(unit + np.arange(v.shape[0])) % 6].astype(np.float32)
            unit += v.shape[0]
        elif k == "dense/kernel":
            w[k] = (2.0 ** (np.arange(v.shape[0]) % 3)).astype(np.float32).reshape(v.shape)      # (1, 2, 4: a denormal times one is exact)
        elif tiny:
            w[k] = np.zeros(v.shape, np.float32)      # embeddings, linear weights, global bias: the output is the head's sum alone
        else:
            w[k] = (rng.randint(-8, 9, v.shape) / 8.0).astype(np.float32)
    assert set(w) == {k for k, _ in names}
    model.set_weights_by_name(w)
    return w


@pytest.fixture(scope="module")
def data():
    """F -> the columns and the id / dense values of the largest shape, drawn once; the smaller shapes take its first rows."""
    n = max(s[1] for s in _shapes())
    return {F: _cols_feed(np.random.RandomState(61 + F), n, F) for F in sorted({f for _, f in MODELS})}


@pytest.mark.parametrize("act", ["relu", "linear"])
@pytest.mark.parametrize("units,F", MODELS)
def test_exact_preactivations_give_the_tile_kernels_bits(device, data, units, F, act):
    from deepctr_amd.models import DeepFM
    cols, feed_all = data[F]
    rng = np.random.RandomState(len(units) * 7 + len(act))
    model = DeepFM(cols, cols, dnn_hidden_units=units, dnn_activation=act, device=device)
    w = _exact_weights(model, rng, tiny=False)
    for what, n, tile_rows in _shapes():
        feed = {k: v[:n] for k, v in feed_all.items()}
        y = _predict(model, feed, n, tile_rows=tile_rows)
        assert _last_kernel() == "chain", what
        y32 = _predict(model, feed, n, tile_rows=32)
        assert _last_kernel() == "tile", what
        diff = int((y.view(np.uint32) != y32.view(np.uint32)).sum())
        print("%s %r %s: %d of %d rows differ from the tile kernel" % (act, units, what, diff, n))
        assert diff == 0, "%s %r %s: %d rows differ from the 32-row tile kernel" % (act, units, what, diff)
        rows = np.unique(np.concatenate([np.arange(0, min(n, 300)), np.arange(max(0, n - 300), n)]))
        ref = RM.deepfm(cols, cols, w, {k: v[rows] for k, v in feed.items()}, dnn_hidden_units=units, dnn_activation=act, dtype=np.float64)
        check_probs(y[rows], ref.astype(np.float32), "exact pre-activations, %s %r %s" % (act, units, what))


@pytest.mark.parametrize("act", ["relu", "linear"])
@pytest.mark.parametrize("units,F", MODELS)
def test_denormal_head_sum_is_the_output(device, data, units, F, act):
    """The `tiny` model: the output is sum_i head_w[i] * act(bias_last[i]) over denormals and zeros — exact, whatever the order."""
    from deepctr_amd.models import DeepFM
    cols, feed_all = data[F]
    model = DeepFM(cols, cols, dnn_hidden_units=units, dnn_activation=act, task="regression", device=device)
    w = _exact_weights(model, np.random.RandomState(5), tiny=True)
    b = w[[k for k in w if k.startswith("dnn/bias")][-1]].astype(np.float64)
    h = w["dense/kernel"].astype(np.float64).reshape(-1)
    want = np.float32((h * (np.maximum(b, 0.0) if act == "relu" else b)).sum())
    assert want != 0.0 and abs(float(want)) < 1e-36
    for what, n, tile_rows in _shapes():
        feed = {k: v[:n] for k, v in feed_all.items()}
        y = _predict(model, feed, n, tile_rows=tile_rows)
        assert _last_kernel() == "chain", what
        bad = int((y.view(np.uint32) != np.float32(want).view(np.uint32)).sum())
        print("%s %r %s: want %r, first output %r, %d of %d rows differ" % (act, units, what, want, y[0, 0], bad, n))
        assert bad == 0, "%s %r %s: %d rows are not %r (first: %r)" % (act, units, what, bad, want, y[0, 0])
        assert np.array_equal(_predict(model, feed, n, tile_rows=32).view(np.uint32), y.view(np.uint32)), what


@pytest.mark.parametrize("act", ["relu", "linear"])
@pytest.mark.parametrize("units,F", MODELS)
def test_random_weights_same_bits_in_every_phase(device, data, units, F, act):
    from deepctr_amd.models import DeepFM
    cols, feed_all = data[F]
    rng = np.random.RandomState(len(units) * 11 + len(act))
    model = DeepFM(cols, cols, dnn_hidden_units=units, dnn_activation=act, device=device)
    _randomise(model, rng)
    for what, n, tile_rows in _shapes():
        feed = {k: v[:n] for k, v in feed_all.items()}
        y = _predict(model, feed, n, tile_rows=tile_rows)
        assert _last_kernel() == "chain", what
        assert_close(y, _predict(model, feed, n, tile_rows=32), rtol=2e-6, atol=2e-7, what="chain vs 32-row kernel, %s %r %s" % (act, units, what))
        if tile_rows == 0:      # the rows of the main and tail phases against the forced 256-row shape
            assert np.array_equal(_predict(model, feed, n, tile_rows=256), y), "%s %r %s vs the forced 256-row shape" % (act, units, what)
