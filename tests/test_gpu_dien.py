"""GPU: dctr_gru_fwd (the whole GRU / AGRU / AUGRU time loop in one launch) against the float64 oracle (tests/ref_dien.py) over a sweep of
shapes, cells, flags, routes and lengths, its saturated values, DIEN and DynamicGRU against the reference's own outputs
(tests/golden/model_dien_*.npz, gru_layer.npz), DIEN's forward against the oracle over a seeded fuzz of configurations,
live weights, fit() on the autograd step and the reference's example program through the ``deepctr`` facade.

Tolerance: the attention stack's bar (``within_bar`` of tests/test_gpu_bst.py: |err| <= 1e-4 |ref| + 2e-6 max|ref of the sample|) against
the float64 oracle, and rtol 1e-4, atol 2e-5 on model logits as the BST fuzz uses.  The recurrence compounds rounding over T, so the bar
was first checked against the float32 NumPy restatement of the same loop (tests/test_dien_cpu.py
test_float32_restatement_against_float64_on_the_op_sweep): over this sweep's shapes and at T = 50 its error is at most 0.16 of the bar,
below the half that would have widened it, so the bar stands as it is.  The kernel's own error sets nothing."""
import numpy as np
import pytest
import torch

from tests import ref_dien as RD
from tests.test_gpu_bst import within_bar
from tests.util import assert_close

pytestmark = pytest.mark.gpu

DIEN_FIXTURES = ["model_dien_gru", "model_dien_aigru", "model_dien_agru", "model_dien_augru", "model_dien_augru_nonorm", "model_dien_hash",
                 "model_dien_bn", "model_dien_regression", "model_dien_one", "model_dien_extra", "model_dien_neg"]
LAYER_TAGS = ["gru_seq", "gru_last", "agru_seq", "agru_last", "augru_seq", "augru_last", "scaled_seq", "scaled_last"]
SWEEP_E = [4, 12, 16, 40, "streamed"]       # "streamed": the smallest E the library routes there (read from dctr_gru_route)
SWEEP_T = [1, 2, 6]
SWEEP_B = [1, 17, 33]


def make_layers(rng, E, L):
    """Gate / candidate kernels at a scale that keeps the gates off saturation, biases away from their initial (1, 0)."""
    s = 0.7 / np.sqrt(2 * E)
    return [((rng.standard_normal((2 * E, 2 * E)) * s).astype(np.float32), (1 + 0.3 * rng.standard_normal(2 * E)).astype(np.float32),
             (rng.standard_normal((2 * E, E)) * s * 1.5).astype(np.float32), (0.3 * rng.standard_normal(E)).astype(np.float32))
            for _ in range(L)]


def draw_lengths(rng, B, T):
    """<= 0, 1, T and T + 3 in the first rows; with more than one tile, every sample of the second tile has length 0."""
    base = np.array([T, -2, 0, 1, T + 3])
    lens = rng.randint(0, T + 4, size=B)
    n = min(B, base.size)
    lens[:n] = base[:n]
    if B > 16:
        lens[16:32] = 0
    return lens.astype(np.int32)


def smallest_streamed_dim(n_layers=1):
    from deepctr_amd import ops
    E = 1
    while ops.gru_route(6, E, n_layers) != "streamed":
        E += 1
        assert E < 4096
    return E


def to_dev(layers, device):
    return [tuple(torch.from_numpy(w).to(device) for w in layer) for layer in layers]


def sweep_variants():
    """(n_layers, cell, scale_input, return_sequence) of every run of a sweep case."""
    out = []
    for rs in (True, False):
        out += [(1, "GRU", False, rs), (2, "GRU", False, rs), (1, "AGRU", False, rs), (1, "AUGRU", False, rs), (1, "GRU", True, rs),
                (2, "GRU", True, rs)]
    return out


@pytest.mark.parametrize("E", SWEEP_E)
def test_gru_op_vs_float64_oracle(device, E):
    from deepctr_amd import ops
    if E == "streamed":
        E = smallest_streamed_dim()
        assert ops.gru_route(6, E - 1) == "resident"
    worst_all = 0.0
    for T in SWEEP_T:
        for B in SWEEP_B:
            rng = np.random.RandomState(E * 1000 + T * 10 + B)
            layers = make_layers(rng, E, 2)
            tl = to_dev(layers, device)
            lens = draw_lengths(rng, B, T)
            pad = 3
            xbuf = rng.standard_normal((B, T, E + pad)).astype(np.float32)        # padding columns after every step
            x = xbuf[:, :, :E]
            att = rng.rand(B, T).astype(np.float32)
            xt = torch.from_numpy(xbuf).to(device)[:, :, :E]
            lt, at = torch.from_numpy(lens).to(device), torch.from_numpy(att).to(device)
            for L, cell, scale, rs in sweep_variants():
                need_att = cell != "GRU" or scale
                got = ops.dynamic_gru(xt, lt, tl[:L], cell=cell, att_scores=at if need_att else None, scale_input=scale, return_sequence=rs)
                torch.cuda.synchronize()
                got = got.cpu().numpy()
                ref = RD.dynamic_gru(x, lens, layers[:L], cell, att if need_att else None, scale, rs)
                assert got.shape == ref.shape and np.isfinite(got).all()
                what = "E %d T %d B %d L %d %s scale %d seq %d" % (E, T, B, L, cell, scale, rs)
                dead = np.clip(lens, 0, T)
                if rs:          # rows past the length are exact zeros; samples of length <= 0 are all zero
                    assert not got[np.arange(T)[None, :] >= dead[:, None]].any(), what
                else:
                    assert not got[dead == 0].any(), what
                worst = within_bar(got, ref)
                worst_all = max(worst_all, worst)
                assert worst <= 1.0, "%s: max err / bar %.3g" % (what, worst)
    print("E %d (%s): max err / bar %.3g" % (E, ops.gru_route(6, E), worst_all))


def test_both_routes_and_the_workspace_route_agree_with_the_oracle(device):
    from deepctr_amd import ops
    rng = np.random.RandomState(21)
    T, E, B = 6, 16, 21
    for L in (1, 2):
        layers = make_layers(rng, E, L)
        x = rng.standard_normal((B, T, E)).astype(np.float32)
        lens = draw_lengths(rng, B, T)
        ref = RD.dynamic_gru(x, lens, layers)
        assert ops.gru_route(T, E, L, route="resident") == "resident" and ops.gru_route(T, E, L, route="streamed") == "streamed"
        outs = []
        for route in ("resident", "streamed"):
            got = ops.dynamic_gru(torch.from_numpy(x).to(device), torch.from_numpy(lens).to(device), to_dev(layers, device), route=route)
            outs.append(got.cpu().numpy())
            worst = within_bar(outs[-1], ref)
            assert worst <= 1.0, "%s route, %d layers: max err / bar %.3g" % (route, L, worst)
        assert np.array_equal(outs[0], outs[1]), "the two routes run the same step code in the same order"
    # past the LDS the tiles of a workgroup live in the workspace
    E = 16
    while ops.gru_workspace_bytes(3, 2, E) == 0:
        E += 8
        assert E < 4096
    assert ops.gru_route(2, E) == "streamed"
    B, T = 18, 2
    layers = make_layers(rng, E, 1)
    x = rng.standard_normal((B, T, E)).astype(np.float32)
    lens = draw_lengths(rng, B, T)
    att = rng.rand(B, T).astype(np.float32)
    got = ops.dynamic_gru(torch.from_numpy(x).to(device), torch.from_numpy(lens).to(device), to_dev(layers, device), cell="AUGRU",
                          att_scores=torch.from_numpy(att).to(device)).cpu().numpy()
    worst = within_bar(got, RD.dynamic_gru(x, lens, layers, "AUGRU", att))
    print("workspace route at E %d: max err / bar %.3g" % (E, worst))
    assert worst <= 1.0


def test_strided_outputs_leave_their_neighbours_alone(device):
    from deepctr_amd import ops
    rng = np.random.RandomState(22)
    T, E, B = 5, 12, 19
    layers = make_layers(rng, E, 1)
    x = rng.standard_normal((B, T, E)).astype(np.float32)
    lens = draw_lengths(rng, B, T)
    att = rng.rand(B, T).astype(np.float32)
    xt, lt, at, tl = torch.from_numpy(x).to(device), torch.from_numpy(lens).to(device), torch.from_numpy(att).to(device), to_dev(layers, device)
    # the final state straight into columns [7, 7 + E) of a wider buffer, as DIEN writes it into the DNN input
    wide = torch.full((B, 7 + E + 5), float("nan"), device=device)
    ops.dynamic_gru(xt, lt, tl, cell="AUGRU", att_scores=at, return_sequence=False, out=wide[:, 7:], out_stride=wide.stride(0))
    got = wide.cpu().numpy()
    assert np.isnan(got[:, :7]).all() and np.isnan(got[:, 7 + E:]).all()
    assert within_bar(got[:, 7:7 + E], RD.dynamic_gru(x, lens, layers, "AUGRU", att, return_sequence=False)) <= 1.0
    # the sequence into a buffer with padding after every step
    seq = torch.full((B, T, E + 3), float("nan"), device=device)
    ops.dynamic_gru(xt, lt, tl, out=seq[:, :, :E])
    got = seq.cpu().numpy()
    assert np.isnan(got[:, :, E:]).all()
    assert within_bar(got[:, :, :E], RD.dynamic_gru(x, lens, layers)) <= 1.0
    assert torch.equal(xt.cpu(), torch.from_numpy(x)), "the input was written"


def saturated_cases(sign):
    """(x, lens, att) and the (what, layers, cell) runs of the saturation test: zero kernels, so every pre-activation is its bias.  The
    candidate sits at 30 * sign.  Each sample holds units of every (r, u) saturation: r alternates in sign unit by unit and u pair by
    pair, and ``gate_sign`` flips them all.  A unit whose u is 1 keeps the zero initial state, where float64 leaves the 1e-13 residue
    of 1 - u and float32 (the reference's arithmetic) leaves 0; next to units of size 1 in the same sample the bar's
    2e-6 max|ref of the sample| covers that, where a sample of nothing but such units would be measured against the residue itself."""
    rng = np.random.RandomState(23)
    T, E, B = 4, 12, 5
    x = rng.standard_normal((B, T, E)).astype(np.float32)
    lens = np.array([T, 0, 1, T + 3, 2], dtype=np.int32)
    att = rng.rand(B, T).astype(np.float32)
    j = np.arange(E)
    flip = np.concatenate([np.where(j % 2 == 0, 1.0, -1.0), np.where(j % 4 < 2, 1.0, -1.0)])
    wg, wc = np.zeros((2 * E, 2 * E), np.float32), np.zeros((2 * E, E), np.float32)
    runs = []
    for gate_sign in (1.0, -1.0):
        layers = [(wg, (30 * gate_sign * flip).astype(np.float32), wc, np.full(E, 30 * sign, np.float32))]
        runs += [("+-30, gates %+d, %s" % (gate_sign, cell), layers, cell) for cell in RD.CELLS]
        # and far past every exponent range
        layers = [(wg, (200 * gate_sign * flip).astype(np.float32), wc, np.full(E, 200 * sign, np.float32))]
        runs.append(("+-200, gates %+d" % gate_sign, layers, "GRU"))
    return (x, lens, att), runs


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_saturated_gates_give_the_oracles_values_and_no_nan(device, sign):
    """Pre-activations of +-30 (zero kernels, biases of +-30): sigmoid and tanh saturate to 0 / 1 / -1 without an inf / inf.  The float32
    restatement is inside half the bar on the same runs (tests/test_dien_cpu.py
    test_float32_restatement_against_float64_on_the_saturated_runs)."""
    from deepctr_amd import ops
    (x, lens, att), runs = saturated_cases(sign)
    xt, lt, at = torch.from_numpy(x).to(device), torch.from_numpy(lens).to(device), torch.from_numpy(att).to(device)
    for what, layers, cell in runs:
        got = ops.dynamic_gru(xt, lt, to_dev(layers, device), cell=cell, att_scores=at).cpu().numpy()
        ref = RD.dynamic_gru(x, lens, layers, cell, att)
        assert np.isfinite(got).all(), what
        worst = within_bar(got, ref)
        print("%s: max err / bar %.3g" % (what, worst))
        assert worst <= 1.0, what
        if cell == "GRU":       # the units whose u is 0 hold the candidate's saturated value itself
            full = got[0, -1]
            assert np.abs(np.abs(full) - 1.0).min() < 1e-6 and np.abs(full).min() < 1e-6, what


def test_layer_api_and_live_weights(device):
    """DynamicGRU through the reference's call forms; a weight changed in place between two calls changes the output."""
    from deepctr_amd.layers import DynamicGRU
    rng = np.random.RandomState(24)
    B, T, E = 9, 5, 8
    x = rng.standard_normal((B, T, E)).astype(np.float32)
    lens = draw_lengths(rng, B, T)
    att = rng.rand(B, T, 1).astype(np.float32)
    xt, lt, at = torch.from_numpy(x).to(device), torch.from_numpy(lens.reshape(-1, 1)).to(device), torch.from_numpy(att).to(device)
    for gru_type, rs in (("GRU", True), ("AGRU", False), ("AUGRU", False), ("AUGRU", True)):
        layer = DynamicGRU(None, gru_type=gru_type, return_sequence=rs, device=device)
        inputs = [xt, lt] if gru_type == "GRU" else [xt, lt, at]
        y0 = layer(inputs).clone()
        assert tuple(y0.shape) == ((B, T, E) if rs else (B, 1, E)) and layer.num_units == E
        assert torch.equal(layer(inputs), y0)
        for w in layer.operands():
            with torch.no_grad():
                w.add_(0.05)
            y1 = layer(inputs).clone()
            assert not torch.equal(y1, y0)
            y0 = y1
        ref = RD.dynamic_gru(x, lens, [tuple(w.cpu().numpy() for w in layer.operands())], layer.cell,
                             None if gru_type == "GRU" else att, False, rs)
        assert within_bar(y0.cpu().numpy().reshape(ref.shape), ref) <= 1.0


@pytest.mark.parametrize("name", DIEN_FIXTURES)
def test_dien_matches_reference_code(device, name):
    """A model fixture: probabilities at three batch sizes and a list feed, the logits against the float64 oracle."""
    from tests.test_dien_cpu import build_dien, fixture_feed, fixture_weights
    from tests.test_gpu_models import check_probs
    from tests.util import golden_meta, load_golden
    g = load_golden(name)
    meta = golden_meta(g)
    model = build_dien(meta, device)
    model.set_weights_by_name(fixture_weights(g))
    feed = fixture_feed(g)
    assert (feed["seq_length"] == 0).any()                                  # length-0 rows are compared, not excluded
    rows = np.ones(g["y"].shape[0], bool)
    for bs in (256, 5, 37):
        check_probs(model.predict(feed, batch_size=bs), g["y"], "%s bs=%d" % (name, bs), rows)
    y = model.predict([feed[n] for n in model.input_names], batch_size=64)
    check_probs(y, g["y"], name + " list feed", rows)
    assert_close(np.asarray(model.predict_logits(feed, batch_size=256)).reshape(-1),
                 RD.run_fixture(g, np.float64, task="regression").reshape(-1), rtol=1e-4, atol=2e-5, what=name + " logits vs float64")


def test_dynamic_gru_layer_matches_reference_code(device):
    from deepctr_amd.layers import DynamicGRU
    from tests.test_dien_cpu import layer_case
    from tests.util import load_golden
    g = load_golden("gru_layer")
    for tag in LAYER_TAGS:
        cfg, x, att, lens, ws, y = layer_case(g, tag)
        layer = DynamicGRU(None, gru_type=cfg["gru_type"], return_sequence=cfg["return_sequence"], device=device)
        layer.build([(None,) + x.shape[1:], (None, 1)])
        layer.set_weights(list(ws))
        xin = x * att if cfg["scale_input"] else x
        inputs = [torch.from_numpy(xin).to(device), torch.from_numpy(lens.reshape(-1, 1)).to(device)]
        if cfg["gru_type"] != "GRU":
            inputs.append(torch.from_numpy(att).to(device))
        got = layer(inputs).cpu().numpy()
        assert got.shape == y.shape
        ref = RD.dynamic_gru(x, lens, [ws], cfg["gru_type"], att, cfg["scale_input"], cfg["return_sequence"]).reshape(y.shape)
        assert within_bar(got, ref) <= 1.0, tag
        assert within_bar(got, y.astype(np.float64)) <= 1.0, tag


def dien_problem(rng, n, n_hist=2, T=6, widths=(8, 4), hash_=False, extra_seq=False, dense=False, vocab=30, neg=False):
    from deepctr_amd.feature_column import DenseFeat, SparseFeat, VarLenSparseFeat
    names = ["item_id", "cate_id", "shop_id"][:n_hist]
    cols = [SparseFeat("user", 7, 4, use_hash=hash_)]
    cols += [SparseFeat(nm, vocab, w, use_hash=hash_) for nm, w in zip(names, widths)]
    cols += [VarLenSparseFeat(SparseFeat("hist_" + nm, vocab, w, embedding_name=nm, use_hash=hash_), T, length_name="seq_length")
             for nm, w in zip(names, widths)]
    hi = 10 ** 6 if hash_ else vocab
    feed = {"user": rng.randint(0, 10 ** 6 if hash_ else 7, n).astype(np.int32)}
    lens = rng.randint(0, T + 4, n).astype(np.int32)
    lens[:min(n, 4)] = np.array([T, 0, 1, T + 3])[:min(n, 4)]
    feed["seq_length"] = lens
    for nm in names:
        feed[nm] = rng.randint(1, hi, n).astype(np.int32)
        for prefix in ("hist_",) + (("neg_hist_",) if neg else ()):
            ids = rng.randint(1, hi, (n, T)).astype(np.int32)
            ids[np.arange(T)[None, :] >= lens[:, None]] = 0
            feed[prefix + nm] = ids
    if neg:
        cols += [VarLenSparseFeat(SparseFeat("neg_hist_" + nm, vocab, w, embedding_name=nm, use_hash=hash_), T, length_name="seq_length")
                 for nm, w in zip(names, widths)]
    if extra_seq:
        cols.append(VarLenSparseFeat(SparseFeat("other_seq", 11, 6), 4, combiner="mean"))
        ids = rng.randint(1, 11, (n, 4)).astype(np.int32)
        ol = rng.randint(1, 5, n)
        ids[np.arange(4)[None, :] >= ol[:, None]] = 0
        feed["other_seq"] = ids
    if dense:
        cols.append(DenseFeat("pay_score", 1))
        feed["pay_score"] = rng.rand(n).astype(np.float32)
    return cols, names, feed


def randomise(model, rng):
    """Trained-like weights: embeddings of order 0.3 so that the gates move, GRU biases away from (1, 0)."""
    new = {}
    for k, v in model.get_weights_by_name().items():
        draw = rng.standard_normal(v.shape)
        if k.endswith("embeddings"):
            a = 0.3 * draw
        elif k.endswith("gates/bias"):
            a = 1.0 + 0.3 * draw
        elif k.endswith("moving_variance"):
            a = rng.uniform(0.5, 1.5, v.shape)
        elif k.endswith("dice_alpha"):
            a = 0.25 * draw
        elif "bias" in k or k.endswith("beta") or k.endswith("moving_mean"):
            a = 0.1 * draw
        elif k.endswith("gamma"):
            a = 1.0 + 0.2 * draw
        else:
            a = draw * (v.std() if v.std() > 0 else 0.1)
        new[k] = a.astype(np.float32)
    model.set_weights_by_name(new)
    return new


@pytest.mark.parametrize("seed", range(20))
def test_fuzz_predict_logits_vs_oracle(device, seed):
    """Seeded random DIEN configurations against the float64 oracle: rtol 1e-4, atol 2e-5 on the logit, as the BST fuzz."""
    from deepctr_amd.models import DIEN
    rng = np.random.RandomState(4000 + seed)
    gru_type = ("GRU", "AIGRU", "AGRU", "AUGRU")[seed % 4]
    n_hist = int(rng.randint(1, 4))
    T = int(rng.randint(1, 13))
    widths = [int(rng.choice([2, 4, 6, 8])) for _ in range(n_hist)]
    hash_, use_bn = bool(rng.rand() < 0.3), bool(rng.rand() < 0.3)
    task = "regression" if rng.rand() < 0.25 else "binary"
    norm = bool(rng.rand() < 0.6)
    act = str(rng.choice(["dice", "sigmoid", "relu"]))
    neg = gru_type == "AUGRU" and bool(rng.rand() < 0.5)
    n = int(rng.randint(3, 200))
    cols, names, feed = dien_problem(rng, n, n_hist, T, widths, hash_, extra_seq=bool(rng.rand() < 0.5), dense=bool(rng.rand() < 0.5), neg=neg)
    kw = dict(gru_type=gru_type, use_negsampling=neg, use_bn=use_bn, dnn_hidden_units=(16, 8), att_hidden_units=(16, 8), att_activation=act,
              att_weight_normalization=norm, task=task)
    model = DIEN(cols, names, device=device, **kw)
    w = randomise(model, rng)
    what = "seed %d: %s hist=%d T=%d widths=%s hash=%d bn=%d norm=%d %s neg=%d %s n=%d" % (seed, gru_type, n_hist, T, widths, hash_, use_bn,
                                                                                      norm, act, neg, task, n)
    got = np.asarray(model.predict_logits(feed, batch_size=64)).reshape(-1)
    ref = RD.dien(cols, names, w, feed, **dict(kw, task="regression")).reshape(-1)
    assert np.isfinite(got).all()
    assert_close(got, ref, rtol=1e-4, atol=2e-5, what=what)
    if neg:         # predict ignores the neg_hist_* columns: the same answer without them
        slim = {k: v for k, v in feed.items() if not k.startswith("neg_")}
        assert np.array_equal(np.asarray(model.predict_logits(slim, batch_size=64)).reshape(-1), got)


def test_live_model_weights(device):
    from deepctr_amd.models import DIEN
    rng = np.random.RandomState(31)
    cols, names, feed = dien_problem(rng, 50)
    for gru_type in ("GRU", "AUGRU"):
        model = DIEN(cols, names, gru_type=gru_type, dnn_hidden_units=(16, 8), device=device)
        randomise(model, rng)
        y0 = np.asarray(model.predict(feed, batch_size=64)).copy()
        assert np.array_equal(np.asarray(model.predict(feed, batch_size=64)), y0)
        for layer in (model.gru1, model.gru2):
            for w in layer.operands():
                with torch.no_grad():
                    w.add_(0.05)
                y1 = np.asarray(model.predict(feed, batch_size=64)).copy()
                assert not np.array_equal(y1, y0), layer.name
                y0 = y1
        ref = RD.dien(cols, names, {k: np.asarray(v) for k, v in model.get_weights_by_name().items()}, feed, gru_type=gru_type,
                      dnn_hidden_units=(16, 8), task="regression").reshape(-1)
        assert_close(np.asarray(model.predict_logits(feed, batch_size=64)).reshape(-1), ref, rtol=1e-4, atol=2e-5, what="live " + gru_type)


@pytest.mark.parametrize("gru_type,neg", [("GRU", False), ("AIGRU", False), ("AGRU", False), ("AUGRU", False), ("AUGRU", True)])
def test_fit_takes_the_autograd_step_and_predict_follows(device, gru_type, neg):
    from deepctr_amd import engine, training, training_hip
    from deepctr_amd.models import DIEN
    rng = np.random.RandomState(9)
    n = 1024
    cols, names, feed = dien_problem(rng, n, T=6, vocab=20, neg=neg)
    y = ((feed["item_id"] % 2) ^ (feed["hist_item_id"][:, 0] % 2)).astype(np.float32)
    model = DIEN(cols, names, gru_type=gru_type, use_negsampling=neg, dnn_hidden_units=(32, 16), device=device)
    assert not training_hip.supported(model)
    before = {k: t.clone() for layer in (model.gru1, model.gru2) for k, t in layer.named_weights()}
    if neg:
        before.update({k: t.clone() for k, t in model.aux_dnn.named_weights()})
    model.compile("adam", "binary_crossentropy")
    hist = model.fit(feed, y, batch_size=256, epochs=1, verbose=0)
    assert np.isfinite(hist.history["loss"][0])
    after = dict(model.named_weights())
    unchanged = [k for k in before if torch.equal(before[k], after[k])]
    assert not unchanged, "weights the fit did not move: %s" % unchanged
    sub = {k: v[:256] for k, v in feed.items()}
    staged = engine.Staged(256)
    model._stage_inputs(sub, staged)
    model._begin()
    with torch.no_grad():
        ref = training.model_logits(model, staged, 0, 256).cpu().numpy()
    assert_close(np.asarray(model.predict_logits(sub, batch_size=256)).reshape(-1), ref, rtol=1e-4, atol=2e-5,
                 what="predict after fit vs model_logits")


def test_the_reference_example_program_runs_through_the_facade(device):
    """examples/run_dien.py's shape of program: the columns of DIEN_test.get_xy_fd(use_neg=True), compile, fit, predict."""
    from deepctr.feature_column import DenseFeat, SparseFeat, VarLenSparseFeat, get_feature_names
    from deepctr.models import DIEN
    feature_columns = [SparseFeat('user', 3, embedding_dim=10), SparseFeat('gender', 2, embedding_dim=4),
                       SparseFeat('item_id', 3 + 1, embedding_dim=8), SparseFeat('cate_id', 2 + 1, embedding_dim=4), DenseFeat('pay_score', 1)]
    feature_columns += [
        VarLenSparseFeat(SparseFeat('hist_item_id', vocabulary_size=3 + 1, embedding_dim=8, embedding_name='item_id'), maxlen=4,
                         length_name="seq_length"),
        VarLenSparseFeat(SparseFeat('hist_cate_id', 2 + 1, embedding_dim=4, embedding_name='cate_id'), maxlen=4, length_name="seq_length"),
        VarLenSparseFeat(SparseFeat('neg_hist_item_id', vocabulary_size=3 + 1, embedding_dim=8, embedding_name='item_id'), maxlen=4,
                         length_name="seq_length"),
        VarLenSparseFeat(SparseFeat('neg_hist_cate_id', 2 + 1, embedding_dim=4, embedding_name='cate_id'), maxlen=4, length_name="seq_length")]
    hist_iid = np.array([[1, 2, 3, 0], [1, 2, 3, 0], [1, 2, 0, 0]])
    hist_cate = np.array([[1, 2, 2, 0], [1, 2, 2, 0], [1, 2, 0, 0]])
    feature_dict = {'user': np.array([0, 1, 2]), 'gender': np.array([0, 1, 0]), 'item_id': np.array([1, 2, 3]), 'cate_id': np.array([1, 2, 2]),
                    'hist_item_id': hist_iid, 'hist_cate_id': hist_cate, 'pay_score': np.array([0.1, 0.2, 0.3]),
                    "seq_length": np.array([3, 3, 2]), 'neg_hist_item_id': hist_iid, 'neg_hist_cate_id': hist_cate}
    x = {name: feature_dict[name] for name in get_feature_names(feature_columns)}
    y = np.array([1, 0, 1])
    model = DIEN(feature_columns, ["item_id", "cate_id"], dnn_hidden_units=[4, 4, 4], dnn_dropout=0.6, gru_type="AUGRU", use_negsampling=True)
    model.compile('adam', 'binary_crossentropy', metrics=['binary_crossentropy'])
    history = model.fit(x, y, verbose=0, epochs=3)
    assert len(history.history["loss"]) == 3 and np.isfinite(history.history["loss"]).all()
    p = np.asarray(model.predict(x, batch_size=2))
    assert p.shape == (3, 1) and ((p > 0) & (p < 1)).all()
