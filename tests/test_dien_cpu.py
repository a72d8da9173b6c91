"""CPU: DIEN / DynamicGRU — the NumPy oracle (tests/ref_dien.py) against the reference's own outputs (tests/golden/model_dien_*.npz,
gru_layer.npz; scripts/make_golden_dien.py) and the conditions that script records, the torch restatement the training path uses
(training._gru, DIEN's model_logits and auxiliary loss) against the fixtures and the float64 oracle, its autograd gradients against finite differences of that oracle, the conditions the
comparisons lean on (unsaturated gates, visible cell kinds and length rule), the float32 error that fixes the GPU tests' bar, fit() on
the autograd step, the API contract, and the C ABI's argument checks (no launch)."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from tests import ref_dien as RD
from tests.test_gpu_bst import within_bar
from tests.test_gpu_dien import DIEN_FIXTURES, LAYER_TAGS, dien_problem, draw_lengths, make_layers, randomise, sweep_variants
from tests.spec import columns_from_spec
from tests.util import assert_close, golden_meta, load_golden, sigmoid_inv

CPU = torch.device("cpu")
GRU_TYPES = ["GRU", "AIGRU", "AGRU", "AUGRU"]


def build_dien(meta, device):
    from deepctr_amd.models import DIEN
    return DIEN(columns_from_spec(meta["dnn"]), meta["extra_args"][0], device=device, **meta["kwargs"])


def fixture_feed(g):
    return {k[5:]: v for k, v in g.items() if k.startswith("feed/")}


def fixture_weights(g):
    return {k[2:]: v for k, v in g.items() if k.startswith("w/")}


def layer_case(g, tag):
    """(cfg, x, att [B,T,1], lengths, (Wg, bg, Wc, bc), y) of a gru_layer.npz case."""
    import json
    cfg = json.loads(bytes(g[tag + "/cfg"]).decode())
    named = {n[len(tag) + 3:]: v for n, v in g.items() if n.startswith(tag + "/w/")}
    scope = "gru/gru_cell/" if "gru/gru_cell/gates/kernel" in named else "gru/"
    ws = tuple(named[scope + k] for k in ("gates/kernel", "gates/bias", "candidate/kernel", "candidate/bias"))
    return cfg, g[tag + "/x"], g[tag + "/att"], g[tag + "/lengths"], ws, g[tag + "/y"]


@pytest.mark.parametrize("name", DIEN_FIXTURES)
def test_oracle_matches_reference_code_and_the_fixture_conditions_hold(name):
    g = load_golden(name)
    meta = golden_meta(g)
    kw = meta["kwargs"]
    ref = g["y"]
    stats = []
    y64, aux = RD.run_fixture(g, np.float64, stats=stats, want_aux=True)
    assert y64.shape == ref.shape
    assert_close(y64, ref, rtol=1e-4, atol=1e-6, what=name + " float64")
    assert_close(RD.run_fixture(g, np.float32), ref, rtol=1e-4, atol=1e-6, what=name + " float32")
    if kw.get("task") != "regression":
        assert ref.min() > 1e-3 and ref.max() < 1 - 1e-3
        assert_close(sigmoid_inv(y64), sigmoid_inv(ref), rtol=1e-4, atol=2e-5, what=name + " logit")
    if kw.get("use_negsampling"):
        assert abs(aux - float(g["aux_loss"])) <= 1e-5 * abs(aux) and aux > 0.1          # alpha x the auxiliary loss, float32 there
    stats = np.asarray(stats)
    assert ((stats > 1e-3) & (stats < 0.999)).mean() >= 0.9             # the gates are not saturated
    lens = fixture_feed(g)["seq_length"].reshape(-1)
    assert lens[:4].tolist() == [6, 0, 1, 9]
    for k, v in fixture_weights(g).items():                             # dropping a GRU bias is visible
        if k.endswith("gates/bias"):
            assert np.abs(v - 1).min() > 0 and np.abs(v - 1).max() > 0.3
        if k.endswith("candidate/bias"):
            assert np.abs(v).max() > 0.3
    gru_type = kw["gru_type"]
    if gru_type != "GRU":
        logit = RD.run_fixture(g, np.float64, task="regression")
        live, short = lens > 0, (lens > 0) & (lens < 6)
        kind = "GRU" if gru_type == "AIGRU" else gru_type
        for other in [c for c in RD.CELLS if c != kind]:
            alt = RD.run_fixture(g, np.float64, task="regression", cell=other)
            assert np.abs(alt - logit)[live].max() >= 100 * 1e-4 * np.abs(logit[live]).max(), (name, other)
        if gru_type != "AGRU":      # (AGRU: the attention's own length mask makes a = 0, h' = h exactly; gru_layer.npz shows it there)
            free = RD.run_fixture(g, np.float64, task="regression", ignore_length=True)
            assert np.abs(free - logit)[short].max() >= 100 * 1e-4 * np.abs(logit[short]).max(), name


@pytest.mark.parametrize("tag", LAYER_TAGS)
def test_layer_oracle_matches_reference_code(tag):
    g = load_golden("gru_layer")
    cfg, x, att, lens, ws, y = layer_case(g, tag)
    cell = cfg["gru_type"]
    assert lens.tolist() == [0, 1, 5, 8, 2, 4]
    for dt in (np.float32, np.float64):
        got = RD.dynamic_gru(x, lens, [ws], cell, att, cfg["scale_input"], cfg["return_sequence"], dtype=dt)
        if not cfg["return_sequence"]:
            got = got[:, None, :]
        assert got.shape == y.shape
        assert within_bar(got, y.astype(np.float64)) <= 1.0, tag
    # the length rule and the cell kind are visible: each moves the rows shorter than T by >= 100 x the bar
    short = (lens > 0) & (lens < 5)
    base = RD.dynamic_gru(x, lens, [ws], cell, att, cfg["scale_input"], False)
    assert within_bar(RD.dynamic_gru(x, lens, [ws], cell, att, cfg["scale_input"], False, ignore_length=True)[short], base[short]) >= 100
    for other in [c for c in RD.CELLS if c != cell]:
        assert within_bar(RD.dynamic_gru(x, lens, [ws], other, att, cfg["scale_input"], False)[lens > 0], base[lens > 0]) >= 100


# (model_dien_hash is left to the GPU suite: the integer Hash runs inside the HIP kernels only)
@pytest.mark.parametrize("name", [n for n in DIEN_FIXTURES if n != "model_dien_hash"])
def test_torch_restatement_matches_the_fixture_and_the_oracle(name):
    from deepctr_amd import engine, training
    g = load_golden(name)
    meta = golden_meta(g)
    model = build_dien(meta, CPU)
    model.set_weights_by_name(fixture_weights(g))
    n = g["y"].shape[0]
    staged = engine.Staged(n)
    model._stage_inputs(fixture_feed(g), staged)
    model._begin()
    with torch.no_grad():
        logit32 = training.model_logits(model, staged, 0, n).numpy().reshape(-1)
    added32 = model._autograd_added_loss()
    want = g["y"].reshape(-1) if meta["kwargs"].get("task") == "regression" else sigmoid_inv(g["y"].reshape(-1))
    assert_close(logit32, want, rtol=1e-4, atol=2e-5, what=name + " model_logits vs the fixture")
    if meta["kwargs"].get("use_negsampling"):
        assert abs(float(added32) - float(g["aux_loss"])) <= 1e-5 * float(g["aux_loss"])     # the auxiliary-loss value
    else:
        assert added32 is None
    for layer in model.layers:
        _to_float64(layer)
    with torch.no_grad():
        logit = training.model_logits(model, staged, 0, n)
    assert logit.dtype == torch.float64
    ref = RD.run_fixture(g, np.float64, task="regression").reshape(-1)
    assert_close(logit.numpy().reshape(-1), ref, rtol=1e-6, atol=1e-7, what=name + " model_logits vs the oracle")


@pytest.mark.parametrize("name", DIEN_FIXTURES)
def test_weight_names_and_shapes_match_the_fixture(name):
    g = load_golden(name)
    model = build_dien(golden_meta(g), CPU)
    mine = {k: tuple(v.shape) for k, v in model.get_weights_by_name().items()}
    ref = {k: tuple(v.shape) for k, v in fixture_weights(g).items()}
    assert mine == ref
    assert "gru1/gru_cell/gates/kernel" in mine


@pytest.mark.parametrize("tag", LAYER_TAGS)
def test_torch_layer_restatement_matches_the_fixture(tag):
    from deepctr_amd import training
    g = load_golden("gru_layer")
    cfg, x, att, lens, ws, y = layer_case(g, tag)
    with torch.no_grad():
        got = training._gru(torch.from_numpy(x), torch.from_numpy(lens), [tuple(torch.from_numpy(w) for w in ws)], cfg["gru_type"],
                            torch.from_numpy(att), cfg["scale_input"], cfg["return_sequence"]).numpy()
    assert within_bar(got.reshape(y.shape), y.astype(np.float64)) <= 1.0


def t64(layers):
    return [tuple(torch.from_numpy(w).double() for w in layer) for layer in layers]


def _to_float64(layer):
    for k in list(layer._weights):
        layer._weights[k] = layer._weights[k].double()
    for sub in layer._sublayers:
        _to_float64(sub)


@pytest.mark.parametrize("E,T,B", [(4, 1, 3), (8, 5, 6), (12, 6, 17)])
def test_torch_gru_restatement_matches_oracle_in_float64(E, T, B):
    from deepctr_amd import training
    rng = np.random.RandomState(E * 10 + T)
    layers = make_layers(rng, E, 2)
    x = rng.standard_normal((B, T, E)).astype(np.float32)
    lens = draw_lengths(rng, B, T)
    att = rng.rand(B, T).astype(np.float32)
    for L, cell, scale, rs in sweep_variants():
        with torch.no_grad():
            got = training._gru(torch.from_numpy(x).double(), torch.from_numpy(lens), t64(layers[:L]), cell, torch.from_numpy(att).double(),
                                scale, rs).numpy()
        ref = RD.dynamic_gru(x, lens, layers[:L], cell, att, scale, rs)
        assert_close(got, ref, rtol=1e-9, atol=1e-12, what="_gru L %d %s scale %d seq %d" % (L, cell, scale, rs))
        dead = np.clip(lens, 0, T)
        if rs:
            assert not ref[np.arange(T)[None, :] >= dead[:, None]].any()
        else:
            assert not ref[dead == 0].any()
            full = RD.dynamic_gru(x, lens, layers[:L], cell, att, scale, True)       # the final state is the state at min(length, T)
            for b in np.nonzero(dead)[0]:
                assert np.array_equal(ref[b], full[b, dead[b] - 1])


def test_oracle_conditions_cell_kinds_and_the_length_rule_are_visible():
    """What the comparisons lean on, from the float64 oracle alone: the gates are not saturated (>= 90 % of final-state entries with |h|
    in (1e-3, 0.999)), swapping the cell kind and ignoring the lengths each move the output by >= 100 x the comparison bar."""
    rng = np.random.RandomState(5)
    B, T, E = 33, 6, 12
    layers = make_layers(rng, E, 1)
    x = rng.standard_normal((B, T, E)).astype(np.float32)
    lens = draw_lengths(rng, B, T)
    att = rng.rand(B, T).astype(np.float32)
    outs = {c: RD.dynamic_gru(x, lens, layers, c, att, return_sequence=False) for c in RD.CELLS}
    live = lens > 0
    for c, h in outs.items():
        a = np.abs(h[live])
        assert ((a > 1e-3) & (a < 0.999)).mean() >= 0.9, c
    for c1, c2 in (("AGRU", "AUGRU"), ("AUGRU", "GRU"), ("AGRU", "GRU")):
        assert within_bar(outs[c1][live], outs[c2][live]) >= 100, (c1, c2)
    short = (lens < T) & live
    assert short.sum() >= 3
    for c in RD.CELLS:
        free = RD.dynamic_gru(x, lens, layers, c, att, return_sequence=False, ignore_length=True)
        assert within_bar(free[short], outs[c][short]) >= 100, c
    # a dropped gate or candidate bias is visible too
    wg, bg, wc, bc = layers[0]
    for alt in ((wg, np.zeros_like(bg), wc, bc), (wg, bg, wc, np.zeros_like(bc))):
        assert within_bar(RD.dynamic_gru(x, lens, [alt], "GRU", return_sequence=False)[live], outs["GRU"][live]) >= 100


def test_float32_restatement_against_float64_on_the_op_sweep():
    """The float32 NumPy restatement of the loop against the float64 oracle on the GPU op sweep's own shapes and at T = 50, as a fraction
    of that sweep's bar (|err| <= 1e-4 |ref| + 2e-6 max|ref of the sample|).  The recurrence compounds rounding over T; had the
    fraction passed one half, the bar would have become twice the float32 error.  Measured: at most 0.16 (printed per width), so the bar
    stands; DESIGN.md §4.17 quotes the figure."""
    from tests import test_gpu_dien as G
    worst_all = 0.0
    for E in [e for e in G.SWEEP_E if e != "streamed"] + [72]:
        worst = 0.0
        for T in G.SWEEP_T + [50]:
            rng = np.random.RandomState(E * 100 + T)
            B = 33
            layers = make_layers(rng, E, 2)
            x = rng.standard_normal((B, T, E)).astype(np.float32)
            lens = draw_lengths(rng, B, T)
            att = rng.rand(B, T).astype(np.float32)
            for L, cell, scale, rs in sweep_variants():
                ref = RD.dynamic_gru(x, lens, layers[:L], cell, att, scale, rs)
                got = RD.dynamic_gru(x, lens, layers[:L], cell, att, scale, rs, dtype=np.float32)
                worst = max(worst, within_bar(got, ref))
        print("E %d: float32 NumPy / bar %.3f" % (E, worst))
        worst_all = max(worst_all, worst)
    assert worst_all < 0.5


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_float32_restatement_against_float64_on_the_saturated_runs(sign):
    """The same measurement on the runs of the GPU saturation test: float32 rounds 1 - sigmoid(30) to 0 where float64 keeps 9e-14, which
    the bar has to carry.  Measured: at most 1e-3 of the bar (printed per run)."""
    from tests import test_gpu_dien as G
    (x, lens, att), runs = G.saturated_cases(sign)
    for what, layers, cell in runs:
        ref = RD.dynamic_gru(x, lens, layers, cell, att)
        got = RD.dynamic_gru(x, lens, layers, cell, att, dtype=np.float32)
        assert np.isfinite(ref).all() and np.isfinite(got).all()
        worst = within_bar(got, ref)
        print("%s: float32 NumPy / bar %.3g" % (what, worst))
        assert worst < 0.5, what
        assert np.abs(ref[0]).max() > 0.1, "a sample of nothing but the residue of 1 - u"


@pytest.mark.parametrize("cell", RD.CELLS)
def test_autograd_gradients_of_the_restatement_match_finite_differences_of_the_oracle(cell):
    from deepctr_amd import training
    rng = np.random.RandomState(17)
    B, T, E = 3, 3, 4
    layers = make_layers(rng, E, 1)
    x = rng.standard_normal((B, T, E))
    lens = np.array([3, 1, 2], dtype=np.int32)
    att = rng.rand(B, T)
    proj = rng.standard_normal((B, T, E))

    def value(xv, av, ws):
        return float((RD.dynamic_gru(xv, lens, [ws], cell, av) * proj).sum())

    tx = torch.from_numpy(x).requires_grad_(True)
    ta = torch.from_numpy(att).requires_grad_(True)
    tw = [torch.from_numpy(w.astype(np.float64)).requires_grad_(True) for w in layers[0]]
    (training._gru(tx, torch.from_numpy(lens), [tuple(tw)], cell, ta) * torch.from_numpy(proj)).sum().backward()
    ws64 = [w.astype(np.float64) for w in layers[0]]
    eps = 1e-6

    def fd(arr, rebuild):
        g = np.zeros_like(arr)
        it = np.nditer(arr, flags=["multi_index"])
        for _ in it:
            i = it.multi_index
            hi, lo = arr.copy(), arr.copy()
            hi[i] += eps
            lo[i] -= eps
            g[i] = (rebuild(hi) - rebuild(lo)) / (2 * eps)
        return g

    assert_close(tx.grad.numpy(), fd(x, lambda v: value(v, att, ws64)), rtol=1e-5, atol=1e-8, what="d x")
    if cell != "GRU":
        assert_close(ta.grad.numpy(), fd(att, lambda v: value(x, v, ws64)), rtol=1e-5, atol=1e-8, what="d att")
        assert np.abs(ta.grad.numpy()).max() > 1e-3
    for k in range(4):
        g = fd(ws64[k], lambda v: value(x, att, ws64[:k] + [v] + ws64[k + 1:]))
        assert_close(tw[k].grad.numpy(), g, rtol=1e-5, atol=1e-8, what="d weight %d" % k)
    # the step of sample 1 past its length takes no gradient
    assert not tx.grad.numpy()[1, 1:].any()


MODEL_CASES = [  # tag, gru_type, problem kwargs, model kwargs
    ("gru", "GRU", {}, {}), ("aigru", "AIGRU", {}, {}), ("agru", "AGRU", {}, {}), ("augru", "AUGRU", {}, {}),
    ("augru_nonorm", "AUGRU", {}, {"att_weight_normalization": False}), ("bn", "AUGRU", {}, {"use_bn": True}),
    ("regression", "GRU", {}, {"task": "regression"}), ("one", "AGRU", {"n_hist": 1, "widths": (8,)}, {}),
    ("extra", "AIGRU", {"extra_seq": True, "dense": True}, {}), ("sigmoid_att", "GRU", {}, {"att_activation": "sigmoid"}),
    ("neg", "AUGRU", {"neg": True}, {"use_negsampling": True, "alpha": 0.5}),
]


def build_case(tag, gru_type, pkw, mkw, seed=3):
    from deepctr_amd import engine
    from deepctr_amd.models import DIEN
    rng = np.random.RandomState(seed)
    n = 32
    cols, names, feed = dien_problem(rng, n, **pkw)
    kw = dict(gru_type=gru_type, dnn_hidden_units=(16, 8), **mkw)
    model = DIEN(cols, names, device=CPU, **kw)
    w = randomise(model, rng)
    staged = engine.Staged(n)
    model._stage_inputs(feed, staged)
    model._begin()
    return model, cols, names, feed, kw, w, staged, n


@pytest.mark.parametrize("tag,gru_type,pkw,mkw", MODEL_CASES)
def test_model_logits_match_oracle_in_float64(tag, gru_type, pkw, mkw):
    from deepctr_amd import training
    model, cols, names, feed, kw, w, staged, n = build_case(tag, gru_type, pkw, mkw)
    assert set([0, 1, 6, 9]) <= set(feed["seq_length"].tolist())
    for layer in model.layers:
        _to_float64(layer)
    with torch.no_grad():
        logit = training.model_logits(model, staged, 0, n)
    added = model._autograd_added_loss()
    assert logit.dtype == torch.float64
    stats = []
    ref, aux = RD.dien(cols, names, w, feed, **dict(kw, task="regression", want_aux=True, stats=stats))
    assert_close(logit.numpy().reshape(-1), ref.reshape(-1), rtol=1e-6, atol=1e-7, what=tag + " model_logits")
    # the comparison is one of moving gates and distinguishable predictions
    stats = np.asarray(stats)
    assert ((stats > 1e-3) & (stats < 0.999)).mean() >= 0.9
    if kw.get("task") != "regression":
        p = 1 / (1 + np.exp(-ref))
        assert p.min() > 1e-3 and p.max() < 1 - 1e-3
    if mkw.get("use_negsampling"):
        assert aux is not None and aux > 0
        assert abs(float(added) - aux) <= 1e-9 * abs(aux), "alpha x auxiliary loss"
        assert model._autograd_added_loss() is None                     # handed over once per forward
    else:
        assert added is None and aux is None
    if gru_type != "GRU":           # the cell kind and the length rule are visible in the logits
        live = feed["seq_length"] > 0
        short = live & (feed["seq_length"] < 6)
        kind = "GRU" if gru_type == "AIGRU" else gru_type
        for other in [c for c in RD.CELLS if c != kind]:
            alt = RD.dien(cols, names, w, feed, **dict(kw, task="regression", cell=other))
            assert np.abs(alt - ref)[live].max() >= 100 * 1e-4 * np.abs(ref[live]).max(), (tag, other)
        if gru_type != "AGRU":
            # (inside the model AGRU cannot show it: the attention layer masks the scores by the same lengths, and a = 0 is h' = h
            # exactly; test_oracle_conditions_... shows the rule for AGRU with free scores)
            free = RD.dien(cols, names, w, feed, **dict(kw, task="regression", ignore_length=True))
            assert np.abs(free - ref)[short].max() >= 100 * 1e-4 * np.abs(ref[short]).max(), tag


@pytest.mark.parametrize("gru_type,neg", [(g, False) for g in GRU_TYPES] + [("AUGRU", True)])
def test_cpu_fit_on_the_autograd_step_lowers_the_loss(gru_type, neg):
    """training._fit_torch is device-agnostic torch code: a CPU-built DIEN trains for two epochs on a planted signal, the GRUs (and the
    auxiliary DNN) move."""
    from deepctr_amd import engine, training
    from deepctr_amd.models import DIEN
    rng = np.random.RandomState(4)
    n = 512
    cols, names, feed = dien_problem(rng, n, T=4, vocab=12, neg=neg)
    y = ((feed["item_id"] % 2) ^ (feed["hist_item_id"][:, 0] % 2)).astype(np.float32)
    torch.manual_seed(0)
    np.random.seed(0)
    model = DIEN(cols, names, gru_type=gru_type, use_negsampling=neg, dnn_hidden_units=(16, 8), device=CPU)
    model.compile("adam", "binary_crossentropy")
    staged = engine.Staged(n)
    model._stage_inputs(feed, staged)
    before = {k: t.clone() for k, t in model.named_weights() if k.startswith(("gru", "dnn/") if neg else "gru")}
    losses = []

    class End(object):
        def __call__(self, ep, loss):
            losses.append(loss)
            return False

        def finish(self):
            return losses

    training._fit_torch(model, staged, torch.from_numpy(y), n, 64, 2, True, End())
    assert len(losses) == 2 and losses[1] < losses[0]
    after = dict(model.named_weights())
    assert not [k for k in before if torch.equal(before[k], after[k])]
    assert len(before) == (8 + 6 if neg else 8)
    if neg:         # the shown loss carries alpha x the auxiliary loss: above the plain log loss of a coin
        assert losses[0] > 0.7


def test_signature_defaults_match_the_reference():
    from deepctr_amd.layers import DynamicGRU
    from deepctr_amd.models import DIEN
    params = inspect.signature(DIEN).parameters
    want = dict(gru_type="GRU", use_negsampling=False, alpha=1.0, use_bn=False, dnn_hidden_units=(256, 128, 64), dnn_activation='relu',
                att_hidden_units=(64, 16), att_activation="dice", att_weight_normalization=True, l2_reg_dnn=0, l2_reg_embedding=1e-6,
                dnn_dropout=0, seed=1024, task='binary')
    names = list(params)
    assert names[:2] == ["dnn_feature_columns", "history_feature_list"]
    assert names[2:2 + len(want)] == list(want) and names[2 + len(want):] == ["device"]
    for k, v in want.items():
        assert params[k].default == v, k
    lp = inspect.signature(DynamicGRU.__init__).parameters
    assert [(k, lp[k].default) for k in list(lp)[1:4]] == [("num_units", None), ("gru_type", "GRU"), ("return_sequence", True)]


def _cols(length_name="seq_length", neg=False):
    from deepctr_amd.feature_column import SparseFeat, VarLenSparseFeat
    cols = [SparseFeat("item_id", 10, 8), SparseFeat("cate_id", 5, 4),
            VarLenSparseFeat(SparseFeat("hist_item_id", 10, 8, embedding_name="item_id"), 4, length_name=length_name),
            VarLenSparseFeat(SparseFeat("hist_cate_id", 5, 4, embedding_name="cate_id"), 4, length_name=length_name)]
    if neg:
        cols += [VarLenSparseFeat(SparseFeat("neg_hist_item_id", 10, 8, embedding_name="item_id"), 4, length_name=length_name),
                 VarLenSparseFeat(SparseFeat("neg_hist_cate_id", 5, 4, embedding_name="cate_id"), 4, length_name=length_name)]
    return cols


def test_construction_errors_and_regularizers():
    from deepctr_amd.layers import DynamicGRU
    from deepctr_amd.models import DIEN
    both = ["item_id", "cate_id"]
    with pytest.raises(ValueError, match="^gru_type error $"):
        DIEN(_cols(), both, gru_type="LSTM", device=CPU)
    with pytest.raises(ValueError, match="history_feature_list"):
        DIEN(_cols()[:2], both, device=CPU)
    with pytest.raises(ValueError, match="seq_length"):          # (the reference: KeyError from features["seq_length"])
        DIEN(_cols("hist_len"), both, device=CPU)
    with pytest.raises(ValueError, match="neg_hist_"):
        DIEN(_cols(), both, gru_type="AUGRU", use_negsampling=True, device=CPU)
    with pytest.raises(ValueError, match="AUGRU"):               # (the reference: TypeError from alpha * None, dien.py:213)
        DIEN(_cols(neg=True), both, gru_type="GRU", use_negsampling=True, device=CPU)
    m = DIEN(_cols(neg=True), both, gru_type="AUGRU", use_negsampling=True, l2_reg_dnn=0.1, l2_reg_embedding=0.2, device=CPU)
    assert m.regularizers == {"embedding": 0.2, "linear": 0.0, "dnn": 0.1} and not m._hip_supported()
    assert m.key_hash_mode == 1 and m.key_mask_from_ids is False
    # neg_hist_* columns are neither pooled nor fed to the DNN: the same DNN input width with and without them
    assert m.stage_plan.in_dim == DIEN(_cols(), both, gru_type="AUGRU", device=CPU).stage_plan.in_dim == 8 + 4 + 12
    layer = DynamicGRU(5, device=CPU)
    with pytest.raises(NotImplementedError, match="num_units"):
        layer.build([(None, 4, 7), (None, 1)])


def test_layer_contract_weight_names_and_initial_values():
    from deepctr_amd.layers import DynamicGRU, custom_objects
    from deepctr_amd.models import DIEN
    assert custom_objects["DynamicGRU"] is DynamicGRU
    layer = DynamicGRU(None, gru_type="AUGRU", return_sequence=False, name="gru2", device=CPU)
    layer.build([(None, 5, 6), (None, 1), (None, 5, 1)])
    got = [(n, tuple(t.shape)) for n, t in layer.named_weights()]
    assert got == [("gru2/gates/kernel", (12, 12)), ("gru2/gates/bias", (12,)), ("gru2/candidate/kernel", (12, 6)),
                   ("gru2/candidate/bias", (6,))]
    wg, bg, wc, bc = layer.operands()
    assert float(bg.min()) == 1.0 == float(bg.max()) and not bc.any()
    lim = (6.0 / 24) ** 0.5                                         # glorot_uniform over [2E, 2E]
    assert float(wg.abs().max()) <= lim and float(wg.abs().max()) > 0.5 * lim and float(wc.abs().max()) <= (6.0 / 18) ** 0.5
    assert layer.num_units == 6 and layer.cell == "AUGRU"
    assert layer.compute_output_shape([(None, 5, 6), (None, 1)]) == (None, 1, 6)
    cfg = layer.get_config()
    assert {k: cfg[k] for k in ("num_units", "gru_type", "return_sequence", "name")} == dict(num_units=6, gru_type="AUGRU",
                                                                                           return_sequence=False, name="gru2")
    again = DynamicGRU.from_config(dict(cfg, device=CPU))
    assert again.get_config() == cfg
    plain = DynamicGRU(device=CPU)
    plain.build([(None, 5, 6), (None, 1)])
    assert [n.split("/", 1)[1] for n, _ in plain.named_weights()] == ["gru_cell/gates/kernel", "gru_cell/gates/bias",
                                                                     "gru_cell/candidate/kernel", "gru_cell/candidate/bias"]
    assert plain.compute_output_shape([(None, 5, 6), (None, 1)]) == (None, 5, 6) and plain.cell == "GRU"
    m = DIEN(_cols(neg=True), ["item_id", "cate_id"], gru_type="AUGRU", use_negsampling=True, dnn_hidden_units=(8,), device=CPU)
    names = list(m.get_weights_by_name())
    for k in ("gru1/gru_cell/gates/kernel", "gru1/gru_cell/candidate/bias", "gru2/gates/kernel", "gru2/candidate/bias", "dnn/kernel2",
              "local_activation_unit/kernel", "dnn_2/kernel0"):
        assert k in names, k
    assert tuple(m.get_weights_by_name()["dnn/kernel0"].shape) == (24, 100)          # the auxiliary DNN [100, 50, 1] over [h_t | e_{t+1}]


def test_save_and_load_weights_round_trip(tmp_path):
    from deepctr_amd.models import DIEN
    rng = np.random.RandomState(8)
    a = DIEN(_cols(neg=True), ["item_id", "cate_id"], gru_type="AUGRU", use_negsampling=True, dnn_hidden_units=(8,), device=CPU)
    w = randomise(a, rng)
    path = str(tmp_path / "dien.npz")
    a.save_weights(path)
    b = DIEN(_cols(neg=True), ["item_id", "cate_id"], gru_type="AUGRU", use_negsampling=True, dnn_hidden_units=(8,), device=CPU)
    b.load_weights(path)
    got = b.get_weights_by_name()
    assert list(got) == list(w)
    for k in w:
        assert np.array_equal(np.asarray(got[k]), w[k]), k


def test_reference_import_names():
    import deepctr
    import deepctr_amd.layers
    import deepctr_amd.models
    from deepctr.layers.sequence import DynamicGRU
    from deepctr.models import DIEN
    from deepctr.models.sequence import DIEN as D3
    from deepctr.models.sequence.dien import DIEN as D2
    assert DIEN is deepctr_amd.models.DIEN is D2 is D3 is deepctr.models.DIEN
    assert DynamicGRU is deepctr_amd.layers.DynamicGRU is deepctr.layers.DynamicGRU


def _args(**kw):
    from deepctr_amd import _C
    base = dict(batch=4, x_stride=5 * 8, x_row_stride=8, att_stride=5, seq_len=5, dim=8, n_layers=1, cell=0, scale_input=0,
                return_sequence=1, out_stride=5 * 8, out_row_stride=8)
    base.update(kw)
    return _C.gru.Args(**base)


def test_abi_argument_errors_without_a_gpu():
    from deepctr_amd import _C
    lib = _C.lib()
    assert lib.dctr_abi_version() == 13 == _C.ABI_VERSION
    f = lambda a: lib.dctr_gru_fwd(ctypes.byref(a), None)       # noqa: E731
    r = lambda a: lib.dctr_gru_route(ctypes.byref(a))           # noqa: E731
    assert lib.dctr_gru_fwd(None, None) == -1 and lib.dctr_gru_route(None) == -1 and lib.dctr_gru_workspace_bytes(None) == 0
    assert f(_args()) == -1                                       # x / lengths / layers / out missing
    assert b"gru_fwd" in lib.dctr_last_error()
    for bad in (dict(seq_len=0), dict(dim=0), dict(n_layers=0), dict(n_layers=3), dict(batch=-1), dict(x_row_stride=7), dict(x_stride=39),
                dict(out_row_stride=7), dict(out_stride=39), dict(return_sequence=0, out_stride=7), dict(cell=1, att_stride=4),
                dict(scale_input=1, att_stride=0)):
        assert f(_args(**bad)) == -2 and r(_args(**bad)) == -2, bad
    for bad in (dict(cell=3), dict(cell=-1), dict(route=3), dict(scale_input=2), dict(return_sequence=-1), dict(n_layers=2, cell=2)):
        assert f(_args(**bad)) == -4, bad
    ptrs = (ctypes.c_void_p * 4)(16, 16, None, 16)
    a = _args(x=16, lengths=16, out=16, layers=ctypes.cast(ptrs, ctypes.c_void_p))
    assert f(a) == -1 and b"layer 0" in lib.dctr_last_error()     # a null weight is reported before anything is launched
    ptrs[2] = 16
    a.cell = 2
    assert f(a) == -1 and b"att_scores" in lib.dctr_last_error()
    a.cell, a.batch = 0, 0
    assert f(a) == 0                                              # complete arguments, empty batch: a no-op
    big = _args(dim=600, x_row_stride=600, x_stride=3000, out_row_stride=600, out_stride=3000, x=16, lengths=16, out=16,
                layers=ctypes.cast(ptrs, ctypes.c_void_p))
    assert r(big) == _C.gru.ROUTE_STREAMED and f(big) == -1 and b"workspace" in lib.dctr_last_error()
    big.route = _C.gru.ROUTE_RESIDENT
    assert r(big) == -5


def test_routes_and_workspace_sizes_without_a_gpu():
    """The resident route holds 6 E^2 floats per layer next to the tiles within the CU's 160 KiB of LDS."""
    from deepctr_amd import ops
    assert ops.gru_route(50, 32) == "resident" and ops.gru_route(50, 32, 2) == "resident"
    assert ops.gru_workspace_bytes(4096, 50, 32, 2) == 0
    assert ops.gru_route(6, 12, 2) == "resident" and ops.gru_route(1, 1) == "resident"
    assert ops.gru_route(6, 16, route="streamed") == "streamed" and ops.gru_workspace_bytes(9, 6, 16, route="streamed") == 0
    e1 = next(e for e in range(1, 512) if ops.gru_route(6, e) == "streamed")
    e2 = next(e for e in range(1, 512) if ops.gru_route(6, e, 2) == "streamed")
    assert e2 < e1
    for e, L in ((e1, 1), (e2, 2)):            # the first width that no longer fits: weights + biases alone approach the 160 KiB
        assert L * (6 * e * e + 3 * e) * 4 <= 160 * 1024 < L * (6 * e * e + 3 * e) * 4 + 2 * 160 * 1024 // 3
        assert L * (6 * (e - 1) ** 2) * 4 < 160 * 1024
    with pytest.raises(Exception):
        ops.gru_route(6, e1, route="resident")
    big = ops.gru_workspace_bytes(3, 2, 600)
    assert big > 0 and big % 16 == 0 and big == ops.gru_workspace_bytes(70000, 2, 600) and big <= 256 << 20
    with pytest.raises(ValueError, match="cell must be"):
        ops.gru_route(5, 8, cell="LSTM")
    assert ops.gru_macs(50, 32) == 50 * 6 * 1024 and ops.gru_macs(50, 32, 2) == 2 * 307200


def test_args_mirror_has_the_layout_the_c_compiler_gives_the_header(tmp_path):
    import os
    import shutil
    import subprocess
    from deepctr_amd import _C
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    cls = _C.gru.Args
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dctr.h"', "int main(void) {",
             '    printf("sizeof %zu\\n", sizeof(dctr_gru_args_t));', '    printf("ptrs %d\\n", DCTR_GRU_LAYER_PTRS);',
             '    printf("abi %d\\n", DCTR_ABI_VERSION);', '    printf("cells %d\\n", DCTR_GRU_CELL_GRU + 10 * DCTR_GRU_CELL_AGRU + 100 * DCTR_GRU_CELL_AUGRU);',
             '    printf("routes %d\\n", DCTR_GRU_ROUTE_AUTO + 10 * DCTR_GRU_ROUTE_RESIDENT + 100 * DCTR_GRU_ROUTE_STREAMED);']
    for fname, _ in cls._fields_:
        lines.append('    printf("%s %%zu\\n", offsetof(dctr_gru_args_t, %s));' % (fname, fname))
    lines += ["    return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    for line in filter(None, out):
        field, val = line.split()
        if field == "ptrs":
            want = _C.gru.LAYER_PTRS
        elif field == "abi":
            want = 13
        elif field == "cells":
            want = _C.gru.CELL_GRU + 10 * _C.gru.CELL_AGRU + 100 * _C.gru.CELL_AUGRU
        elif field == "routes":
            want = _C.gru.ROUTE_AUTO + 10 * _C.gru.ROUTE_RESIDENT + 100 * _C.gru.ROUTE_STREAMED
        else:
            want = ctypes.sizeof(cls) if field == "sizeof" else getattr(cls, field).offset
        assert int(val) == want, "%s: C says %s, ctypes %d" % (field, val, want)
