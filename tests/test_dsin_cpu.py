"""CPU: DSIN / BiLSTM / BiasEncoding — the NumPy oracle (tests/ref_dsin.py) against the reference's own outputs (tests/golden/model_dsin_*.npz,
bilstm_layer.npz, bias_encoding_layer.npz; scripts/make_golden_dsin.py) and the conditions that script records, the torch restatement
the training path uses (training._bilstm, DSIN's model_logits) against the fixtures and the float64 oracle, its autograd gradients
against finite differences of that oracle, fit() on the autograd step, the API contract, and the C ABI's argument checks, routes and
workspace sizes (no launch)."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from tests import ref_dsin as RS
from tests.test_gpu_bst import within_bar
from tests.dsin_util import (BILSTM_TAGS, DSIN_FIXTURES, bias_encoding_case, bilstm_case, build_dsin, dsin_problem, fixture_feed, fixture_weights,
                             make_layers)
from tests.util import assert_close, golden_meta, load_golden, sigmoid_inv

CPU = torch.device("cpu")
SWAPS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]


def _to_float64(layer):
    for k in list(layer._weights):
        layer._weights[k] = layer._weights[k].double()
    for sub in layer._sublayers:
        _to_float64(sub)


@pytest.mark.parametrize("name", DSIN_FIXTURES)
def test_oracle_matches_reference_code_and_the_fixture_conditions_hold(name):
    g = load_golden(name)
    meta = golden_meta(g)
    kw = meta["kwargs"]
    ref = RS.run_fixture(g, np.float64)
    assert np.abs(ref.reshape(-1) - g["y"].reshape(-1)).max() < 1e-5
    feed = fixture_feed(g)
    S = kw["sess_max_count"]
    sl = feed["sess_length"]
    first = feed["sess_0_item"]
    assert first[0].all() and sl[0] == S and sl[1] == 0                     # a full sample, a sample of sess_length 0
    assert not first[2].any() and sl[2] >= 1 and not first[3].any()         # an empty session inside sess_length
    if kw.get("task") != "regression":
        assert g["y"].min() > 1e-3 and g["y"].max() < 1 - 1e-3
    stats = []
    base = RS.run_fixture(g, np.float64, task="regression", stats=stats).reshape(-1)
    tol = 1e-4 * np.abs(base).max()

    def moved(**pk):
        return np.abs(RS.run_fixture(g, np.float64, task="regression", **pk).reshape(-1) - base).max() / tol
    for a, b in SWAPS:
        order = [b if q == a else a if q == b else q for q in range(4)]
        assert moved(gate_order=tuple(order)) >= 100, (a, b)
    if S > 1:       # one session has nothing to reverse and pools to itself at any length
        assert moved(reverse_back=False) >= 100 and moved(ignore_sess_length=True) >= 100
    assert moved(empty_session_zero=True) >= 100
    assert (np.asarray(stats) < 4).mean() >= 0.9


@pytest.mark.parametrize("tag", BILSTM_TAGS)
def test_layer_oracle_matches_reference_code(tag):
    cfg, x, ws, y = bilstm_case(load_golden("bilstm_layer"), tag)
    ref = RS.bilstm(x, ws, cfg["res_layers"], cfg["merge_mode"])
    ref = np.stack(ref, axis=1) if cfg["merge_mode"] is None else ref
    assert ref.shape == y.shape and np.abs(ref - y).max() < 1e-5
    assert len(ws) == cfg["layers"] and ws[0][0].shape == (x.shape[2], 4 * cfg["units"])


def test_bilstm_fixture_covers_the_cases_and_tells_the_variants_apart():
    import json
    g = load_golden("bilstm_layer")
    cfgs = {tag: json.loads(bytes(g[tag + "/cfg"]).decode()) for tag in BILSTM_TAGS}
    assert set(c["merge_mode"] for c in cfgs.values()) == set(RS.MERGE_MODES)
    assert set(c["layers"] for c in cfgs.values()) == {1, 2, 3}
    assert any(c["res_layers"] == c["layers"] for c in cfgs.values()) and any(c["res_layers"] == 1 < c["layers"] for c in cfgs.values())
    assert g["din/x"].shape[2] != cfgs["din"]["units"]
    cfg, x, ws, y = bilstm_case(g, "ave")
    base = RS.bilstm(x, ws, 0, "ave")
    for a, b in SWAPS:
        order = tuple(b if q == a else a if q == b else q for q in range(4))
        assert within_bar(RS.bilstm(x, ws, 0, "ave", gate_order=order), base) >= 100
    assert within_bar(RS.bilstm(x, ws, 0, "ave", reverse_back=False), base) >= 100
    assert within_bar(RS.bilstm(x, [tuple(np.zeros_like(w) if k % 3 == 2 else w for k, w in enumerate(lw)) for lw in ws], 0, "ave"), base) >= 100


@pytest.mark.parametrize("tag", ["sess3", "sess2"])
def test_bias_encoding_oracle_matches_reference_code(tag):
    S, xs, ws, ys = bias_encoding_case(load_golden("bias_encoding_layer"), tag)
    ref = RS.bias_encoding(np.stack(xs, axis=1).astype(np.float64), *ws)
    assert np.abs(ref - np.stack(ys, axis=1)).max() < 1e-6
    for k in range(3):      # every one of the three biases is visible
        zeroed = [np.zeros_like(w) if i == k else w for i, w in enumerate(ws)]
        assert np.abs(RS.bias_encoding(np.stack(xs, axis=1).astype(np.float64), *zeroed) - ref).max() > 1e-2


@pytest.mark.parametrize("u,T,B,Din", [(4, 1, 3, 4), (8, 5, 6, 8), (12, 5, 17, 7)])
def test_torch_bilstm_restatement_matches_oracle_in_float64(u, T, B, Din):
    from deepctr_amd import training
    rng = np.random.RandomState(u * 10 + T)
    layers = make_layers(rng, Din, u, 3)
    x = rng.standard_normal((B, T, Din))
    t64 = [tuple(torch.from_numpy(w.astype(np.float64)) for w in lw) for lw in layers]
    for L in (1, 2, 3):
        for mm in RS.MERGE_MODES:
            for res in sorted({0, 1, L} if Din == u else {0, min(1, L - 1)}):
                for act in ("sigmoid", "hard_sigmoid"):
                    got = training._bilstm(torch.from_numpy(x), t64[:L], res, mm, act)
                    ref = RS.bilstm(x, layers[:L], res, mm, act)
                    if mm is None:
                        got, ref = torch.stack(got), np.stack(ref)
                    assert got.dtype == torch.float64 and np.abs(got.numpy() - ref).max() <= 1e-9, (L, mm, res, act)


@pytest.mark.parametrize("act", ["sigmoid", "hard_sigmoid"])
def test_autograd_gradients_of_the_restatement_match_finite_differences_of_the_oracle(act):
    from deepctr_amd import training
    rng = np.random.RandomState(17)
    B, T, u = 2, 3, 3
    layers = [[w.astype(np.float64) for w in lw] for lw in make_layers(rng, u, u, 2)]
    x = rng.standard_normal((B, T, u))
    proj = rng.standard_normal((B, T, 2 * u))

    def value(xv, ws):
        return float((RS.bilstm(xv, ws, 1, "concat", act) * proj).sum())

    tx = torch.from_numpy(x).requires_grad_(True)
    tw = [[torch.from_numpy(w).requires_grad_(True) for w in lw] for lw in layers]
    (training._bilstm(tx, [tuple(lw) for lw in tw], 1, "concat", act) * torch.from_numpy(proj)).sum().backward()
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

    assert_close(tx.grad.numpy(), fd(x, lambda v: value(v, layers)), rtol=1e-5, atol=1e-8, what="d x")
    for li in range(2):
        for k in range(6):
            def rebuild(v, li=li, k=k):
                ws = [list(lw) for lw in layers]
                ws[li][k] = v
                return value(x, ws)
            assert_close(tw[li][k].grad.numpy(), fd(layers[li][k], rebuild), rtol=1e-5, atol=1e-8, what="d layer %d weight %d" % (li, k))
            assert np.abs(tw[li][k].grad.numpy()).max() > 1e-4


# (model_dsin_hash is left to the GPU suite: the integer Hash runs inside the HIP kernels only)
@pytest.mark.parametrize("name", [n for n in DSIN_FIXTURES if n != "model_dsin_hash"])
def test_torch_restatement_matches_the_fixture_and_the_oracle(name):
    from deepctr_amd import engine, training
    g = load_golden(name)
    meta = golden_meta(g)
    model = build_dsin(meta, CPU)
    model.set_weights_by_name(fixture_weights(g))
    n = g["y"].shape[0]
    staged = engine.Staged(n)
    model._stage_inputs(fixture_feed(g), staged)
    model._begin()
    with torch.no_grad():
        logit32 = training.model_logits(model, staged, 0, n).numpy().reshape(-1)
    want = g["y"].reshape(-1) if meta["kwargs"].get("task") == "regression" else sigmoid_inv(g["y"].reshape(-1))
    assert_close(logit32, want, rtol=1e-4, atol=2e-5, what=name + " model_logits vs the fixture")
    for layer in model.layers:
        _to_float64(layer)
    with torch.no_grad():
        logit = training.model_logits(model, staged, 0, n)
    assert logit.dtype == torch.float64
    ref = RS.run_fixture(g, np.float64, task="regression").reshape(-1)
    assert_close(logit.numpy().reshape(-1), ref, rtol=1e-6, atol=1e-7, what=name + " model_logits vs the oracle")


@pytest.mark.parametrize("name", DSIN_FIXTURES)
def test_weight_names_and_shapes_match_the_fixture(name):
    g = load_golden(name)
    model = build_dsin(golden_meta(g), CPU)
    mine = {k: tuple(v.shape) for k, v in model.get_weights_by_name().items()}
    ref = {k: tuple(v.shape) for k, v in fixture_weights(g).items()}
    assert mine == ref
    assert "lstm_3/recurrent_kernel" in mine and "sparse_emb_1-item/embeddings" in mine
    assert model.input_names[-1] == "sess_length"


def test_training_dropout_is_one_mask_per_lstm_shared_over_the_steps():
    from deepctr_amd import training
    torch.manual_seed(5)
    B, T, u = 64, 6, 4
    x = torch.ones(B, T, u, dtype=torch.float64)
    # zero recurrent kernels and biases, a kernel that copies x into the candidate: i = f = o = 1/2 and c_t = c_{t-1} / 2 + tanh(x_t) / 2,
    # so a unit whose input is dropped stays exactly zero at EVERY step only if the steps share one mask
    w = torch.zeros(u, 4 * u, dtype=torch.float64)
    w[:, 2 * u:3 * u] = torch.eye(u, dtype=torch.float64)
    zu, b = torch.zeros(u, 4 * u, dtype=torch.float64), torch.zeros(4 * u, dtype=torch.float64)
    fw, bw = training._bilstm(x, [(w, zu, b, w, zu, b)], 0, None, "sigmoid", dropout_rate=0.5, training=True)
    dropped = fw[:, 0] == 0
    assert 0.3 < float(dropped.double().mean()) < 0.7
    for t in range(T):
        assert torch.equal(fw[:, t] == 0, dropped)
    assert not torch.equal(bw[:, 0] == 0, dropped)                            # the backward LSTM draws its own mask
    kept = fw[:, 0][~dropped]
    assert float((kept - 0.5 * np.tanh(0.5 * np.tanh(2.0))).abs().max()) < 1e-12    # inverted scaling: x / (1 - rate)
    assert not (training._bilstm(x, [(w, zu, b, w, zu, b)], 0, "fw", "sigmoid", dropout_rate=0.5, training=False) == 0).any()


def test_cpu_fit_on_the_autograd_step_lowers_the_loss():
    """training._fit_torch is device-agnostic torch code: a CPU-built DSIN trains for three epochs on a planted signal; the LSTMs, the
    Transformer and the bias encoding move."""
    from deepctr_amd import engine, training
    from deepctr_amd.models import DSIN
    rng = np.random.RandomState(9)
    n = 512
    cols, names, feed = dsin_problem(rng, n, vocab=12)
    y = ((feed["item"] % 2) ^ (feed["sess_0_item"][:, 0] % 2)).astype(np.float32)
    torch.manual_seed(0)
    np.random.seed(0)
    model = DSIN(cols, names, sess_max_count=3, bias_encoding=True, att_embedding_size=3, att_head_num=4, dnn_hidden_units=(16, 8), device=CPU)
    model.compile("adam", "binary_crossentropy")
    staged = engine.Staged(n)
    model._stage_inputs(feed, staged)
    before = {k: t.clone() for k, t in model.named_weights() if k.startswith(("lstm", "transformer", "bias_encoding"))}
    losses = []

    class End(object):
        def __call__(self, ep, loss):
            losses.append(loss)
            return False

        def finish(self):
            return losses

    training._fit_torch(model, staged, torch.from_numpy(y), n, 64, 3, True, End())
    assert len(losses) == 3 and np.isfinite(losses).all() and losses[-1] < losses[0]
    after = dict(model.named_weights())
    assert len(before) == 12 + 5 + 3 and not [k for k in before if torch.equal(before[k], after[k])]


def test_signature_defaults_match_the_reference():
    from deepctr_amd.layers import BiasEncoding, BiLSTM
    from deepctr_amd.models import DSIN
    sig = inspect.signature(DSIN)
    want = dict(sess_max_count=5, bias_encoding=False, att_embedding_size=1, att_head_num=8, dnn_hidden_units=(256, 128, 64), dnn_activation='relu',
                dnn_dropout=0, dnn_use_bn=False, l2_reg_dnn=0, l2_reg_embedding=1e-6, seed=1024, task='binary', device=None)
    assert list(sig.parameters) == ["dnn_feature_columns", "sess_feature_list"] + list(want)
    assert {k: sig.parameters[k].default for k in want} == want
    sig = inspect.signature(BiLSTM.__init__)
    assert [(k, p.default) for k, p in list(sig.parameters.items())[2:6]] == [("layers", 2), ("res_layers", 0), ("dropout_rate", 0.2),
                                                                            ("merge_mode", "ave")]
    assert inspect.signature(BiasEncoding.__init__).parameters["seed"].default == 1024


def test_argument_checks_and_their_messages():
    from deepctr_amd import ops
    from deepctr_amd.layers import BiLSTM
    from deepctr_amd.models import DSIN
    msg = 'Merge mode should be one of {"fw","bw","sum", "mul", "ave", "concat", None}'
    with pytest.raises(ValueError) as e:
        BiLSTM(4, merge_mode="max")
    assert msg in str(e.value) and str(e.value).startswith("Invalid merge mode.")
    rng = np.random.RandomState(1)
    layers = [tuple(torch.from_numpy(w) for w in lw) for lw in make_layers(rng, 6, 4, 2)]
    x = torch.zeros(3, 5, 6)
    with pytest.raises(ValueError) as e:
        ops.bilstm(x, layers, merge_mode="max")
    assert msg in str(e.value)
    with pytest.raises(ValueError) as e:
        ops.bilstm(x, layers, res_layers=2)                                 # a residual over layer 0 whose inputs are wider than its units
    assert "residual" in str(e.value)
    with pytest.raises(ValueError) as e:
        BiLSTM(4, layers=2, res_layers=2, device=CPU).build((None, 5, 6))
    assert "residual" in str(e.value)
    BiLSTM(4, layers=2, res_layers=1, device=CPU).build((None, 5, 6))         # the residual over layer 1 alone is fine
    with pytest.raises(ValueError):
        ops.bilstm(x, layers, recurrent_activation="tanh")
    with pytest.raises(ValueError):
        ops.bilstm(x, layers, route="fast")
    with pytest.raises(ValueError) as e:
        ops.bilstm(torch.zeros(3, 6), layers)
    assert "expect to be 3 dimensions" in str(e.value)
    with pytest.raises(ValueError):
        ops.bilstm(x, [layers[0][:5]])
    with pytest.raises(ValueError):
        ops.bilstm(x, [layers[0][:1] + (layers[0][1].t(),) + layers[0][2:]])
    layer = BiLSTM(6, device=CPU)
    with pytest.raises(NotImplementedError):
        layer(x, mask=torch.ones(3, 5, dtype=torch.bool))
    with pytest.raises(ValueError) as e:
        BiLSTM(6, device=CPU).build((None, 6))
    assert "expect to be 3 dimensions" in str(e.value)
    cols, names, _ = dsin_problem(rng, 8)
    with pytest.raises(ValueError) as e:
        DSIN(cols, names, sess_max_count=3, att_embedding_size=4, att_head_num=2, device=CPU)
    assert str(e.value) == "hist_emb_size must equal to att_embedding_size * att_head_num ,got 12 != 4 *2"
    with pytest.raises(KeyError):
        DSIN(cols, names, sess_max_count=4, att_embedding_size=6, att_head_num=2, device=CPU)    # no sess_3_* columns
    m = DSIN(cols, names, sess_max_count=3, att_embedding_size=6, att_head_num=2, l2_reg_dnn=0.5, l2_reg_embedding=0.25, device=CPU)
    assert m.regularizers == {"embedding": 0.25, "linear": 0.0, "dnn": 0.5}
    with pytest.raises(ValueError):
        ops.bias_encoding(torch.zeros(2, 3, 4), torch.zeros(3), torch.zeros(4), torch.zeros(5))


def test_layer_contract_weight_names_initial_values_and_config_round_trip():
    from deepctr_amd.layers import BiasEncoding, BiLSTM, custom_objects
    layer = BiLSTM(6, layers=2, res_layers=1, dropout_rate=0.1, merge_mode="concat", device=CPU)
    layer.build((None, 5, 9))
    names = [n.split("/")[1] for n, _ in layer.named_weights()]
    assert names == ["kernel", "recurrent_kernel", "bias"] * 4
    shapes = [tuple(t.shape) for t in layer.weights]
    assert shapes[:3] == [(9, 24), (6, 24), (24,)] and shapes[6:9] == [(6, 24), (6, 24), (24,)]
    for f in layer.fw_lstm + layer.bw_lstm:
        k, u, b = f.operands()
        assert torch.equal(b, torch.ones(24)) and float(k.abs().max()) <= (6.0 / (k.shape[0] + 24)) ** 0.5
        assert float((u @ u.t() - torch.eye(6)).abs().max()) < 1e-5           # orthogonal rows
    assert layer.compute_output_shape((None, 5, 9)) == (None, 5, 18) and layer.supports_masking
    cfg = layer.get_config()
    assert {k: cfg[k] for k in ("units", "layers", "res_layers", "dropout_rate", "merge_mode")} == dict(
        units=6, layers=2, res_layers=1, dropout_rate=0.1, merge_mode="concat")
    assert BiLSTM.from_config(cfg).get_config() == cfg
    be = BiasEncoding(3, seed=7, device=CPU)
    be.build([(None, 5, 8)] * 3)
    assert [(n, tuple(t.shape)) for n, t in be.named_weights()] == [
        (be.name + "/sess_bias_embedding", (3, 1, 1)), (be.name + "/seq_bias_embedding", (1, 5, 1)), (be.name + "/item_bias_embedding", (1, 1, 8))]
    assert all(float(t.abs().max()) <= 2e-4 for t in be.weights)
    cfg = be.get_config()
    assert cfg["sess_max_count"] == 3 and cfg["seed"] == 7 and BiasEncoding.from_config(cfg).get_config() == cfg
    assert custom_objects["BiLSTM"] is BiLSTM and custom_objects["BiasEncoding"] is BiasEncoding


def test_orthogonal_initializer():
    from deepctr_amd.initializers import Orthogonal
    for shape in ((6, 24), (24, 6), (5, 5)):
        q = Orthogonal(seed=3)(shape).double()
        small = q @ q.t() if shape[0] <= shape[1] else q.t() @ q
        assert float((small - torch.eye(min(shape), dtype=torch.float64)).abs().max()) < 1e-6
        assert torch.equal(Orthogonal(seed=3)(shape), Orthogonal(seed=3)(shape))
    assert float((Orthogonal(gain=2.0, seed=3)((4, 4)) - 2 * Orthogonal(seed=3)((4, 4))).abs().max()) < 1e-6


def test_reference_import_names():
    import deepctr.layers.sequence as seq
    import deepctr.models
    import deepctr.models.sequence.dsin as dsin_mod
    import deepctr_amd.layers.sequence
    import deepctr_amd.models.sequence.dsin
    from deepctr.layers import custom_objects
    from deepctr.models import DSIN
    assert dsin_mod is deepctr_amd.models.sequence.dsin and dsin_mod.DSIN is DSIN and deepctr.models.sequence.DSIN is DSIN
    assert seq.BiLSTM is deepctr_amd.layers.sequence.BiLSTM and seq.BiasEncoding is deepctr_amd.layers.sequence.BiasEncoding
    assert custom_objects["BiLSTM"] is seq.BiLSTM


def _args(**kw):
    from deepctr_amd import _C
    base = dict(batch=4, x_stride=40, x_row_stride=8, seq_len=5, in_dim=8, units=8, n_layers=2, res_layers=0, merge_mode=4,
                recurrent_activation=0, route=0, out_stride=40, out_row_stride=8, out_bw_stride=40, out_bw_row_stride=8)
    base.update(kw)
    return _C.lstm.Args(**base)


def test_abi_argument_errors_without_a_gpu():
    from deepctr_amd import _C
    lib = _C.lib()
    f = lambda a: lib.dctr_bilstm_fwd(ctypes.byref(a), None)        # noqa: E731
    r = lambda a: lib.dctr_bilstm_route(ctypes.byref(a))           # noqa: E731
    assert lib.dctr_bilstm_fwd(None, None) == -1 and lib.dctr_bilstm_route(None) == -1 and lib.dctr_bilstm_workspace_bytes(None) == 0
    assert f(_args()) == -1                                         # x / layers / out missing
    assert b"bilstm_fwd" in lib.dctr_last_error()
    for bad in (dict(seq_len=0), dict(in_dim=0), dict(units=0), dict(n_layers=0), dict(n_layers=9), dict(batch=-1), dict(res_layers=-1),
                dict(x_row_stride=7), dict(x_stride=39), dict(out_row_stride=7), dict(out_stride=39), dict(merge_mode=5, out_row_stride=15),
                dict(merge_mode=6, out_bw_row_stride=7), dict(in_dim=6, x_row_stride=6, res_layers=2)):
        assert f(_args(**bad)) == -2 and r(_args(**bad)) == -2, bad
    for bad in (dict(merge_mode=7), dict(merge_mode=-1), dict(recurrent_activation=2), dict(route=4), dict(route=-1)):
        assert f(_args(**bad)) == -4, bad
    ptrs = (ctypes.c_void_p * 12)(*([16] * 12))
    ptrs[7] = None
    a = _args(x=16, out=16, layers=ctypes.cast(ptrs, ctypes.c_void_p))
    assert f(a) == -1 and b"layer 1" in lib.dctr_last_error()      # a null weight is reported before anything is launched
    ptrs[7] = 16
    a.merge_mode = 6
    assert f(a) == -1 and b"out_bw" in lib.dctr_last_error()
    a.merge_mode = 4
    ptrs[3] = 20
    assert r(a) == _C.lstm.ROUTE_RESIDENT and f(a) == -3 and b"16-B aligned" in lib.dctr_last_error()   # the resident copy reads 16 bytes
    a.route = _C.lstm.ROUTE_STREAMED
    a.batch = 0
    assert f(a) == 0                                                # the streamed route takes any kernel alignment
    ptrs[3], a.route = 16, _C.lstm.ROUTE_AUTO
    assert f(a) == 0                                                # complete arguments, empty batch: a no-op
    a.batch, a.route = 4, _C.lstm.ROUTE_WORKSPACE
    assert r(a) == _C.lstm.ROUTE_STREAMED and f(a) == -1 and b"workspace" in lib.dctr_last_error()
    a.workspace, a.workspace_bytes = 24, 1 << 30
    assert f(a) == -3                                               # a workspace that is not 16-byte aligned
    big = _args(units=2000, in_dim=2000, x_row_stride=2000, x_stride=10000, out_row_stride=2000, out_stride=10000, x=16, out=16,
                layers=ctypes.cast(ptrs, ctypes.c_void_p))
    assert r(big) == _C.lstm.ROUTE_STREAMED and f(big) == -1 and b"workspace" in lib.dctr_last_error()
    big.route = _C.lstm.ROUTE_RESIDENT
    assert r(big) == -5
    assert lib.dctr_bias_encoding_fwd(None, 4, 3, 5, 8, 120, 40, 8, None, None, None, None) == -1
    assert lib.dctr_bias_encoding_fwd(None, 0, 3, 5, 8, 120, 40, 8, None, None, None, None) == 0
    for bad in ((4, 0, 5, 8, 120, 40, 8), (4, 3, 5, 8, 120, 40, 7), (4, 3, 5, 8, 120, 39, 8), (4, 3, 5, 8, 119, 40, 8)):
        assert lib.dctr_bias_encoding_fwd(16, *(bad + (16, 16, 16, None))) == -2, bad


def test_routes_and_workspace_sizes_without_a_gpu():
    from deepctr_amd import ops
    u = 1
    while ops.bilstm_route(5, u, u, 3) == "resident":
        u += 1
    assert 16 < u < 128 and ops.bilstm_route(5, u, u, 3) == "streamed" and ops.bilstm_route(5, u - 1, u - 1, 3) == "resident"
    assert ops.bilstm_route(5, u - 1, u - 1, 3, route="streamed") == "streamed"
    with pytest.raises(Exception):
        ops.bilstm_route(5, u, u, 3, route="resident")
    # one layer needs two sequence tiles, not four: the boundary moves up; fewer steps move it up too
    assert ops.bilstm_route(5, u, u, 1) == "resident" and ops.bilstm_route(1, u, u, 3) == "resident"
    # DSIN's shapes: E = 32 keeps its kernels in LDS, E = 64 streams them
    assert ops.bilstm_route(5, 32, 32, 2) == "resident" and ops.bilstm_route(5, 64, 64, 2) == "streamed"
    assert ops.bilstm_workspace_bytes(4096, 5, 64, 64, 2) == 0
    # the tiles of a workgroup past the LDS: a workspace for at most 256 workgroups, capped at 256 MiB
    small, large = ops.bilstm_workspace_bytes(16, 5, 1024, 1024, 2), ops.bilstm_workspace_bytes(1 << 20, 5, 1024, 1024, 2)
    assert small == large > 160 * 1024 and large <= 256 << 20 and large % 16 == 0
    forced = ops.bilstm_workspace_bytes(16, 5, 16, 16, 2, route="workspace")
    assert 0 < forced < small
    assert ops.bilstm_macs(5, 64, 64, 2) == 5 * 2 * 4 * 64 * 128 * 2


def test_args_mirror_has_the_layout_the_c_compiler_gives_the_header(tmp_path):
    import os
    import shutil
    import subprocess
    from deepctr_amd import _C
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    cls = _C.lstm.Args
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dctr.h"', "int main(void) {",
             '    printf("sizeof %zu\\n", sizeof(dctr_lstm_args_t));', '    printf("ptrs %d\\n", DCTR_LSTM_LAYER_PTRS);',
             '    printf("maxl %d\\n", DCTR_LSTM_MAX_LAYERS);', '    printf("abi %d\\n", DCTR_ABI_VERSION);',
             '    printf("merges %d\\n", DCTR_LSTM_MERGE_FW + 10 * DCTR_LSTM_MERGE_BW + 100 * DCTR_LSTM_MERGE_SUM + 1000 * DCTR_LSTM_MERGE_MUL'
             ' + 10000 * DCTR_LSTM_MERGE_AVE + 100000 * DCTR_LSTM_MERGE_CONCAT + 1000000 * DCTR_LSTM_MERGE_NONE);',
             '    printf("routes %d\\n", DCTR_LSTM_ROUTE_AUTO + 10 * DCTR_LSTM_ROUTE_RESIDENT + 100 * DCTR_LSTM_ROUTE_STREAMED'
             ' + 1000 * DCTR_LSTM_ROUTE_WORKSPACE);']
    for fname, _ in cls._fields_:
        lines.append('    printf("%s %%zu\\n", offsetof(dctr_lstm_args_t, %s));' % (fname, fname))
    lines += ["    return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    M, R = _C.lstm.MERGES, _C.lstm.ROUTES
    for line in filter(None, out):
        field, val = line.split()
        if field == "ptrs":
            want = _C.lstm.LAYER_PTRS
        elif field == "maxl":
            want = _C.lstm.MAX_LAYERS
        elif field == "abi":
            want = 13
        elif field == "merges":
            want = sum(10 ** i * M[k] for i, k in enumerate(("fw", "bw", "sum", "mul", "ave", "concat", None)))
        elif field == "routes":
            want = sum(10 ** i * R[k] for i, k in enumerate((None, "resident", "streamed", "workspace")))
        else:
            want = ctypes.sizeof(cls) if field == "sizeof" else getattr(cls, field).offset
        assert int(val) == want, "%s: C says %s, ctypes %d" % (field, val, want)
