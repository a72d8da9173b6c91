"""GPU: dctr_bilstm_fwd (both LSTM stacks in one launch) and dctr_bias_encoding_fwd against the float64 oracle (tests/ref_dsin.py) over a
sweep of shapes, layers, merge modes, residuals, routes and recurrent activations, the saturated values, DSIN, BiLSTM and BiasEncoding
against the reference's own outputs (tests/golden/model_dsin_*.npz, bilstm_layer.npz, bias_encoding_layer.npz), DSIN's forward against
the oracle over a seeded fuzz of configurations, live weights, fit() on the autograd step and a user's program through the
``deepctr`` facade.

Tolerance: the attention stack's bar (``within_bar`` of tests/test_gpu_bst.py: |err| <= 1e-4 |ref| + 2e-6 max|ref of the sample|) against
the float64 oracle, and rtol 1e-4, atol 2e-5 on model logits as the BST and DIEN fuzzes use."""
import ctypes

import numpy as np
import pytest
import torch

from tests import ref_dsin as RS
from tests.dsin_util import DSIN_FIXTURES, dsin_problem, make_layers, oracle, randomise, to_dev
from tests.test_gpu_bst import within_bar
from tests.util import assert_close

pytestmark = pytest.mark.gpu

SWEEP_U = [4, 12, 16, 40, "streamed"]       # "streamed": the smallest u the library routes there (read from dctr_bilstm_route)
SWEEP_T = [1, 2, 5]
SWEEP_B = [1, 17, 33]


def smallest_streamed_units(T=5, L=3):
    from deepctr_amd import ops
    u = 1
    while ops.bilstm_route(T, u, u, L) != "streamed":
        u += 1
        assert u < 4096
    return u


def sweep_variants(L):
    """(res_layers, merge_mode, recurrent_activation) of every run of a sweep case."""
    return ([(0, mm, "sigmoid") for mm in RS.MERGE_MODES] + [(1, "ave", "sigmoid"), (L, "concat", "sigmoid"), (0, "sum", "hard_sigmoid"),
                                                              (L, None, "hard_sigmoid")])


def run_op(ops, xt, tl, res, mm, act, **kw):
    got = ops.bilstm(xt, tl, res_layers=res, merge_mode=mm, recurrent_activation=act, **kw)
    torch.cuda.synchronize()
    return np.stack([g.cpu().numpy() for g in got], axis=1) if mm is None else got.cpu().numpy()


@pytest.mark.parametrize("u", SWEEP_U)
def test_bilstm_op_vs_float64_oracle(device, u):
    from deepctr_amd import ops
    streamed = u == "streamed"
    if streamed:
        u = smallest_streamed_units()
        assert ops.bilstm_route(5, u - 1, u - 1, 3) == "resident"
    worst_all, routes = 0.0, set()
    for T in SWEEP_T:
        for B in SWEEP_B:
            rng = np.random.RandomState(u * 1000 + T * 10 + B)
            pad = 3
            xbuf = rng.standard_normal((B, T, u + pad)).astype(np.float32)        # padding columns after every step
            xt = torch.from_numpy(xbuf).to(device)
            for L in (1, 2, 3):
                for Din in (u, u + pad):                                          # the second: inputs wider than the units
                    layers = make_layers(rng, Din, u, L)
                    tl = to_dev(layers, device)
                    routes.add(ops.bilstm_route(T, Din, u, L))
                    variants = sweep_variants(L) if Din == u else [(0, "ave", "sigmoid"), (min(1, L - 1), "mul", "sigmoid")]
                    for res, mm, act in variants:
                        got = run_op(ops, xt[:, :, :Din], tl, res, mm, act)
                        ref = oracle(xbuf[:, :, :Din], layers, res, mm, act)
                        what = "u %d Din %d T %d B %d L %d res %d %s %s" % (u, Din, T, B, L, res, mm, act)
                        assert got.shape == ref.shape and np.isfinite(got).all(), what
                        worst = within_bar(got, ref)
                        worst_all = max(worst_all, worst)
                        assert worst <= 1.0, "%s: max err / bar %.3g" % (what, worst)
    assert not streamed or "streamed" in routes
    print("u %d (%s): max err / bar %.3g" % (u, "/".join(sorted(routes)), worst_all))


def test_both_routes_and_the_workspace_route_agree_with_the_oracle(device):
    from deepctr_amd import _C, ops
    rng = np.random.RandomState(21)
    T, u, B = 5, 16, 21
    for L in (1, 2):
        layers = make_layers(rng, u, u, L)
        x = rng.standard_normal((B, T, u)).astype(np.float32)
        ref = RS.bilstm(x, layers)
        assert ops.bilstm_route(T, u, u, L, route="resident") == "resident" and ops.bilstm_route(T, u, u, L, route="streamed") == "streamed"
        assert ops.bilstm_workspace_bytes(B, T, u, u, L, route="streamed") == 0 and ops.bilstm_workspace_bytes(B, T, u, u, L, route="workspace") > 0
        outs = []
        for route in ("resident", "streamed", "workspace"):
            outs.append(run_op(ops, torch.from_numpy(x).to(device), to_dev(layers, device), 0, "ave", "sigmoid", route=route))
            worst = within_bar(outs[-1], ref)
            print("%s route, %d layers: max err / bar %.3g" % (route, L, worst))
            assert worst <= 1.0
        assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2]), "the routes run the same step code in the same order"
    # the workspace route without a workspace is refused before anything is launched
    xt, tl = torch.from_numpy(x).to(device), to_dev(layers, device)
    out = torch.full((B, T, u), float("nan"), device=device)
    flat = [w for layer in tl for w in layer]
    ptrs = ops._ptr_array(flat)
    a = ops._bilstm_args(B, T, u, u, L, 0, "ave", "sigmoid", "workspace")
    a.x, a.out, a.layers = xt.data_ptr(), out.data_ptr(), ctypes.cast(ptrs, ctypes.c_void_p)
    assert _C.lib().dctr_bilstm_fwd(ctypes.byref(a), _C.stream_ptr()) == -1 and b"workspace" in _C.lib().dctr_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    # past the LDS the tiles go to the workspace on their own
    big = 64
    while ops.bilstm_workspace_bytes(3, 2, big, big, 1) == 0:
        big += 64
        assert big < 8192
    assert ops.bilstm_route(2, big, big, 1) == "streamed"
    layers = make_layers(rng, big, big, 1)
    x = rng.standard_normal((3, 2, big)).astype(np.float32)
    worst = within_bar(run_op(ops, torch.from_numpy(x).to(device), to_dev(layers, device), 1, "ave", "sigmoid"), RS.bilstm(x, layers, 1))
    print("workspace route at u %d: max err / bar %.3g" % (big, worst))
    assert worst <= 1.0


def test_strided_views_leave_their_neighbours_alone(device):
    from deepctr_amd import ops
    rng = np.random.RandomState(22)
    T, u, B = 5, 12, 19
    layers = make_layers(rng, u, u, 2)
    tl = to_dev(layers, device)
    xbuf = rng.standard_normal((B, T + 1, u + 5)).astype(np.float32)               # padding after every step and after every sample
    x = xbuf[:, :T, :u]
    xt = torch.from_numpy(xbuf).to(device)
    nan = np.float32("nan").view(np.uint32)
    for mm, w in (("ave", u), ("concat", 2 * u), (None, u)):
        bufs = [torch.full((B, T + 2, w + 3), float("nan"), device=device) for _ in range(2 if mm is None else 1)]
        views = [b[:, 1:T + 1, 2:2 + w] for b in bufs]
        ops.bilstm(xt[:, :T, :u], tl, merge_mode=mm, out=tuple(views) if mm is None else views[0])
        ref = RS.bilstm(x, layers, 0, mm)
        for b, r in zip(bufs, ref if mm is None else [ref]):
            got = b.cpu().numpy()
            assert within_bar(got[:, 1:T + 1, 2:2 + w], r) <= 1.0, mm
            got[:, 1:T + 1, 2:2 + w] = np.nan
            assert (got.view(np.uint32) == nan).all(), "%s: the padding was written" % (mm,)
    assert torch.equal(xt.cpu(), torch.from_numpy(xbuf)), "the input was written"


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_saturated_gates_give_the_oracles_values_and_no_nan(device, sign):
    """Zero kernels, biases of +-30 (and +-200): every pre-activation is its bias.  Inside every sample the gate units alternate in
    sign — i unit by unit, f pair by pair, o four by four — so that each sample holds units of size 1 beside the units float64 leaves
    at the 1e-13 residue of a saturated sigmoid and float32 at 0: the bar is scaled by the former."""
    from deepctr_amd import ops
    rng = np.random.RandomState(23)
    T, u, B = 4, 16, 5
    x = rng.standard_normal((B, T, u)).astype(np.float32)
    xt = torch.from_numpy(x).to(device)
    j = np.arange(u)
    zero_w, zero_u = np.zeros((u, 4 * u), np.float32), np.zeros((u, 4 * u), np.float32)
    for mag in (30.0, 200.0):
        for gate_sign in (1.0, -1.0):
            b = np.concatenate([np.where(j % 2 == 0, 1.0, -1.0) * gate_sign, np.where(j % 4 < 2, 1.0, -1.0) * gate_sign, np.full(u, sign),
                                np.where(j % 8 < 4, 1.0, -1.0) * gate_sign]).astype(np.float32) * mag
            layers = [(zero_w, zero_u, b, zero_w, zero_u, -b if gate_sign > 0 else b)] * 2
            for act in ("sigmoid", "hard_sigmoid"):
                for mm in ("ave", "mul", "concat"):
                    got = run_op(ops, xt, to_dev(layers, device), 0, mm, act)
                    ref = RS.bilstm(x, layers, 0, mm, act)
                    what = "+-%g, gates %+d, %s, %s" % (mag, gate_sign, act, mm)
                    assert np.isfinite(got).all(), what
                    worst = within_bar(got, ref)
                    print("%s: max err / bar %.3g" % (what, worst))
                    assert worst <= 1.0, what


@pytest.mark.parametrize("B", [1, 33])
def test_bias_encoding_in_place_on_a_strided_view(device, B):
    from deepctr_amd import ops
    rng = np.random.RandomState(24 + B)
    S, T, E = 3, 5, 12
    buf = rng.standard_normal((B, S + 1, T + 2, E + 3)).astype(np.float32)
    sess, seq, item = (rng.standard_normal(n).astype(np.float32) for n in (S, T, E))
    bt = torch.from_numpy(buf).to(device)
    y = ops.bias_encoding(bt[:, :S, 1:T + 1, :E], *(torch.from_numpy(v).to(device) for v in (sess.reshape(S, 1, 1), seq.reshape(1, T, 1),
                                                                                           item.reshape(1, 1, E))))
    assert y.data_ptr() == bt[:, :S, 1:T + 1, :E].data_ptr()
    got = bt.cpu().numpy()
    ref = RS.bias_encoding(buf[:, :S, 1:T + 1, :E].astype(np.float64), sess, seq, item)
    assert within_bar(got[:, :S, 1:T + 1, :E], ref) <= 1.0
    keep = np.ones(buf.shape, bool)
    keep[:, :S, 1:T + 1, :E] = False
    assert np.array_equal(got[keep], buf[keep]), "the padding was written"


def test_layer_fixtures_match_reference_code(device):
    from deepctr_amd.layers import BiasEncoding, BiLSTM
    from tests.dsin_util import BILSTM_TAGS, bias_encoding_case, bilstm_case
    from tests.util import load_golden
    g = load_golden("bilstm_layer")
    for tag in BILSTM_TAGS:
        cfg, x, ws, y = bilstm_case(g, tag)
        layer = BiLSTM(cfg["units"], layers=cfg["layers"], res_layers=cfg["res_layers"], merge_mode=cfg["merge_mode"], device=device)
        layer.build((None,) + x.shape[1:])
        layer.set_weights([w for lw in ws for w in lw])
        got = layer(torch.from_numpy(x).to(device))
        got = np.stack([t.cpu().numpy() for t in got], axis=1) if cfg["merge_mode"] is None else got.cpu().numpy()
        ref = oracle(x, ws, cfg["res_layers"], cfg["merge_mode"], "sigmoid")
        assert got.shape == y.shape, tag
        print("%s: max err / bar %.3g (oracle) %.3g (reference code)" % (tag, within_bar(got, ref), within_bar(got, y.astype(np.float64))))
        assert within_bar(got, ref) <= 1.0 and within_bar(got, y.astype(np.float64)) <= 1.0, tag
    g = load_golden("bias_encoding_layer")
    for tag in ("sess3", "sess2"):
        S, xs, ws, ys = bias_encoding_case(g, tag)
        layer = BiasEncoding(S, device=device)
        inputs = [torch.from_numpy(x).to(device) for x in xs]
        layer.build([(None,) + xs[0].shape[1:]] * S)
        layer.set_weights(list(ws))
        got = layer(inputs)
        assert len(got) == S
        for o, y in zip(got, ys):
            assert within_bar(o.cpu().numpy(), y.astype(np.float64)) <= 1.0, tag


@pytest.mark.parametrize("name", DSIN_FIXTURES)
def test_dsin_matches_reference_code(device, name):
    """A model fixture: probabilities at three batch sizes and a list feed, the logits against the float64 oracle."""
    from tests.dsin_util import build_dsin, fixture_feed, fixture_weights
    from tests.test_gpu_models import check_probs
    from tests.util import golden_meta, load_golden
    g = load_golden(name)
    model = build_dsin(golden_meta(g), device)
    model.set_weights_by_name(fixture_weights(g))
    feed = fixture_feed(g)
    assert (feed["sess_length"] == 0).any()                                 # length-0 rows are compared, not excluded
    rows = np.ones(g["y"].shape[0], bool)
    for bs in (256, 5, 37):
        check_probs(model.predict(feed, batch_size=bs), g["y"], "%s bs=%d" % (name, bs), rows)
    y = model.predict([feed[n] for n in model.input_names], batch_size=64)
    check_probs(y, g["y"], name + " list feed", rows)
    assert_close(np.asarray(model.predict_logits(feed, batch_size=256)).reshape(-1),
                 RS.run_fixture(g, np.float64, task="regression").reshape(-1), rtol=1e-4, atol=2e-5, what=name + " logits vs float64")


@pytest.mark.parametrize("seed", range(20))
def test_fuzz_predict_logits_vs_oracle(device, seed):
    """Seeded random DSIN configurations against the float64 oracle: rtol 1e-4, atol 2e-5 on the logit, as the BST and DIEN fuzzes."""
    from deepctr_amd.models import DSIN
    rng = np.random.RandomState(5000 + seed)
    heads = int(rng.choice([1, 2, 4]))
    d = int(rng.choice([1, 2, 3, 4]))
    E = heads * d
    n_feat = 2 if E >= 2 and rng.rand() < 0.6 else 1
    w0 = E if n_feat == 1 else int(rng.randint(1, E))
    feats = (("item", w0),) if n_feat == 1 else (("item", w0), ("cate", E - w0))
    S, T = int(rng.randint(1, 6)), int(rng.randint(1, 8))
    bias, hash_, use_bn = bool(seed % 2), bool(rng.rand() < 0.3), bool(rng.rand() < 0.3)
    task = "regression" if rng.rand() < 0.25 else "binary"
    n = int(rng.randint(4, 150))
    cols, names, feed = dsin_problem(rng, n, feats, S, T, hash_, extra=bool(rng.rand() < 0.5))
    assert (feed["sess_length"] == 0).any() and feed["sess_length"][3] == S and not feed["sess_0_item"][3].any()   # empty sessions inside sess_length
    kw = dict(sess_max_count=S, bias_encoding=bias, att_embedding_size=d, att_head_num=heads, dnn_hidden_units=(16, 8), dnn_use_bn=use_bn,
              task=task)
    model = DSIN(cols, names, device=device, **kw)
    w = randomise(model, rng)
    what = "seed %d: heads=%d d=%d feats=%s S=%d T=%d bias=%d hash=%d bn=%d %s n=%d" % (seed, heads, d, feats, S, T, bias, hash_, use_bn, task, n)
    got = np.asarray(model.predict_logits(feed, batch_size=64)).reshape(-1)
    ref = RS.dsin(cols, names, w, feed, **dict(kw, task="regression")).reshape(-1)
    assert np.isfinite(got).all()
    assert_close(got, ref, rtol=1e-4, atol=2e-5, what=what)


def test_live_model_weights(device):
    from deepctr_amd.models import DSIN
    rng = np.random.RandomState(31)
    cols, names, feed = dsin_problem(rng, 50)
    model = DSIN(cols, names, sess_max_count=3, bias_encoding=True, att_embedding_size=3, att_head_num=4, dnn_hidden_units=(16, 8), device=device)
    randomise(model, rng)
    y0 = np.asarray(model.predict(feed, batch_size=64)).copy()
    assert np.array_equal(np.asarray(model.predict(feed, batch_size=64)), y0)
    for ws in model.bilstm.operands() + [tuple(model.bias_enc.weights)]:
        for w in ws:
            with torch.no_grad():
                w.add_(0.05)
            y1 = np.asarray(model.predict(feed, batch_size=64)).copy()
            assert not np.array_equal(y1, y0)
            y0 = y1
    ref = RS.dsin(cols, names, {k: np.asarray(v) for k, v in model.get_weights_by_name().items()}, feed, sess_max_count=3, bias_encoding=True,
                  att_embedding_size=3, att_head_num=4, dnn_hidden_units=(16, 8), task="regression").reshape(-1)
    assert_close(np.asarray(model.predict_logits(feed, batch_size=64)).reshape(-1), ref, rtol=1e-4, atol=2e-5, what="live weights")


@pytest.mark.parametrize("bias", [False, True])
def test_fit_takes_the_autograd_step_and_predict_follows(device, bias):
    from deepctr_amd import engine, training, training_hip
    from deepctr_amd.models import DSIN
    rng = np.random.RandomState(9)
    n = 1024
    cols, names, feed = dsin_problem(rng, n, vocab=20)
    y = ((feed["item"] % 2) ^ (feed["sess_0_item"][:, 0] % 2)).astype(np.float32)
    model = DSIN(cols, names, sess_max_count=3, bias_encoding=bias, att_embedding_size=3, att_head_num=4, dnn_hidden_units=(32, 16), device=device)
    assert not training_hip.supported(model)
    before = {k: t.clone() for k, t in model.bilstm.named_weights() + model.transformer.named_weights()}
    model.compile("adam", "binary_crossentropy")
    hist = model.fit(feed, y, batch_size=256, epochs=4, verbose=0)
    loss = hist.history["loss"]
    assert np.isfinite(loss).all() and loss[-1] < loss[0], loss
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


def test_a_users_program_runs_through_the_facade(device):
    """Two sessions of two behaviour features that share their SparseFeats' embeddings, sess_length, compile, fit, predict."""
    from deepctr.feature_column import DenseFeat, SparseFeat, VarLenSparseFeat, get_feature_names
    from deepctr.models import DSIN
    n_rows, n_videos, n_genres, steps = 6, 9, 4, 3
    rng = np.random.RandomState(3)
    columns = [SparseFeat("viewer", n_rows, embedding_dim=6), SparseFeat("video", n_videos + 1, embedding_dim=4),
               SparseFeat("genre", n_genres + 1, embedding_dim=4), DenseFeat("watch_share", 1)]
    data = {"viewer": np.arange(n_rows), "video": rng.randint(1, n_videos + 1, n_rows), "genre": rng.randint(1, n_genres + 1, n_rows),
            "watch_share": rng.rand(n_rows), "sess_length": np.array([2, 1, 0, 2, 1, 2])}
    for s in range(2):
        for feat, top in (("video", n_videos), ("genre", n_genres)):
            name = "sess_%d_%s" % (s, feat)
            columns.append(VarLenSparseFeat(SparseFeat(name, top + 1, embedding_dim=4, embedding_name=feat), maxlen=steps))
            watched = rng.randint(1, top + 1, (n_rows, steps))
            watched[np.arange(steps)[None, :] >= rng.randint(0, steps + 1, (n_rows, 1))] = 0
            data[name] = watched
    x = {name: data[name] for name in get_feature_names(columns)}
    x["sess_length"] = data["sess_length"]
    y = np.array([1, 0, 0, 1, 1, 0])
    model = DSIN(columns, ["video", "genre"], sess_max_count=2, att_embedding_size=2, att_head_num=4, dnn_hidden_units=[8, 4], dnn_dropout=0.3)
    model.compile("adam", "binary_crossentropy", metrics=["binary_crossentropy"])
    history = model.fit(x, y, verbose=0, epochs=3)
    assert len(history.history["loss"]) == 3 and np.isfinite(history.history["loss"]).all()
    p = np.asarray(model.predict(x, batch_size=4))
    assert p.shape == (n_rows, 1) and ((p > 0) & (p < 1)).all()
