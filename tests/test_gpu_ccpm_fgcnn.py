"""GPU: dctr_fieldconv_fwd (the conv / pool stack of CCPM and FGCNNLayer in one launch) and dctr_kmax_pool_fwd against the float64 oracle
(tests/ref_fieldconv.py) over a sweep of shapes, widths, channel chains, poolings, stage counts, routes and strided operands, the
saturated values, CCPM, FGCNN, FGCNNLayer and KMaxPooling against the reference's own outputs (tests/golden/model_ccpm_*.npz,
model_fgcnn_*.npz, fgcnn_layer.npz, kmax_layer.npz), the models' forwards against the oracle over a seeded fuzz of configurations, live
weights, fit() on the autograd step and a user's program through the ``deepctr`` facade.

Tolerance: k-max pooling is bit-exact; the conv stack holds the attention stack's bar (``within_bar`` of tests/test_gpu_bst.py:
|err| <= 1e-4 |ref| + 2e-6 max|ref of the sample|) against the float64 oracle (sorted top-k and max are 1-Lipschitz in the sup norm, so a
float32 near-tie that selects another element than float64 does not break it), and rtol 1e-4, atol 2e-5 on model logits as the BST, DIEN
and DSIN tests use."""
import ctypes

import numpy as np
import pytest
import torch

from tests import ref_fieldconv as RF
from tests.ccpm_fgcnn_util import (CCPM_FIXTURES, FGCNN_FIXTURES, FGCNN_LAYER_TAGS, FIXTURES, build_model, fgcnn_layer_case, fixture_feed,
                                   fixture_weights, make_stack, problem, randomise)
from tests.test_gpu_bst import within_bar
from tests.util import assert_close, golden_meta, load_golden

pytestmark = pytest.mark.gpu

SWEEP_F = [1, 2, 5, 7, 13]
SWEEP_E = [1, 4, 5, 17]
SWEEP_B = [1, 17, 33]
CHAINS = [(1, 3), (1, 16, 17), (4, 20, 1)]


def to_dev(arrs, device):
    return [torch.from_numpy(a).to(device) for a in arrs]


def run_op(ops, x, ks, bs, pools, device, **kw):
    got = ops.field_conv(torch.from_numpy(x).to(device), to_dev(ks, device), to_dev(bs, device), pools, **kw)
    torch.cuda.synchronize()
    if isinstance(got, tuple):
        return got[0].cpu().numpy(), [m.cpu().numpy() for m in got[1]]
    return got.cpu().numpy()


def pools_for(rng, F, n, kind):
    """n poolings over F rows of the wanted kind ('kmax', 'max' or 'mixed'), k in {1, 3, rows} and p in {1, 2, 3}, never an empty map."""
    out, rows = [], F
    for s in range(n):
        kmax = kind == "kmax" or (kind == "mixed" and (s + F) % 2 == 0)
        if kmax:
            arg = min(int(rng.choice([1, 3, rows])), rows)
            out.append(("kmax", arg))
            rows = arg
        else:
            arg = int(rng.choice([p for p in (1, 2, 3) if p <= rows]))
            out.append(("max", arg))
            rows //= arg
    return out


@pytest.mark.parametrize("n", [1, 2, 7, 65])
def test_kmax_pool_is_bit_exact(device, n):
    from deepctr_amd import ops
    for inner in (1, 5, 64):
        rng = np.random.RandomState(n * 100 + inner)
        x = rng.standard_normal((3, n, inner)).astype(np.float32)
        x[0] = np.round(x[0])                                   # repeated values
        if n > 1:
            x[1, 0], x[1, -1] = np.inf, -np.inf
            x[2, :, 0] = 1.5                                    # a line of one value
        xt = torch.from_numpy(x).to(device)
        for k in sorted(set((1, min(3, n), n))):
            got = ops.kmax_pool(xt, k, 1).cpu().numpy()
            assert np.array_equal(got, (-np.sort(-x, axis=1))[:, :k]), (n, inner, k)
    # any axis of a tensor of any rank
    x = np.random.RandomState(n).standard_normal((2, 3, n, 2, 3)).astype(np.float32)
    for axis in range(5):
        k = min(2, x.shape[axis])
        got = ops.kmax_pool(torch.from_numpy(x).to(device), k, axis).cpu().numpy()
        assert np.array_equal(got, RF.kmax(x, k, axis)), axis
    assert np.array_equal(ops.kmax_pool(torch.from_numpy(x).to(device), 1, -3).cpu().numpy(), RF.kmax(x, 1, 2))


@pytest.mark.parametrize("F", SWEEP_F)
def test_field_conv_op_vs_float64_oracle(device, F):
    from deepctr_amd import ops
    worst_all, runs = 0.0, 0
    for E in SWEEP_E:
        for B in SWEEP_B:
            rng = np.random.RandomState(F * 1000 + E * 10 + B)
            for chain in CHAINS:
                L = len(chain) - 1
                for kind in ("kmax", "max", "mixed"):
                    widths = [int(w) for w in rng.choice([1, 2, 6, 7, F + 3], size=L)]
                    if kind == "mixed" and B == 17:
                        widths[0] = F + 3                           # wider than the map
                    ks, bs = make_stack(rng, chain, widths)
                    pools = pools_for(rng, F, L, kind)
                    x = (0.7 * rng.standard_normal((B, F, E) + ((chain[0],) if chain[0] > 1 else ()))).astype(np.float32)
                    souts = (B + E) % 2 == 0
                    got = run_op(ops, x, ks, bs, pools, device, stage_outs=True if souts else None)
                    ref, maps = RF.field_conv(x, ks, bs, pools)
                    what = "F %d E %d B %d chain %s widths %s pools %s" % (F, E, B, chain, widths, pools)
                    if souts:
                        got, gmaps = got
                        for a, b in zip(gmaps, maps):
                            assert a.shape == b.shape and within_bar(a, b) <= 1.0, what
                    assert got.shape == ref.shape and np.isfinite(got).all(), what
                    worst = within_bar(got, ref)
                    worst_all = max(worst_all, worst)
                    runs += 1
                    assert worst <= 1.0, "%s: max err / bar %.3g" % (what, worst)
    print("F %d: %d runs, max err / bar %.3g" % (F, runs, worst_all))


@pytest.mark.parametrize("L", [1, 2, 4])
def test_stage_counts_and_mixed_poolings_in_one_stack(device, L):
    from deepctr_amd import ops
    rng = np.random.RandomState(40 + L)
    B, F, E = 33, 13, 5
    chain = (1, 14, 16, 18, 20)[:L + 1]
    widths = (7, 6, 2, F + 3)[:L]
    pools = [("max", 2), ("kmax", 5), ("max", 3), ("kmax", 1)][:L]
    ks, bs = make_stack(rng, chain, widths)
    x = (0.7 * rng.standard_normal((B, F, E))).astype(np.float32)
    got, gmaps = run_op(ops, x, ks, bs, pools, device, stage_outs=True)
    ref, maps = RF.field_conv(x, ks, bs, pools)
    assert within_bar(got, ref) <= 1.0 and len(gmaps) == L
    for a, b in zip(gmaps, maps):
        assert a.shape == b.shape and within_bar(a, b) <= 1.0
    assert np.array_equal(gmaps[-1], got)
    assert np.array_equal(run_op(ops, x, ks, bs, pools, device), got), "the stage outputs change nothing"
    # keras' 4-D kernels [w, 1, C_in, C_out] are the same operands
    got4 = run_op(ops, x, [k[:, None] for k in ks], bs, pools, device)
    assert np.array_equal(got4, got)


def smallest_streamed_channels(F=13, E=5):
    from deepctr_amd import ops
    c = 1
    while ops.field_conv_route(F, E, [(7, 1, c), (7, c, c)], [("max", 2), ("kmax", 3)]) != "streamed":
        c += 1
        assert c < 4096
    return c


def test_every_route_agrees_with_the_oracle_and_with_the_others(device):
    from deepctr_amd import _C, ops
    rng = np.random.RandomState(21)
    B, F, E = 21, 13, 5
    for chain, widths, pools in (((1, 16, 17), (7, 2), [("max", 2), ("kmax", 3)]), ((4, 20, 1), (6, 16), [("kmax", 7), ("max", 3)])):
        ks, bs = make_stack(rng, chain, widths)
        x = (0.7 * rng.standard_normal((B, F, E) + ((chain[0],) if chain[0] > 1 else ()))).astype(np.float32)
        ref, _ = RF.field_conv(x, ks, bs, pools)
        assert ops.field_conv_route(F, E, ks, pools, route="resident") == "resident"
        assert ops.field_conv_route(F, E, ks, pools, route="streamed") == "streamed"
        assert ops.field_conv_workspace_bytes(B, F, E, ks, pools, route="streamed") == 0
        assert ops.field_conv_workspace_bytes(B, F, E, ks, pools, route="workspace") > 0
        outs = []
        for route in ("resident", "streamed", "workspace"):
            outs.append(run_op(ops, x, ks, bs, pools, device, route=route))
            worst = within_bar(outs[-1], ref)
            print("%s route, chain %s: max err / bar %.3g" % (route, chain, worst))
            assert worst <= 1.0
        assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2]), "the routes run the same step code in the same order"
    # the workspace route without a workspace is refused before anything is written
    xt, kt, bt = torch.from_numpy(x).to(device), to_dev(ks, device), to_dev(bs, device)
    out = torch.full(ref.shape, float("nan"), device=device)
    a, keep, _, _ = ops._field_conv_args("field_conv", B, F, E, ks, pools, "workspace")
    kp, bp = ops._ptr_array(kt), ops._ptr_array(bt)
    a.x, a.out = xt.data_ptr(), out.data_ptr()
    a.kernels, a.biases = ctypes.cast(kp, ctypes.c_void_p), ctypes.cast(bp, ctypes.c_void_p)
    assert _C.lib().dctr_fieldconv_fwd(ctypes.byref(a), _C.stream_ptr()) == -1 and b"workspace" in _C.lib().dctr_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    # the smallest shape the library itself routes off "resident"
    c = smallest_streamed_channels(F, E)
    assert ops.field_conv_route(F, E, [(7, 1, c - 1), (7, c - 1, c - 1)], [("max", 2), ("kmax", 3)]) == "resident"
    ks, bs = make_stack(rng, (1, c, c), (7, 7))
    pools = [("max", 2), ("kmax", 3)]
    x = (0.7 * rng.standard_normal((3, F, E))).astype(np.float32)
    worst = within_bar(run_op(ops, x, ks, bs, pools, device), RF.field_conv(x, ks, bs, pools)[0])
    print("streamed on its own at %d channels: max err / bar %.3g" % (c, worst))
    assert worst <= 1.0
    # past the LDS the maps go to the workspace on their own
    big = 64
    while ops.field_conv_workspace_bytes(3, F, 2, [(3, 1, big)], [("max", 2)]) == 0:
        big += 64
        assert big < 65536
    ks, bs = make_stack(rng, (1, big), (3,))
    x = (0.7 * rng.standard_normal((3, F, 2))).astype(np.float32)
    worst = within_bar(run_op(ops, x, ks, bs, [("max", 2)], device), RF.field_conv(x, ks, bs, [("max", 2)])[0])
    print("workspace route at %d channels: max err / bar %.3g" % (big, worst))
    assert worst <= 1.0


def test_a_workgroup_walks_several_tiles(device):
    """More tiles than workgroups on every route: the workspace route holds 256 workgroups, the others 2048, so a workgroup takes a
    second tile with the maps (and, resident, the kernels' images) of its first one still in place."""
    from deepctr_amd import ops
    rng = np.random.RandomState(25)
    F, chain, widths, pools = 5, (1, 3, 17), (6, 3), [("max", 2), ("kmax", 2)]
    ks, bs = make_stack(rng, chain, widths)
    for B, E, routes in ((1031, 4, ("workspace",)), (8200, 17, ("resident", "streamed"))):
        x = (0.7 * rng.standard_normal((B, F, E))).astype(np.float32)
        ref, maps = RF.field_conv(x, ks, bs, pools)
        for route in routes:
            cols_per_tile = 16 if route == "workspace" else 64
            assert B * E > cols_per_tile * (256 if route == "workspace" else 2048)
            assert route == "workspace" or ops.field_conv_workspace_bytes(B, F, E, ks, pools, route=route) == 0
            got, gmaps = run_op(ops, x, ks, bs, pools, device, route=route, stage_outs=True)
            worst = max(within_bar(got, ref), within_bar(gmaps[0], maps[0]))
            print("%s route, %d columns: max err / bar %.3g" % (route, B * E, worst))
            assert got.shape == ref.shape and worst <= 1.0, route


def test_strided_operands_leave_their_neighbours_alone(device):
    from deepctr_amd import ops
    rng = np.random.RandomState(22)
    B, F, E = 19, 7, 5
    chain, widths, pools = (1, 3, 17), (6, 3), [("max", 2), ("kmax", 2)]
    ks, bs = make_stack(rng, chain, widths)
    kt, bt = to_dev(ks, device), to_dev(bs, device)
    x_off, out_off = 3, 5
    xbuf = rng.standard_normal((B, x_off + F * E + 4)).astype(np.float32)
    x = xbuf[:, x_off:x_off + F * E].reshape(B, F, E)
    ref, maps = RF.field_conv(x, ks, bs, pools)
    n_out = ref[0].size
    out = torch.full((B, out_off + n_out + 6), float("nan"), device=device)
    s0 = torch.full((B, maps[0][0].size + 7), float("nan"), device=device)
    ret = ops.field_conv(torch.from_numpy(xbuf).to(device), kt, bt, pools, fields=F, dim=E, x_offset=x_off, out=out, out_offset=out_off,
                         stage_outs=[s0, None])
    torch.cuda.synchronize()
    assert ret[0] is out and ret[1][0] is s0
    got = out.cpu().numpy()
    assert within_bar(got[:, out_off:out_off + n_out], ref.reshape(B, -1)) <= 1.0
    assert np.isnan(got[:, :out_off]).all() and np.isnan(got[:, out_off + n_out:]).all(), "the surroundings were written"
    g0 = s0.cpu().numpy()
    assert within_bar(g0[:, :maps[0][0].size], maps[0].reshape(B, -1)) <= 1.0 and np.isnan(g0[:, maps[0][0].size:]).all()
    # the same through every route
    for route in ("streamed", "workspace"):
        o2 = torch.full_like(out, float("nan"))
        ops.field_conv(torch.from_numpy(xbuf).to(device), kt, bt, pools, fields=F, dim=E, x_offset=x_off, out=o2, out_offset=out_off, route=route)
        assert np.array_equal(o2.cpu().numpy(), got, equal_nan=True), route


def test_saturated_values_are_exactly_one_without_nan(device):
    from deepctr_amd import ops
    rng = np.random.RandomState(23)
    B, F, E = 5, 7, 4
    for mag in (30.0, 1e4, 1e30):
        x = (mag * np.sign(rng.standard_normal((B, F, E)))).astype(np.float32)
        ks = [np.full((1, 1, 3), 1.0, np.float32), (np.eye(3, dtype=np.float32) * 40.0).reshape(1, 3, 3)]
        bs = [np.zeros(3, np.float32), np.zeros(3, np.float32)]
        for pools in ([("max", 1), ("max", 1)], [("kmax", F), ("max", 2)]):
            got, gmaps = run_op(ops, x, ks, bs, pools, device, stage_outs=True)
            assert np.isfinite(got).all() and np.isfinite(gmaps[0]).all(), (mag, pools)
            assert set(np.unique(gmaps[0])) <= {-1.0, 1.0} and set(np.unique(got)) <= {-1.0, 1.0}, (mag, pools)
            ref, _ = RF.field_conv(x, ks, bs, pools)
            assert np.array_equal(got, ref.astype(np.float32)), (mag, pools)


def test_layer_fixtures_match_reference_code(device):
    from deepctr_amd.layers import FGCNNLayer, KMaxPooling
    g = load_golden("fgcnn_layer")
    for tag in FGCNN_LAYER_TAGS:
        cfg, x, w, y = fgcnn_layer_case(g, tag)
        layer = FGCNNLayer(cfg["filters"], cfg["kernel_width"], cfg["new_maps"], cfg["pooling_width"], device=device)
        layer.build((None,) + x.shape[1:])
        layer.set_weights([w["%s/%s" % (n, p)] for i in range(len(cfg["filters"])) for n in RF.conv_names(i + 1)[-1:] + RF.conv_names(i + 1, "dense")[-1:]
                           for p in ("kernel", "bias")])
        got = layer(torch.from_numpy(x).to(device)).cpu().numpy()
        ref = RF.fgcnn_layer(x, w, cfg["filters"], cfg["kernel_width"], cfg["new_maps"], cfg["pooling_width"])
        assert got.shape == y.shape, tag
        print("%s: max err / bar %.3g (oracle) %.3g (reference code)" % (tag, within_bar(got, ref), within_bar(got, y.astype(np.float64))))
        assert within_bar(got, ref) <= 1.0 and within_bar(got, y.astype(np.float64)) <= 1.0, tag
    g = load_golden("kmax_layer")
    for tag in ("d3", "d4"):
        x = g[tag + "/x"]
        for axis in range(1, x.ndim):
            for k in sorted(set((1, min(3, x.shape[axis]), x.shape[axis]))):
                got = KMaxPooling(k=k, axis=axis, device=device)(torch.from_numpy(x).to(device)).cpu().numpy()
                assert np.array_equal(got, g["%s/axis%d/k%d" % (tag, axis, k)]), (tag, axis, k)


@pytest.mark.parametrize("name", FIXTURES)
def test_models_match_reference_code(device, name):
    """A model fixture: probabilities at three batch sizes and a list feed, the logits against the float64 oracle."""
    from tests.test_gpu_models import check_probs
    g = load_golden(name)
    model = build_model(golden_meta(g), device)
    model.set_weights_by_name(fixture_weights(g))
    feed = fixture_feed(g)
    rows = np.ones(g["y"].shape[0], bool)
    for bs in (256, 5, 37):
        check_probs(model.predict(feed, batch_size=bs), g["y"], "%s bs=%d" % (name, bs), rows)
    y = model.predict([feed[n] for n in model.input_names], batch_size=64)
    check_probs(y, g["y"], name + " list feed", rows)
    assert_close(np.asarray(model.predict_logits(feed, batch_size=256)).reshape(-1),
                 RF.run_fixture(g, np.float64, task="regression").reshape(-1), rtol=1e-4, atol=2e-5, what=name + " logits vs float64")


def fuzz_case(rng, seed):
    E = int(rng.choice([1, 2, 4, 5, 8]))
    F = int(rng.randint(2, 10))
    L = int(rng.randint(0, 4))
    widths = [int(rng.choice([1, 2, 3, 6, 7])) for _ in range(L)]
    filters = [int(rng.choice([1, 3, 4, 17])) for _ in range(L)]
    kw = dict(conv_kernel_width=widths, conv_filters=filters, dnn_hidden_units=(16, 8) if rng.rand() < 0.8 else (),
              task="regression" if rng.rand() < 0.25 else "binary")
    if seed % 2:
        pools, rows = [], F
        for _ in range(L):
            pools.append(int(rng.choice([p for p in (1, 2, 3) if p <= rows])))
            rows //= pools[-1]
        kw.update(new_maps=[int(rng.randint(1, 4)) for _ in range(L)], pooling_width=pools)
    return F, E, kw


@pytest.mark.parametrize("seed", range(12))
def test_fuzz_predict_logits_vs_oracle(device, seed):
    """Seeded random CCPM (even seeds) and FGCNN (odd seeds) configurations against the float64 oracle: rtol 1e-4, atol 2e-5 on the logit."""
    from deepctr_amd import models
    rng = np.random.RandomState(7000 + seed)
    F, E, kw = fuzz_case(rng, seed)
    fg = bool(seed % 2)
    n = int(rng.randint(4, 150))
    cols, feed = problem(rng, n, F=F, E=E, hash_=bool(rng.rand() < 0.3), seq=bool(rng.rand() < 0.5), dense=fg and bool(rng.rand() < 0.5))
    model = (models.FGCNN if fg else models.CCPM)(cols, cols, device=device, **kw)
    w = randomise(model, rng)
    what = "seed %d: %s F=%d E=%d n=%d %s" % (seed, "FGCNN" if fg else "CCPM", F, E, n, kw)
    got = np.asarray(model.predict_logits(feed, batch_size=64)).reshape(-1)
    ref = (RF.fgcnn if fg else RF.ccpm)(cols, cols, w, feed, **dict(kw, task="regression", dtype=np.float64)).reshape(-1)
    assert np.isfinite(got).all()
    assert_close(got, ref, rtol=1e-4, atol=2e-5, what=what)


@pytest.mark.parametrize("which", ["CCPM", "FGCNN"])
def test_live_model_weights(device, which):
    from deepctr_amd import models
    rng = np.random.RandomState(31)
    cols, feed = problem(rng, 50, F=7, E=4, seq=True)
    kw = dict(conv_kernel_width=(6, 3), conv_filters=(4, 3), dnn_hidden_units=(16, 8))
    if which == "FGCNN":
        kw.update(new_maps=(2, 1), pooling_width=(2, 2))
    model = getattr(models, which)(cols, cols, device=device, **kw)
    randomise(model, rng)
    y0 = np.asarray(model.predict(feed, batch_size=64)).copy()
    assert np.array_equal(np.asarray(model.predict(feed, batch_size=64)), y0)
    names = [k for k, _ in model.named_weights() if k.startswith("conv2d") or (which == "FGCNN" and k.startswith(("dense/", "dense_1/", "fgsparse")))]
    assert len(names) >= 4
    live = dict(model.named_weights())
    for k in names:
        with torch.no_grad():
            live[k].add_(0.05)
        y1 = np.asarray(model.predict(feed, batch_size=64)).copy()
        assert not np.array_equal(y1, y0), k
        y0 = y1
    w = {k: np.asarray(v) for k, v in model.get_weights_by_name().items()}
    ref = (RF.fgcnn if which == "FGCNN" else RF.ccpm)(cols, cols, w, feed, **dict(kw, task="regression", dtype=np.float64)).reshape(-1)
    assert_close(np.asarray(model.predict_logits(feed, batch_size=64)).reshape(-1), ref, rtol=1e-4, atol=2e-5, what="live weights")


@pytest.mark.parametrize("which", ["CCPM", "FGCNN"])
def test_fit_takes_the_autograd_step_and_predict_follows(device, which):
    from deepctr_amd import engine, models, training, training_hip
    rng = np.random.RandomState(9)
    n = 1024
    cols, feed = problem(rng, n, F=6, E=4, vocab=10, seq=True)
    y = ((feed["C0"] % 2) ^ (feed["C1"] % 2)).astype(np.float32)
    kw = dict(conv_kernel_width=(4, 3), conv_filters=(4, 4), dnn_hidden_units=(32, 16))
    if which == "FGCNN":
        kw.update(new_maps=(2, 1), pooling_width=(2, 2))
    model = getattr(models, which)(cols, cols, device=device, **kw)
    assert not training_hip.supported(model)
    before = {k: t.clone() for k, t in model.named_weights() if k.startswith(("conv2d", "fgsparse"))}
    model.compile("adam", "binary_crossentropy")
    hist = model.fit(feed, y, batch_size=256, epochs=2, verbose=0)
    loss = hist.history["loss"]
    assert np.isfinite(loss).all() and loss[-1] < loss[0], loss
    after = dict(model.named_weights())
    unchanged = [k for k in before if torch.equal(before[k], after[k])]
    assert len(before) >= 4 and not unchanged, "weights the fit did not move: %s" % unchanged
    sub = {k: v[:256] for k, v in feed.items()}
    staged = engine.Staged(256)
    model._stage_inputs(sub, staged)
    model._begin()
    with torch.no_grad():
        ref = training.model_logits(model, staged, 0, 256).cpu().numpy()
    assert_close(np.asarray(model.predict_logits(sub, batch_size=256)).reshape(-1), ref, rtol=1e-4, atol=2e-5,
                 what="predict after fit vs model_logits")


def test_a_users_program_runs_through_the_facade(device):
    """The same columns through both constructors under the reference's import names: compile, fit, predict."""
    from deepctr.feature_column import SparseFeat, VarLenSparseFeat, get_feature_names
    from deepctr.models import CCPM, FGCNN
    n_rows = 8
    rng = np.random.RandomState(3)
    columns = [SparseFeat("viewer", n_rows, embedding_dim=4), SparseFeat("video", 10, embedding_dim=4), SparseFeat("genre", 5, embedding_dim=4),
               SparseFeat("hour", 24, embedding_dim=4), VarLenSparseFeat(SparseFeat("watched", 10, embedding_dim=4), maxlen=3)]
    data = {"viewer": np.arange(n_rows), "video": rng.randint(0, 10, n_rows), "genre": rng.randint(0, 5, n_rows),
            "hour": rng.randint(0, 24, n_rows), "watched": rng.randint(0, 10, (n_rows, 3))}
    x = {name: data[name] for name in get_feature_names(columns)}
    y = np.array([1, 0, 0, 1, 1, 0, 1, 0])
    for model in (CCPM(columns, columns, conv_kernel_width=(3, 2), conv_filters=(2, 2), dnn_hidden_units=[8, 4], dnn_dropout=0.3),
                  FGCNN(columns, columns, conv_kernel_width=(3, 3), conv_filters=(4, 5), new_maps=(2, 2), pooling_width=(2, 2),
                        dnn_hidden_units=[8, 4])):
        model.compile("adam", "binary_crossentropy", metrics=["binary_crossentropy"])
        history = model.fit(x, y, verbose=0, epochs=3)
        assert len(history.history["loss"]) == 3 and np.isfinite(history.history["loss"]).all()
        p = np.asarray(model.predict(x, batch_size=4))
        assert p.shape == (n_rows, 1) and np.isfinite(p).all() and (p > 0).all() and (p < 1).all()
