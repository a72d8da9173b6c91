"""GPU: EDCN's forward (ops.edcn: dctr_edcn_fwd, or the layered route) against the reference's own outputs, the two layers against
the layer fixture, the tower op against the float64 oracle over a sweep of shapes (every output combination, both routes, aligned and
unaligned slices, relu / linear, with and without the BatchNormalization affine), fit() on the autograd step, and a seeded fuzz."""
import numpy as np
import pytest
import torch

from tests import ref_edcn as RE
from tests.test_autoint_cpu import att_rows
from tests.test_edcn_cpu import FIXTURES, FUSED_BRIDGES, REG_TAGS, SWEEP, bridge_case, build_model, ref_tower, tower_case
from tests.test_gpu_models import check_probs
from tests.util import assert_close, assert_close_terms, golden_meta, load_golden

pytestmark = pytest.mark.gpu


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)


def deep_dev(v, device):
    if v is None:
        return None
    if isinstance(v, (list, tuple)):
        return type(v)(deep_dev(e, device) for e in v)
    return dev(v, device)


@pytest.mark.parametrize("name", FIXTURES)
def test_model_matches_reference_code(device, name):
    g = load_golden(name)
    meta = golden_meta(g)
    model = build_model(meta, device)
    model.set_weights_by_name({k[2:]: v for k, v in g.items() if k.startswith("w/")})
    feed = {k[5:]: v for k, v in g.items() if k.startswith("feed/")}
    rows = att_rows(meta, feed, g["y"].shape[0])
    assert rows.sum() >= 0.5 * rows.size
    assert model.route() == ("layered" if meta["kwargs"]["bridge_type"] == "attention_pooling" else "fused")
    for bs in (256, 5):
        check_probs(model.predict(feed, batch_size=bs), g["y"], "%s bs=%d" % (name, bs), rows)
    y = model.predict([feed[n] for n in model.input_names], batch_size=64)
    check_probs(y, g["y"], name + " list feed", rows)
    model.span_rows = 0
    model.span_batches = False
    y1 = model.predict(feed, batch_size=7)
    check_probs(y1, g["y"], name + " bs=7, no spans", rows)
    assert_close(y1[rows], y[rows], rtol=2e-6, atol=2e-7, what=name + ": spans vs per-batch calls")


@pytest.mark.parametrize("tag", REG_TAGS)
def test_regulation_layer_matches_the_layer_fixture(device, tag):
    from deepctr_amd.layers import RegulationModule
    g = load_golden("edcn_layer")
    x, w, tau, y = g[tag + "/x"], g[tag + "/g"], float(g[tag + "/tau"]), g[tag + "/y"]
    layer = RegulationModule(tau, device=device)
    layer.build((None,) + x.shape[1:])
    layer.set_weights([w])
    got = layer(torch.from_numpy(x).to(device))
    assert tuple(got.shape) == y.shape
    mag = np.abs(x.astype(np.float64)).reshape(x.shape[0], -1) * np.repeat(RE.gate(w, tau), x.shape[2])[None, :]
    assert_close_terms(got.cpu().numpy(), y, mag, what="RegulationModule " + tag)


@pytest.mark.parametrize("bridge_type", RE.BRIDGES)
def test_bridge_layer_matches_the_layer_fixture(device, bridge_type):
    from deepctr_amd.layers import BridgeModule
    x, h, w, y = bridge_case(load_golden("edcn_layer"), bridge_type)
    layer = BridgeModule(bridge_type, device=device)
    layer.build([(None, 12), (None, 12)])
    if bridge_type == "concatenation":
        layer.set_weights(list(w))
    elif bridge_type == "attention_pooling":
        layer.set_weights([half[k] for half in w for k in (0, 2, 1, 3)])          # keras order: kernel0, kernel1, bias0, bias1
    got = layer([torch.from_numpy(x).to(device), torch.from_numpy(h).to(device)])
    assert tuple(got.shape) == y.shape
    assert_close_terms(got.cpu().numpy(), y, RE.bridge(x, h, bridge_type, w, absolute=True), what="BridgeModule " + bridge_type)


def _run(ops, t, F, d, bridge_type, par, activation, **kw):
    return ops.edcn(t["xbuf"], F, d, t["gates"], t["cross_kernels"], t["cross_biases"], t["dnn_kernels"], t["dnn_biases"], bridge_type=bridge_type,
                    parameterization=par, tau=t["tau"], activation=activation, bn=t["bn"], dice=t["dice"], bridge_weights=t["bridge_weights"],
                    x_offset=t["off"], **kw)


def _check_case(device, F, d, L, B, bridge_type, par, off, activation, bn=False, dice=False, layered_only=False):
    from deepctr_amd import ops
    D = F * d
    case = tower_case(F, d, L, B, bridge_type, par, off, (0.5, 2.0)[(F + off) % 2], F * 100 + d + off, bn=bn, dice=dice)
    t = {k: (deep_dev(v, device) if k not in ("tau", "off") else v) for k, v in case.items()}
    what = "F=%d d=%d L=%d B=%d %s %s off=%d %s bn=%d" % (F, d, L, B, bridge_type, par, off, activation, bn)
    route = ops.edcn_route(F, d, L, bridge_type, par, activation)
    assert route == ("layered" if layered_only or D > 624 else "fused"), what
    ref_l, ref_o = ref_tower(case, F, d, bridge_type, par, activation)
    mag_l, mag_o = ref_tower(case, F, d, bridge_type, par, activation, absolute=True)
    ref_a, _ = ref_tower(case, F, d, bridge_type, par, activation, extras=False)
    mag_a, _ = ref_tower(case, F, d, bridge_type, par, activation, extras=False, absolute=True)
    bar = dict(rtol=1e-4, rtol_terms=RE.TOWER_RTOL_TERMS)
    # the logit with add / bias (no sigmoid: compared as a sum), and c / h / br into a strided buffer between NaN sentinels
    obuf = torch.full((B, 3 * D + 9), float("nan"), device=device)
    logit, out = _run(ops, t, F, d, bridge_type, par, activation, head_w=t["head"], add=[t["add"]], global_bias=t["bias"], logit=True, out=obuf,
                      out_offset=2)
    assert out is obuf and tuple(logit.shape) == (B,)
    assert torch.isnan(obuf[:, :2]).all() and torch.isnan(obuf[:, 2 + 3 * D:]).all()
    assert_close_terms(obuf[:, 2:2 + 3 * D].cpu().numpy(), ref_o, mag_o, what="c / h / br, " + what, **bar)
    assert_close_terms(logit.cpu().numpy(), ref_l, mag_l, what="logit + add + bias, " + what, **bar)
    # the sigmoid of the same logit
    prob, none = _run(ops, t, F, d, bridge_type, par, activation, head_w=t["head"], add=[t["add"]], global_bias=t["bias"], sigmoid_out=True)
    assert none is None
    assert_close(prob.cpu().numpy(), 1.0 / (1.0 + np.exp(-logit.cpu().numpy().astype(np.float64))), rtol=1e-6, atol=1e-7, what="sigmoid, " + what)
    # the logit alone; the outputs alone (a new tensor)
    l2, none = _run(ops, t, F, d, bridge_type, par, activation, head_w=t["head"])
    assert none is None
    assert_close_terms(l2.cpu().numpy(), ref_a, mag_a, what="logit alone, " + what, **bar)
    none, o2 = _run(ops, t, F, d, bridge_type, par, activation)
    assert none is None and tuple(o2.shape) == (B, 3 * D) and torch.equal(o2, obuf[:, 2:2 + 3 * D])
    # the same bits on a second call
    l3, o3 = _run(ops, t, F, d, bridge_type, par, activation, head_w=t["head"], add=[t["add"]], global_bias=t["bias"], logit=True, out=True)
    assert torch.equal(l3, logit) and torch.equal(o3, o2)
    if route == "fused":        # both routes take the shape: fused vs layered
        l4, o4 = _run(ops, t, F, d, bridge_type, par, activation, head_w=t["head"], add=[t["add"]], global_bias=t["bias"], logit=True, out=True,
                      route="layered")
        assert_close_terms(o4.cpu().numpy(), o2.cpu().numpy(), mag_o, what="fused vs layered c / h / br, " + what, **bar)
        assert_close_terms(l4.cpu().numpy(), logit.cpu().numpy(), mag_l, what="fused vs layered logit, " + what, **bar)


@pytest.mark.parametrize("off", [3, 4])
@pytest.mark.parametrize("par", ["vector", "matrix"])
@pytest.mark.parametrize("bridge_type", FUSED_BRIDGES)
@pytest.mark.parametrize("F,d,L,B", SWEEP)
def test_tower_op_vs_float64_oracle(device, F, d, L, B, bridge_type, par, off):
    for activation, bn in (("relu", False), ("linear", True)):
        _check_case(device, F, d, L, B, bridge_type, par, off, activation, bn=bn)


@pytest.mark.parametrize("off", [3, 4])
@pytest.mark.parametrize("kind", ["attention_pooling", "dice"])
@pytest.mark.parametrize("F,d,L,B", SWEEP)
def test_layered_route_alone_vs_float64_oracle(device, F, d, L, B, kind, off):
    if kind == "dice":
        _check_case(device, F, d, L, B, "hadamard_product", "vector", off, "dice", dice=True, layered_only=True)
    else:
        _check_case(device, F, d, L, B, "attention_pooling", "matrix", off, "relu", layered_only=True)


def test_more_rounds_than_one_launch_holds(device):
    """cross_num = 35: two chained launches through the workspace that carries br."""
    _check_case(device, 3, 4, 35, 21, "hadamard_product", "vector", 3, "relu")


@pytest.mark.parametrize("route", [None, "layered"])
def test_tower_reads_the_live_weights(device, route):
    from deepctr_amd import ops
    F, d, L = 5, 4, 2
    case = tower_case(F, d, L, 37, "concatenation", "matrix", 0, 0.5, 3)
    t = {k: (deep_dev(v, device) if k not in ("tau", "off") else v) for k, v in case.items()}
    _, o0 = _run(ops, t, F, d, "concatenation", "matrix", "relu", route=route)
    case["gates"][2][0, 1, 0] = case["gates"][2][0, 1, 0] * 0.5 + 1.0
    t["gates"][2][0, 1, 0].mul_(0.5).add_(1.0)
    case["gates"][1][0, 3, 0] -= 2.0
    t["gates"][1][0, 3, 0].sub_(2.0)
    _, o1 = _run(ops, t, F, d, "concatenation", "matrix", "relu", route=route)
    assert not torch.equal(o0, o1)
    _, ref = ref_tower(case, F, d, "concatenation", "matrix", head=False)
    _, mag = ref_tower(case, F, d, "concatenation", "matrix", head=False, absolute=True)
    assert_close_terms(o1.cpu().numpy(), ref, mag, rtol_terms=RE.TOWER_RTOL_TERMS, what="after an in-place write to g")


def _cols(F, E, seq=False, hash_=False, vocab=50):
    from deepctr_amd.feature_column import SparseFeat, VarLenSparseFeat
    cols = []
    for k in range(F):
        if seq and k % 3 == 2:
            cols.append(VarLenSparseFeat(SparseFeat("S%d" % k, 9 + k, E), maxlen=4, combiner=("mean", "sum")[k % 2]))
        else:
            cols.append(SparseFeat("C%d" % k, vocab + 3 * k, E, use_hash=bool(hash_ and k == 1)))
    return cols


def _feed(rng, cols, n):
    from deepctr_amd.feature_column import SparseFeat
    feed = {}
    for fc in cols:
        if isinstance(fc, SparseFeat):
            feed[fc.name] = rng.randint(0, 10 ** 6 if fc.use_hash else fc.vocabulary_size, n).astype(np.int32)
        else:
            ids = rng.randint(1, fc.vocabulary_size, (n, fc.maxlen)).astype(np.int32)
            lens = rng.randint(1, fc.maxlen + 1, n)
            ids[np.arange(fc.maxlen)[None, :] >= lens[:, None]] = 0
            feed[fc.name] = ids
    return feed


def _randomise(model, rng):
    from tests.test_gpu_models import _randomise as base
    w = base(model, rng)
    w = {k: (rng.uniform(0.5, 1.5, v.shape).astype(np.float32) if k.endswith("moving_variance") else
             (rng.standard_normal(v.shape).astype(np.float32) if k.endswith("_field_weight") else v)) for k, v in w.items()}
    model.set_weights_by_name(w)
    return w


def test_fit_takes_the_autograd_step_and_learns(device):
    from deepctr_amd import engine, training, training_hip
    from deepctr_amd.models import EDCN
    rng = np.random.RandomState(9)
    n = 8192
    cols = _cols(6, 8)
    feed = _feed(rng, cols, n)
    y = ((feed["C0"] % 2) ^ (feed["C1"] % 3 == 0)).astype(np.float32)          # planted signal
    model = EDCN(cols, cols, cross_num=2, bridge_type="concatenation", tau=0.5, device=device)
    assert not training_hip.supported(model)
    gates0 = [r.g.clone() for r in model.regulations]
    dense0 = model.bridges[0].dense.w("kernel").clone()
    model.compile("adam", "binary_crossentropy")
    hist = model.fit(feed, y, batch_size=256, epochs=2, verbose=0)
    assert getattr(model, "_hip_trainer", None) is None
    assert hist.history["loss"][1] < hist.history["loss"][0]
    assert all(not torch.equal(r.g, g0) for r, g0 in zip(model.regulations, gates0))       # the field weights trained
    assert not torch.equal(model.bridges[0].dense.w("kernel"), dense0)                     # and the bridge's Dense
    sub = {k: v[:1024] for k, v in feed.items()}
    staged = engine.Staged(1024)
    model._stage_inputs(sub, staged)
    model._begin()
    with torch.no_grad():
        ref = training.model_logits(model, staged, 0, 1024).cpu().numpy()
    assert_close(np.asarray(model.predict_logits(sub, batch_size=1024)).reshape(-1), ref, rtol=1e-4, atol=2e-5, what="predict after fit vs model_logits")


@pytest.mark.parametrize("seed", range(40))
def test_fuzz_predict_logits_vs_oracle(device, seed):
    from deepctr_amd.models import EDCN
    rng = np.random.RandomState(2000 + seed)
    F, E, L = int(rng.randint(1, 7)), int(rng.choice([1, 3, 4, 5, 8, 12, 16, 20])), int(rng.randint(1, 5))
    bridge_type, par = RE.BRIDGES[seed % 4], ("vector", "matrix")[(seed // 4) % 2]
    use_bn, task = bool(rng.rand() < 0.3), "regression" if rng.rand() < 0.25 else "binary"
    tau = float(rng.choice([0.5, 1.0, 2.0]))
    cols = _cols(F, E, seq=bool(rng.rand() < 0.5), hash_=bool(rng.rand() < 0.4), vocab=20)
    lin = cols if rng.rand() < 0.8 else []
    model = EDCN(lin, cols, cross_num=L, cross_parameterization=par, bridge_type=bridge_type, tau=tau, dnn_use_bn=use_bn, task=task,
                 device=device)
    w = _randomise(model, rng)
    n = int(rng.randint(3, 200))
    feed = _feed(rng, cols, n)
    what = "seed %d: F=%d E=%d L=%d %s %s bn=%d tau=%g %s" % (seed, F, E, L, bridge_type, par, use_bn, tau, task)
    got = np.asarray(model.predict_logits(feed, batch_size=64)).reshape(-1)
    kw = dict(cross_num=L, cross_parameterization=par, bridge_type=bridge_type, tau=tau, dnn_use_bn=use_bn, dtype=np.float64)
    ref = RE.edcn(lin, cols, w, feed, task="regression", **kw).reshape(-1)
    if use_bn:      # (no magnitude mode through BatchNormalization: the model-level bar of tests/test_gpu_models.py:check_probs)
        assert_close(got, ref, rtol=1e-4, atol=2e-5, what=what)
    else:
        mag = RE.edcn(lin, cols, w, feed, absolute=True, **kw).reshape(-1)
        assert_close_terms(got, ref, mag, rtol_terms=4e-6, what=what)
