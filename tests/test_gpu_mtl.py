"""GPU: the multi-task models' forward (ops.mtl_level / ops.mtl_towers: dctr_mtl_level_fwd, dctr_mtl_towers_fwd, or the layered route
with dctr_mtl_mix) against the reference's own outputs, one level against the layer fixture, the two ops against the float64 oracle over
a sweep of shapes (both routes, relu / linear, with and without the BatchNormalization affine), fit() on the autograd step, and a seeded
fuzz over the four constructors."""
import numpy as np
import pytest
import torch

from tests import ref_mtl as RM
from tests.test_autoint_cpu import att_rows
from tests.test_gpu_models import check_probs
from tests.test_mtl_cpu import (CENSUS, FIXTURES, SWEEP, TOWER_SWEEP, _feed, _weights, build_model, layer_case, level_case, ref_level,
                                ref_towers, towers_case)
from tests.util import assert_close, assert_close_terms, golden_meta, load_golden

pytestmark = pytest.mark.gpu
BAR = dict(rtol=1e-4, rtol_terms=RM.OP_RTOL_TERMS)


def deep_dev(v, device):
    if v is None or isinstance(v, (int, float)):
        return v
    if isinstance(v, (list, tuple)):
        return type(v)(deep_dev(e, device) for e in v)
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(device)


def run_level(case, device, activation="relu", **kw):
    from deepctr_amd import ops
    t = {k: (deep_dev(v, device) if k not in ("in_dim", "x_offsets", "members", "expert_src", "gate_src") else v) for k, v in case.items()}
    x = t.pop("xbuf")
    return ops.mtl_level(x, t.pop("in_dim"), t.pop("x_offsets"), t.pop("expert_kernels"), t.pop("expert_biases"), t.pop("gate_kernels"),
                         t.pop("members"), activation=activation, **dict(t, **kw))


def level_route(case, activation="relu"):
    from deepctr_amd import ops
    gd = case.get("gate_dnn_kernels")
    return ops.mtl_route(case["in_dim"], [k.shape[1] for k in case["expert_kernels"][0]], len(case["expert_kernels"]), case["members"],
                         [k.shape[1] for k in gd[0]] if gd else (), n_slots=len(case["x_offsets"]), expert_src=case["expert_src"],
                         gate_src=case["gate_src"], activation=activation)


@pytest.mark.parametrize("name", FIXTURES + [CENSUS])
def test_model_matches_reference_code(device, name):
    g = load_golden(name)
    meta = golden_meta(g)
    model = build_model(meta, device)
    model.set_weights_by_name(_weights(g))
    feed, ref = _feed(g), g["y"]
    T, n = ref.shape[:2]
    rows = att_rows(meta, feed, n)
    assert rows.sum() >= 0.5 * n
    assert model.route() == "fused"

    def check(ys, what):
        assert isinstance(ys, list) and len(ys) == T
        for t in range(T):
            check_probs(ys[t], ref[t], "%s output %d %s" % (name, t, what), rows)
    for bs in (256, 5):
        check(model.predict(feed, batch_size=bs), "bs=%d" % bs)
    y = model.predict([feed[k] for k in model.input_names], batch_size=64)
    check(y, "list feed")
    model.span_rows = 0
    model.span_batches = False
    y1 = model.predict(feed, batch_size=7)
    check(y1, "bs=7, no spans")
    for t in range(T):
        assert_close(y1[t][rows], y[t][rows], rtol=2e-6, atol=2e-7, what="%s output %d: spans vs per-batch calls" % (name, t))
    model._route = "layered"
    assert model.route() == "layered"
    check(model.predict(feed, batch_size=64), "layered route")
    model._route = None
    logits = model.predict_logits(feed, batch_size=64)
    ref_l = RM.run_fixture(g, np.float64, logits=True)
    for t in range(T):
        assert_close(logits[t][rows], ref_l[t][rows], rtol=1e-4, atol=2e-5, what="%s logit %d" % (name, t))
    pt = model.predict_tensor(feed)
    assert tuple(pt.shape) == (T, n) and pt.is_cuda


@pytest.mark.parametrize("tag", ["mmoe", "ple0", "ple1"])
def test_level_matches_the_layer_fixture(device, tag):
    case, y = layer_case(load_golden("mtl_layer"), tag)
    mag = ref_level(case, absolute=True)
    for route in (None, "layered"):
        got = run_level(case, device, route=route)
        assert tuple(got.shape) == y.shape
        assert_close_terms(got.cpu().numpy(), y, mag, what="level %s route %s" % (tag, route))


@pytest.mark.parametrize("i", range(len(SWEEP)))
def test_level_op_vs_float64_oracle(device, i):
    Din, units, layout, gate_units, B, required = SWEEP[i]
    for act, bn in (("relu", False), ("linear", True)):
        case = level_case(Din, units, layout, gate_units, B, 100 + i, bn=bn)
        what = "Din=%d units=%s %s gate=%s B=%d %s bn=%d" % (Din, units, layout, gate_units, B, act, bn)
        route = level_route(case, act)
        assert route in ("fused", "layered") and (required is None or route == required), what
        ref, mag = ref_level(case, act), ref_level(case, act, absolute=True)
        G, H = len(case["members"]), units[-1]
        obuf = torch.full((B, G * H + 5), float("nan"), device=device)          # a strided buffer between NaN sentinels
        out = run_level(case, device, act, out=obuf, out_offset=2)
        assert out is obuf and torch.isnan(obuf[:, :2]).all() and torch.isnan(obuf[:, 2 + G * H:]).all()
        assert_close_terms(obuf[:, 2:2 + G * H].cpu().numpy(), ref, mag, what=what + " route " + route, **BAR)
        again = run_level(case, device, act)
        assert tuple(again.shape) == (B, G * H) and torch.equal(again, obuf[:, 2:2 + G * H])          # the same bits on a second call
        lay = run_level(case, device, act, route="layered")
        assert_close_terms(lay.cpu().numpy(), ref, mag, what=what + " layered", **BAR)
        assert torch.equal(run_level(case, device, act, route="layered"), lay)
        if route == "fused" and B > 16:
            small = run_level(case, device, act, tile_rows=16)                                       # another tile height, the same sums
            assert torch.equal(small, again)


def test_other_activations_and_dice(device):
    from deepctr_amd import ops
    case = level_case(36, (16, 8), ("mmoe", 3, 2), (6,), 21, 7)
    for act in ("sigmoid", "tanh"):
        assert level_route(case, act) == "fused"
        ref, mag = ref_level(case, act), ref_level(case, act, absolute=True)
        for route in (None, "layered"):
            # (the hardware sigmoid of the epilogue is ~2 ulp: the model-level bar on top of the measured one)
            assert_close_terms(run_level(case, device, act, route=route).cpu().numpy(), ref, mag, rtol=1e-4, rtol_terms=2e-6,
                               what="%s route %s" % (act, route))
    assert level_route(case, "dice") == "layered"
    assert ops.mtl_route(11, (8,), 2, towers=True, n_slots=2, expert_src=[0, 1], activation="dice") == "layered"
    rng = np.random.RandomState(8)
    dice = lambda n, units: [[(0.3 * rng.standard_normal(u).astype(np.float32), 0.1 * rng.standard_normal(u).astype(np.float32),       # noqa: E731
                               rng.uniform(0.5, 1.5, u).astype(np.float32)) for u in units] for _ in range(n)]
    case["expert_dice"], case["gate_dice"] = dice(3, (16, 8)), dice(2, (6,))
    ref = ref_level(case, "dice")
    assert_close(run_level(case, device, "dice").cpu().numpy(), ref, rtol=1e-4, atol=2e-6, what="dice, layered")


@pytest.mark.parametrize("i", range(len(TOWER_SWEEP)))
def test_towers_op_vs_oracle_and_vs_mlp_calls(device, i):
    from deepctr_amd import ops
    T, units, types, esmm, B = TOWER_SWEEP[i]
    binary = [t == "binary" for t in types]
    for act, bn in (("relu", False), ("linear", True)):
        case = towers_case(T, units, 11, B, 200 + i, bn=bn and bool(units))
        t = {k: (deep_dev(v, device) if k not in ("in_dim", "x_offsets") else v) for k, v in case.items()}
        what = "T=%d units=%s %s esmm=%d B=%d %s bn=%d" % (T, units, types, esmm, B, act, bn)
        run = lambda **kw: ops.mtl_towers(t["xbuf"], 11, t["x_offsets"], t["kernels"], t["biases"], t["head_ws"], t["global_biases"],   # noqa: E731
                                          activation=act, bn=t["bn"], **kw)
        assert ops.mtl_route(11, units, T, towers=True, n_slots=T, expert_src=list(range(T)), activation=act, esmm=esmm) == "fused"
        none = [False] * T
        ref, mag = ref_towers(case, none, act), ref_towers(case, none, act, absolute=True)
        logit = run(binary=none)
        assert tuple(logit.shape) == (T, B)
        assert_close_terms(logit.cpu().numpy(), ref, mag, what="logits, " + what, **BAR)
        lay = run(binary=none, route="layered")
        assert_close_terms(lay.cpu().numpy(), ref, mag, what="logits by ops.mlp, " + what, **BAR)
        want = ref_towers(case, binary, act, esmm=esmm)
        for route in (None, "layered"):
            got = run(binary=binary, esmm=esmm, route=route)
            assert_close(got.cpu().numpy(), want, rtol=1e-4, atol=1e-6, what="outputs route %s, %s" % (route, what))
            assert torch.equal(run(binary=binary, esmm=esmm, route=route), got)


def test_fit_on_the_census_rows(device):
    g = load_golden(CENSUS)
    meta = golden_meta(g)
    feed = _feed(g)
    ys = [g["label/label_income"], g["label/label_marital"]]
    hists = []
    for dev in (device, torch.device("cpu")):
        model = build_model(meta, dev)
        model.set_weights_by_name(_weights(g))
        model.compile("sgd", loss=["binary_crossentropy", "binary_crossentropy"], metrics=["binary_crossentropy"])
        if dev.type == "cpu":
            from deepctr_amd import engine
            from deepctr_amd.models.multitask import _fit
            staged = engine.Staged(200)
            model._stage_inputs(feed, staged)
            hists.append(_fit.fit_torch(model, staged, torch.from_numpy(np.stack(ys)), 200, 64, 1, False,
                                        _fit.EpochEnd(model, None, 64, 1, 0)).history)
        else:
            hists.append(model.fit(feed, ys, batch_size=64, epochs=2, verbose=0, shuffle=False, validation_split=0.2).history)
            staged = None
    h = hists[0]
    names = ["loss"] + ["%s_%s" % (n, k) for n in ("label_income", "label_marital") for k in ("loss", "binary_crossentropy")]
    assert sorted(h) == sorted(names + ["val_" + n for n in names])
    assert h["loss"][1] < h["loss"][0]
    # (the CPU run trains on all 200 rows, the GPU run on the first 160: compare a run without the split)
    model = build_model(meta, device)
    model.set_weights_by_name(_weights(g))
    model.compile("sgd", loss=["binary_crossentropy", "binary_crossentropy"], metrics=["binary_crossentropy"])
    first = model.fit(feed, {"label_marital": ys[1], "label_income": ys[0]}, batch_size=64, epochs=1, verbose=0, shuffle=False).history
    assert abs(first["loss"][0] - hists[1]["loss"][0]) <= 1e-4 * abs(hists[1]["loss"][0])
    total = model.train_on_batch(feed, ys)
    ev = model.evaluate(feed, ys, batch_size=64)
    assert len(ev) == 5 and np.isfinite(total) and ev[0] < first["loss"][0]
    with pytest.raises(NotImplementedError, match="sample_weight"):
        model.fit(feed, ys, sample_weight=np.ones(200), verbose=0)
    with pytest.raises(NotImplementedError, match="callbacks"):
        model.fit(feed, ys, callbacks=[object()], verbose=0)


def _cols(rng, F, E, dense):
    from deepctr_amd.feature_column import DenseFeat, SparseFeat, VarLenSparseFeat
    cols = []
    for k in range(F):
        if k % 3 == 2:
            cols.append(VarLenSparseFeat(SparseFeat("S%d" % k, 9 + k, E), maxlen=4, combiner=("mean", "sum")[k % 2]))
        else:
            cols.append(SparseFeat("C%d" % k, 20 + 3 * k, E, use_hash=bool(k == 1 and rng.rand() < 0.3)))
    return cols + [DenseFeat("D%d" % k, 1 + k) for k in range(dense)]


def _fuzz_feed(rng, cols, n):
    from deepctr_amd.feature_column import DenseFeat, SparseFeat
    feed = {}
    for fc in cols:
        if isinstance(fc, SparseFeat):
            feed[fc.name] = rng.randint(0, 10 ** 6 if fc.use_hash else fc.vocabulary_size, n).astype(np.int32)
        elif isinstance(fc, DenseFeat):
            feed[fc.name] = rng.rand(n, fc.dimension).astype(np.float32) if fc.dimension > 1 else rng.rand(n).astype(np.float32)
        else:
            ids = rng.randint(1, fc.vocabulary_size, (n, fc.maxlen)).astype(np.int32)
            lens = rng.randint(1, fc.maxlen + 1, n)
            ids[np.arange(fc.maxlen)[None, :] >= lens[:, None]] = 0
            feed[fc.name] = ids
    return feed


@pytest.mark.parametrize("seed", range(40))
def test_fuzz_predict_vs_oracle(device, seed):
    from deepctr_amd import models
    from tests.test_gpu_models import _randomise
    rng = np.random.RandomState(3000 + seed)
    kind = ("MMOE", "PLE", "SharedBottom", "ESMM")[seed % 4]
    T = 2 if kind == "ESMM" else int(rng.randint(2, 4))
    units = lambda lo=0: [int(u) for u in rng.choice([1, 3, 8, 16, 17, 32], int(rng.randint(lo, 3)))]      # noqa: E731
    kw = dict(task_names=["t%d" % t for t in range(T)], tower_dnn_hidden_units=units(), dnn_use_bn=bool(rng.rand() < 0.3),
              task_types=["binary"] * T if kind == "ESMM" else [str(rng.choice(["binary", "regression"])) for _ in range(T)])
    if kind == "MMOE":
        kw.update(num_experts=int(rng.randint(2, 6)), expert_dnn_hidden_units=units(1), gate_dnn_hidden_units=units())
    elif kind == "PLE":
        kw.update(shared_expert_num=int(rng.randint(0, 3)), specific_expert_num=int(rng.randint(1, 3)), num_levels=int(rng.randint(1, 4)),
                  expert_dnn_hidden_units=units(1), gate_dnn_hidden_units=units())
    elif kind == "SharedBottom":
        kw.update(bottom_dnn_hidden_units=units())
    cols = _cols(rng, int(rng.randint(1, 6)), int(rng.choice([1, 4, 5, 8, 16])), int(rng.randint(0, 3)))
    model = getattr(models, kind)(cols, device=device, **kw)
    w = _randomise(model, rng)
    w = {k: (rng.uniform(0.5, 1.5, v.shape).astype(np.float32) if k.endswith("moving_variance") else
             (rng.standard_normal(v.shape).astype(np.float32) if "gate_softmax" in k else v)) for k, v in w.items()}
    model.set_weights_by_name(w)
    n = int(rng.randint(3, 200))
    feed = _fuzz_feed(rng, cols, n)
    what = "seed %d: %s %s" % (seed, kind, kw)
    got = model.predict(feed, batch_size=64)
    ref = RM.model(kind, cols, w, feed, kw, dtype=np.float64)
    for t in range(T):
        r = ref[t].reshape(-1)
        keep = np.ones(n, dtype=bool) if kw["task_types"][t] != "binary" else (r > 1e-3) & (r < 1 - 1e-3)
        assert keep.sum() >= 0.5 * n, what                   # (a seed that saturates is replaced, not skipped)
        check_probs(got[t], ref[t].astype(np.float32), "%s output %d" % (what, t), keep)
