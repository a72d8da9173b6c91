"""CPU: SharedBottom / ESMM / MMOE / PLE — the NumPy oracle (tests/ref_mtl.py) against the reference's own outputs
(tests/golden/model_{mmoe,ple,sb,esmm}_*.npz, mtl_layer.npz, model_mmoe_census.npz; scripts/make_golden_mtl.py), what the fixtures can
see, the float32-vs-float64 run that sets the bar of the GPU op tests, the torch restatement the training path uses, the composition of
the multi-task loss, the API contract, and the argument checks of the ops and of the C ABI (no launch)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import ref_mtl as RM
from tests.spec import columns_from_spec
from tests.test_autoint_cpu import att_rows
from tests.util import assert_close, assert_close_terms, golden_meta, load_golden

FIXTURES = ["model_mmoe_base", "model_mmoe_gate", "model_mmoe_bn", "model_mmoe_hash", "model_mmoe_nodense", "model_ple_22", "model_ple_11",
            "model_ple_01", "model_ple_3x3", "model_sb_base", "model_sb_nobottom", "model_sb_regbin", "model_esmm_base", "model_esmm_notower"]
CENSUS = "model_mmoe_census"
GATED = [n for n in FIXTURES + [CENSUS] if "mmoe" in n or "ple" in n]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (Din, expert units, layout, gate units, B, required route): the smallest shapes at which the level kernel can still go wrong.
# layout: ("mmoe", E, T), or ("ple", specific, shared, last) with two tasks and S = 3 slots
SWEEP = [
    (1, (1,), ("mmoe", 2, 2), (), 5, "fused"),                  # minimal
    (6, (3,), ("mmoe", 2, 2), (), 17, "fused"),                 # scalar loads; the slice sits at offset 3 of a wider row
    (36, (16, 8), ("mmoe", 3, 2), (), 65, "fused"),             # one full tile plus a row
    (85, (17,), ("mmoe", 4, 3), (6,), 40, "fused"),             # odd widths, a gate DNN
    (16, (16,), ("ple", 2, 2, False), (), 33, "fused"),         # G = T + 1, member subsets
    (16, (16,), ("ple", 1, 0, True), (), 33, "fused"),          # n_g = 1
    (127, (256, 128), ("mmoe", 3, 2), (), 130, "fused"),        # the example's shape, ragged last tile
    (429, (256, 128), ("mmoe", 8, 2), (), 20, None),            # Criteo, near the LDS limit
    (1024, (512, 256), ("mmoe", 4, 2), (), 19, None),
]
# (T, tower units, task types, esmm, B)
TOWER_SWEEP = [(2, (), ("binary", "regression"), False, 5), (3, (8,), ("binary", "regression", "binary"), False, 65),
               (2, (8,), ("binary", "binary"), True, 65), (2, (), ("binary", "binary"), True, 5), (3, (), ("regression",) * 3, False, 65),
               (2, (8,), ("regression", "binary"), False, 5)]


def build_model(meta, device, **more):
    from deepctr_amd import models
    kw = dict(meta["kwargs"])
    kw.update(more)
    return getattr(models, meta["model"])(columns_from_spec(meta["dnn"]), device=device, **kw)


def _has_hash(meta):
    return any(d.get("use_hash") or d.get("sparsefeat", {}).get("use_hash") for d in meta["dnn"])


def _feed(g):
    return {k[5:]: v for k, v in g.items() if k.startswith("feed/")}


def _weights(g):
    return {k[2:]: v for k, v in g.items() if k.startswith("w/")}


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _dnns(rng, n, in_dim, units, bn):
    ks, bs, bns = [], [], []
    for _ in range(n):
        dims = [in_dim] + list(units)
        ks.append([_f32(rng.standard_normal((dims[i], dims[i + 1])) / np.sqrt(dims[i])) for i in range(len(units))])
        bs.append([_f32(rng.standard_normal(u) * 0.1) for u in units])
        bns.append([(_f32(1.0 + 0.2 * rng.standard_normal(u)), _f32(0.1 * rng.standard_normal(u))) for u in units])
    return ks, bs, (bns if bn else None)


def level_case(Din, units, layout, gate_units, B, seed, bn=False):
    """Seeded operands of ops.mtl_level / RM.level_op as NumPy arrays (keyword arguments of both): gate kernels N(0, 1)."""
    rng = np.random.RandomState(seed)
    if layout[0] == "mmoe":
        _, E, T = layout
        S, off, esrc, gsrc, members = 1, (3 if Din == 6 else 0), [0] * E, [0] * T, [list(range(E)) for _ in range(T)]
    else:
        _, ns, nh, last = layout
        T, S, off = 2, 3, 4
        E = T * ns + nh
        esrc = [i for i in range(T) for _ in range(ns)] + [T] * nh
        gsrc = list(range(T)) + ([] if last else [T])
        members = [list(range(i * ns, (i + 1) * ns)) + list(range(T * ns, E)) for i in range(T)] + ([] if last else [list(range(E))])
    G = len(members)
    xbuf = _f32(rng.standard_normal((B, off + S * Din + 5)) * 0.5)
    ek, eb, ebn = _dnns(rng, E, Din, units, bn)
    case = dict(xbuf=xbuf, in_dim=Din, x_offsets=[off + s * Din for s in range(S)], expert_kernels=ek, expert_biases=eb, members=members,
                expert_src=esrc, gate_src=gsrc, expert_bn=ebn)
    dz = Din
    if gate_units:
        case["gate_dnn_kernels"], case["gate_dnn_biases"], case["gate_bn"] = _dnns(rng, G, Din, gate_units, bn)
        dz = gate_units[-1]
    case["gate_kernels"] = [_f32(rng.standard_normal((dz, len(ms)))) for ms in members]
    return case


def ref_level(case, activation="relu", **kw):
    args = dict(case)
    xbuf = args.pop("xbuf")
    return RM.level_op(xbuf, args.pop("in_dim"), args.pop("x_offsets"), args.pop("expert_kernels"), args.pop("expert_biases"),
                       args.pop("gate_kernels"), args.pop("members"), activation=activation, **dict(args, **kw))


def towers_case(T, units, in_dim, B, seed, bn=False):
    rng = np.random.RandomState(seed)
    ks, bs, bns = _dnns(rng, T, in_dim, units, bn)
    last = units[-1] if units else in_dim
    return dict(xbuf=_f32(rng.standard_normal((B, 2 + T * in_dim + 3)) * 0.5), in_dim=in_dim, x_offsets=[2 + t * in_dim for t in range(T)],
                kernels=ks, biases=bs, head_ws=[_f32(rng.standard_normal((last, 1)) / np.sqrt(last)) for _ in range(T)],
                global_biases=[_f32(rng.standard_normal(1) * 0.3) for _ in range(T)], bn=bns)


def ref_towers(case, binary, activation="relu", esmm=False, **kw):
    return RM.towers_op(case["xbuf"], case["in_dim"], case["x_offsets"], case["kernels"], case["biases"], case["head_ws"], case["global_biases"],
                        binary, activation, case["bn"], esmm=esmm, **kw)


def _miss(y, ref):
    """Per row: off the fixture by more than the probability bar of check_probs (1e-4 relative + 1e-6)."""
    y, ref = np.asarray(y, dtype=np.float64).reshape(-1), np.asarray(ref, dtype=np.float64).reshape(-1)
    return np.abs(y - ref) > 1e-4 * np.abs(ref) + 1e-6


@pytest.mark.parametrize("name", FIXTURES + [CENSUS])
def test_oracle_matches_reference_code(name):
    from tests.test_gpu_models import check_probs
    g = load_golden(name)
    meta = golden_meta(g)
    T, n = g["y"].shape[:2]
    assert g["y"].shape == (T, n, 1) and T == len(meta["kwargs"]["task_names"])
    rows = att_rows(meta, _feed(g), n)
    assert rows.sum() >= 0.5 * n                   # at least half of the rows carry no all-padding max-pooled sequence
    y, y64 = RM.run_fixture(g), RM.run_fixture(g, np.float64)
    for t, task in enumerate(meta["kwargs"]["task_types"]):
        check_probs(y[t].astype(np.float32), g["y"][t], "%s output %d" % (name, t), rows)
        if task == "binary":
            assert ((g["y"][t][rows] > 1e-3) & (g["y"][t][rows] < 1 - 1e-3)).all()         # none of the compared rows is saturated
        assert_close(y64[t][rows], g["y"][t][rows], rtol=1e-4, atol=1e-6, what="%s float64 output %d" % (name, t))


@pytest.mark.parametrize("name", FIXTURES + [CENSUS])
def test_fixture_sees_the_gates_and_the_heads(name):
    """Uniform gates, and zeroed heads, each miss the fixture on at least half of the kept rows of every output."""
    g = load_golden(name)
    meta = golden_meta(g)
    rows = att_rows(meta, _feed(g), g["y"].shape[1])
    y0 = RM.run_fixture(g, np.float64, zero_heads=True)
    for t in range(g["y"].shape[0]):
        assert _miss(y0[t][rows], g["y"][t][rows]).sum() >= 0.5 * rows.sum(), "output %d is blind to its head" % t
    if name not in GATED:
        return
    yu, gates = RM.run_fixture(g, np.float64, uniform_gates=True), RM.run_fixture(g, np.float64, return_gates=True)[1]
    if name == "model_ple_01":          # one member per task gate: nothing to see, the weights are exactly 1
        T = g["y"].shape[0]
        assert all(p.shape[1] == 1 and (p == 1.0).all() for level in gates for p in level[:T])
        return
    for t in range(g["y"].shape[0]):
        assert _miss(yu[t][rows], g["y"][t][rows]).sum() >= 0.5 * rows.sum(), "output %d is blind to the gates" % t


def test_fixtures_cover_what_they_are_for():
    kw = lambda name: golden_meta(load_golden(name))["kwargs"]      # noqa: E731
    k = kw("model_mmoe_base")
    assert (k["num_experts"], k["expert_dnn_hidden_units"], k["tower_dnn_hidden_units"], k["gate_dnn_hidden_units"], k["task_types"]) == \
        (3, [16, 8], [8], [], ["binary", "regression"])
    k = kw("model_mmoe_gate")
    assert (k["num_experts"], k["tower_dnn_hidden_units"], k["gate_dnn_hidden_units"], k["task_types"]) == (4, [], [6], ["binary"] * 3)
    assert kw("model_mmoe_bn")["dnn_use_bn"] is True and _has_hash(golden_meta(load_golden("model_mmoe_hash")))
    assert not any(d["type"] == "dense" for d in golden_meta(load_golden("model_mmoe_nodense"))["dnn"])
    pk = lambda n: tuple(kw(n)[k] for k in ("shared_expert_num", "specific_expert_num", "num_levels", "gate_dnn_hidden_units"))   # noqa: E731
    assert pk("model_ple_22") == (2, 2, 2, [5]) and pk("model_ple_11")[:3] == (1, 1, 1) and pk("model_ple_01")[:3] == (0, 1, 2)
    assert kw("model_ple_3x3")["num_levels"] == 3 and len(kw("model_ple_3x3")["task_names"]) == 3
    assert kw("model_sb_nobottom")["bottom_dnn_hidden_units"] == [] and kw("model_sb_regbin")["task_types"] == ["regression", "binary"]
    assert kw("model_esmm_base")["tower_dnn_hidden_units"] == [16, 8] and kw("model_esmm_notower")["tower_dnn_hidden_units"] == []
    c = kw(CENSUS)
    assert c["tower_dnn_hidden_units"] == [] and c["task_names"] == ["label_income", "label_marital"]
    for name in FIXTURES + [CENSUS, "mtl_layer"]:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) < 1024 * 1024


def layer_case(g, tag):
    """(operands of ops.mtl_level / RM.level_op, the reference's output [B, G * H]) of mtl_layer.npz: 'mmoe', 'ple0' or 'ple1'."""
    key = "mmoe" if tag == "mmoe" else "ple"
    w = {k[len(key) + 3:]: v for k, v in g.items() if k.startswith(key + "/w/")}
    names, x = ["ctr", "ctcvr"], g[key + "/x"]
    dn = lambda n: ([w[n + "/kernel%d" % i] for i in range(8) if n + "/kernel%d" % i in w],       # noqa: E731
                    [w[n + "/bias%d" % i] for i in range(8) if n + "/bias%d" % i in w])
    if tag == "mmoe":
        ex = [dn("expert_%d" % i) for i in range(3)]
        gd = [dn("gate_" + n) for n in names]
        case = dict(xbuf=x, in_dim=12, x_offsets=[0], expert_kernels=[e[0] for e in ex], expert_biases=[e[1] for e in ex],
                    gate_dnn_kernels=[d[0] for d in gd], gate_dnn_biases=[d[1] for d in gd],
                    gate_kernels=[w["gate_softmax_%s/kernel" % n] for n in names], members=[[0, 1, 2]] * 2)
        return case, g["mmoe/out"].reshape(x.shape[0], -1)
    lvl = int(tag[-1])
    p = "level_%d_" % lvl
    ex = [dn("%stask_%s_expert_specific_%d" % (p, n, j)) for n in names for j in range(2)] + [dn("%sexpert_shared_%d" % (p, k)) for k in range(2)]
    gk = [w["%sgate_softmax_specific_%s/kernel" % (p, n)] for n in names] + ([w[p + "gate_softmax_shared/kernel"]] if lvl == 0 else [])
    members = [[0, 1, 4, 5], [2, 3, 4, 5]] + ([[0, 1, 2, 3, 4, 5]] if lvl == 0 else [])
    if lvl == 0:
        case = dict(xbuf=x, in_dim=12, x_offsets=[0], expert_src=[0] * 6, gate_src=[0] * 3)
    else:
        case = dict(xbuf=_f32(g["ple/out0"].reshape(x.shape[0], -1)), in_dim=16, x_offsets=[0, 16, 32], expert_src=[0, 0, 1, 1, 2, 2],
                    gate_src=[0, 1])
    case.update(expert_kernels=[e[0] for e in ex], expert_biases=[e[1] for e in ex], gate_kernels=gk, members=members)
    return case, g["ple/out%d" % lvl].reshape(x.shape[0], -1)


@pytest.mark.parametrize("tag", ["mmoe", "ple0", "ple1"])
def test_level_oracle_matches_the_layer_fixture_and_uniform_gates_miss(tag):
    case, y = layer_case(load_golden("mtl_layer"), tag)
    mag = ref_level(case, absolute=True)
    for dt in (np.float32, np.float64):
        assert_close_terms(ref_level(case, dtype=dt), y, mag, what="level " + tag)
    uni = ref_level(case, uniform_gates=True)
    assert (np.abs(uni - y) > 1e-4 * np.abs(y) + 2e-6 * mag).mean() > 0.5


def test_float32_ops_against_float64_set_the_bar():
    """The float32 NumPy run of level_op and towers_op against the float64 run over the sweeps of the GPU tests: the worst error in units
    of the summed magnitude (2.22e-7 when the bar was set), times two (the MFMA tile sums k in another order) and rounded up, is RM.OP_RTOL_TERMS = 4.5e-7.
    Asserted here with room for another BLAS: the float32 run passes the bar, and the bar is within 4x of it."""
    worst = 0.0
    for i, (Din, units, layout, gate_units, B, _route) in enumerate(SWEEP):
        for act, bn in (("relu", False), ("linear", True)):
            case = level_case(Din, units, layout, gate_units, B, 100 + i, bn=bn)
            o64, o32, om = ref_level(case, act), ref_level(case, act, dtype=np.float32), ref_level(case, act, absolute=True)
            worst = max(worst, float((np.abs(o32 - o64) / om).max()))
    for i, (T, units, types, esmm, B) in enumerate(TOWER_SWEEP):
        for act, bn in (("relu", False), ("linear", True)):
            case = towers_case(T, units, 11, B, 200 + i, bn=bn and bool(units))
            none = [False] * T
            l64, l32 = ref_towers(case, none, act), ref_towers(case, none, act, dtype=np.float32)
            worst = max(worst, float((np.abs(l32 - l64) / ref_towers(case, none, act, absolute=True)).max()))
    print("float32 vs float64 level / towers: worst error / summed magnitude = %.3g" % worst)
    assert worst <= RM.OP_RTOL_TERMS <= 4 * worst, worst


def test_magnitude_mode_bounds_the_plain_run():
    case = level_case(36, (16, 8), ("mmoe", 3, 2), (6,), 9, 5, bn=True)
    assert (ref_level(case, absolute=True) >= np.abs(ref_level(case))).all()
    tc = towers_case(2, (8,), 11, 9, 6)
    assert (ref_towers(tc, [False] * 2, absolute=True) >= np.abs(ref_towers(tc, [False] * 2))).all()
    p = ref_towers(tc, [True, True], esmm=True)
    q = ref_towers(tc, [True, True])
    assert np.allclose(p[0], q[0]) and np.allclose(p[1], q[0] * q[1])


def _staged(model, feed, n):
    from deepctr_amd import engine
    staged = engine.Staged(n)
    model._stage_inputs(feed, staged)
    model._begin()
    return staged


@pytest.mark.parametrize("name", FIXTURES + [CENSUS])
def test_torch_restatement_matches_oracle(name):
    g = load_golden(name)
    meta = golden_meta(g)
    if _has_hash(meta):
        pytest.skip("hashed ids are staged on the device")
    model = build_model(meta, torch.device("cpu"))
    model.set_weights_by_name(_weights(g))
    feed, n = _feed(g), g["y"].shape[1]
    staged = _staged(model, feed, n)
    with torch.no_grad():
        logits = model.autograd_logits(staged, 0, n)
        outs, has_logit = model.autograd_outputs(logits)
    rows = att_rows(meta, feed, n)
    ref_l, ref_p = RM.run_fixture(g, np.float64, logits=True), RM.run_fixture(g, np.float64)
    assert has_logit == ([True, False] if meta["model"] == "ESMM" else [True] * len(outs))
    for t in range(len(outs)):
        assert_close(logits[t].numpy()[rows], ref_l[t].reshape(-1)[rows], rtol=1e-4, atol=2e-5, what="%s logit %d" % (name, t))
        assert_close(outs[t].numpy()[rows], ref_p[t].reshape(-1)[rows], rtol=1e-4, atol=2e-5, what="%s output %d" % (name, t))


@pytest.mark.parametrize("name", FIXTURES + [CENSUS])
def test_weight_names_and_shapes_match_the_fixture(name):
    g = load_golden(name)
    model = build_model(golden_meta(g), torch.device("cpu"))
    mine = {k: tuple(v.shape) for k, v in model.get_weights_by_name().items()}
    assert mine == {k: tuple(v.shape) for k, v in _weights(g).items()}


SIGNATURES = {
    "SharedBottom": dict(bottom_dnn_hidden_units=(256, 128), tower_dnn_hidden_units=(64,), l2_reg_embedding=0.00001, l2_reg_dnn=0, seed=1024,
                         dnn_dropout=0, dnn_activation='relu', dnn_use_bn=False, task_types=('binary', 'binary'), task_names=('ctr', 'ctcvr')),
    "ESMM": dict(tower_dnn_hidden_units=(256, 128, 64), l2_reg_embedding=0.00001, l2_reg_dnn=0, seed=1024, dnn_dropout=0, dnn_activation='relu',
                 dnn_use_bn=False, task_types=('binary', 'binary'), task_names=('ctr', 'ctcvr')),
    "MMOE": dict(num_experts=3, expert_dnn_hidden_units=(256, 128), tower_dnn_hidden_units=(64,), gate_dnn_hidden_units=(),
                 l2_reg_embedding=0.00001, l2_reg_dnn=0, seed=1024, dnn_dropout=0, dnn_activation='relu', dnn_use_bn=False,
                 task_types=('binary', 'binary'), task_names=('ctr', 'ctcvr')),
    "PLE": dict(shared_expert_num=1, specific_expert_num=1, num_levels=2, expert_dnn_hidden_units=(256,), tower_dnn_hidden_units=(64,),
                gate_dnn_hidden_units=(), l2_reg_embedding=0.00001, l2_reg_dnn=0, seed=1024, dnn_dropout=0, dnn_activation='relu',
                dnn_use_bn=False, task_types=('binary', 'binary'), task_names=('ctr', 'ctcvr')),
}


@pytest.mark.parametrize("ctor", sorted(SIGNATURES))
def test_reference_import_names_and_signatures(ctor):
    import deepctr
    import deepctr.models.multitask
    import deepctr_amd.models
    import deepctr_amd.models.multitask as mt
    mod = __import__("deepctr.models.multitask." + ctor.lower(), fromlist=[ctor])
    fn = getattr(deepctr.models, ctor)
    assert fn is getattr(mod, ctor) is getattr(mt, ctor) is getattr(deepctr_amd.models, ctor) is getattr(deepctr.models.multitask, ctor)
    params = inspect.signature(fn).parameters
    want = dict(SIGNATURES[ctor], device=None)
    assert list(params) == ["dnn_feature_columns"] + list(want)
    for k, v in want.items():
        assert params[k].default == v, k


def test_construction_errors():
    from deepctr_amd.feature_column import SparseFeat
    from deepctr_amd.models import ESMM, MMOE, PLE, SharedBottom
    cols = [SparseFeat("a", 5, 4), SparseFeat("b", 5, 4)]
    for ctor in (SharedBottom, MMOE, PLE):
        with pytest.raises(ValueError, match="num_tasks must be greater than 1"):
            ctor(cols, task_types=("binary",), task_names=("ctr",), device="cpu")
        with pytest.raises(ValueError, match="num_tasks must be equal to the length of task_types"):
            ctor(cols, task_types=("binary",), task_names=("ctr", "cvr"), device="cpu")
        with pytest.raises(ValueError, match="task must be binary or regression, multiclass is illegal"):
            ctor(cols, task_types=("binary", "multiclass"), device="cpu")
    with pytest.raises(ValueError, match="num_experts must be greater than 1"):
        MMOE(cols, num_experts=1, device="cpu")
    with pytest.raises(ValueError, match="the length of task_names must be equal to 2"):
        ESMM(cols, task_names=("a", "b", "c"), device="cpu")
    with pytest.raises(ValueError, match="task must be binary in ESMM, regression is illegal"):
        ESMM(cols, task_types=("binary", "regression"), device="cpu")


def _loss_setup(l2_dnn=0.02, weights=(1.0, 0.5)):
    g = load_golden("model_mmoe_base")
    meta = golden_meta(g)
    model = build_model(meta, torch.device("cpu"), l2_reg_dnn=l2_dnn)
    model.set_weights_by_name(_weights(g))
    model.compile("sgd", loss_weights=list(weights), metrics=["mse"])
    n = g["y"].shape[1]
    rng = np.random.RandomState(3)
    ys = np.stack([(rng.rand(n) < 0.4).astype(np.float32), rng.standard_normal(n).astype(np.float32)])
    return g, model, _staged(model, _feed(g), n), ys, n


def test_loss_is_the_weighted_sum_of_task_losses_plus_penalties():
    """One step on 32 rows reports sum_t w_t loss_t + the l2 penalties, as float64 NumPy computes them from the oracle's outputs."""
    from deepctr_amd.models.multitask import _fit
    g, model, staged, ys, n = _loss_setup()
    hist = _fit.fit_torch(model, staged, torch.from_numpy(ys), n, n, 1, False, _fit.EpochEnd(model, None, n, 1, 0)).history
    p = RM.run_fixture(g, np.float64).reshape(2, n)
    pc = np.clip(p[0], 1e-7, 1 - 1e-7)
    bce = float(-(ys[0] * np.log(pc) + (1 - ys[0]) * np.log(1 - pc)).mean())
    mse = float(((p[1] - ys[1]) ** 2).mean())
    w = {k: v.astype(np.float64) for k, v in _weights(g).items()}
    pen = sum(0.02 * (v ** 2).sum() for k, v in w.items() if re.search(r"/kernel\d+$", k)) + \
        sum(1e-5 * (v ** 2).sum() for k, v in w.items() if k.endswith("/embeddings"))
    assert pen > 0.01
    want = bce + 0.5 * mse + pen
    assert abs(hist["loss"][0] - want) <= 1e-5 * abs(want), (hist["loss"][0], want, bce, mse, pen)
    assert abs(hist["ctr_loss"][0] - bce) <= 1e-5 * bce and abs(hist["ctcvr_loss"][0] - mse) <= 1e-5 * mse
    assert sorted(hist) == sorted(["loss", "ctr_loss", "ctcvr_loss", "ctr_mse", "ctcvr_mse"])          # tf.keras' keys


def test_every_parameter_group_gets_a_gradient():
    g = load_golden("model_mmoe_bn")
    model = build_model(golden_meta(g), torch.device("cpu"), dnn_use_bn=False)
    model.set_weights_by_name({k: v for k, v in _weights(g).items() if not k.startswith("batch_normalization")})
    n = g["y"].shape[1]
    staged = _staged(model, _feed(g), n)
    leaves = [(k, t.requires_grad_(True)) for k, t in model.named_weights()]
    sum(l.sum() for l in model.autograd_logits(staged, 0, n, training=True)).backward()
    groups = ("expert_", "gate_ctr/", "gate_softmax_", "tower_", "dense", "bias0", "global_bias", "sparse_emb_", "sparse_seq_emb_")
    for k, t in leaves:
        assert t.grad is not None and 0 < float(t.grad.abs().max()) < float("inf"), k
    assert all(any(grp in k for k, _ in leaves) for grp in groups)


def test_compile_and_fit_options():
    from deepctr_amd.models.multitask import _fit
    g, model, staged, ys, n = _loss_setup()
    model.compile("adam", loss={"ctr": "binary_crossentropy"}, loss_weights={"ctcvr": 2.0})
    assert model._compiled["loss"] == ["binary_crossentropy", "mse"] and model._compiled["loss_weights"] == [1.0, 2.0]
    model.compile("adam", loss="mse")
    assert model._compiled["loss"] == ["mse", "mse"]
    with pytest.raises(ValueError, match="unknown task names"):
        model.compile("adam", loss={"nope": "mse"})
    with pytest.raises(ValueError, match="3 entries for 2 tasks"):
        model.compile("adam", loss_weights=[1, 2, 3])
    with pytest.raises(NotImplementedError):
        model.compile("adam", loss="hinge")
    assert model._labels({"ctcvr": ys[1], "ctr": ys[0]}).tolist() == ys.tolist()
    with pytest.raises(ValueError, match="one label array per task"):
        model._labels([ys[0]])
    feed = _feed(g)
    for opt, val in (("sample_weight", np.ones(n)), ("class_weight", {0: 1.0, 1: 2.0}), ("callbacks", [object()]), ("_dp", object())):
        with pytest.raises(NotImplementedError, match=r"fit\(%s=\.\.\.\) is not implemented for multi-task models" % opt):
            model.fit(feed, list(ys), verbose=0, **{opt: val})             # raised before anything touches a device
    with pytest.raises(TypeError, match="unexpected keyword argument 'nope'"):
        model.fit(feed, list(ys), nope=1)
    assert _fit.fit_multitask is not None
    with pytest.raises(NotImplementedError, match="multi-output"):
        model.sharded_predict(None)


def test_regularised_weights_are_every_dnn_kernel():
    from deepctr_amd import training
    g = load_golden("model_ple_22")
    model = build_model(golden_meta(g), "cpu", l2_reg_embedding=0.2, l2_reg_dnn=0.3)
    names = {t.data_ptr(): n for n, t in model.named_weights()}
    got = sorted((names[t.data_ptr()], l2) for t, l2 in training.regularized_weights(model))
    want = sorted([(n, 0.2) for n, _ in model.named_weights() if n.endswith("/embeddings")] +
                  [(n, 0.3) for n, _ in model.named_weights() if re.search(r"/kernel\d+$", n)])
    assert got == want and not any("gate_softmax" in n or n.startswith("dense") for n, _ in got)


def test_census_preprocessing_through_the_facade_reproduces_the_feed():
    pd = pytest.importorskip("pandas")
    pytest.importorskip("sklearn")
    from sklearn.preprocessing import LabelEncoder, MinMaxScaler
    from deepctr.feature_column import DenseFeat, SparseFeat, get_feature_names
    from deepctr.models import MMOE
    from scripts.make_golden_mtl import CENSUS_COLUMNS, CENSUS_SPARSE
    g = load_golden(CENSUS)
    data = pd.read_csv(os.path.join(ROOT, "tests", "golden", "census-income.sample"), header=None, names=CENSUS_COLUMNS)
    data['label_income'] = data['income_50k'].map({' - 50000.': 0, ' 50000+.': 1})
    data['label_marital'] = data['marital_stat'].apply(lambda x: 1 if x == ' Never married' else 0)
    data.drop(labels=['income_50k', 'marital_stat'], axis=1, inplace=True)
    dense = [c for c in data.columns.values.tolist() if c not in CENSUS_SPARSE and c not in ['label_income', 'label_marital']]
    data[CENSUS_SPARSE] = data[CENSUS_SPARSE].fillna('-1', )
    data[dense] = data[dense].fillna(0, )
    data[dense] = MinMaxScaler(feature_range=(0, 1)).fit_transform(data[dense])
    for feat in CENSUS_SPARSE:
        data[feat] = LabelEncoder().fit_transform(data[feat])
    cols = [SparseFeat(feat, data[feat].max() + 1, embedding_dim=4) for feat in CENSUS_SPARSE] + [DenseFeat(feat, 1, ) for feat in dense]
    names = get_feature_names(cols + cols)
    assert sorted(names) == sorted(_feed(g))
    for n in names:
        assert np.array_equal(data[n].values.astype(g["feed/" + n].dtype), g["feed/" + n]), n
    assert np.array_equal(data['label_income'].values, g["label/label_income"])
    model = MMOE(cols, tower_dnn_hidden_units=[], task_types=['binary', 'binary'], task_names=['label_income', 'label_marital'], device="cpu")
    assert {k: tuple(v.shape) for k, v in model.get_weights_by_name().items()} == {k: tuple(v.shape) for k, v in _weights(g).items()}
    model.compile("adam", loss=["binary_crossentropy", "binary_crossentropy"], metrics=['binary_crossentropy'], )


def test_op_argument_errors_raise_before_any_launch():
    from deepctr_amd import ops
    t = lambda a: torch.from_numpy(a) if isinstance(a, np.ndarray) else a      # noqa: E731
    deep = lambda v: [deep(e) for e in v] if isinstance(v, (list, tuple)) and v and not isinstance(v[0], int) else t(v)   # noqa: E731
    case = {k: deep(v) for k, v in level_case(6, (3,), ("mmoe", 2, 2), (), 7, 1).items()}
    x = case.pop("xbuf")
    call = lambda **kw: ops.mtl_level(x, case["in_dim"], case["x_offsets"], case["expert_kernels"], case["expert_biases"],   # noqa: E731
                                      case["gate_kernels"], **dict(dict(members=case["members"]), **kw))
    with pytest.raises(ValueError, match=r"members \[0, 2\] with 2 experts"):
        call(members=[[0, 2], [0, 1]])
    with pytest.raises(ValueError, match="mixes no expert"):
        call(members=[[], [0, 1]])
    with pytest.raises(ValueError, match="source slots"):
        call(expert_src=[0, 1])
    with pytest.raises(ValueError, match="gate_kernels"):
        call(members=[[0], [0, 1]])
    with pytest.raises(ValueError, match="route"):
        call(route="fused")
    with pytest.raises(ValueError, match="unit column stride"):
        ops.mtl_level(x[:, :8], 6, [3], case["expert_kernels"], case["expert_biases"], case["gate_kernels"], case["members"])
    with pytest.raises(ValueError, match="expert 1 kernel0"):
        ops.mtl_level(x, 6, [3], [case["expert_kernels"][0], [case["expert_kernels"][1][0][:5]]], case["expert_biases"], case["gate_kernels"],
                      case["members"])
    with pytest.raises(_C_error()):
        call()                                      # CPU tensors: refused by the device check, after every operand check
    tc = {k: deep(v) for k, v in towers_case(2, (8,), 11, 5, 2).items()}
    tw = lambda **kw: ops.mtl_towers(tc["xbuf"], 11, tc["x_offsets"], tc["kernels"], tc["biases"], tc["head_ws"], tc["global_biases"], **kw)   # noqa: E731
    with pytest.raises(ValueError, match="esmm takes two binary towers"):
        tw(binary=[True, False], esmm=True)
    with pytest.raises(ValueError, match="one task type"):
        tw(binary=[True])
    with pytest.raises(ValueError, match="out must be a float32"):
        tw(out=torch.empty(5, 2))
    with pytest.raises(ValueError, match="members"):
        ops.mtl_mix(torch.zeros(5, 6), 2, 3, [torch.zeros(5, 4)], [torch.zeros(4, 2)], [[0, 2]])
    with pytest.raises(ValueError, match="h must be"):
        ops.mtl_mix(torch.zeros(5, 5), 2, 3, [torch.zeros(5, 4)], [torch.zeros(4, 2)], [[0, 1]])


def _C_error():
    from deepctr_amd import _C
    return _C.DctrExtensionError


def _abi_args(kind=0, **kw):
    from deepctr_amd import _C, ops
    # (batch = 0: whatever the checks let through returns before a launch — this file also runs where a GPU is present)
    base = dict(batch=0, x_stride=12, x_offsets=[0, 6], in_dim=6, units=[3], expert_src=[0, 1], activation="relu", route=None,
                gate_units=[], gate_src=[0, 1], members=[[0, 1], [1]])
    if kind == 1:
        base.update(gate_src=[], members=[])
    fields = {k: kw.pop(k) for k in list(kw) if k not in base and k not in ("esmm", "tile_rows")}
    base.update(kw)
    a, keep = ops._mtl_args("test", kind, **base)
    for k, v in fields.items():
        setattr(a, k, v)
    return a, keep


def test_abi_argument_errors_without_a_gpu():
    from deepctr_amd import _C
    lib = _C.lib()
    ptrs = (ctypes.c_void_p * 4)(16, 16, 16, 16)
    arr = ctypes.cast(ptrs, ctypes.c_void_p)
    i32 = (ctypes.c_int32 * 2)(1, 0)
    full = dict(x=16, expert_w=arr, expert_b=arr, gate_kernel=arr, out=16, out_stride=6)
    lvl = lambda **kw: lib.dctr_mtl_level_fwd(ctypes.byref(_abi_args(0, **dict(full, **kw))[0]), None)      # noqa: E731
    assert lib.dctr_mtl_level_fwd(None, None) == -1 and lib.dctr_mtl_towers_fwd(None, None) == -1 and lib.dctr_mtl_route(None, 0) == -1
    assert lib.dctr_mtl_mix(None, None) == -1 and lib.dctr_mtl_route(ctypes.byref(_abi_args()[0]), 2) == -4
    assert lvl() == 0                                                                   # an empty batch is a no-op
    assert lvl(members=[[0, 2], [1]]) == -2 and b"member" in lib.dctr_last_error()       # members out of range
    assert lvl(members=[[0, 1], []]) == -2                                              # n_g < 1
    assert lvl(expert_src=[0, 2]) == -2 and lvl(gate_src=[2, 0]) == -2                  # src >= S
    assert lvl(x_offsets=[0, 7]) == -2 and lvl(units=[0]) == -2 and lvl(batch=-1) == -2 and lvl(in_dim=0) == -2
    assert lvl(out_stride=5) == -2 and lvl(out_stride=7, out_offset=2) == -2
    assert lvl(route="layered") == -5 and lvl(activation="dice") == -5                 # the layered route's: declined, not launched
    a, keep = _abi_args(0, **full)
    a.activation = 7
    assert lib.dctr_mtl_level_fwd(ctypes.byref(a), None) == -4
    a, keep = _abi_args(0, **full)
    a.tile_rows = 24
    assert lib.dctr_mtl_level_fwd(ctypes.byref(a), None) == -4
    for k in ("x", "expert_w", "expert_b", "gate_kernel", "out"):
        assert lvl(**{k: None}) == -1, k
    assert lvl(expert_bn_scale=arr) == -1                                               # scale without shift
    assert lvl(gate_units=[4]) == -1                                                    # a gate DNN without its weights
    for a_kw in (dict(), dict(units=[])):
        tw = lambda **kw: lib.dctr_mtl_towers_fwd(ctypes.byref(_abi_args(1, **dict(dict(x=16, expert_w=arr, expert_b=arr, head_w=arr,   # noqa: E731
                                                  binary=ctypes.cast(i32, ctypes.c_void_p), probs=16, probs_stride=4), **dict(a_kw, **kw)))[0]), None)
        assert tw() == 0 and tw(probs_stride=3, batch=4) == -2 and tw(head_w=None) == -1 and tw(probs=None) == -1 and tw(binary=None) == -1
        assert tw(esmm=True, expert_src=[0, 1, 0], x_offsets=[0, 6]) == -4              # the ESMM head takes two towers
    assert lib.dctr_mtl_route(ctypes.byref(_abi_args(0)[0]), 0) == _C.mtl.ROUTE_FUSED
    assert lib.dctr_mtl_route(ctypes.byref(_abi_args(0, activation="dice")[0]), 0) == _C.mtl.ROUTE_LAYERED
    assert lib.dctr_mtl_route(ctypes.byref(_abi_args(0, in_dim=4096, x_stride=8192, x_offsets=[0, 4096], units=[2048])[0]), 0) == _C.mtl.ROUTE_LAYERED
    assert lib.dctr_mtl_route(ctypes.byref(_abi_args(1, units=[])[0]), 1) == _C.mtl.ROUTE_FUSED
    # dctr_mtl_mix
    m = _C.mtl.MixArgs
    i64 = (ctypes.c_int64 * 2)(4, 4)
    gn, mem = (ctypes.c_int32 * 2)(2, 1), (ctypes.c_int32 * 3)(0, 1, 1)
    cast = lambda p: ctypes.cast(p, ctypes.c_void_p)      # noqa: E731
    good = dict(batch=0, h=16, h_stride=6, n_experts=2, width=3, n_gates=2, z_dim=4, z=arr, z_stride=cast(i64), gate_kernel=arr, gate_n=cast(gn),
                members=cast(mem), members_dev=16, out=16, out_stride=6, out_offset=0)
    mix = lambda **kw: lib.dctr_mtl_mix(ctypes.byref(m(**dict(good, **kw))), None)      # noqa: E731
    assert mix() == 0 and mix(h=None) == -1 and mix(members_dev=None) == -1 and mix(h_stride=5) == -2 and mix(out_stride=5) == -2
    assert mix(n_experts=1, h_stride=3) == -2 and mix(z_dim=5) == -2 and mix(width=0) == -2
    assert mix(gate_n=cast((ctypes.c_int32 * 2)(2, 0))) == -2


def test_header_declares_the_entry_points_and_the_mirror_matches_the_c_layout(tmp_path):
    import shutil
    import subprocess
    from deepctr_amd import _C
    header = open(os.path.join(ROOT, "include", "dctr.h")).read()
    assert "#define DCTR_ABI_VERSION 13" in header and _C.ABI_VERSION == 13              # no existing struct changed
    for sym in ("dctr_mtl_route", "dctr_mtl_level_fwd", "dctr_mtl_towers_fwd"):
        assert re.search(r"\bint %s\(const dctr_mtl_args_t\* args" % sym, header), sym
    assert re.search(r"\bint dctr_mtl_mix\(const dctr_mtl_mix_args_t\* args", header)
    assert _C.SYMBOLS["dctr_mtl_level_fwd"] == (ctypes.c_int, [ctypes.POINTER(_C.mtl.Args), ctypes.c_void_p])
    assert "mtl_kernels.hip" in __import__("deepctr_amd.build", fromlist=["SOURCES"]).SOURCES
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    for cls, cname in ((_C.mtl.Args, "dctr_mtl_args_t"), (_C.mtl.MixArgs, "dctr_mtl_mix_args_t")):
        lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dctr.h"', "int main(void) {",
                 '    printf("enums %d %d %d %d %d\\n", DCTR_MTL_LEVEL, DCTR_MTL_TOWERS, DCTR_MTL_ROUTE_AUTO, DCTR_MTL_ROUTE_FUSED, '
                 'DCTR_MTL_ROUTE_LAYERED);', '    printf("sizeof %%zu\\n", sizeof(%s));' % cname]
        for fname, _ in cls._fields_:
            lines.append('    printf("%s %%zu\\n", offsetof(%s, %s));' % (fname, cname, fname))
        lines += ["    return 0;", "}"]
        src = tmp_path / (cname + ".c")
        src.write_text("\n".join(lines) + "\n")
        exe = tmp_path / cname
        subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
        out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
        seen = 0
        for line in filter(None, out):
            field, *vals = line.split()
            if field == "enums":
                e = _C.mtl
                assert [int(v) for v in vals] == [e.LEVEL, e.TOWERS, e.ROUTE_AUTO, e.ROUTE_FUSED, e.ROUTE_LAYERED]
                continue
            want = ctypes.sizeof(cls) if field == "sizeof" else getattr(cls, field).offset
            assert int(vals[0]) == want, "%s: C says %s, ctypes %d" % (field, vals[0], want)
            seen += 1
        assert seen == 1 + len(cls._fields_)
