"""CPU: the optimizer objects of deepctr_amd.optimizers — constructors, configs, optimizers.get, the schedules, the torch restatement
(training.KerasOptimizer) against the float64 oracle (tests/ref_optimizers.py), fit()'s routing, and the C layout of the two structs
of dctr_opt_apply."""
import inspect
import os
import shutil
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_optimizers as RO  # noqa: E402

from deepctr_amd import optimizers  # noqa: E402
from deepctr_amd.optimizers import SGD, Adadelta, Adagrad, Adam, Adamax, Ftrl, RMSprop  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIGNATURES = {
    SGD: [("learning_rate", 0.01), ("momentum", 0.0), ("nesterov", False), ("name", "SGD")],
    Adagrad: [("learning_rate", 0.001), ("initial_accumulator_value", 0.1), ("epsilon", 1e-7), ("name", "Adagrad")],
    RMSprop: [("learning_rate", 0.001), ("rho", 0.9), ("momentum", 0.0), ("epsilon", 1e-7), ("centered", False), ("name", "RMSprop")],
    Adam: [("learning_rate", 0.001), ("beta_1", 0.9), ("beta_2", 0.999), ("epsilon", 1e-7), ("amsgrad", False), ("name", "Adam")],
    Adamax: [("learning_rate", 0.001), ("beta_1", 0.9), ("beta_2", 0.999), ("epsilon", 1e-7), ("name", "Adamax")],
    Adadelta: [("learning_rate", 0.001), ("rho", 0.95), ("epsilon", 1e-7), ("name", "Adadelta")],
    Ftrl: [("learning_rate", 0.001), ("learning_rate_power", -0.5), ("initial_accumulator_value", 0.1), ("l1_regularization_strength", 0.0),
           ("l2_regularization_strength", 0.0), ("name", "Ftrl"), ("l2_shrinkage_regularization_strength", 0.0), ("beta", 0.0)],
}


@pytest.mark.parametrize("cls", list(SIGNATURES), ids=lambda c: c.__name__)
def test_constructor_arguments_are_keras_in_name_order_and_default(cls):
    ps = [p for p in inspect.signature(cls.__init__).parameters.values() if p.name != "self" and p.kind != p.VAR_KEYWORD]
    assert [(p.name, p.default) for p in ps] == SIGNATURES[cls]
    o = cls()
    for name, default in SIGNATURES[cls]:
        assert getattr(o, name) == default
    assert o.iterations == 0 and o.decay == 0.0 and o.clipnorm is None and o.clipvalue is None and o.global_clipnorm is None
    assert cls(0.25).learning_rate == 0.25 and cls(lr=0.5).learning_rate == 0.5 and cls(lr=0.5).lr == 0.5
    assert not callable(o), "a callable optimizer is a torch.optim factory to fit()"
    with pytest.raises(TypeError):
        cls(no_such_argument=1)


@pytest.mark.parametrize("cls", list(SIGNATURES), ids=lambda c: c.__name__)
def test_config_round_trip(cls):
    o = cls(0.02, clipvalue=0.5, decay=0.01)
    cfg = o.get_config()
    assert cfg["name"] == cls.__name__ and cfg["learning_rate"] == 0.02 and cfg["clipvalue"] == 0.5 and cfg["decay"] == 0.01
    assert set(k for k, _ in SIGNATURES[cls]) <= set(cfg)
    assert cls.from_config(cfg).get_config() == cfg
    sched = cls(optimizers.schedules.ExponentialDecay(0.1, 10, 0.5, staircase=True), global_clipnorm=2.0)
    again = cls.from_config(sched.get_config())
    assert again.get_config() == sched.get_config() and again.current_lr(25) == 0.1 * 0.25 and again.global_clipnorm == 2.0


def test_get_takes_names_objects_configs_and_foreign_objects():
    for name, cls in (("adam", Adam), ("Adam", Adam), ("SGD", SGD), ("rmsprop", RMSprop), ("adagrad", Adagrad), ("adamax", Adamax),
                      ("Adadelta", Adadelta), ("FTRL", Ftrl)):
        assert type(optimizers.get(name)) is cls
    o = Ftrl(0.05, beta=0.1)
    assert optimizers.get(o) is o
    d = optimizers.get({"class_name": "Adagrad", "config": {"learning_rate": 0.1024, "initial_accumulator_value": 0.2}})
    assert type(d) is Adagrad and d.learning_rate == 0.1024 and d.initial_accumulator_value == 0.2

    class KerasLike(object):                    # what a tf.keras optimizer instance shows: get_config() with `name` and Keras' keys
        def get_config(self):
            return {"name": "RMSprop", "learning_rate": 0.003, "decay": 0.0, "rho": 0.8, "momentum": 0.5, "epsilon": 1e-6, "centered": True,
                    "jit_compile": False}       # (a key of a later Keras: ignored)
    f = optimizers.get(KerasLike())
    assert type(f) is RMSprop and (f.learning_rate, f.rho, f.momentum, f.epsilon, f.centered) == (0.003, 0.8, 0.5, 1e-6, True)

    class Adam2(object):                        # a renamed instance: the class name decides
        def get_config(self):
            return {"name": "my_optimizer", "learning_rate": 0.5}
    Adam2.__name__ = "Adam"
    assert type(optimizers.get(Adam2())) is Adam
    # keys of a newer Keras: ignored while they leave the rule alone, refused when they would change it
    for extra, ok in ((dict(weight_decay=None, use_ema=False, ema_momentum=0.99), True), (dict(weight_decay=0.01), False),
                      (dict(use_ema=True), False), (dict(some_new_switch=1), False)):
        cfg = {"class_name": "Adam", "config": dict({"name": "Adam", "learning_rate": 0.5}, **extra)}
        if ok:
            assert optimizers.get(cfg).learning_rate == 0.5
        else:
            with pytest.raises(ValueError):
                optimizers.get(cfg)
    from deepctr_amd.optimizers.schedules import ExponentialDecay           # tf.keras' spelling
    assert ExponentialDecay is optimizers.schedules.ExponentialDecay
    for junk in ("nadam", "junk", 3, None, object(), {"config": {}}, {"class_name": "Nadam", "config": {}}, Adam):
        with pytest.raises(ValueError):
            optimizers.get(junk)


def test_keras_refusals():
    with pytest.raises(ValueError):
        Adam(clipnorm=1.0, global_clipnorm=1.0)
    for kw in (dict(learning_rate_power=0.5), dict(initial_accumulator_value=-0.1), dict(l1_regularization_strength=-1.0),
               dict(l2_regularization_strength=-1.0), dict(l2_shrinkage_regularization_strength=-1.0)):
        with pytest.raises(ValueError):
            Ftrl(**kw)
    with pytest.raises(ValueError):
        SGD(momentum=1.5)
    with pytest.raises(ValueError):
        Adagrad(initial_accumulator_value=-1.0)
    with pytest.raises(ValueError):
        Adam(clipvalue=-1.0)


def test_schedules_against_hand_computed_values():
    S = optimizers.schedules
    e = S.ExponentialDecay(0.1, 10, 0.5)
    assert e(0) == 0.1 and abs(e(5) - 0.1 * 0.5 ** 0.5) < 1e-15 and abs(e(10) - 0.05) < 1e-15 and abs(e(25) - 0.1 * 0.5 ** 2.5) < 1e-15
    es = S.ExponentialDecay(0.1, 10, 0.5, staircase=True)
    assert [es(s) for s in (0, 9, 10, 19, 20)] == [0.1, 0.1, 0.05, 0.05, 0.025]
    i = S.InverseTimeDecay(0.1, 10, 0.5)
    assert i(0) == 0.1 and abs(i(5) - 0.1 / 1.25) < 1e-15 and abs(i(20) - 0.05) < 1e-15
    ist = S.InverseTimeDecay(0.1, 10, 0.5, staircase=True)
    assert [ist(s) for s in (0, 9, 10, 25)] == [0.1, 0.1, 0.1 / 1.5, 0.05]
    p = S.PiecewiseConstantDecay([3, 6], [1.0, 0.5, 0.1])
    assert [p(s) for s in (0, 3, 4, 6, 7, 100)] == [1.0, 1.0, 0.5, 0.5, 0.1, 0.1]
    with pytest.raises(ValueError):
        S.PiecewiseConstantDecay([3, 6], [1.0, 0.5])
    for sch, ref in ((e, lambda s: RO.exponential_decay(0.1, 10, 0.5, s)), (es, lambda s: RO.exponential_decay(0.1, 10, 0.5, s, True)),
                     (i, lambda s: RO.inverse_time_decay(0.1, 10, 0.5, s)), (ist, lambda s: RO.inverse_time_decay(0.1, 10, 0.5, s, True)),
                     (p, lambda s: RO.piecewise_constant([3, 6], [1.0, 0.5, 0.1], s))):
        for s in range(0, 40, 3):
            assert abs(sch(s) - ref(s)) < 1e-15
    # the rate of an update is taken at `iterations` before the increment; decay=d is lr / (1 + d iterations)
    o = SGD(S.PiecewiseConstantDecay([0], [1.0, 0.5]))
    assert o.current_lr() == 1.0 and o._step_lr(1) == 1.0 and o._step_lr(2) == 0.5
    assert abs(Adam(0.1, decay=0.5).current_lr(4) - 0.1 / 3.0) < 1e-15
    assert SGD(lambda step: 0.1 / (1 + step)).current_lr(3) == 0.025


# ---- the torch restatement against the float64 oracle ------------------------------------------------------------------------------
STEPS, SIZES = 6, (1, 5, 1031)


def run_torch(name, kw, ws, gs, l2s, dtype=torch.float32):
    """training.KerasOptimizer over copies of ws; the gradient it is handed holds the l2 term, as the autograd step's does."""
    from deepctr_amd import training
    opt = getattr(optimizers, name)(**kw)
    params = [torch.tensor(w, dtype=dtype) for w in ws]
    ko = training.KerasOptimizer(params, opt)
    for g in gs:
        for p, gg, l2 in zip(params, g, l2s):
            p.grad = torch.tensor(gg, dtype=dtype) + (2.0 * l2) * p.detach()
        ko.step()
    return [p.detach().numpy() for p in params], opt


def run_oracle(rule, okw, ws, gs, l2s, lr_of):
    o = RO.Oracle(rule, **okw)
    w64 = [np.asarray(w, dtype=np.float64).copy() for w in ws]
    for t, g in enumerate(gs):
        o.update(w64, g, l2s, lr_of(t))
    return w64, o


def draw(case, rng, shapes, l2s, steps):
    cid, name, kw, rule, okw = case
    if rule == "ftrl":
        return RO.ftrl_draw(rng, shapes, l2s, steps, kw["learning_rate"], okw)
    return ([rng.uniform(-0.5, 0.5, s).astype(np.float32) for s in shapes],
            [[rng.normal(0, 0.1, s).astype(np.float32) for s in shapes] for _ in range(steps)])


@pytest.mark.parametrize("l2", [0.0, 0.01])
@pytest.mark.parametrize("case", RO.CASES, ids=RO.CASE_IDS)
def test_torch_restatement_matches_the_float64_oracle(case, l2):
    cid, name, kw, rule, okw = case
    rng = np.random.RandomState(zlib.crc32(cid.encode()) % 1000)
    shapes, l2s = [(n,) for n in SIZES], [l2] * len(SIZES)
    ws, gs = draw(case, rng, shapes, l2s, STEPS)
    want, _ = run_oracle(rule, okw, ws, gs, l2s, lambda t: kw["learning_rate"])
    # float64 torch: the same rule, to rounding.  float32 torch: each update rounds a dozen operations to 6e-8 relative on quantities
    # of at most ~1 (the weights are below 0.5, an update below 0.1), so six updates stay below 6 x 12 x 6e-8 = 4e-6; the bar is 5 x that
    got64, opt = run_torch(name, kw, ws, gs, l2s, torch.float64)
    assert opt.iterations == STEPS
    for a, b in zip(got64, want):
        assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max()), (cid, np.abs(a - b).max())
    got32, _ = run_torch(name, kw, ws, gs, l2s, torch.float32)
    for a, b in zip(got32, want):
        assert np.abs(a - b).max() <= 2e-5 * max(1.0, np.abs(b).max()), (cid, np.abs(a - b).max())
    if rule == "ftrl" and okw.get("l1_regularization_strength", 0) >= 0.05:
        zeros = sum(int((b == 0).sum()) for b in want)
        assert 0 < zeros < sum(b.size for b in want), "the l1 case should land some weights exactly on 0"
        for a, b in zip(got32, want):
            assert np.array_equal(a == 0, b == 0)


def test_schedule_and_decay_reach_the_update():
    rng = np.random.RandomState(3)
    ws = [rng.uniform(-0.5, 0.5, (37,)).astype(np.float32)]
    gs = [[rng.normal(0, 0.1, (37,)).astype(np.float32)] for _ in range(STEPS)]
    sch = optimizers.schedules.ExponentialDecay(0.01, 2, 0.5)
    want, _ = run_oracle("adam", dict(amsgrad=True), ws, gs, [0.0], lambda t: RO.exponential_decay(0.01, 2, 0.5, t))
    got, _ = run_torch("Adam", dict(learning_rate=sch, amsgrad=True), ws, gs, [0.0], torch.float64)
    assert np.abs(got[0] - want[0]).max() < 1e-12
    want, _ = run_oracle("sgd", {}, ws, gs, [0.0], lambda t: 0.1 / (1 + 0.5 * t))
    got, _ = run_torch("SGD", dict(learning_rate=0.1, decay=0.5), ws, gs, [0.0], torch.float64)
    assert np.abs(got[0] - want[0]).max() < 1e-12


def _torch_run(make, ws, gs):
    params = [torch.tensor(w, dtype=torch.float64) for w in ws]
    o = make(params)
    for g in gs:
        for p, gg in zip(params, g):
            p.grad = torch.tensor(gg, dtype=torch.float64)
        o.step()
    return [p.detach().numpy() for p in params]


def test_cross_checks_with_torch_optim_where_the_rule_is_the_same():
    from deepctr_amd import training
    rng = np.random.RandomState(5)
    ws = [rng.uniform(-0.5, 0.5, (n,)) for n in SIZES]
    gs = [[rng.normal(0, 0.1, (n,)) for n in SIZES] for _ in range(STEPS)]
    mine = lambda o: _torch_run(lambda p: training.KerasOptimizer(p, o), ws, gs)      # noqa: E731
    # torch's momentum buffer is -a / lr of Keras' accumulator: the same weights under a constant rate
    for nesterov in (False, True):
        a = mine(SGD(0.05, momentum=0.9, nesterov=nesterov))
        b = _torch_run(lambda p: torch.optim.SGD(p, lr=0.05, momentum=0.9, nesterov=nesterov), ws, gs)
        assert max(np.abs(x - y).max() for x, y in zip(a, b)) < 1e-12
    a = mine(Adadelta(0.5, rho=0.9, epsilon=1e-6))
    b = _torch_run(lambda p: torch.optim.Adadelta(p, lr=0.5, rho=0.9, eps=1e-6), ws, gs)
    assert max(np.abs(x - y).max() for x, y in zip(a, b)) < 1e-12
    # the four names fit() takes today: their objects' defaults give what training._OPTS' optimizers give
    for name in ("adam", "adagrad", "rmsprop", "sgd"):
        a = mine(optimizers.get(name))
        b = _torch_run(training._OPTS[name], ws, gs)
        assert max(np.abs(x - y).max() for x, y in zip(a, b)) < 1e-12, name


# ---- fit()'s routing ---------------------------------------------------------------------------------------------------------------
def _deepfm():
    from deepctr_amd.feature_column import DenseFeat, SparseFeat
    from deepctr_amd.models import DeepFM
    cols = [SparseFeat("a", 20, 4), SparseFeat("b", 9, 4), DenseFeat("d", 2)]
    return DeepFM(cols, cols, dnn_hidden_units=(8, 4), device="cpu"), cols


def test_an_optimizer_object_takes_the_hip_step_and_a_factory_does_not():
    from deepctr_amd import models, training, training_hip
    from deepctr_amd.feature_column import SparseFeat
    from deepctr_amd.models.multitask import _fit
    m, _ = _deepfm()
    obj = Adam(0.01)
    m.compile(obj, "binary_crossentropy")
    assert m._compiled["optimizer"] is obj, "compile() keeps storing what it is given"
    assert training_hip.supported(m) and training_hip.takes_optimizer(m) and training.compiled_optimizer(m) is obj
    m.compile(lambda params: torch.optim.SGD(params, lr=0.1), "binary_crossentropy")
    assert not training_hip.takes_optimizer(m)
    m.compile("nadam", "binary_crossentropy")
    assert not training_hip.takes_optimizer(m)
    for name in ("adam", "Adagrad", "rmsprop", "SGD"):
        m.compile(name, "binary_crossentropy")
        assert training_hip.takes_optimizer(m) and training.compiled_optimizer(m) == name.lower()
    m.compile("ftrl", "binary_crossentropy")
    first = training.compiled_optimizer(m)
    assert type(first) is Ftrl and training.compiled_optimizer(m) is first and training_hip.takes_optimizer(m)

    class KerasLike(object):
        def get_config(self):
            return {"name": "Adagrad", "learning_rate": 0.1024}
    foreign = KerasLike()
    m.compile(foreign, "binary_crossentropy")
    assert m._compiled["optimizer"] is foreign
    conv = training.compiled_optimizer(m)
    assert type(conv) is Adagrad and conv.learning_rate == 0.1024 and training.compiled_optimizer(m) is conv     # converted once
    m.compile(KerasLike(), "binary_crossentropy")
    assert training.compiled_optimizer(m) is not conv
    for bad in (object(), Adam):                    # junk, and the class where an instance is meant
        m.compile(bad, "binary_crossentropy")
        with pytest.raises(ValueError):
            training.compiled_optimizer(m)

    cols = [SparseFeat("a", 20, 4), SparseFeat("b", 9, 4)]
    mm = models.MMOE(cols, task_types=("binary", "binary"), device="cpu")
    mm.compile(Adam(0.01))
    assert _fit.takes_hip_step(mm)
    mm.compile(lambda params: torch.optim.SGD(params, lr=0.1))
    assert not _fit.takes_hip_step(mm)
    mm.compile(RMSprop(0.01, momentum=0.5, centered=True))
    assert _fit.takes_hip_step(mm)
    mm.hip_training = False
    assert not _fit.takes_hip_step(mm)


def test_ftrl_trains_an_autoint_on_the_autograd_step():
    from deepctr_amd import engine, training
    from deepctr_amd.feature_column import SparseFeat
    from deepctr_amd.models import AutoInt
    rng = np.random.RandomState(4)
    n = 512
    cols = [SparseFeat("a", 20, 4), SparseFeat("b", 9, 4), SparseFeat("c", 5, 4)]
    model = AutoInt(cols, cols, att_layer_num=1, att_embedding_size=4, att_head_num=2, dnn_hidden_units=(8,), device="cpu")
    feed = {"a": rng.randint(0, 20, n), "b": rng.randint(0, 9, n), "c": rng.randint(0, 5, n)}
    y = (feed["a"] % 2).astype(np.float32)
    opt = Ftrl(0.05, l1_regularization_strength=1e-3)
    model.compile(opt, "binary_crossentropy")
    staged = engine.Staged(n)
    model._stage_inputs(feed, staged)
    h = training._fit_torch(model, staged, torch.from_numpy(y), n, 64, 6, True, training._EpochEnd(model, feed, y, n, 0, 64, 6, 0, None, None))
    assert h.history["loss"][-1] < h.history["loss"][0] - 0.01, h.history["loss"]
    assert opt.iterations == 6 * (n // 64)
    # a second fit() continues the same torch optimizer (state and update count), as the HIP step continues its trainer;
    # compile() with another object starts afresh
    ko = model._keras_optimizer[0]
    n_state = len(ko.state)
    assert n_state > 0
    training._fit_torch(model, staged, torch.from_numpy(y), n, 64, 1, True, training._EpochEnd(model, feed, y, n, 0, 64, 1, 0, None, None))
    assert model._keras_optimizer[0] is ko and len(ko.state) == n_state and opt.iterations == 7 * (n // 64)
    other = Ftrl(0.05)
    model.compile(other, "binary_crossentropy")
    training._fit_torch(model, staged, torch.from_numpy(y), n, 64, 1, True, training._EpochEnd(model, feed, y, n, 0, 64, 1, 0, None, None))
    assert model._keras_optimizer[0] is not ko and other.iterations == n // 64 and opt.iterations == 7 * (n // 64)


def test_one_object_in_two_optimizers_counts_once_per_update():
    from deepctr_amd import training
    opt = Adam(0.01)
    a, b = torch.zeros(3), torch.zeros(3)
    ka, kb = training.KerasOptimizer([a], opt), training.KerasOptimizer([b], opt)
    for k, p in ((ka, a), (kb, b), (ka, a)):
        p.grad = torch.ones(3)
        k.step()
    assert opt.iterations == 3


# ---- the C side --------------------------------------------------------------------------------------------------------------------
def test_the_two_new_structs_have_the_layout_the_c_compiler_gives_the_header(tmp_path):
    import ctypes
    from deepctr_amd import _C
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    pairs = {"Seg": "dctr_opt_seg_t", "Args": "dctr_opt_args_t"}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dctr.h"', "int main(void) {"]
    for py, c in pairs.items():
        lines.append('    printf("%s sizeof %%zu\\n", sizeof(%s));' % (py, c))
        for fname, _ in getattr(_C.opt, py)._fields_:
            lines.append('    printf("%s %s %%zu\\n", offsetof(%s, %s));' % (py, fname, c, fname))
    lines += ['    printf("kinds %d %d %d %d %d %d %d\\n", DCTR_OPT_ADAM, DCTR_OPT_ADAGRAD, DCTR_OPT_RMSPROP, DCTR_OPT_SGD, DCTR_OPT_ADAMAX, '
              'DCTR_OPT_ADADELTA, DCTR_OPT_FTRL);', "    return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    seen = 0
    for line in filter(None, out):
        parts = line.split()
        if parts[0] == "kinds":
            o = _C.opt
            assert [int(v) for v in parts[1:]] == [o.ADAM, o.ADAGRAD, o.RMSPROP, o.SGD, o.ADAMAX, o.ADADELTA, o.FTRL]
            assert [int(v) for v in parts[1:]] == [optimizers.KIND_ADAM, optimizers.KIND_ADAGRAD, optimizers.KIND_RMSPROP, optimizers.KIND_SGD,
                                                   optimizers.KIND_ADAMAX, optimizers.KIND_ADADELTA, optimizers.KIND_FTRL]
            continue
        py, field, val = parts
        cls = getattr(_C.opt, py)
        want = ctypes.sizeof(cls) if field == "sizeof" else getattr(cls, field).offset
        assert int(val) == want, "%s.%s: C says %s, ctypes %d" % (py, field, val, want)
        seen += 1
    assert seen == 2 + len(_C.opt.Seg._fields_) + len(_C.opt.Args._fields_)


def test_opt_apply_reports_bad_arguments_before_any_launch():
    import ctypes
    from deepctr_amd import _C
    lib = _C.lib()
    a = _C.opt.Args(kind=_C.opt.ADAM, lr=0.1)
    assert lib.dctr_opt_apply(None, None, 1, 4, None) == -1                        # DCTR_E_NULL
    assert lib.dctr_opt_apply(ctypes.byref(a), None, 1, 4, None) == -1
    assert lib.dctr_opt_apply(ctypes.byref(a), None, 0, 4, None) == 0              # nothing to do
    for kind in (-1, 7, 9):
        assert lib.dctr_opt_apply(ctypes.byref(_C.opt.Args(kind=kind)), None, 1, 4, None) == -4        # DCTR_E_ENUM
    assert lib.dctr_opt_apply(ctypes.byref(_C.opt.Args(kind=_C.opt.FTRL, lr=0.1, lr_power=0.5)), None, 1, 4, None) == -4
    assert lib.dctr_opt_apply(ctypes.byref(a), ctypes.c_void_p(4100), 1, 4, None) == -3             # DCTR_E_ALIGN (nothing dereferenced)
    a.clip_scale = 4098
    assert lib.dctr_opt_apply(ctypes.byref(a), ctypes.c_void_p(4096), 1, 4, None) == -3
    assert lib.dctr_opt_multi(9, None, 1, 4, 0.1, 0.9, 0.999, 1e-7, 1, None) == -4                  # the old entry point keeps its four kinds
    need = lib.dctr_grad_clip_scales_workspace_bytes(3, 1000)
    assert need == 3 * (1 + 1) * 8 and lib.dctr_grad_clip_scales_workspace_bytes(2, 10 ** 9) == 2 * 513 * 8
    seg, ws, out = ctypes.c_void_p(4096), ctypes.c_void_p(8192), ctypes.c_void_p(12288)
    assert lib.dctr_grad_clip_scales(seg, 3, 1000, 0, 1.0, ws, need - 8, out, None) == -1          # too small a workspace
    assert lib.dctr_grad_clip_scales(seg, 3, 1000, 0, 1.0, None, need, out, None) == -1
    assert lib.dctr_grad_clip_scales(seg, 3, 1000, 2, 1.0, ws, need, out, None) == -4
    assert lib.dctr_grad_clip_scales(seg, 3, 1000, 0, 1.0, ctypes.c_void_p(8196), need, out, None) == -3
    assert "opt_kernels.hip" in __import__("deepctr_amd.build", fromlist=["SOURCES"]).SOURCES
