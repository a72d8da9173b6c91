"""CPU: CCPM / FGCNN / KMaxPooling / FGCNNLayer — the NumPy oracle (tests/ref_fieldconv.py) against the reference's own outputs
(tests/golden/model_ccpm_*.npz, model_fgcnn_*.npz, kmax_layer.npz, fgcnn_layer.npz; scripts/make_golden_ccpm_fgcnn.py) and the
conditions that script records, the torch restatement the training path uses (training._field_conv, the models' model_logits) against
the fixtures and the float64 oracle, fit() on the autograd step, the API contract, and the C ABI's argument checks, routes and
workspace sizes (no launch)."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from tests import ref_fieldconv as RF
from tests.ccpm_fgcnn_util import (CCPM_FIXTURES, FGCNN_FIXTURES, FGCNN_LAYER_TAGS, FIXTURES, build_model, fgcnn_layer_case, fixture_feed,
                                   fixture_weights, make_stack, problem)
from tests.util import assert_close, golden_meta, load_golden, sigmoid_inv

CPU = torch.device("cpu")


def _to_float64(layer):
    for k in list(layer._weights):
        layer._weights[k] = layer._weights[k].double()
    for sub in layer._sublayers:
        _to_float64(sub)


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_matches_reference_code_and_the_fixture_conditions_hold(name):
    g = load_golden(name)
    meta = golden_meta(g)
    ref = RF.run_fixture(g, np.float64)
    assert g["y"].shape[0] == 32 and np.abs(ref.reshape(-1) - g["y"].reshape(-1)).max() < 1e-5
    if meta["kwargs"].get("task") != "regression":
        assert g["y"].min() > 1e-3 and g["y"].max() < 1 - 1e-3
    stats = []
    base = RF.run_fixture(g, np.float64, task="regression", stats=stats).reshape(-1)
    tol = 1e-4 * np.abs(base).max()
    muts = RF.applicable(meta)
    for m in muts:
        assert np.abs(RF.run_fixture(g, np.float64, task="regression", mutate=(m,)).reshape(-1) - base).max() / tol >= 100, m
    if "noconv" in name:
        assert not muts and not stats
    else:
        assert (np.concatenate(stats) < 3).mean() >= 0.9


def test_every_mutation_is_told_apart_by_some_fixture():
    seen = set()
    for name in FIXTURES:
        seen.update(RF.applicable(golden_meta(load_golden(name))))
    assert seen == set(RF.MUTATIONS)
    # the three-layer CCPM fixture is the one where min(k, rows) bites: the schedule alone would ask for 3 of 1 row
    meta = golden_meta(load_golden("model_ccpm_l3"))
    n, l = len(meta["dnn"]), len(meta["kwargs"]["conv_filters"])         # noqa: E741
    assert [RF.ccpm_k(i, l, n) for i in range(1, l + 1)] == [4, 1, 3]


def test_kmax_layer_fixture_against_the_oracle():
    g = load_golden("kmax_layer")
    seen = 0
    for tag in ("d3", "d4"):
        x = g[tag + "/x"]
        assert x.shape[0] == 32 and len(np.unique(x[0])) < x[0].size       # repeated values
        for axis in range(1, x.ndim):
            for k in sorted(set((1, min(3, x.shape[axis]), x.shape[axis]))):
                y = g["%s/axis%d/k%d" % (tag, axis, k)]
                assert np.array_equal(y, RF.kmax(x, k, axis)) and y.shape[axis] == k
                if 1 < k:
                    assert not np.array_equal(y, RF.kmax(x, k, axis, mutate=("keep_order",)))
                seen += 1
    assert seen == len([k for k in g if "/axis" in k])


@pytest.mark.parametrize("tag", FGCNN_LAYER_TAGS)
def test_fgcnn_layer_oracle_matches_reference_code(tag):
    cfg, x, w, y = fgcnn_layer_case(load_golden("fgcnn_layer"), tag)
    ref = RF.fgcnn_layer(x, w, cfg["filters"], cfg["kernel_width"], cfg["new_maps"], cfg["pooling_width"])
    assert ref.shape == y.shape and np.abs(ref - y).max() < 1e-5
    from deepctr_amd.layers import FGCNNLayer
    from deepctr_amd.layers.base import name_scope
    layer = FGCNNLayer(cfg["filters"], cfg["kernel_width"], cfg["new_maps"], cfg["pooling_width"], device=CPU)
    assert layer.compute_output_shape((None,) + x.shape[1:]) == (None,) + y.shape[1:]
    with name_scope():          # keras' auto names from zero: conv2d, dense, conv2d_1, dense_1
        layer.build((None,) + x.shape[1:])
    assert {k: tuple(v.shape) for k, v in layer.named_weights()} == {k: tuple(v.shape) for k, v in w.items()}
    got = _torch_layer(layer, w, x)
    assert_close(got, y, rtol=1e-4, atol=2e-6, what=tag)


def _torch_layer(layer, w, x):
    from deepctr_amd import training
    for name, t in layer.named_weights():
        t.copy_(torch.from_numpy(w[name]))
    return training._fgcnn_layer(layer, torch.from_numpy(x)).numpy()


def test_fgcnn_layer_fixture_covers_odd_and_even_fields_and_an_even_width():
    g = load_golden("fgcnn_layer")
    cases = {t: fgcnn_layer_case(g, t) for t in FGCNN_LAYER_TAGS}
    assert cases["odd"][1].shape[1] % 2 == 1 and cases["even"][1].shape[1] % 2 == 0
    assert any(w % 2 == 0 for w in cases["even"][0]["kernel_width"]) and max(cases["even"][0]["filters"]) > 16
    cfg, x, w, y = cases["even"]
    args = (cfg["filters"], cfg["kernel_width"], cfg["new_maps"], cfg["pooling_width"])
    for m in ("pad_side", "flip", "channel_first", "pool_pad", "recombine_ew"):
        assert np.abs(RF.fgcnn_layer(x, w, *args, mutate=(m,)) - y).max() > 1e-2, m


@pytest.mark.parametrize("B,F,E,chain,widths,pools", [
    (3, 5, 4, (1, 3), (6,), [("kmax", 3)]),
    (2, 7, 3, (1, 16, 17), (7, 2), [("max", 2), ("kmax", 3)]),
    (2, 7, 2, (4, 20, 1), (10, 6, 1), [("max", 3), ("kmax", 2), ("max", 1)]),
    (1, 1, 1, (1, 1), (4,), [("max", 1)]),
])
def test_torch_restatement_matches_oracle_in_float64(B, F, E, chain, widths, pools):
    from deepctr_amd import training
    rng = np.random.RandomState(F * 10 + E)
    ks, bs = make_stack(rng, chain, widths)
    x = rng.standard_normal((B, F, E) + ((chain[0],) if chain[0] > 1 else ()))
    got, maps = training._field_conv(torch.from_numpy(x), [torch.from_numpy(k.astype(np.float64)) for k in ks],
                                     [torch.from_numpy(b.astype(np.float64)) for b in bs], pools)
    ref, rmaps = RF.field_conv(x, ks, bs, pools)
    assert got.dtype == torch.float64 and got.shape == ref.shape and np.abs(got.numpy() - ref).max() <= 1e-12
    for a, b in zip(maps, rmaps):
        assert np.abs(a.numpy() - b).max() <= 1e-12
    # keras' 4-D kernel [w, 1, C_in, C_out] is the same stack
    got4, _ = training._field_conv(torch.from_numpy(x), [torch.from_numpy(k.astype(np.float64)).unsqueeze(1) for k in ks],
                                   [torch.from_numpy(b.astype(np.float64)) for b in bs], pools)
    assert torch.equal(got, got4)


# (the hashed fixtures are left to the GPU suite: the integer Hash runs inside the HIP kernels only)
@pytest.mark.parametrize("name", [n for n in FIXTURES if not n.endswith("_hash")])
def test_torch_restatement_matches_the_fixture_and_the_oracle(name):
    from deepctr_amd import engine, training
    g = load_golden(name)
    meta = golden_meta(g)
    model = build_model(meta, CPU)
    mine = {k: tuple(v.shape) for k, v in model.get_weights_by_name().items()}
    assert mine == {k: tuple(v.shape) for k, v in fixture_weights(g).items()}
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
    for sp in (model.stage_plan, getattr(model, "fg_stage", None)):         # (the plans hold the tables themselves)
        for f in (sp.fields if sp is not None else ()):
            f.table = f.table.double()
            f.lin_table = None if f.lin_table is None else f.lin_table.double()
    with torch.no_grad():
        logit = training.model_logits(model, staged, 0, n)
    assert logit.dtype == torch.float64
    ref = RF.run_fixture(g, np.float64, task="regression").reshape(-1)
    assert_close(logit.numpy().reshape(-1), ref, rtol=1e-6, atol=1e-7, what=name + " model_logits vs the oracle")


def test_k_schedule_is_the_reference_expression():
    from deepctr_amd.models.ccpm import kmax_schedule
    for l in range(1, 5):           # noqa: E741
        for n in range(1, 41):
            want, rows = [], n
            for i in range(1, l + 1):
                rows = min(RF.ccpm_k(i, l, n), rows)
                want.append(rows)
            assert kmax_schedule(n, l) == want, (l, n)
            assert all(1 <= k <= n for k in want)
    assert kmax_schedule(26, 2) == [13, 3] and kmax_schedule(5, 3) == [4, 1, 1] and kmax_schedule(2, 1) == [2] and kmax_schedule(7, 0) == []


def test_cpu_fit_on_the_autograd_step_lowers_the_loss():
    """training._fit_torch is device-agnostic torch code: CPU-built models train for three epochs on a planted signal and the conv
    kernels (and FGCNN's second embedding set and recombination) move."""
    from deepctr_amd import engine, training
    from deepctr_amd.models import CCPM, FGCNN
    for ctor, kw, moving in ((CCPM, dict(conv_kernel_width=(4, 3), conv_filters=(3, 3)), ("conv2d",)),
                             (FGCNN, dict(conv_kernel_width=(3, 3), conv_filters=(3, 4), new_maps=(2, 1), pooling_width=(2, 2)),
                              ("conv2d", "fgsparse_emb", "dense/", "dense_1/"))):
        rng = np.random.RandomState(9)
        n = 512
        cols, feed = problem(rng, n, F=6, E=4, vocab=8, seq=True)
        y = ((feed["C0"] % 2) ^ (feed["C1"] % 2)).astype(np.float32)
        torch.manual_seed(0)
        np.random.seed(0)
        model = ctor(cols, cols, dnn_hidden_units=(16, 8), device=CPU, **kw)
        model.compile("adam", "binary_crossentropy")
        staged = engine.Staged(n)
        model._stage_inputs(feed, staged)
        before = {k: t.clone() for k, t in model.named_weights() if k.startswith(moving)}
        losses = []

        class End(object):
            def __call__(self, ep, loss):
                losses.append(loss)
                return False

            def finish(self):
                return losses

        training._fit_torch(model, staged, torch.from_numpy(y), n, 64, 3, True, End())
        assert len(losses) == 3 and np.isfinite(losses).all() and losses[-1] < losses[0], (ctor.__name__, losses)
        after = dict(model.named_weights())
        assert len(before) >= 4 and not [k for k in before if torch.equal(before[k], after[k])]


def test_regularizer_groups_reach_both_embedding_sets():
    from deepctr_amd import training
    from deepctr_amd.models import CCPM, FGCNN
    cols, _ = problem(np.random.RandomState(0), 4, F=4, dense=False)
    m = FGCNN(cols, cols, conv_kernel_width=(3,), conv_filters=(2,), new_maps=(1,), pooling_width=(2,), dnn_hidden_units=(4,),
              l2_reg_linear=0.5, l2_reg_embedding=0.25, l2_reg_dnn=0.125, device=CPU)
    assert m.regularizers == {"embedding": 0.25, "linear": 0.5, "dnn": 0.125}
    regs = {t.data_ptr(): l2 for t, l2 in training.regularized_weights(m)}
    by_name = dict(m.named_weights())
    assert regs[by_name["fgsparse_emb_C0/embeddings"].data_ptr()] == 0.25 and regs[by_name["sparse_emb_C0/embeddings"].data_ptr()] == 0.25
    assert regs[by_name["linear0sparse_emb_C0/embeddings"].data_ptr()] == 0.5 and regs[by_name["dnn/kernel0"].data_ptr()] == 0.125
    assert by_name["conv2d/kernel"].data_ptr() not in regs and by_name["dense/kernel"].data_ptr() not in regs
    c = CCPM(cols, cols, l2_reg_dnn=0.5, device=CPU)
    assert c.regularizers == {"embedding": 1e-5, "linear": 1e-5, "dnn": 0.5}


def test_signature_defaults_match_the_reference():
    from deepctr_amd.layers import FGCNNLayer, KMaxPooling
    from deepctr_amd.models import CCPM, FGCNN
    sig = inspect.signature(CCPM)
    want = dict(conv_kernel_width=(6, 5), conv_filters=(4, 4), dnn_hidden_units=(128, 64), l2_reg_linear=1e-5, l2_reg_embedding=1e-5,
                l2_reg_dnn=0, dnn_dropout=0, seed=1024, task='binary', device=None)
    assert list(sig.parameters) == ["linear_feature_columns", "dnn_feature_columns"] + list(want)
    assert {k: sig.parameters[k].default for k in want} == want
    sig = inspect.signature(FGCNN)
    want = dict(conv_kernel_width=(7, 7, 7, 7), conv_filters=(14, 16, 18, 20), new_maps=(3, 3, 3, 3), pooling_width=(2, 2, 2, 2),
                dnn_hidden_units=(256, 128, 64), l2_reg_linear=1e-5, l2_reg_embedding=1e-5, l2_reg_dnn=0, dnn_dropout=0, seed=1024,
                task='binary', device=None)
    assert list(sig.parameters) == ["linear_feature_columns", "dnn_feature_columns"] + list(want)
    assert {k: sig.parameters[k].default for k in want} == want
    sig = inspect.signature(KMaxPooling.__init__)
    assert [(k, p.default) for k, p in list(sig.parameters.items())[1:3]] == [("k", 1), ("axis", -1)]
    sig = inspect.signature(FGCNNLayer.__init__)
    assert [(k, p.default) for k, p in list(sig.parameters.items())[1:5]] == [("filters", (14, 16)), ("kernel_width", (7, 7)),
                                                                            ("new_maps", (3, 3)), ("pooling_width", (2, 2))]


def test_argument_checks_and_their_messages():
    from deepctr_amd import ops
    from deepctr_amd.feature_column import DenseFeat
    from deepctr_amd.layers import FGCNNLayer, KMaxPooling
    from deepctr_amd.models import CCPM, FGCNN
    rng = np.random.RandomState(1)
    cols, _ = problem(rng, 4, F=5)
    with pytest.raises(ValueError) as e:
        CCPM(cols, cols, conv_kernel_width=(6, 5), conv_filters=(4,), device=CPU)
    assert str(e.value) == "conv_kernel_width must have same element with conv_filters"
    with pytest.raises(ValueError) as e:
        CCPM(cols, cols + [DenseFeat("price", 1)], device=CPU)
    assert str(e.value) == "DenseFeat is not supported in dnn_feature_columns"
    mixed, _ = problem(rng, 4, F=3)
    with pytest.raises(ValueError) as e:
        CCPM(cols, mixed[:2] + [mixed[2]._replace(embedding_dim=8)], device=CPU)
    assert "one embedding_dim" in str(e.value)
    CCPM(cols, cols, conv_kernel_width=(), conv_filters=(), dnn_hidden_units=(), device=CPU)        # both empty lists are legal
    with pytest.raises(ValueError) as e:
        FGCNN(cols, cols, conv_kernel_width=(7, 7), device=CPU)
    assert str(e.value) == "conv_kernel_width,conv_filters,new_maps  and pooling_width must have same length"
    with pytest.raises(ValueError) as e:
        FGCNN(cols, cols, conv_kernel_width=(3, 3), conv_filters=(2, 2), new_maps=(1, 1), pooling_width=(3, 2), device=CPU)   # 5 -> 1 -> 0 rows
    assert "empty feature map" in str(e.value)
    with pytest.raises(ValueError):
        FGCNN(cols + [DenseFeat("price", 1)], cols, conv_kernel_width=(), conv_filters=(), new_maps=(), pooling_width=(), device=CPU)
    m = FGCNN(cols, cols + [DenseFeat("price", 1)], conv_kernel_width=(), conv_filters=(), new_maps=(), pooling_width=(), device=CPU)
    assert m.fgcnn is None and m.dnn_in_dim == 5 * 4 + 10 and m.input_names[-1] == "price"      # the dense value is an input, and ignored
    with pytest.raises(ValueError) as e:
        FGCNNLayer(filters=(1, 2), kernel_width=(3,))
    assert str(e.value) == "length of argument must be equal"
    with pytest.raises(ValueError) as e:
        FGCNNLayer(device=CPU).build((None, 8))
    assert str(e.value) == "Unexpected inputs dimensions 2, expect to be 3 dimensions"
    with pytest.raises(ValueError) as e:
        KMaxPooling(k=1, axis=-1).build((None, 5, 4))               # the reference's default axis is refused by its own build
    assert str(e.value) == "axis must be 1~3,now is -1"
    with pytest.raises(ValueError) as e:
        KMaxPooling(k=1, axis=4).build((None, 5, 4))
    assert str(e.value) == "axis must be 1~3,now is 4"
    for k in (0, 6):
        with pytest.raises(ValueError) as e:
            KMaxPooling(k=k, axis=1).build((None, 5, 4))
        assert str(e.value) == "k must be in 1 ~ 5,now k is %d" % k
    x = torch.zeros(3, 5, 4)
    ks, bs = make_stack(rng, (1, 3, 2), (3, 2))
    ks, bs = [torch.from_numpy(k) for k in ks], [torch.from_numpy(b) for b in bs]
    for bad in (dict(pools=[("kmax", 3)]), dict(pools=[("kmax", 6), ("max", 1)]), dict(pools=[("max", 2), ("max", 3)]),
                dict(pools=[("avg", 2), ("max", 1)]), dict(pools=[("kmax", 0), ("max", 1)]), dict(pools=[("max", 1)] * 2, route="fast")):
        with pytest.raises(ValueError):
            ops.field_conv(x, ks, bs, **bad)
    with pytest.raises(ValueError):
        ops.field_conv(x, ks, bs[:1], [("max", 1)] * 2)
    with pytest.raises(ValueError):
        ops.field_conv(x, [ks[0], ks[1].transpose(1, 2)], bs, [("max", 1)] * 2)         # C_in of stage 1 is not C_out of stage 0
    with pytest.raises(ValueError) as e:
        ops.field_conv(torch.zeros(3, 20), ks, bs, [("max", 1)] * 2)
    assert "expect to be 3 or 4 dimensions" in str(e.value)
    with pytest.raises(ValueError):
        ops.field_conv(torch.zeros(3, 19), ks, bs, [("max", 1)] * 2, fields=5, dim=4)   # the buffer is narrower than F E
    with pytest.raises(ValueError):
        ops.kmax_pool(torch.zeros(3, 5), 6, 1)
    with pytest.raises(ValueError):
        ops.kmax_pool(torch.zeros(3, 5), 1, 2)
    assert ops.field_conv_macs(26, 8, [(6, 1, 4), (5, 4, 4)], [("kmax", 13), ("kmax", 3)]) == 8 * (26 * 6 * 4 + 13 * 5 * 4 * 4)


def test_layer_contract_weight_names_initial_values_and_config_round_trip():
    from deepctr_amd.layers import FGCNNLayer, KMaxPooling, custom_objects
    layer = FGCNNLayer((3, 5), (6, 3), (2, 1), (2, 3), device=CPU)
    layer.build((None, 13, 4))
    names = [n.split("/")[1] for n, _ in layer.named_weights()]
    assert names == ["kernel", "bias"] * 4
    shapes = [tuple(t.shape) for t in layer.weights]
    assert shapes == [(6, 1, 1, 3), (3,), (6 * 4 * 3, 6 * 4 * 2), (6 * 4 * 2,), (3, 1, 3, 5), (5,), (2 * 4 * 5, 2 * 4 * 1), (2 * 4 * 1,)]
    k0, b0, d0 = layer.weights[0], layer.weights[1], layer.weights[2]
    assert torch.equal(b0, torch.zeros(3)) and float(k0.abs().max()) <= (6.0 / (6 * 1 + 6 * 3)) ** 0.5 and float(k0.abs().max()) > 0
    assert float(d0.abs().max()) <= (6.0 / (72 + 48)) ** 0.5
    assert layer.compute_output_shape((None, 13, 4)) == (None, 6 * 2 + 2 * 1, 4) and layer.new_features == 14
    cfg = layer.get_config()
    assert {k: cfg[k] for k in ("filters", "kernel_width", "new_maps", "pooling_width")} == dict(
        filters=(3, 5), kernel_width=(6, 3), new_maps=(2, 1), pooling_width=(2, 3))
    assert FGCNNLayer.from_config(cfg).get_config() == cfg
    km = KMaxPooling(k=3, axis=2, device=CPU)
    km.build((None, 4, 6, 2))
    assert km.compute_output_shape((None, 4, 6, 2)) == (None, 4, 3, 2) and not km.weights
    cfg = km.get_config()
    assert cfg["k"] == 3 and cfg["axis"] == 2 and KMaxPooling.from_config(cfg).get_config() == cfg
    assert custom_objects["FGCNNLayer"] is FGCNNLayer and custom_objects["KMaxPooling"] is KMaxPooling


def test_reference_import_names():
    import deepctr.layers.interaction as inter
    import deepctr.layers.sequence as seq
    import deepctr.models
    import deepctr.models.ccpm as ccpm_mod
    import deepctr.models.fgcnn as fgcnn_mod
    import deepctr_amd.models.ccpm
    import deepctr_amd.models.fgcnn
    from deepctr.layers import custom_objects
    from deepctr.models import CCPM, FGCNN
    assert ccpm_mod is deepctr_amd.models.ccpm and ccpm_mod.CCPM is CCPM and deepctr.models.ccpm is ccpm_mod
    assert fgcnn_mod is deepctr_amd.models.fgcnn and fgcnn_mod.FGCNN is FGCNN and deepctr.models.fgcnn is fgcnn_mod
    assert custom_objects["KMaxPooling"] is seq.KMaxPooling and custom_objects["FGCNNLayer"] is inter.FGCNNLayer
    assert "MLR" not in dir(deepctr.models)


def _args(keep, **kw):
    from deepctr_amd import _C
    arr = lambda v: (ctypes.c_int32 * len(v))(*v)       # noqa: E731
    stages = dict(widths=[6, 5], channels=[4, 4], pool_kinds=[0, 0], pool_args=[3, 3])
    for k in list(stages):
        if k in kw:
            stages[k] = kw.pop(k)
    base = dict(batch=4, x_stride=28, x_offset=0, fields=7, dim=4, in_channels=1, n_stages=len(stages["widths"]), route=0,
                out_stride=3 * 4 * stages["channels"][-1], out_offset=0)
    base.update(kw)
    a = _C.fieldconv.Args(**base)
    for k, v in stages.items():
        keep.append(arr(v))
        setattr(a, k, ctypes.cast(keep[-1], ctypes.c_void_p))
    return a


def test_abi_argument_errors_without_a_gpu():
    from deepctr_amd import _C
    lib = _C.lib()
    keep = []
    f = lambda a: lib.dctr_fieldconv_fwd(ctypes.byref(a), None)        # noqa: E731
    r = lambda a: lib.dctr_fieldconv_route(ctypes.byref(a))           # noqa: E731
    assert lib.dctr_fieldconv_fwd(None, None) == -1 and lib.dctr_fieldconv_route(None) == -1 and lib.dctr_fieldconv_workspace_bytes(None) == 0
    assert f(_args(keep)) == -1 and b"fieldconv_fwd" in lib.dctr_last_error()          # x / kernels / biases / out missing
    assert r(_args(keep)) == _C.fieldconv.ROUTE_RESIDENT
    for bad in (dict(fields=0), dict(dim=0), dict(in_channels=0), dict(batch=-1), dict(n_stages=0), dict(n_stages=9), dict(x_stride=27),
                dict(x_offset=1), dict(x_offset=-1), dict(out_stride=47), dict(out_offset=1), dict(pool_args=[8, 3]), dict(pool_args=[3, 4]),
                dict(pool_args=[0, 1]), dict(widths=[0, 5]), dict(channels=[4, 0]), dict(pool_kinds=[1, 1], pool_args=[2, 4])):
        assert f(_args(keep, **bad)) == -2 and r(_args(keep, **bad)) == -2, bad
    for bad in (dict(route=4), dict(route=-1), dict(pool_kinds=[2, 0]), dict(pool_kinds=[0, -1])):
        assert f(_args(keep, **bad)) == -4, bad
    ptrs = (ctypes.c_void_p * 2)(16, 16)
    holes = (ctypes.c_void_p * 2)(16, None)
    a = _args(keep, x=16, out=16, kernels=ctypes.cast(ptrs, ctypes.c_void_p), biases=ctypes.cast(holes, ctypes.c_void_p))
    assert f(a) == -1 and b"stage 1" in lib.dctr_last_error()        # a null bias is reported before anything is launched
    a.biases = ctypes.cast(ptrs, ctypes.c_void_p)
    souts = (ctypes.c_void_p * 2)(16, None)
    strides = (ctypes.c_int64 * 2)(47, 0)
    a.stage_outs, a.stage_out_strides = ctypes.cast(souts, ctypes.c_void_p), ctypes.cast(strides, ctypes.c_void_p)
    assert f(a) == -2 and b"stage_out" in lib.dctr_last_error()      # stage 0's map is [3, 4, 4] = 48 floats
    strides[0] = 48
    a.batch = 0
    assert f(a) == 0                                                 # complete arguments, empty batch: a no-op
    a.batch, a.route = 4, _C.fieldconv.ROUTE_WORKSPACE
    assert r(a) == _C.fieldconv.ROUTE_STREAMED and lib.dctr_fieldconv_workspace_bytes(ctypes.byref(a)) > 0
    assert f(a) == -1 and b"workspace" in lib.dctr_last_error()      # a forced route without its workspace, before anything is written
    a.workspace, a.workspace_bytes = 24, 1 << 30
    assert f(a) == -3                                                # a workspace that is not 16-byte aligned
    big = _args(keep, widths=[7, 7], channels=[400, 400], pool_kinds=[1, 1], pool_args=[1, 1], fields=40, x_stride=160,
                out_stride=40 * 4 * 400)
    assert r(big) == _C.fieldconv.ROUTE_STREAMED
    big.route = _C.fieldconv.ROUTE_RESIDENT
    assert r(big) == -5 and f(big) == -5 and lib.dctr_fieldconv_workspace_bytes(ctypes.byref(big)) == 0
    assert lib.dctr_kmax_pool_fwd(None, 4, 5, 3, 2, None, None) == -1
    assert lib.dctr_kmax_pool_fwd(None, 0, 5, 3, 2, None, None) == 0
    for bad in ((4, 0, 3, 1), (4, 5, 3, 0), (4, 5, 3, 6), (-1, 5, 3, 2), (4, 5, -1, 2)):
        assert lib.dctr_kmax_pool_fwd(16, bad[0], bad[1], bad[2], bad[3], 16, None) == -2, bad


def test_routes_and_workspace_sizes_without_a_gpu():
    from deepctr_amd import ops
    ccpm = ([(6, 1, 4), (5, 4, 4)], [("kmax", 13), ("kmax", 3)])
    fg = ([(7, 1, 14), (7, 14, 16), (7, 16, 18), (7, 18, 20)], [("max", 2)] * 4)
    # CCPM's default stack keeps its kernels in LDS; FGCNN's (53 KiB of kernels beside the maps) would cost a workgroup per CU: streamed
    assert ops.field_conv_route(26, 8, *ccpm) == "resident"
    for F, E in ((26, 8), (39, 16)):
        assert ops.field_conv_route(F, E, *fg) == "streamed" and ops.field_conv_workspace_bytes(4096, F, E, *fg) == 0
        assert ops.field_conv_route(F, E, *fg, route="resident") == "resident"          # it fits the 160 KiB when asked for
    # the smallest channel count at which the kernels no longer fit next to the maps
    c = 1
    stack = lambda c: ([(7, 1, c), (7, c, c)], [("max", 2), ("max", 2)])       # noqa: E731
    while ops.field_conv_route(26, 8, *stack(c)) == "resident":
        c += 1
    assert 8 < c < 200 and ops.field_conv_route(26, 8, *stack(c)) == "streamed" and ops.field_conv_route(26, 8, *stack(c - 1)) == "resident"
    assert ops.field_conv_route(26, 8, *stack(c - 1), route="streamed") == "streamed"
    assert ops.field_conv_route(26, 8, *stack(c), route="resident") == "resident"      # forced, the route holds up to the whole LDS
    with pytest.raises(Exception):
        ops.field_conv_route(26, 8, *stack(400), route="resident")
    assert ops.field_conv_workspace_bytes(4096, 26, 8, *stack(c)) == 0          # streamed kernels, the maps still in LDS
    # 16 columns' maps past the LDS: a workspace for at most 256 workgroups, capped at 256 MiB
    wide = ([(3, 1, 600)], [("max", 1)])
    small, large = ops.field_conv_workspace_bytes(1, 40, 8, *wide), ops.field_conv_workspace_bytes(1 << 20, 40, 8, *wide)
    assert small == large > 160 * 1024 and large <= 256 << 20 and large % 16 == 0
    assert ops.field_conv_route(40, 8, *wide) == "streamed"
    forced = ops.field_conv_workspace_bytes(16, 7, 4, *ccpm[:1], [("kmax", 3), ("kmax", 3)], route="workspace")
    assert 0 < forced < small


def test_args_mirror_has_the_layout_the_c_compiler_gives_the_header(tmp_path):
    import os
    import shutil
    import subprocess
    from deepctr_amd import _C
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    cls = _C.fieldconv.Args
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dctr.h"', "int main(void) {",
             '    printf("sizeof %zu\\n", sizeof(dctr_fieldconv_args_t));', '    printf("maxs %d\\n", DCTR_FIELDCONV_MAX_STAGES);',
             '    printf("abi %d\\n", DCTR_ABI_VERSION);',
             '    printf("pools %d\\n", DCTR_FIELDCONV_POOL_KMAX + 10 * DCTR_FIELDCONV_POOL_MAX);',
             '    printf("routes %d\\n", DCTR_FIELDCONV_ROUTE_AUTO + 10 * DCTR_FIELDCONV_ROUTE_RESIDENT + 100 * DCTR_FIELDCONV_ROUTE_STREAMED'
             ' + 1000 * DCTR_FIELDCONV_ROUTE_WORKSPACE);']
    for fname, _ in cls._fields_:
        lines.append('    printf("%s %%zu\\n", offsetof(dctr_fieldconv_args_t, %s));' % (fname, fname))
    lines += ["    return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    P, R = _C.fieldconv.POOLS, _C.fieldconv.ROUTES
    for line in filter(None, out):
        field, val = line.split()
        if field == "maxs":
            want = _C.fieldconv.MAX_STAGES
        elif field == "abi":
            want = 13
        elif field == "pools":
            want = P["kmax"] + 10 * P["max"]
        elif field == "routes":
            want = sum(10 ** i * R[k] for i, k in enumerate((None, "resident", "streamed", "workspace")))
        else:
            want = ctypes.sizeof(cls) if field == "sizeof" else getattr(cls, field).offset
        assert int(val) == want, "%s: C says %s, ctypes %d" % (field, val, want)
