"""CPU: the float64 oracle of dctr_transformer_bwd (tests/ref_transformer_bwd.py) against torch double autograd over
training._transformer, the room tests.util.assert_close_terms leaves a float32 implementation, what the case table covers and can
tell apart, the host-only entry points (no launch), the C layout of the args struct, and the autograd step's transformer on the CPU.

Worst err / bar of float32 torch autograd of training._transformer on the CPU against the oracle (-s prints every case):
bst 0.021, dsin_pe 0.029, dsin_t1 0.032, sum_general 0.089, no_res 0.010, no_ffn 0.018 — so the default bar stands."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import ref_transformer_bwd as RT
from tests.util import TERMS_REPORT, assert_close_terms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [c.name for c in RT.CASES]


def _torch_grads(case, dtype):
    """{oracle key: gradient} from torch autograd over training._transformer, layer by layer, on the CPU."""
    from deepctr_amd import training
    inp = RT.case_inputs(case)
    x = torch.tensor(inp.x, dtype=dtype, requires_grad=True)
    layers = [RT.TorchLayer(W, case.cfg, dtype) for W in inp.layers]
    qm, km = torch.tensor(inp.qmask), torch.tensor(inp.kmask)
    y = x
    for i, layer in enumerate(layers):
        layer.output_type = case.cfg.out if i == len(layers) - 1 else None
        y = training._transformer(layer, y, y, qm, km, False)
    if case.cfg.out is not None:
        y = y.squeeze(1)
    y.backward(torch.tensor(inp.d_out, dtype=dtype))
    G = {"dx": x.grad.double().numpy()}
    for l, layer in enumerate(layers):
        for k, g in layer.grads().items():
            if RT.live_weights(case.cfg)[k[1:]]:
                G["%s%d" % (k, l)] = g
    return G


def test_case_table_covers_what_was_agreed():
    cs = RT.CASES
    assert {c.cfg.E for c in cs} == {8, 12, 16, 20, 32} and {c.cfg.T for c in cs} == {1, 2, 17} and {c.B for c in cs} >= {1, 17, 33}
    assert any(c.cfg.E == 8 and c.cfg.H == 8 for c in cs) and {c.cfg.L for c in cs} == {1, 2, 3}
    for flag in ("pe", "res", "ffn", "ln", "blind"):
        assert {bool(getattr(c.cfg, flag)) for c in cs} == {False, True}, flag
    assert {c.cfg.out for c in cs} == {None, "mean", "sum"} and {c.outputs for c in cs} == {"both", "dx", "weights"}
    assert {c.masks for c in cs} == {"lengths", "mask", "mask2", None}
    assert any(c.cfg[4:] == (True, True, True, True, False, None) for c in cs)                     # BST
    assert {c.cfg.pe for c in cs if c.cfg[5:] == (True, True, False, True, "mean")} == {False, True}  # DSIN, bias encoding on / off
    assert any(c.B == 33 and c.max_blocks == 2 for c in cs)
    assert any(c.route == "general" and RT.plan(c.cfg, c.B).route == "fused" for c in cs)
    assert any(c.cfg.T == 1 and c.cfg.blind for c in cs)
    lens = RT.case_inputs(RT.CASE_BY_NAME["bst"]).lengths
    assert lens[1] == 0 and lens[0] == 17
    m2 = RT.case_inputs(RT.CASE_BY_NAME["no_res"])
    assert m2.qmask[1].all() and not m2.kmask[1].any() and not m2.qmask[2, 0] and m2.kmask[2].all()
    assert not RT.CASE_BY_NAME["no_res"].cfg.res and RT.CASE_BY_NAME["no_res"].cfg.ln
    for c in cs:        # a persistent walk with a ragged last tile where max_blocks asks for one
        p = RT.plan(c.cfg, c.B, c.route, c.max_blocks)
        if c.max_blocks:
            assert -(-c.B // p.S) > p.grid == c.max_blocks and c.B % p.S, (c.name, p)


@pytest.mark.parametrize("name", IDS)
def test_relu_margin_holds(name):
    case = RT.CASE_BY_NAME[name]
    inp = RT.case_inputs(case)
    assert RT.sample_margins(inp.x, inp.layers, case.cfg, inp.qmask, inp.kmask).min() > RT.RELU_MARGIN


@pytest.mark.parametrize("name", IDS)
def test_oracle_matches_torch_double_autograd(name):
    case = RT.CASE_BY_NAME[name]
    inp = RT.case_inputs(case)
    G, T = RT.transformer_bwd(inp.x, inp.layers, case.cfg, inp.qmask, inp.kmask, inp.d_out)
    ref = _torch_grads(case, torch.float64)
    assert set(G) == set(ref) == {"dx"} | {k for k, _, _ in RT.grad_keys(case.cfg)}
    for k in G:
        assert G[k].shape == ref[k].shape, k
        assert (np.abs(G[k] - ref[k]) <= 1e-10 * T[k] + 1e-300).all(), (k, float((np.abs(G[k] - ref[k]) / (T[k] + 1e-300)).max()))
        assert (T[k] >= np.abs(G[k]) * (1 - 1e-12)).all(), k          # the terms bound the result they were summed to


def test_oracle_tells_a_wrong_softmax_backward_apart():
    case = RT.CASE_BY_NAME["bst"]
    inp = RT.case_inputs(case)
    G, T = RT.transformer_bwd(inp.x, inp.layers, case.cfg, inp.qmask, inp.kmask, inp.d_out)
    W, _ = RT.transformer_bwd(inp.x, inp.layers, case.cfg, inp.qmask, inp.kmask, inp.d_out, drop_delta=True)
    with pytest.raises(AssertionError):
        assert_close_terms(W["dx"], G["dx"], T["dx"], what="wrong on purpose")
    TERMS_REPORT.pop()


@pytest.mark.parametrize("name", IDS)
def test_float32_autograd_has_room_under_the_bar(name, capsys):
    case = RT.CASE_BY_NAME[name]
    inp = RT.case_inputs(case)
    G, T = RT.transformer_bwd(inp.x, inp.layers, case.cfg, inp.qmask, inp.kmask, inp.d_out)
    got = _torch_grads(case, torch.float32)
    worst = 0.0
    for k in G:
        assert_close_terms(got[k], G[k], T[k], what="%s %s" % (name, k))
        worst = max(worst, TERMS_REPORT[-1][4])
    with capsys.disabled():
        print("\n  transformer_bwd float32 autograd on the CPU: %-12s worst err / bar %.3f" % (name, worst))


def _train_args(case, B=None, route="case", max_blocks=None):
    from deepctr_amd import ops
    cfg = case.cfg
    return ops._transformer_train_shape(case.B if B is None else B, cfg.T, cfg.E, cfg.H, cfg.L, cfg.pe, cfg.res, cfg.ffn, cfg.ln, cfg.blind,
                                        cfg.out, case.route if route == "case" else route,
                                        case.max_blocks if max_blocks is None else max_blocks)


@pytest.mark.parametrize("name", IDS)
def test_host_arithmetic_matches_the_library(name):
    from deepctr_amd import _C, ops
    case = RT.CASE_BY_NAME[name]
    cfg = case.cfg
    for B in (case.B, 1, 4096):
        for route in (case.route, None, "general"):
            for mb in (case.max_blocks, 0, 3):
                p = RT.plan(cfg, B, route, mb)
                t = _train_args(case, B, route, mb)
                assert _C.lib().dctr_transformer_bwd_supported(ctypes.byref(t)) == 1 and p.supported
                assert _C.lib().dctr_transformer_bwd_workspace_bytes(ctypes.byref(t)) == p.workspace_bytes, (B, route, mb, p)
                assert _C.lib().dctr_transformer_tape_bytes(ctypes.byref(t.fwd)) == p.tape_bytes
    assert ops.transformer_bwd_workspace_bytes(case.B, cfg.T, cfg.E, cfg.H, cfg.L, cfg.pe, cfg.res, cfg.ffn, cfg.ln, cfg.blind, cfg.out,
                                               case.route, case.max_blocks) == RT.plan(cfg, case.B, case.route, case.max_blocks).workspace_bytes
    assert ops.transformer_tape_bytes(case.B, cfg.T, cfg.E, cfg.H, cfg.L) == RT.plan(cfg, case.B).tape_bytes


def test_models_shapes_are_supported_up_to_four_layers():
    """The two models' golden configurations, the defaults of scripts/bench_bst.py / bench_dsin.py and DSIN's default d = 1."""
    from deepctr_amd import ops
    bst = dict(use_positional_encoding=True, use_res=True, use_feed_forward=True, use_layer_norm=True, blinding=False)
    dsin = dict(use_positional_encoding=False, use_res=True, use_feed_forward=True, use_layer_norm=False, blinding=True, output_type="mean")
    for L in (1, 2, 4):
        for T, E, H in ((50, 16, 8), (50, 32, 8), (4, 8, 2), (6, 8, 4), (8, 8, 2)):
            assert ops.transformer_bwd_supported(T, E, H, L, **bst), (T, E, H, L)
        for T, E, H in ((10, 32, 8), (10, 64, 8), (10, 8, 8), (4, 8, 8), (3, 4, 2), (4, 4, 2)):
            assert ops.transformer_bwd_supported(T, E, H, L, **dsin), (T, E, H, L)
            assert ops.transformer_bwd_supported(T, E, H, L, **dict(dsin, use_positional_encoding=True)), (T, E, H, L)
    assert not ops.transformer_bwd_supported(50, 16, 8, 9, **bst)           # more layers than the backward holds
    assert ops.transformer_bwd_supported(50, 16, 8, 8, **bst)
    assert not ops.transformer_bwd_supported(4000, 64, 8, 1, route="fused", **bst)      # a sample past the LDS, fused asked


def test_host_entry_points_refuse_without_a_launch():
    from deepctr_amd import _C
    case = RT.CASE_BY_NAME["bst"]
    lib = _C.lib()
    t = _train_args(case)
    t.fwd.n_layers = 9
    assert lib.dctr_transformer_bwd_supported(ctypes.byref(t)) == 0 and lib.dctr_transformer_bwd_workspace_bytes(ctypes.byref(t)) == 0
    assert lib.dctr_transformer_tape_bytes(ctypes.byref(t.fwd)) == 0
    assert lib.dctr_transformer_bwd(ctypes.byref(t), None) == -5 and lib.dctr_transformer_train_fwd(ctypes.byref(t), None) == -5
    t = _train_args(case)
    t.fwd.keys = 16         # any pointer that is not the queries: separate keys
    assert lib.dctr_transformer_bwd_supported(ctypes.byref(t)) == 0
    assert lib.dctr_transformer_bwd(ctypes.byref(t), None) == -5
    for field, value, code in (("accumulate", 2, -4), ("max_blocks", -1, -4), ("dx_row_stride", 1, None), ("d_out_stride", 1, None)):
        t = _train_args(case)
        if field == "dx_row_stride":
            t.dx = 16
        if field == "d_out_stride":
            t.d_out = 16
        setattr(t, field, value)
        assert lib.dctr_transformer_bwd_supported(ctypes.byref(t)) == 0, field
        assert lib.dctr_transformer_bwd(ctypes.byref(t), None) == (code if code is not None else -2), field
    t = _train_args(case)
    t.fwd.head_num = 3      # d * H != E: the forward's own check
    assert lib.dctr_transformer_bwd(ctypes.byref(t), None) == -2
    t = _train_args(case)   # everything valid but the pointers: DCTR_E_NULL before anything is launched
    assert lib.dctr_transformer_bwd(ctypes.byref(t), None) == -1 and lib.dctr_transformer_train_fwd(ctypes.byref(t), None) == -1


def test_train_args_layout_matches_the_header():
    """The ctypes mirror has the header's fields in the header's order."""
    from deepctr_amd import _C
    text = open(os.path.join(ROOT, "include", "dctr.h")).read()
    body = text[text.index("#define DCTR_TRANSFORMER_BWD_MAX_LAYERS"):text.index("} dctr_transformer_train_args_t;")]
    body = re.sub(r"/\*.*?\*/", "", body[body.index("typedef struct {") + len("typedef struct {"):], flags=re.S)
    names = [re.split(r"[\s\*]+", decl.strip())[-1] for decl in body.split(";") if decl.strip()]
    assert names == [f[0] for f in _C.transformer.TrainArgs._fields_]
    assert _C.transformer.BWD_MAX_LAYERS == int(re.search(r"#define DCTR_TRANSFORMER_BWD_MAX_LAYERS (\d+)", text).group(1)) == RT.MAX_LAYERS
    assert ctypes.sizeof(_C.transformer.TrainArgs) == ctypes.sizeof(_C.transformer.Args) + 12 * 8


def test_training_transformer_takes_the_torch_ops_on_the_cpu(monkeypatch):
    """Without a GPU training.transformer is _transformer layer by layer: the same values, and the HIP function is never built."""
    from deepctr_amd import ops, training
    case = RT.CASE_BY_NAME["bst"]
    inp = RT.case_inputs(case)
    monkeypatch.setattr(ops.TransformerFunction, "apply", None)
    layers = [RT.TorchLayer(W, case.cfg, torch.float64) for W in inp.layers]
    x = torch.tensor(inp.x, dtype=torch.float64, requires_grad=True)
    qm = torch.tensor(inp.qmask)
    y = training.transformer(layers, x, qm, qm, False, lengths=torch.tensor(inp.lengths))
    _, out = RT.forward(inp.x, inp.layers, case.cfg, inp.qmask, inp.kmask)
    assert np.abs(y.detach().numpy() - out).max() <= 1e-10 * np.abs(out).max()
