"""CPU: the float64 oracle of dctr_interacting_bwd (tests/ref_interacting_bwd.py) against torch double autograd over
training._interacting, the room tests.util.assert_close_terms leaves an fp32 implementation, the ReLU margin of every case, the host-only
entry points (no launch), the C layout of the args struct, and the autograd step's interacting_stack on the CPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import ref_interacting_bwd as RB
from tests.util import TERMS_REPORT, assert_close_terms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [c.name for c in RB.CASES]


def _torch_grads(case, dtype):
    """(grads by the oracle's keys) from torch autograd over training._interacting on the CPU."""
    from deepctr_amd import training
    F, E, d, H, L, use_res, scaling, B = case.shape
    x, weights, dy = RB.case_inputs(case)
    xt = torch.tensor(x, dtype=dtype, requires_grad=True)
    wt = [[torch.tensor(w, dtype=dtype, requires_grad=True) for w in layer] for layer in weights]
    h = xt
    for layer in wt:
        h = training._interacting(RB.Layer(layer, d, H, use_res, scaling), h)
    h.reshape(B, -1).backward(torch.tensor(dy, dtype=dtype))
    out = {"dx": xt.grad.numpy()}
    for l, layer in enumerate(wt):
        for name, w in zip(("query", "key", "value", "res"), layer):
            out["d%s%d" % (name, l)] = w.grad.numpy()
    return out


def _oracle(case, **kw):
    F, E, d, H, L, use_res, scaling, B = case.shape
    x, weights, dy = RB.case_inputs(case)
    return RB.interacting_bwd(x, weights, d, H, use_res, scaling, dy, **kw)


@pytest.mark.parametrize("name", IDS)
def test_oracle_matches_torch_double_autograd(name):
    case = RB.CASE_BY_NAME[name]
    G, T = _oracle(case)
    ref = _torch_grads(case, torch.float64)
    assert sorted(G) == sorted(ref) and sorted(T) == sorted(G)
    for k in G:
        assert G[k].shape == ref[k].shape, k
        scale = np.abs(ref[k]).max()
        assert np.abs(G[k] - ref[k]).max() <= 1e-10 * scale, (k, float(np.abs(G[k] - ref[k]).max() / scale))
        assert (T[k] >= np.abs(G[k]) * (1 - 1e-12)).all(), k          # the terms bound the result they were summed to


def test_a_wrong_backward_is_told_apart():
    """The softmax backward without its row term misses the bar by orders of magnitude: the comparison has teeth."""
    case = RB.CASE_BY_NAME["three_layers"]
    G, T = _oracle(case)
    W, _ = _oracle(case, drop_delta=True)
    with pytest.raises(AssertionError):
        assert_close_terms(W["dx"], G["dx"], T["dx"], what="wrong dx")


@pytest.mark.parametrize("name", IDS)
def test_float32_autograd_sits_inside_the_bar(name, capsys):
    """torch's float32 autograd on the CPU against the oracle under assert_close_terms' defaults: the room the bar leaves an fp32
    implementation with another summation order.  Worst err / bar per case (largest over the outputs), measured here:
    one_field 0.003, d1_h1 0 (d = H = 1: every sum has one or two terms), three_layers 0.11, d17 0.16, criteo 0.68, criteo_walk 0.97,
    no_res 0.16, past_lds 0.036.  The two large ones are the last layer's d res (1,820 and 7,800 rows summed in sequence by the CPU's
    GEMM; every dx stays below 0.03): a sum over the batch in one fp32 chain has little room left at a few thousand rows, a kernel
    that sums per tile and then across tiles has more."""
    case = RB.CASE_BY_NAME[name]
    G, T = _oracle(case)
    got = _torch_grads(case, torch.float32)
    worst = {}
    for k in sorted(G):
        n0 = len(TERMS_REPORT)
        assert_close_terms(got[k], G[k], T[k], what="%s %s (float32 autograd)" % (name, k))
        worst[k] = TERMS_REPORT[n0][4]
    with capsys.disabled():
        print("\n[interacting_bwd float32 autograd] %s: worst err / bar %.3g (%s)"
              % (name, max(worst.values()), ", ".join("%s %.2g" % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize("name", IDS)
def test_relu_margin_of_every_case(name):
    """No pre-activation of any layer lies within 1e-5 of its summed magnitude of zero: the fp32 kernel and the oracle take the same
    ReLU branch at every element, so no element is excluded from any comparison."""
    case = RB.CASE_BY_NAME[name]
    F, E, d, H, L, use_res, scaling, B = case.shape
    x, weights, _ = RB.case_inputs(case)
    assert RB.relu_margin(x, weights, d, H, use_res, scaling) > RB.RELU_MARGIN


def test_case_table_is_the_one_agreed():
    assert [(c.shape, c.max_blocks) for c in RB.CASES] == [
        ((1, 3, 8, 2, 1, True, False, 5), 0), ((2, 4, 1, 1, 2, False, True, 33), 0), ((4, 3, 8, 2, 3, True, True, 5), 0),
        ((5, 6, 17, 3, 2, True, False, 40), 0), ((26, 16, 8, 2, 3, True, False, 70), 0), ((26, 16, 8, 2, 3, True, False, 300), 3),
        ((39, 32, 16, 4, 2, False, False, 19), 0), ((200, 32, 16, 4, 1, True, False, 6), 0)]


# ---------------------------------------------------------------------------------------------------
# host-only entry points
# ---------------------------------------------------------------------------------------------------
def test_supported_and_workspace_for_the_table():
    from deepctr_amd import ops
    for c in RB.CASES:
        F, E, d, H, L, use_res, scaling, B = c.shape
        pl = RB.plan(F, E, d, H, L, use_res)
        assert pl.supported and pl.route == c.route, c.name
        assert ops.interacting_bwd_supported(F, E, L, d, H, use_res), c.name
        assert ops.interacting_bwd_workspace_bytes(B, F, E, L, d, H, use_res) == pl.workspace_bytes, c.name
        assert (pl.workspace_bytes > 0) == (c.route == "workspace")
    # ragged tiles and several tiles per workgroup in the table: the Criteo shape packs 3 samples into a tile
    assert RB.plan(26, 16, 8, 2, 3, True).S == 3 and 70 % 3 and 300 // 3 > 3
    assert RB.plan(2, 4, 1, 1, 2, False).S == 16
    # more than 32 layers are declined, 32 are not
    assert ops.interacting_bwd_supported(3, 4, 32, 2, 2, True) and not ops.interacting_bwd_supported(3, 4, 33, 2, 2, True)
    assert not RB.plan(3, 4, 2, 2, 33, True).supported
    assert ops.interacting_bwd_workspace_bytes(8, 3, 4, 33, 2, 2, True) == 0


def _bwd_args(**kw):
    from deepctr_amd import _C
    fwd = dict(x=16, batch=4, x_stride=12, fields=3, dim=4, n_layers=1, att_embedding_size=2, head_num=2, use_res=1, scaling=0)
    top = dict(dy=16, dy_stride=12, dx=16, dx_stride=12)
    for k, v in kw.items():
        (fwd if k in fwd or k in ("workspace", "workspace_bytes", "layers") else top)[k] = v
    layers = (ctypes.c_void_p * 4)(16, 16, 16, 16)
    b = _C.interacting.BwdArgs(**top)
    fwd.setdefault("layers", ctypes.cast(layers, ctypes.c_void_p))
    b.fwd = _C.interacting.Args(**fwd)
    b._keep = layers
    return b


def test_argument_errors_without_a_gpu():
    """Every refusal precedes the launch: these calls carry made-up pointers and run where no GPU exists."""
    from deepctr_amd import _C
    lib = _C.lib()
    f = lambda b: lib.dctr_interacting_bwd(ctypes.byref(b), None)   # noqa: E731
    assert lib.dctr_interacting_bwd(None, None) == -1 and lib.dctr_interacting_bwd_supported(None) == 0
    assert lib.dctr_interacting_bwd_workspace_bytes(None) == 0
    assert f(_bwd_args(batch=0)) == 0                                # an empty batch: a no-op
    assert f(_bwd_args(dy=None)) == -1
    assert b"interacting_bwd" in lib.dctr_last_error()
    assert f(_bwd_args(x=None)) == -1 and f(_bwd_args(layers=None)) == -1
    assert f(_bwd_args(dx_stride=11)) == -2                          # dx_stride < F * dim
    assert f(_bwd_args(dx=None, dx_stride=0, batch=0)) == 0          # ... which is read with dx only
    assert f(_bwd_args(dy_stride=11)) == -2 and f(_bwd_args(x_stride=11)) == -2
    assert f(_bwd_args(fields=0)) == -2 and f(_bwd_args(batch=-1)) == -2 and f(_bwd_args(max_blocks=-1)) == -2
    assert f(_bwd_args(use_res=2)) == -4 and f(_bwd_args(scaling=-1)) == -4 and f(_bwd_args(accumulate=2)) == -4
    assert f(_bwd_args(n_layers=33)) == _C.E_UNSUPPORTED
    # a sample past the LDS: the workspace is required, large enough and 16-byte aligned
    big = dict(fields=200, dim=32, att_embedding_size=16, head_num=4, x_stride=6400, dy_stride=12800, dx_stride=6400)
    need = RB.plan(200, 32, 16, 4, 1, True).workspace_bytes
    assert lib.dctr_interacting_bwd_workspace_bytes(ctypes.byref(_bwd_args(**big))) == need > 0
    assert f(_bwd_args(**big)) == -1
    assert f(_bwd_args(workspace=4096, workspace_bytes=need - 4, **big)) == -1
    assert f(_bwd_args(workspace=4096 + 4, workspace_bytes=need, **big)) == -3
    assert f(_bwd_args(workspace=4096, workspace_bytes=need, batch=0, **big)) == 0


def test_header_declares_the_entry_points_and_the_mirror_matches_the_c_layout(tmp_path):
    import shutil
    import subprocess
    from deepctr_amd import _C
    header = open(os.path.join(ROOT, "include", "dctr.h")).read()
    assert "#define DCTR_ABI_VERSION 13" in header and _C.ABI_VERSION == 13
    for sym, ret in (("dctr_interacting_bwd", "int"), ("dctr_interacting_bwd_supported", "int"),
                     ("dctr_interacting_bwd_workspace_bytes", "size_t")):
        assert re.search(r"\b%s %s\(const dctr_interacting_bwd_args_t\* args" % (ret, sym), header), sym
        assert _C.SYMBOLS[sym][1][0] == ctypes.POINTER(_C.interacting.BwdArgs)
    assert "interacting_bwd_kernels.hip" in __import__("deepctr_amd.build", fromlist=["SOURCES"]).SOURCES
    assert "interacting_bwd_kernels.hip" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    structs = (("dctr_interacting_args_t", _C.interacting.Args), ("dctr_interacting_bwd_args_t", _C.interacting.BwdArgs))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dctr.h"', "int main(void) {", '    printf("abi %d\\n", DCTR_ABI_VERSION);']
    for cname, cls in structs:
        lines.append('    printf("%s.sizeof %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in cls._fields_:
            lines.append('    printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines += ["    return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    by_name = dict(structs)
    seen = 0
    for line in filter(None, out):
        field, val = line.split()
        if field == "abi":
            assert int(val) == 13
            continue
        cname, fname = field.split(".")
        cls = by_name[cname]
        want = ctypes.sizeof(cls) if fname == "sizeof" else getattr(cls, fname).offset
        assert int(val) == want, "%s: C says %s, ctypes %d" % (field, val, want)
        seen += 1
    assert seen == sum(1 + len(cls._fields_) for _, cls in structs)


# ---------------------------------------------------------------------------------------------------
# the autograd step on the CPU: nothing changes
# ---------------------------------------------------------------------------------------------------
def test_interacting_stack_on_the_cpu_is_the_torch_loop(monkeypatch):
    from deepctr_amd import training
    case = RB.CASE_BY_NAME["three_layers"]
    F, E, d, H, L, use_res, scaling, B = case.shape
    x, weights, _ = RB.case_inputs(case)
    layers = [RB.Layer([torch.tensor(w, requires_grad=True) for w in layer], d, H, use_res, scaling) for layer in weights]
    xt = torch.tensor(x, requires_grad=True)
    want = xt
    for layer in layers:
        want = training._interacting(layer, want)
    assert training.HIP_AUTOGRAD_OPS is True
    for switch in (True, False):
        monkeypatch.setattr(training, "HIP_AUTOGRAD_OPS", switch)
        got = training.interacting_stack(layers, xt)
        assert torch.equal(got, want) and got.grad_fn is not None
        with torch.no_grad():
            assert torch.equal(training.interacting_stack(layers, xt), want)
    assert torch.equal(training.interacting_stack([], xt), xt)


def test_cpu_autoint_still_trains():
    """fit() itself asks for a HIP device before anything else, so a CPU-built model is trained here by the step fit() takes for
    AutoInt: model_logits(training=True), the loss, backward, KerasAdam.  With the switch on it takes the torch loop and its loss falls."""
    from deepctr_amd import engine, models, training, training_hip
    from deepctr_amd.feature_column import DenseFeat, SparseFeat
    rng = np.random.RandomState(5)
    n = 256
    cols = [SparseFeat("c%d" % i, 11 + i, embedding_dim=8) for i in range(4)] + [DenseFeat("v", 1)]
    feed = {"c%d" % i: rng.randint(0, 11 + i, n).astype(np.int32) for i in range(4)}
    feed["v"] = rng.rand(n).astype(np.float32)
    y = torch.from_numpy(((feed["c0"] % 2) ^ (feed["c1"] % 2)).astype(np.float32))
    model = models.AutoInt(cols, cols, att_layer_num=2, dnn_hidden_units=(16,), seed=3, device="cpu")
    assert not training_hip.supported(model) and training.HIP_AUTOGRAD_OPS
    params = [t for layer in model.att_layers for t in layer.weights_qkvr] + [model.dense.w("kernel")] + list(model.dnn.kernels)
    for t in params:
        t.requires_grad_(True)
    opt = training.KerasAdam(params, lr=1e-2)
    staged = engine.Staged(n)
    model._stage_inputs(feed, staged)
    model._begin()
    losses = []
    for _ in range(12):
        opt.zero_grad()
        loss = torch.nn.functional.binary_cross_entropy_with_logits(training.model_logits(model, staged, 0, n, training=True), y)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    for t in params:
        t.requires_grad_(False)
    assert all(t.grad is not None and float(t.grad.abs().max()) > 0 for t in params)
    assert losses[-1] < losses[0]
