"""CPU: the float64 oracle of dctr_bilinear_bwd (tests/ref_bilinear_bwd.py) against torch double autograd over training._bilinear and the
SENET lines of FiBiNET's autograd step, the room tests.util.assert_close_terms leaves an fp32 implementation, the planted errors, the
ReLU margins of the cases' inputs, the host-only entry points (no launch), the C layout of the args struct, the operand checks of
ops.senet_bilinear_bwd and the autograd step's dispatcher on the CPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import ref_bilinear_bwd as RB
from tests.util import TERMS_REPORT, assert_close_terms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = {"many_tiles": 64, "walk": 64}           # cases whose double-autograd check runs their first samples only
RUNS = [(c.name, t, m) for c in RB.CASES for m in RB.MODES for t in (RB.TYPES if m != "senet" else ("interaction",))]
RUN_IDS = ["%s-%s-%s" % r for r in RUNS]


class _Layer(object):
    """What training._bilinear reads of a BilinearInteraction."""

    def __init__(self, bilinear_type, matrices):
        self.bilinear_type, self.matrices = bilinear_type, matrices

    def w(self, name):
        assert name == "bilinear_weight"
        return self.matrices[0]


def _torch_forward(x, w1, w2, Ws, Wr, bilinear_type, mode, dense=None):
    """The forward's output row in torch ops: the lines of FiBiNET's autograd step."""
    from deepctr_amd import training
    B = x.shape[0]
    if mode == "layer":
        return training._bilinear(_Layer(bilinear_type, Wr), x).reshape(B, -1)
    a2 = torch.relu(torch.relu(x.mean(-1) @ w1) @ w2)
    v = x * a2.unsqueeze(-1)
    if mode == "senet":
        return v.reshape(B, -1)
    h = torch.cat([training._bilinear(_Layer(bilinear_type, Ws), v), training._bilinear(_Layer(bilinear_type, Wr), x)], dim=-1)
    return torch.cat([h.reshape(B, -1)] + ([] if dense is None else [dense]), dim=-1)


def _torch_grads(case, bilinear_type, mode, dtype, dense_cols=0, r=None, rows=None):
    x, d_out, w1, w2, Ws, Wr = RB.run_operands(case, bilinear_type, mode, dense_cols, r, rows)
    leaf = lambda a: None if a is None else torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True)    # noqa: E731
    xt, w1t, w2t = leaf(x), leaf(w1), leaf(w2)
    Wst, Wrt = (None if W is None else [leaf(m) for m in W] for W in (Ws, Wr))
    dense = torch.zeros(x.shape[0], dense_cols, dtype=dtype, requires_grad=True) if dense_cols else None
    out = _torch_forward(xt, w1t, w2t, Wst, Wrt, bilinear_type, mode, dense)
    (out * torch.tensor(np.asarray(d_out), dtype=dtype)).sum().backward()
    G = {"dx": xt.grad.numpy()}
    if mode != "layer":
        G["dw1"], G["dw2"] = w1t.grad.numpy(), w2t.grad.numpy()
    if mode == "model":
        G["dws"] = torch.stack([m.grad for m in Wst]).numpy()
    if mode != "senet":
        G["dwr"] = torch.stack([m.grad for m in Wrt]).numpy()
    if dense_cols:
        G["d_dense"] = dense.grad.numpy()
    return G


@pytest.mark.parametrize("name,bilinear_type,mode", RUNS, ids=RUN_IDS)
def test_oracle_matches_torch_double_autograd(name, bilinear_type, mode):
    case = RB.CASE_BY_NAME[name]
    rows = ROWS.get(name)
    assert rows is not None or case.shape[2] <= 100
    dense = RB.DENSE if mode == "model" and name in ("ragged", "criteo") else 0
    G, T = RB.oracle(case, bilinear_type, mode, dense, rows=rows)
    ref = _torch_grads(case, bilinear_type, mode, torch.float64, dense, rows=rows)
    assert sorted(G) == sorted(ref) == sorted(T)
    for k in G:
        assert G[k].shape == ref[k].shape, k
        scale = np.abs(ref[k]).max()
        assert np.abs(G[k] - ref[k]).max() <= 1e-10 * scale, (k, float(np.abs(G[k] - ref[k]).max() / scale))
        assert (T[k] >= np.abs(G[k]) * (1 - 1e-12)).all(), k          # the terms bound the result they were summed to


def test_oracle_with_a_reduction_wider_than_the_fields():
    case = RB.CASE_BY_NAME["ragged"]
    G, _ = RB.oracle(case, "interaction", "model", r=5)
    ref = _torch_grads(case, "interaction", "model", torch.float64, r=5)
    assert G["dw1"].shape == (3, 5) and G["dw2"].shape == (5, 3)
    for k in G:
        assert np.abs(G[k] - ref[k]).max() <= 1e-10 * np.abs(ref[k]).max(), k


@pytest.mark.parametrize("name", [c.name for c in RB.CASES])
def test_relu_gates_keep_their_margin(name):
    """A float32 kernel and the float64 oracle must agree on every gate: each SENET pre-activation stays GATE_MARGIN of its summed
    magnitude away from zero; apart from ``smallest`` both layers have active and inactive units."""
    case = RB.CASE_BY_NAME[name]
    for r in (None, 5) if name == "ragged" else (None,):
        inp = RB.case_inputs(case, r)
        P1, M1, P2, M2 = RB.preactivations(inp.x, inp.w1, inp.w2)
        assert (np.abs(P1) >= RB.GATE_MARGIN * M1).all() and (np.abs(P2) >= RB.GATE_MARGIN * M2).all()
        assert (M1 > 0).all()
        if name != "smallest":
            for P in (P1, P2):
                assert (P > 0).any() and (P < 0).any()


@pytest.mark.parametrize("name", [c.name for c in RB.CASES])
def test_float32_autograd_sits_inside_the_bar(name, capsys):
    """torch's float32 autograd on the CPU against the oracle under assert_close_terms' defaults: the room the bar leaves an fp32
    implementation with another summation order.  Prints the worst err / bar per case (largest over types, modes and outputs)."""
    case = RB.CASE_BY_NAME[name]
    worst = {}
    for _, bilinear_type, mode in [r for r in RUNS if r[0] == name]:
        G, T = RB.oracle(case, bilinear_type, mode)
        got = _torch_grads(case, bilinear_type, mode, torch.float32)
        for k in sorted(G):
            n0 = len(TERMS_REPORT)
            assert_close_terms(got[k], G[k], T[k], what="%s %s %s %s (float32 autograd)" % (name, bilinear_type, mode, k))
            worst["%s/%s/%s" % (bilinear_type, mode, k)] = TERMS_REPORT[n0][4]
    with capsys.disabled():
        top = max(worst, key=worst.get)
        print("\n[bilinear_bwd float32 autograd] %s: worst err / bar %.3g (%s)" % (name, worst[top], top))


@pytest.mark.parametrize("wrong", RB.WRONG)
@pytest.mark.parametrize("name", [c.name for c in RB.CASES if c.shape[0] >= 3])
def test_a_wrong_backward_is_told_apart(name, wrong):
    """The dA2 path dropped; the dx_j half of every pair dropped: each misses the fp32 bar on every case with F >= 3 — the comparison
    has teeth."""
    case = RB.CASE_BY_NAME[name]
    rows = ROWS.get(name)
    x, d_out, w1, w2, Ws, Wr = RB.run_operands(case, "interaction", "model", rows=rows)
    G, T = RB.oracle(case, "interaction", "model", rows=rows)
    W, _ = RB.bilinear_bwd(x, d_out, w1, w2, Ws, Wr, "interaction", "model", wrong=wrong)
    missed = []
    for k in G:
        try:
            assert_close_terms(W[k], G[k], T[k], what="wrong " + k)
        except AssertionError:
            missed.append(k)
    assert "dx" in missed and (wrong != "da2" or ("dw1" in missed and "dw2" in missed)), missed


def test_case_table_is_the_one_agreed():
    assert [(c.name, c.shape, c.max_blocks) for c in RB.CASES] == [
        ("smallest", (2, 1, 5), 0), ("ragged", (3, 4, 33), 0), ("e17", (13, 17, 40), 0), ("criteo", (26, 16, 70), 0),
        ("e32", (7, 32, 21), 0), ("f60", (60, 16, 6), 0), ("many_tiles", (6, 12, 8200), 0), ("general", (200, 4, 5), 0),
        ("walk", (26, 16, 1001), 2)]
    assert RB.reduction_size(26) == 8 and RB.reduction_size(2) == 1


# ---------------------------------------------------------------------------------------------------
# host-only entry points
# ---------------------------------------------------------------------------------------------------
def test_supported_and_workspace_for_the_table():
    from deepctr_amd import ops
    for c in RB.CASES:
        F, E, B = c.shape
        for bilinear_type in RB.TYPES:
            assert ops.senet_bilinear_bwd_supported(F, E, bilinear_type, "model", RB.reduction_size(F)), c.name
            need = ops.senet_bilinear_bwd_workspace_bytes(B, F, E, bilinear_type, "model", RB.reduction_size(F))
            assert (need > 0) == (c.route == "workspace"), (c.name, bilinear_type, need)
            assert need % 16 == 0


def _bwd_args(**kw):
    from deepctr_amd import _C
    # F 3, E 4, P 3: model width 24
    fwd = dict(x=16, batch=4, x_stride=12, fields=3, dim=4, bilinear_type=2, mode=0, reduction_size=1, dense_cols=0, senet_w1=16,
               senet_w2=16, senet_bilinear_w=16, bilinear_w=16)
    top = dict(d_out=16, d_out_stride=24, dx=16, dx_stride=12, d_senet_w1=16, d_senet_w2=16, d_senet_bilinear_w=16, d_bilinear_w=16)
    for k, v in kw.items():
        (fwd if k in fwd else top)[k] = v
    b = _C.bilinear.BwdArgs(**top)
    b.fwd = _C.bilinear.Args(**fwd)
    return b


def test_argument_errors_without_a_gpu():
    """Every refusal precedes the launch: these calls carry made-up pointers and run where no GPU exists."""
    from deepctr_amd import _C
    lib = _C.lib()
    f = lambda b: lib.dctr_bilinear_bwd(ctypes.byref(b), None)   # noqa: E731
    assert lib.dctr_bilinear_bwd(None, None) == -1 and lib.dctr_bilinear_bwd_supported(None) == 0
    assert lib.dctr_bilinear_bwd_workspace_bytes(None) == 0
    assert f(_bwd_args(batch=0)) == 0                                # an empty batch: a no-op
    none = dict(dx=None, d_senet_w1=None, d_senet_w2=None, d_senet_bilinear_w=None, d_bilinear_w=None)
    assert f(_bwd_args(**none)) == -1                                # all five gradient outputs NULL
    assert b"bilinear_bwd" in lib.dctr_last_error()
    assert f(_bwd_args(batch=0, **dict(none, d_senet_w2=16))) == 0   # one is enough
    assert f(_bwd_args(mode=2, **dict(none, d_senet_w1=16))) == -1   # ... if the mode has it
    assert f(_bwd_args(x=None)) == -1 and f(_bwd_args(d_out=None)) == -1 and f(_bwd_args(senet_w1=None)) == -1
    assert f(_bwd_args(bilinear_w=None)) == -1 and f(_bwd_args(senet_bilinear_w=None)) == -1
    assert f(_bwd_args(bilinear_type=3)) == -4 and f(_bwd_args(mode=3)) == -4 and f(_bwd_args(accumulate=2)) == -4
    assert f(_bwd_args(fields=1)) == -2 and f(_bwd_args(batch=-1)) == -2 and f(_bwd_args(max_blocks=-1)) == -2
    assert f(_bwd_args(x_stride=11)) == -2 and f(_bwd_args(dx_stride=11)) == -2 and f(_bwd_args(dx_offset=1)) == -2
    assert f(_bwd_args(d_out_stride=23)) == -2 and f(_bwd_args(d_out_offset=1)) == -2
    assert f(_bwd_args(dense_cols=2)) == -2                          # x, d_out and dx rows all two short
    assert f(_bwd_args(dense_cols=2, x_stride=14, d_out_stride=26, dx_stride=14, batch=0)) == 0
    assert f(_bwd_args(mode=1, dense_cols=2, x_stride=14, d_out_stride=26, dx_stride=14)) == -2     # dense columns: mode MODEL only
    assert f(_bwd_args(reduction_size=0)) == -2 and f(_bwd_args(mode=2, reduction_size=0, batch=0)) == 0
    # a tile past the LDS: the workspace is required, large enough and 16-byte aligned
    big = dict(fields=200, dim=4, x_stride=800, dx_stride=800, d_out_stride=2 * 19900 * 4, reduction_size=66)
    need = lib.dctr_bilinear_bwd_workspace_bytes(ctypes.byref(_bwd_args(**big)))
    assert need > 0
    assert f(_bwd_args(**big)) == -1 and b"workspace" in lib.dctr_last_error()
    assert f(_bwd_args(workspace=4096, workspace_bytes=need - 4, **big)) == -1
    assert f(_bwd_args(workspace=4096 + 4, workspace_bytes=need, **big)) == -3
    assert f(_bwd_args(workspace=4096, workspace_bytes=need, batch=0, **big)) == 0


def test_header_declares_the_entry_points_and_the_mirror_matches_the_c_layout(tmp_path):
    import shutil
    from deepctr_amd import _C
    header = open(os.path.join(ROOT, "include", "dctr.h")).read()
    assert "#define DCTR_ABI_VERSION 13" in header and _C.ABI_VERSION == 13
    for sym, ret in (("dctr_bilinear_bwd", "int"), ("dctr_bilinear_bwd_supported", "int"),
                     ("dctr_bilinear_bwd_workspace_bytes", "size_t")):
        assert re.search(r"\b%s %s\(const dctr_bilinear_bwd_args_t\* args" % (ret, sym), header), sym
        assert _C.SYMBOLS[sym][1][0] == ctypes.POINTER(_C.bilinear.BwdArgs)
    assert "bilinear_bwd_kernels.hip" in __import__("deepctr_amd.build", fromlist=["SOURCES"]).SOURCES
    assert "bilinear_bwd_kernels.hip" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    gcc = shutil.which("gcc")
    assert gcc is not None
    fields = [n for n, _ in _C.bilinear.BwdArgs._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "dctr.h"', 'int main(void) {',
           '  printf("%zu\\n", sizeof(dctr_bilinear_bwd_args_t));']
    src += ['  printf("%%zu\\n", offsetof(dctr_bilinear_bwd_args_t, %s));' % n for n in fields]
    src += ['  return 0;', '}']
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = str(tmp_path / "layout")
    subprocess.check_call([gcc, "-I", os.path.join(ROOT, "include"), str(c), "-o", exe])
    out = [int(v) for v in subprocess.check_output([exe]).split()]
    assert out[0] == ctypes.sizeof(_C.bilinear.BwdArgs)
    assert out[1:] == [getattr(_C.bilinear.BwdArgs, n).offset for n in fields]


# ---------------------------------------------------------------------------------------------------
# ops.senet_bilinear_bwd: the operand checks, driven with CPU tensors (they precede the device check and the launch)
# ---------------------------------------------------------------------------------------------------
def _operands(F=3, E=4, B=5, r=1):
    P = F * (F - 1) // 2
    z = torch.zeros
    return dict(x=z(B, F, E), d_out=z(B, 2 * P * E), senet_w=(z(F, r), z(r, F)), senet_bilinear_w=[z(E, E) for _ in range(P)],
                bilinear_w=[z(E, E) for _ in range(P)], dx=z(B, F * E), d_senet_w=(z(F, r), z(r, F)), d_senet_bilinear_w=z(P, E, E),
                d_bilinear_w=z(P, E, E))


@pytest.mark.parametrize("bad", ["count", "shape", "w1", "forms", "d_out", "dx_stride", "dx_width", "none", "device", "d_w", "fields"])
def test_senet_bilinear_bwd_refuses_bad_operands(bad):
    from deepctr_amd import ops
    kw = _operands()
    x = kw.pop("x")
    if bad == "count":
        kw["bilinear_w"] = kw["bilinear_w"][:-1]
    elif bad == "shape":
        kw["senet_bilinear_w"][1] = torch.zeros(4, 5)
    elif bad == "w1":
        kw["senet_w"] = (torch.zeros(3, 2), torch.zeros(1, 3))
    elif bad == "forms":
        kw["senet_bilinear_w"] = None
    elif bad == "d_out":
        kw["d_out"] = torch.zeros(5, 23)                              # a short row
    elif bad == "dx_stride":
        kw["dx"] = torch.zeros(5, 24)[:, ::2]                         # a non-unit column stride
    elif bad == "dx_width":
        kw["dx"] = torch.zeros(5, 11)
    elif bad == "none":
        kw.update(dx=None, d_senet_w=None, d_senet_bilinear_w=None, d_bilinear_w=None)
    elif bad == "device":
        kw["d_out"] = torch.zeros(5, 24, device="meta")
    elif bad == "d_w":
        kw["d_bilinear_w"] = torch.zeros(3, 4, 4)[:, :, ::2]
    elif bad == "fields":
        x = torch.zeros(5, 1, 4)
    with pytest.raises(ValueError, match="senet_bilinear_bwd"):
        ops.senet_bilinear_bwd(x, **kw)


# ---------------------------------------------------------------------------------------------------
# the dispatcher on the CPU: torch ops, unchanged
# ---------------------------------------------------------------------------------------------------
def test_dispatcher_takes_the_torch_ops_on_the_cpu():
    from deepctr_amd import training
    case = RB.CASE_BY_NAME["ragged"]
    F, E, B = case.shape
    x, d_out, w1, w2, Ws, Wr = RB.run_operands(case, "interaction", "model", RB.DENSE)
    leaf = lambda a: torch.tensor(np.asarray(a), requires_grad=True)    # noqa: E731
    w1t, w2t = leaf(w1), leaf(w2)

    class _Senet(object):
        weights_w12 = (w1t, w2t)

    class _Model(object):
        n_fields, emb_dim, bilinear_type = F, E, "interaction"
        senet = _Senet
        senet_bilinear = _Layer("interaction", [leaf(m) for m in Ws])
        bilinear = _Layer("interaction", [leaf(m) for m in Wr])
    xt = leaf(x)
    dense = torch.rand(B, RB.DENSE)
    got = training.senet_bilinear(_Model, torch.cat([xt.reshape(B, -1), dense], dim=-1))
    want = _torch_forward(xt, w1t, w2t, _Model.senet_bilinear.matrices, _Model.bilinear.matrices, "interaction", "model", dense)
    assert torch.equal(got, want) and got.requires_grad and got.shape == (B, F * (F - 1) * E + RB.DENSE)
