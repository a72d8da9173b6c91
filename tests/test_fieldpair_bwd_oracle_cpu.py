"""CPU: the float64 oracle of dctr_fieldpair_bwd (tests/ref_fieldpair_bwd.py) against torch double autograd over training._fefm and the
FwFM einsum, the room tests.util.assert_close_terms leaves an fp32 implementation, the host-only entry points (no launch), the C layout
of the args struct, and the autograd step's dispatchers on the CPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import ref_fieldpair_bwd as RF
from tests.util import TERMS_REPORT, assert_close_terms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS = [(c.name, kind, combo) for c in RF.CASES for kind in RF.KINDS for combo in RF.COMBOS[kind]]
RUN_IDS = ["%s-%s-%s" % r for r in RUNS]


class _Fefm(object):
    """What training._fefm reads of an FEFMLayer."""

    def __init__(self, matrices):
        self.matrices = matrices


def _torch_grads(case, kind, combo, dtype):
    """{dx, dw} from torch autograd on the CPU: training._fefm (pairs and their row sum), or the einsum of the FwFM autograd step."""
    from deepctr_amd import training
    x, weights, d_pairs, d_logit = RF.case_inputs(case, kind)
    dp, dl = RF.combo_grads(combo, d_pairs, d_logit)
    xt = torch.tensor(x, dtype=dtype, requires_grad=True)
    if kind == "fefm":
        wt = [torch.tensor(w, dtype=dtype, requires_grad=True) for w in weights]
        pairs = training._fefm(_Fefm(wt), xt)
        # (the two upstream gradients are converted before they meet: the op adds them in the oracle's order)
        loss = 0
        if dp is not None:
            loss = loss + (pairs * torch.tensor(dp, dtype=dtype)).sum()
        if dl is not None:
            loss = loss + (pairs.sum(-1) * torch.tensor(dl, dtype=dtype)).sum()
        loss.backward()
        return {"dx": xt.grad.numpy(), "dw": torch.stack([w.grad for w in wt]).numpy()}
    r = torch.tensor(weights, dtype=dtype, requires_grad=True)
    gram = torch.einsum("bie,bje->bij", xt, xt)
    logit = (gram * torch.triu(r, diagonal=1)).sum((1, 2))
    (logit * torch.tensor(dl, dtype=dtype)).sum().backward()
    return {"dx": xt.grad.numpy(), "dw": r.grad.numpy()}


@pytest.mark.parametrize("name,kind,combo", RUNS, ids=RUN_IDS)
def test_oracle_matches_torch_double_autograd(name, kind, combo):
    case = RF.CASE_BY_NAME[name]
    G, T = RF.oracle(case, kind, combo)
    ref = _torch_grads(case, kind, combo, torch.float64)
    assert sorted(G) == sorted(ref) == sorted(T)
    for k in G:
        assert G[k].shape == ref[k].shape, k
        scale = np.abs(ref[k]).max()
        assert np.abs(G[k] - ref[k]).max() <= 1e-10 * scale, (k, float(np.abs(G[k] - ref[k]).max() / scale))
        assert (T[k] >= np.abs(G[k]) * (1 - 1e-12)).all(), k          # the terms bound the result they were summed to
    if kind == "fwfm":
        assert (G["dw"][np.tril_indices(case.shape[0])] == 0).all()


@pytest.mark.parametrize("kind", RF.KINDS)
def test_a_wrong_backward_is_told_apart(kind):
    """dW without its A^T half (FEFM), r' without its mirrored half (FwFM): both miss the double-autograd check and the fp32 bar by
    orders of magnitude — the comparison has teeth."""
    case = RF.CASE_BY_NAME["ragged"]
    combo = RF.COMBOS[kind][-1]
    x, weights, d_pairs, d_logit = RF.case_inputs(case, kind)
    G, T = RF.oracle(case, kind, combo)
    W, _ = RF.fieldpair_bwd(x, weights, kind, *RF.combo_grads(combo, d_pairs, d_logit), wrong=True)
    ref = _torch_grads(case, kind, combo, torch.float64)
    key = "dw" if kind == "fefm" else "dx"
    assert np.abs(W[key] - ref[key]).max() > 1e-3 * np.abs(ref[key]).max()
    with pytest.raises(AssertionError):
        assert_close_terms(W[key], G[key], T[key], what="wrong " + key)


@pytest.mark.parametrize("name", [c.name for c in RF.CASES])
def test_float32_autograd_sits_inside_the_bar(name, capsys):
    """torch's float32 autograd on the CPU against the oracle under assert_close_terms' defaults: the room the bar leaves an fp32
    implementation with another summation order.  Prints the worst err / bar per case (largest over kinds, combinations and outputs)."""
    case = RF.CASE_BY_NAME[name]
    worst = {}
    for kind in RF.KINDS:
        for combo in RF.COMBOS[kind]:
            G, T = RF.oracle(case, kind, combo)
            got = _torch_grads(case, kind, combo, torch.float32)
            for k in sorted(G):
                n0 = len(TERMS_REPORT)
                assert_close_terms(got[k], G[k], T[k], what="%s %s %s %s (float32 autograd)" % (name, kind, combo, k))
                worst["%s/%s/%s" % (kind, combo, k)] = TERMS_REPORT[n0][4]
    with capsys.disabled():
        top = max(worst, key=worst.get)
        print("\n[fieldpair_bwd float32 autograd] %s: worst err / bar %.3g (%s)" % (name, worst[top], top))


def test_case_table_is_the_one_agreed():
    assert [(c.shape, c.max_blocks) for c in RF.CASES] == [
        ((2, 1, 5), 0), ((3, 4, 33), 0), ((13, 17, 40), 0), ((26, 16, 70), 0), ((7, 32, 21), 0), ((60, 16, 6), 0), ((6, 12, 8200), 0),
        ((200, 16, 5), 0), ((26, 16, 1001), 2)]


# ---------------------------------------------------------------------------------------------------
# host-only entry points
# ---------------------------------------------------------------------------------------------------
def test_supported_and_workspace_for_the_table():
    from deepctr_amd import ops
    for c in RF.CASES:
        F, E, B = c.shape
        for kind in RF.KINDS:
            assert ops.fieldpair_bwd_supported(F, E, kind), (c.name, kind)
            need = ops.fieldpair_bwd_workspace_bytes(B, F, E, kind)
            assert (need > 0) == (c.route == "workspace"), (c.name, kind, need)
            assert need % 16 == 0


def _bwd_args(**kw):
    from deepctr_amd import _C
    fwd = dict(x=16, batch=4, x_stride=12, x_offset=0, fields=3, dim=4, kind=0, weights=16)
    top = dict(d_pairs=16, d_pairs_stride=3, d_logit=16, dx=16, dx_stride=12, d_weights=16)
    for k, v in kw.items():
        (fwd if k in fwd or k in ("workspace", "workspace_bytes") else top)[k] = v
    b = _C.fieldpair.BwdArgs(**top)
    b.fwd = _C.fieldpair.Args(**fwd)
    return b


def test_argument_errors_without_a_gpu():
    """Every refusal precedes the launch: these calls carry made-up pointers and run where no GPU exists."""
    from deepctr_amd import _C
    lib = _C.lib()
    f = lambda b: lib.dctr_fieldpair_bwd(ctypes.byref(b), None)   # noqa: E731
    assert lib.dctr_fieldpair_bwd(None, None) == -1 and lib.dctr_fieldpair_bwd_supported(None) == 0
    assert lib.dctr_fieldpair_bwd_workspace_bytes(None) == 0
    assert f(_bwd_args(batch=0)) == 0                                # an empty batch: a no-op
    assert f(_bwd_args(dx=None, d_weights=None)) == 0                # nothing asked for: a no-op
    assert f(_bwd_args(d_pairs=None, d_logit=None)) == -1
    assert b"fieldpair_bwd" in lib.dctr_last_error()
    assert f(_bwd_args(x=None)) == -1 and f(_bwd_args(weights=None)) == -1
    assert f(_bwd_args(kind=1, d_pairs=None, d_logit=None)) == -1    # FwFM needs d_logit
    assert f(_bwd_args(kind=1)) == -2                                # ... and has no d_pairs
    assert f(_bwd_args(kind=2)) == -4 and f(_bwd_args(accumulate=2)) == -4
    assert f(_bwd_args(dx_stride=11)) == -2 and f(_bwd_args(dx_offset=1)) == -2
    assert f(_bwd_args(dx=None, dx_stride=0, batch=0)) == 0          # ... which is read with dx only
    assert f(_bwd_args(d_pairs_stride=2)) == -2 and f(_bwd_args(d_pairs_offset=1)) == -2 and f(_bwd_args(x_stride=11)) == -2
    assert f(_bwd_args(x_offset=1)) == -2 and f(_bwd_args(x_offset=-1, x_stride=20)) == -2
    assert f(_bwd_args(fields=1)) == -2 and f(_bwd_args(batch=-1)) == -2 and f(_bwd_args(max_blocks=-1)) == -2
    # FwFM over so many fields that one tile's [F, F] sums pass 2^30 floats: declined, not an argument error
    huge = dict(kind=1, d_pairs=None, fields=40000, dim=1, x_stride=40000, dx_stride=40000)
    assert lib.dctr_fieldpair_bwd_supported(ctypes.byref(_bwd_args(**huge))) == 0
    assert f(_bwd_args(**huge)) == _C.E_UNSUPPORTED
    # a tile past the LDS: the workspace is required, large enough and 16-byte aligned
    big = dict(fields=200, dim=16, x_stride=3200, dx_stride=3200, d_pairs_stride=19900)
    need = lib.dctr_fieldpair_bwd_workspace_bytes(ctypes.byref(_bwd_args(**big)))
    assert need > 0
    assert f(_bwd_args(**big)) == -1
    assert f(_bwd_args(workspace=4096, workspace_bytes=need - 4, **big)) == -1
    assert f(_bwd_args(workspace=4096 + 4, workspace_bytes=need, **big)) == -3
    assert f(_bwd_args(workspace=4096, workspace_bytes=need, batch=0, **big)) == 0


def test_header_declares_the_entry_points_and_the_mirror_matches_the_c_layout(tmp_path):
    import shutil
    from deepctr_amd import _C
    header = open(os.path.join(ROOT, "include", "dctr.h")).read()
    assert "#define DCTR_ABI_VERSION 13" in header and _C.ABI_VERSION == 13
    for sym, ret in (("dctr_fieldpair_bwd", "int"), ("dctr_fieldpair_bwd_supported", "int"),
                     ("dctr_fieldpair_bwd_workspace_bytes", "size_t")):
        assert re.search(r"\b%s %s\(const dctr_fieldpair_bwd_args_t\* args" % (ret, sym), header), sym
        assert _C.SYMBOLS[sym][1][0] == ctypes.POINTER(_C.fieldpair.BwdArgs)
    assert "fieldpair_bwd_kernels.hip" in __import__("deepctr_amd.build", fromlist=["SOURCES"]).SOURCES
    assert "fieldpair_bwd_kernels.hip" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    gcc = shutil.which("gcc")
    assert gcc is not None
    fields = [n for n, _ in _C.fieldpair.BwdArgs._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "dctr.h"', 'int main(void) {',
           '  printf("%zu\\n", sizeof(dctr_fieldpair_bwd_args_t));']
    src += ['  printf("%%zu\\n", offsetof(dctr_fieldpair_bwd_args_t, %s));' % n for n in fields]
    src += ['  return 0;', '}']
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = str(tmp_path / "layout")
    subprocess.check_call([gcc, "-I", os.path.join(ROOT, "include"), str(c), "-o", exe])
    out = [int(v) for v in subprocess.check_output([exe]).split()]
    assert out[0] == ctypes.sizeof(_C.fieldpair.BwdArgs)
    assert out[1:] == [getattr(_C.fieldpair.BwdArgs, n).offset for n in fields]


# ---------------------------------------------------------------------------------------------------
# the dispatchers on the CPU: torch ops, unchanged
# ---------------------------------------------------------------------------------------------------
def test_dispatchers_take_the_torch_ops_on_the_cpu():
    from deepctr_amd import training
    case = RF.CASE_BY_NAME["ragged"]
    x, weights, _, _ = RF.case_inputs(case, "fefm")
    xt = torch.tensor(x, requires_grad=True)
    layer = _Fefm([torch.tensor(w, requires_grad=True) for w in weights])
    ref = training._fefm(layer, xt)
    pairs, logit = training.fefm_pairs(layer, xt, True, True)
    assert torch.equal(pairs, ref) and torch.equal(logit, ref.sum(-1))
    assert training.fefm_pairs(layer, xt, True, False)[1] is None and training.fefm_pairs(layer, xt, False, True)[0] is None
    assert training.fefm_pairs(layer, xt, False, False) == (None, None)

    class _Fwfm(object):
        field_strengths = torch.tensor(RF.case_inputs(case, "fwfm")[1], requires_grad=True)
    got = training.fwfm_logit(_Fwfm, xt)
    want = (torch.einsum("bie,bje->bij", xt, xt) * torch.triu(_Fwfm.field_strengths, diagonal=1)).sum((1, 2))
    assert torch.equal(got, want) and got.requires_grad
