"""CPU: the float64 oracle of dctr_ifm_bwd (tests/ref_ifm_bwd.py) against torch double autograd over the expression of
InputAwareModel._autograd_logit, the C layout of dctr_ifm_bwd_args_t, the host-only entry points and every argument error (no launch),
and the autograd step's gate on the CPU."""
import ctypes
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import ref_ifm_bwd as RB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [(F, d, n_src, mp, terms, softmax)
         for F, d, n_src, mp, terms, softmax in itertools.product((1, 2, 3, 39), (1, 4, 5), (0, 1, 2), (False, True), (False, True),
                                                                  (False, True))
         if n_src or mp]                   # (without a source m' is mprime itself)


def _torch_grads(c, F, d, softmax):
    """d_out-weighted double autograd over _autograd_logit's expression -> (m, grads as the oracle's dict)."""
    t64 = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=True)    # noqa: E731
    B = c["x"].shape[0]
    x = t64(c["x"][:, :F * d].reshape(B, F, d))
    srcs = [(t64(a), t64(w)) for a, w in c["sources"]]
    mp = None if c["mprime"] is None else t64(c["mprime"])
    terms = None if c["terms"] is None else t64(c["terms"][:, :F])
    mprime = sum(a @ w for a, w in srcs) + (mp if mp is not None else 0)
    m = F * torch.softmax(mprime, dim=1) if softmax else mprime
    r = x * m.unsqueeze(-1)
    logit = 0.5 * (r.sum(1).pow(2) - (r * r).sum(1)).sum(-1)
    if terms is not None:
        logit = logit + (terms * m).sum(-1)
    (logit * torch.tensor(c["d_out"], dtype=torch.float64)).sum().backward()
    g = lambda t: None if t is None else t.grad.numpy()     # noqa: E731
    return m.detach().numpy(), dict(dx=g(x), dterms=g(terms), dmprime=g(mp), dact=[g(a) for a, _ in srcs], dkernel=[g(w) for _, w in srcs])


@pytest.mark.parametrize("F,d,n_src,mp,terms,softmax", CASES)
def test_oracle_matches_torch_double_autograd(F, d, n_src, mp, terms, softmax):
    c = RB.case(F, d, 7, (6, 3)[:n_src], mp, terms, 0, softmax, seed=F * 100 + d * 10 + n_src)
    m, ref = _torch_grads(c, F, d, softmax)
    got = RB.ifm_bwd(c["x"], F, d, m, c["d_out"], c["sources"], c["terms"], softmax)
    mag = RB.ifm_bwd(c["x"], F, d, m, c["d_out"], c["sources"], c["terms"], softmax, absolute=True)

    def check(name, a, r, t):
        if r is None:
            return
        scale = max(np.abs(r).max(), 1e-300)
        assert a.shape == r.shape, name
        assert np.abs(a - r).max() <= 1e-12 * max(scale, np.abs(t).max()), (name, float(np.abs(a - r).max() / scale))
        assert (t >= np.abs(a) * (1 - 1e-12)).all(), name          # the magnitudes bound the result they were summed to

    for k in ("dx", "dterms", "dmprime"):
        check(k, got[k], ref[k], mag[k])
    for s in range(n_src):
        check("dact%d" % s, got["dact"][s], ref["dact"][s], mag["dact"][s])
        check("dkernel%d" % s, got["dkernel"][s], ref["dkernel"][s], mag["dkernel"][s])


def test_sweep_is_the_one_agreed():
    assert [r[:4] for r in RB.SWEEP] == [
        (1, 1, 5, (3,)), (2, 3, 17, ()), (3, 5, 33, (7, 21)), (5, 2, 64, (64,)), (13, 17, 40, (65, 130)), (16, 16, 129, (16,)),
        (7, 64, 21, (100,)), (5, 33, 9, (19,)), (3, 130, 6, (8,)), (64, 1, 70, (5,)), (65, 3, 66, (33, 31)), (600, 2, 19, (40,)),
        (39, 4, 1001, (64,)), (39, 4, 257, (2496, 64))]
    assert [r[4:] for r in RB.SWEEP] == [(False, True, 0), (True, True, 3), (False, False, 5), (True, True, 0), (False, True, 7),
                                         (False, True, 0), (False, True, 1), (False, True, 3), (False, True, 2), (False, True, 0),
                                         (False, False, 1), (False, True, 1), (False, True, 0), (False, True, 0)]


# ---------------------------------------------------------------------------------------------------
# the C side without a GPU
# ---------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points_and_the_mirror_matches_the_c_layout(tmp_path):
    from deepctr_amd import _C
    header = open(os.path.join(ROOT, "include", "dctr.h")).read()
    assert "#define DCTR_ABI_VERSION 13" in header and _C.ABI_VERSION == 13
    for sym, ret in (("dctr_ifm_bwd", "int"), ("dctr_ifm_bwd_supported", "int"), ("dctr_ifm_bwd_workspace_bytes", "size_t")):
        assert re.search(r"\b%s %s\(const dctr_ifm_bwd_args_t\* args" % (ret, sym), header), sym
        assert _C.SYMBOLS[sym][1][0] == ctypes.POINTER(_C.ifm.BwdArgs)
        assert _C.SYMBOLS[sym][0] == (ctypes.c_size_t if ret == "size_t" else ctypes.c_int)
    assert "ifm_bwd_kernels.hip" in __import__("deepctr_amd.build", fromlist=["SOURCES"]).SOURCES
    assert "ifm_bwd_kernels.hip" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    gcc = shutil.which("gcc")
    assert gcc is not None
    structs = (("dctr_ifm_bwd_args_t", _C.ifm.BwdArgs), ("dctr_ifm_src_t", _C.ifm.Src))
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "dctr.h"', 'int main(void) {']
    want = []
    for cname, cls in structs:
        src.append('  printf("%%zu\\n", sizeof(%s));' % cname)
        want.append(ctypes.sizeof(cls))
        for n, _ in cls._fields_:
            src.append('  printf("%%zu\\n", offsetof(%s, %s));' % (cname, n))
            want.append(getattr(cls, n).offset)
    src += ['  return 0;', '}']
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = str(tmp_path / "layout")
    subprocess.check_call([gcc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe])
    assert [int(v) for v in subprocess.check_output([exe]).split()] == want


def _args(**kw):
    """Made-up pointers: 4 samples of 3 fields x 2, one source of K = 5, every output wanted."""
    from deepctr_amd import _C
    top = dict(batch=4, n_fields=3, dim=2, x=16, x_stride=6, factor=16, factor_stride=3, terms=16, terms_stride=3, d_out=16, n_src=1,
               softmax=1, dx=16, dx_stride=6, dterms=16, dterms_stride=3, dmprime=16, dmprime_stride=3, slices=0,
               workspace=4096, workspace_bytes=1 << 20)
    src = dict(act=16, kernel=16, act_stride=5, K=5)
    per = dict(dact=16, dact_stride=5, dkernel=16, dkernel_stride=3)
    for k, v in kw.items():
        (src if k in src else per if k in per else top)[k] = v
    b = _C.ifm.BwdArgs(**top)
    for s in range(min(max(top["n_src"], 0), 2)):
        b.src[s] = _C.ifm.Src(**src)
        for k, v in per.items():
            getattr(b, k)[s] = v
    return b


def test_argument_errors_without_a_gpu():
    """Every refusal precedes the launch: these calls carry made-up pointers and run where no GPU exists."""
    from deepctr_amd import _C
    lib = _C.lib()
    f = lambda b: lib.dctr_ifm_bwd(ctypes.byref(b), None)          # noqa: E731
    assert lib.dctr_ifm_bwd(None, None) == -1 and lib.dctr_ifm_bwd_supported(None) == 0 and lib.dctr_ifm_bwd_workspace_bytes(None) == 0
    assert b"ifm_bwd" in lib.dctr_last_error()
    assert f(_args(batch=0, dkernel=None)) == 0                          # an empty batch without a sum over it: a no-op
    for k in ("x", "factor", "d_out"):
        assert f(_args(**{k: None})) == -1, k
    assert f(_args(kernel=None)) == -1 and f(_args(act=None)) == -1
    assert f(_args(kernel=None, dact=None, batch=0, dkernel=None)) == 0  # (the kernel is read for dact alone)
    assert f(_args(n_fields=0)) == -2 and f(_args(dim=0)) == -2 and f(_args(n_fields=-1)) == -2 and f(_args(dim=-3)) == -2
    assert f(_args(batch=-1)) == -2
    assert f(_args(n_fields=1 << 14, dim=1 << 13, x_stride=1 << 40, dx_stride=1 << 40, factor_stride=1 << 20, terms_stride=1 << 20,
                   dterms_stride=1 << 20, dmprime_stride=1 << 20, dkernel_stride=1 << 20)) == -2        # F * d = 2^27
    for k, short in (("x_stride", 5), ("factor_stride", 2), ("terms_stride", 2), ("dx_stride", 5), ("dterms_stride", 2),
                     ("dmprime_stride", 2), ("act_stride", 4), ("dact_stride", 4), ("dkernel_stride", 2)):
        assert f(_args(**{k: short})) == -2, k
    assert f(_args(terms=None, terms_stride=0, batch=0, dkernel=None)) == 0      # a stride is read only beside its pointer
    assert f(_args(dx=None, dx_stride=0, dact=None, dact_stride=0, batch=0, dkernel=None)) == 0
    assert f(_args(K=0)) == -2
    assert f(_args(n_src=3)) == -2 and f(_args(n_src=-1)) == -2
    assert f(_args(slices=257)) == -2 and f(_args(slices=-1)) == -2
    # sources present: the workspace the library asks for is required, whole and aligned
    need = lib.dctr_ifm_bwd_workspace_bytes(ctypes.byref(_args(dmprime=None)))
    assert need >= 4 * 3 * 4 + 64 * 3 * 4
    assert f(_args(dmprime=None, workspace=None, workspace_bytes=0)) == -1
    assert f(_args(dmprime=None, workspace_bytes=need - 1)) == -1
    assert b"dctr_ifm_bwd_workspace_bytes" in lib.dctr_last_error()
    assert f(_args(dmprime=None, workspace=4096 + 4)) == -3
    need = lib.dctr_ifm_bwd_workspace_bytes(ctypes.byref(_args()))          # dm' goes to dmprime: the partials alone
    assert need == 64 * 3 * 4 and f(_args(workspace_bytes=need - 1)) == -1
    assert lib.dctr_ifm_bwd_workspace_bytes(ctypes.byref(_args(slices=3, batch=1000))) == 3 * need
    assert lib.dctr_ifm_bwd_workspace_bytes(ctypes.byref(_args(dkernel=None))) == 0
    assert lib.dctr_ifm_bwd_workspace_bytes(ctypes.byref(_args(n_src=3))) == 0


def test_supported_and_workspace_queries():
    from deepctr_amd import ops
    assert ops.ifm_bwd_supported(600, 2) is True and ops.ifm_bwd_supported(50000, 1) is False
    assert ops.ifm_bwd_supported(39, 4) and ops.ifm_bwd_supported(40960, 1) and not ops.ifm_bwd_supported(40961, 1)
    assert not ops.ifm_bwd_supported(0, 4)
    assert ops.ifm_bwd_workspace_bytes(4096, 39, 4, ()) == 0
    assert ops.ifm_bwd_workspace_bytes(4096, 39, 4, (64,), dact=False, dkernel=False) == 0
    dm = 4096 * 39 * 4
    assert ops.ifm_bwd_workspace_bytes(4096, 39, 4, (64,), dkernel=False) == dm
    assert ops.ifm_bwd_workspace_bytes(4096, 39, 4, (64,), dmprime=True, dkernel=False) == 0
    # S is a function of the shapes alone: 512 workgroups over the 64-row blocks, at most one slice per 64 samples, at most 256
    block = 64 * 39 * 4
    assert ops.ifm_bwd_workspace_bytes(4096, 39, 4, (64,)) == dm + 64 * block
    assert ops.ifm_bwd_workspace_bytes(65536, 39, 4, (64,), dmprime=True) == 256 * block
    assert ops.ifm_bwd_workspace_bytes(65536, 39, 4, (2496, 64), dmprime=True) == 13 * 40 * block
    assert ops.ifm_bwd_workspace_bytes(65536, 39, 4, (2496, 64), dmprime=True, slices=7) == 7 * 40 * block
    with pytest.raises(ValueError):
        ops.ifm_bwd_workspace_bytes(5, 3, 2, (1, 2, 3))


# ---------------------------------------------------------------------------------------------------
# the gate on the CPU: torch ops, unchanged
# ---------------------------------------------------------------------------------------------------
def _small(rng, n, d=8):
    from deepctr_amd.feature_column import DenseFeat, SparseFeat, VarLenSparseFeat
    cols = [SparseFeat("C%d" % i, 50, d) for i in range(5)] + [VarLenSparseFeat(SparseFeat("S", 30, d), maxlen=4, combiner="mean"),
                                                                 DenseFeat("I0", 1)]
    feed = {"C%d" % i: rng.randint(0, 50, n).astype(np.int32) for i in range(5)}
    feed["S"] = rng.randint(0, 30, (n, 4)).astype(np.int32)
    feed["S"][:, 0] = np.maximum(feed["S"][:, 0], 1)
    feed["I0"] = rng.rand(n).astype(np.float32)
    return cols, feed


@pytest.mark.parametrize("kind", ["IFM", "DIFM"])
def test_cpu_steps_are_bit_identical_with_the_switch_on_and_off(kind, monkeypatch):
    """fit() itself asks for a HIP device, so a CPU-built model is trained by the step fit() takes for it: model_logits(training=True),
    the loss, backward, KerasAdam.  The gate is False on the CPU whatever the switch says: three steps end at the same bits."""
    from deepctr_amd import engine, models, training, training_hip
    rng = np.random.RandomState(4)
    n = 64
    cols, feed = _small(rng, n)
    y = torch.from_numpy(((feed["C0"] % 2) ^ (feed["C1"] % 3 == 0)).astype(np.float32))
    kw = dict(att_embedding_size=4, att_head_num=2) if kind == "DIFM" else {}
    assert training.HIP_AUTOGRAD_OPS is True and training.IFM_HIP_MIN_ROWS >= 0 and training.DIFM_HIP_MIN_ROWS >= 0
    ends = {}
    for switch in (True, False):
        monkeypatch.setattr(training, "HIP_AUTOGRAD_OPS", switch)
        monkeypatch.setattr(training, kind + "_HIP_MIN_ROWS", 0)
        model = getattr(models, kind)(cols, cols, dnn_hidden_units=(16, 8), seed=3, device="cpu", **kw)
        assert not training_hip.supported(model)
        assert training._ifm_on_hip(torch.zeros(n, 6, 8, requires_grad=True)) is False
        params = [t for k, t in model.named_weights()]
        for t in params:
            t.requires_grad_(True)
        opt = training.KerasAdam(params, lr=1e-2)
        staged = engine.Staged(n)
        model._stage_inputs(feed, staged)
        for _ in range(3):
            opt.zero_grad()
            model._begin()
            loss = torch.nn.functional.binary_cross_entropy_with_logits(training.model_logits(model, staged, 0, n, training=True), y)
            loss.backward()
            opt.step()
        for t in params:
            t.requires_grad_(False)
        ends[switch] = {k: t.detach().clone() for k, t in model.named_weights()}
    assert sorted(ends[True]) == sorted(ends[False])
    assert all(torch.equal(ends[True][k], ends[False][k]) for k in ends[True])
    assert not torch.equal(ends[True]["dense/kernel"], getattr(models, kind)(cols, cols, dnn_hidden_units=(16, 8), seed=3, device="cpu",
                                                                            **kw).dense.w("kernel"))
