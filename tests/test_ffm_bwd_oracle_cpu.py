"""CPU: the float64 oracle of dctr_ffm_bwd (tests/ref_ffm_bwd.py) against torch double autograd over the products of
_ONN._autograd_logit, the room tests.util.assert_close_terms leaves a float32 implementation that adds in another order, the host-only
entry points (no launch), the C layout of the args structs, and the autograd step's gate on the CPU."""
import ctypes
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import ref_ffm_bwd as RB
from tests.ref_onn import slot
from tests.util import TERMS_REPORT, assert_close_terms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE_RUNS = [(c.name, s) for c in RB.CASES for s in (False, True)]
CASE_IDS = ["%s-%s" % (n, "sum" if s else "cat") for n, s in CASE_RUNS]


def _torch_grads(case, reduce_sum, dtype):
    """Per field the gradient of its fused table (its pooled rows) from torch autograd on the CPU, over the torch ops of
    _ONN.field_aware_rows / _autograd_logit: per-name views master[:, k, :] gathered by id, multiplied pair by pair, concatenated."""
    from deepctr_amd import training
    ids, masters, g, pooled = RB.case_inputs(case, reduce_sum)
    F, d, B = case.shape
    R = (F - 1) * d
    leaves = [torch.tensor(pooled[j][:, :R].reshape(B, F - 1, d) if j in pooled else masters[j], dtype=dtype, requires_grad=True)
              for j in range(F)]
    embs = []
    for j in range(F):
        rows = torch.from_numpy(ids[j].astype(np.int64))
        embs.append({i: (leaves[j][:, slot(j, i), :] if j in pooled else leaves[j][:, slot(j, i), :][rows]) for i in range(F) if i != j})
    prods = []
    for i, j in zip(*training._pair_indices(F)):
        pr = embs[i][j] * embs[j][i]
        prods.append(pr.sum(-1, keepdim=True) if reduce_sum else pr)
    (torch.cat(prods, dim=-1) * torch.tensor(g, dtype=dtype)).sum().backward()
    return [None if j in case.frozen else leaves[j].grad.numpy() for j in range(F)]


@pytest.mark.parametrize("name,reduce_sum", CASE_RUNS, ids=CASE_IDS)
def test_oracle_matches_torch_double_autograd(name, reduce_sum):
    case = RB.CASE_BY_NAME[name]
    G, T = RB.oracle(case, reduce_sum)
    ref = _torch_grads(case, reduce_sum, torch.float64)
    assert len(G) == len(ref) == len(T) == case.shape[0]
    for j, (a, r, t) in enumerate(zip(G, ref, T)):
        assert (a is None) == (r is None) == (j in case.frozen)
        if a is None:
            continue
        assert a.shape == r.shape, j
        scale = max(np.abs(r).max(), 1e-300)
        assert np.abs(a - r).max() <= 1e-12 * scale, (j, float(np.abs(a - r).max() / scale))
        assert (t >= np.abs(a) * (1 - 1e-12)).all(), j               # the terms bound the result they were summed to


def test_a_wrong_backward_is_told_apart():
    """The partner's row read at the field's own slot index: misses double autograd and the fp32 bar by orders of magnitude."""
    case = RB.CASE_BY_NAME["ragged"]
    ids, masters, g, _ = RB.case_inputs(case, False)
    G, T = RB.oracle(case, False)
    W, _ = RB.ffm_bwd(ids, masters, g, wrong=True)
    ref = _torch_grads(case, False, torch.float64)
    assert np.abs(W[2] - ref[2]).max() > 1e-3 * np.abs(ref[2]).max()
    with pytest.raises(AssertionError):
        assert_close_terms(W[2], G[2], T[2], what="wrong field 2")


def _sequential_float32(case, reduce_sum):
    """The op's arithmetic with the adds in sample order: one float32 product per element, added into a float32 table one sample
    after the other (the atomics add the same products in some other order)."""
    ids, masters, g, pooled = RB.case_inputs(case, reduce_sum)
    F, d, B = case.shape
    R = (F - 1) * d
    rows = [pooled[j][:, :R].reshape(B, F - 1, d) if j in pooled else masters[j][ids[j].astype(np.int64)] for j in range(F)]
    pairs = list(itertools.combinations(range(F), 2))
    out = []
    for j in range(F):
        if j in case.frozen:
            out.append(None)
            continue
        drow = np.zeros((B, F - 1, d), dtype=np.float32)
        for i in range(F):
            if i == j:
                continue
            p = pairs.index((min(i, j), max(i, j)))
            gp = g[:, p:p + 1] if reduce_sum else g[:, p * d:(p + 1) * d]
            drow[:, slot(j, i)] = gp * rows[i][:, slot(i, j)]
        if j in pooled:
            out.append(drow)
            continue
        G = np.zeros(masters[j].shape, dtype=np.float32)
        for b in range(B):
            G[int(ids[j][b])] += drow[b]
        out.append(G)
    return out


@pytest.mark.parametrize("name", [c.name for c in RB.CASES])
def test_sequential_float32_accumulation_sits_inside_the_bar(name, capsys):
    """Float32 products added in sample order against the oracle under assert_close_terms' defaults: at most a quarter of the bar for
    every case, so the bar leaves room for whatever order the atomics arrive in.  Prints the worst err / bar per case."""
    case = RB.CASE_BY_NAME[name]
    worst = 0.0
    for reduce_sum in (False, True):
        G, T = RB.oracle(case, reduce_sum)
        got = _sequential_float32(case, reduce_sum)
        for j, (a, r, t) in enumerate(zip(got, G, T)):
            if r is None:
                assert a is None
                continue
            assert a.dtype == np.float32
            n0 = len(TERMS_REPORT)
            assert_close_terms(a, r, t, what="%s reduce=%d field %d (sequential float32)" % (name, reduce_sum, j))
            worst = max(worst, TERMS_REPORT[n0][4])
    with capsys.disabled():
        print("\n[ffm_bwd sequential float32] %s: worst err / bar %.3g" % (name, worst))
    assert worst <= 0.25


def test_case_table_is_the_one_agreed():
    assert [(c.name, c.shape) for c in RB.CASES] == [
        ("smallest", (2, 1, 1)), ("ragged", (3, 5, 33)), ("vec", (4, 4, 3)), ("dup", (3, 8, 300)), ("tiles", (9, 8, 700)),
        ("pooled", (5, 8, 70)), ("frozen", (3, 5, 33)), ("criteo4", (26, 4, 130)), ("criteo16", (26, 16, 67)), ("direct", (60, 16, 6))]
    by = RB.CASE_BY_NAME
    assert RB.case_vocab(by["smallest"]) == [1, 1] and RB.case_vocab(by["dup"]) == [1, 2, 40]
    assert by["tiles"].max_blocks == (0, 1) and by["pooled"].pooled == (2, 4) and by["frozen"].frozen == (1,)
    assert [c.route for c in RB.CASES] == ["lds"] * 9 + ["direct"]
    assert {RB.ids_dtype(c) for c in RB.CASES[0::2]} == {np.int32} and {RB.ids_dtype(c) for c in RB.CASES[1::2]} == {np.int64}
    # every LDS case on both routes, every case with reduce_sum off and on, tiles also with one workgroup
    assert len(RB.RUNS) == 9 * 2 * 2 + 4 + 2


# ---------------------------------------------------------------------------------------------------
# host-only entry points
# ---------------------------------------------------------------------------------------------------
def test_routes_and_workspace_for_the_table():
    from deepctr_amd import _C, ops
    for c in RB.CASES:
        F, d, B = c.shape
        for reduce_sum in (False, True):
            assert ops.ffm_bwd_route(B, F, d, reduce_sum) == c.route, c.name
            assert ops.ffm_bwd_route(B, F, d, reduce_sum, route="direct") == "direct"
            assert ops.ffm_bwd_workspace_bytes(B, F, d, reduce_sum) == 0
            assert ops.ffm_bwd_workspace_bytes(B, F, d, reduce_sum, route="direct") == 0
    # whatever the forward takes on its LDS route fits the backward's too, and rows past the LDS go direct on both
    for F, d in ((2, 1), (2, 64), (26, 4), (26, 16), (9, 17), (39, 8), (13, 17), (60, 8), (60, 16), (200, 4), (100, 32), (30, 64), (200, 64)):
        for n in (3, 4096, 65536):
            assert ops.ffm_bwd_route(n, F, d) == ops.ffm_route(n, F, d), (F, d, n)
    with pytest.raises(_C.DctrError):
        ops.ffm_bwd_route(5, 1, 4)
    with pytest.raises(ValueError, match="route"):
        ops.ffm_bwd_route(5, 4, 4, route="lds")


def _bwd_args(**kw):
    from deepctr_amd import _C
    fwd = dict(fields=16, batch=4, n_fields=4, dim=3, reduce_sum=0, n_dense=0, route=0)
    top = dict(d_out=16, d_out_stride=18, d_out_offset=0, grads=16, max_blocks=0)
    for k, v in kw.items():
        (top if k in top or k in ("workspace", "workspace_bytes") else fwd)[k] = v
    b = _C.ffm.BwdArgs(**top)
    b.fwd = _C.ffm.Args(**fwd)
    return b


def test_argument_errors_without_a_gpu():
    """Every refusal precedes the launch: these calls carry made-up pointers and run where no GPU exists."""
    from deepctr_amd import _C
    lib = _C.lib()
    f = lambda b: lib.dctr_ffm_bwd(ctypes.byref(b), None)   # noqa: E731
    assert lib.dctr_ffm_bwd(None, None) == -1 and lib.dctr_ffm_bwd_route(None) == -1 and lib.dctr_ffm_bwd_workspace_bytes(None) == 0
    assert f(_bwd_args(batch=0)) == 0                                    # an empty batch: a no-op
    for k in ("fields", "d_out", "grads"):
        assert f(_bwd_args(**{k: None})) == -1, k
    assert b"ffm_bwd" in lib.dctr_last_error()
    assert f(_bwd_args(n_fields=1)) == -2 and f(_bwd_args(n_fields=0)) == -2
    assert f(_bwd_args(dim=0)) == -2 and f(_bwd_args(dim=-3)) == -2
    assert f(_bwd_args(batch=-1)) == -2 and f(_bwd_args(max_blocks=-1)) == -2
    assert f(_bwd_args(d_out_stride=17)) == -2                           # 6 pairs x 3 = 18 columns
    assert f(_bwd_args(d_out_offset=1)) == -2 and f(_bwd_args(d_out_offset=-1, d_out_stride=40)) == -2
    assert f(_bwd_args(d_out_offset=2, d_out_stride=20, batch=0)) == 0
    assert f(_bwd_args(reduce_sum=1, d_out_stride=5)) == -2              # 6 scalars
    assert f(_bwd_args(reduce_sum=1, d_out_stride=6, batch=0)) == 0
    assert f(_bwd_args(route=3)) == -4 and f(_bwd_args(route=-1)) == -4
    assert f(_bwd_args(n_dense=2)) == _C.E_UNSUPPORTED                   # the dense columns and the BatchNormalization stay with the caller
    assert f(_bwd_args(scale=16, shift=16)) == _C.E_UNSUPPORTED
    assert f(_bwd_args(workspace=4096 + 4, workspace_bytes=64)) == -3
    assert f(_bwd_args(n_fields=70000, dim=1, d_out_stride=1 << 40)) == -2
    # out / out_stride / out_offset of the forward are not read
    assert f(_bwd_args(out_stride=3, out_offset=-7, batch=0)) == 0
    assert lib.dctr_ffm_bwd_route(ctypes.byref(_bwd_args(d_out=None, grads=None, fields=None))) == _C.ffm.ROUTE_LDS


def test_header_declares_the_entry_points_and_the_mirrors_match_the_c_layout(tmp_path):
    from deepctr_amd import _C
    header = open(os.path.join(ROOT, "include", "dctr.h")).read()
    assert "#define DCTR_ABI_VERSION 13" in header and _C.ABI_VERSION == 13
    for sym, ret in (("dctr_ffm_bwd", "int"), ("dctr_ffm_bwd_route", "int"), ("dctr_ffm_bwd_workspace_bytes", "size_t")):
        assert re.search(r"\b%s %s\(const dctr_ffm_bwd_args_t\* args" % (ret, sym), header), sym
        assert _C.SYMBOLS[sym][1][0] == ctypes.POINTER(_C.ffm.BwdArgs)
    assert "ffm_bwd_kernels.hip" in __import__("deepctr_amd.build", fromlist=["SOURCES"]).SOURCES
    assert "ffm_bwd_kernels.hip" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    gcc = shutil.which("gcc")
    assert gcc is not None
    structs = (("dctr_ffm_bwd_args_t", _C.ffm.BwdArgs), ("dctr_ffm_grad_t", _C.ffm.Grad))
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


# ---------------------------------------------------------------------------------------------------
# the gate on the CPU: torch ops, unchanged
# ---------------------------------------------------------------------------------------------------
def test_gate_keeps_the_cpu_on_the_torch_ops():
    from deepctr_amd import engine, ops, training
    from deepctr_amd.feature_column import DenseFeat, SparseFeat, VarLenSparseFeat
    from deepctr_amd.models import ONN
    assert training.HIP_AUTOGRAD_OPS is True and training.ONN_HIP_MIN_ROWS >= 0
    rng = np.random.RandomState(3)
    n = 19
    cols = [SparseFeat("a", 8, 4), SparseFeat("b", 6, 4), VarLenSparseFeat(SparseFeat("s", 7, 4), maxlen=3, combiner="mean"),
            DenseFeat("x", 1)]
    feed = {"a": rng.randint(0, 8, n).astype(np.int32), "b": rng.randint(0, 6, n).astype(np.int32),
            "s": rng.randint(0, 7, (n, 3)).astype(np.int32), "x": rng.rand(n).astype(np.float32)}
    model = ONN(cols, cols, dnn_hidden_units=(8,), device="cpu")
    staged = engine.Staged(n)
    model._stage_inputs(feed, staged)
    views = [[model.tables["%s_%s" % (a, b)].embeddings for b in "abs" if b != a] for a in "ab"]
    assert torch.is_grad_enabled()
    assert model._pairs_on_hip(staged, 0, n) is None
    assert training._ffm_on_hip(model.masters[:2] + [None], views + [lambda: 1 / 0], n) is None     # (the pooled rows are not formed)
    model._begin()
    assert training.model_logits(model, staged, 0, n, training=True).shape == (n,)
    assert ops.FieldAwareFunction.inputs_of(model.masters[:2] + [None], views + [lambda: 1 / 0]) is None    # tables on the CPU
