"""CPU: the float64 oracle of dctr_gru_bwd (tests/ref_gru_bwd.py) against torch double autograd over training._gru and against central
differences of tests/ref_dien.py, the room tests.util.assert_close_terms leaves a float32 implementation, the host-only entry points
(no launch), the C layout of the args struct, and the autograd step's dynamic_gru on the CPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import ref_dien
from tests import ref_gru_bwd as RG
from tests.util import TERMS_REPORT, assert_close_terms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [c.name for c in RG.CASES]


def _torch_grads(case, dtype):
    """Gradients by the oracle's keys from torch autograd over training._gru on the CPU."""
    from deepctr_amd import training
    x, lens, layer, att, d_out = RG.case_inputs(case)
    cell, scale = RG.case_options(case)
    need_att = cell != "GRU" or scale
    xt = torch.tensor(x, dtype=dtype, requires_grad=True)
    at = torch.tensor(att, dtype=dtype, requires_grad=need_att)
    ws = [torch.tensor(w, dtype=dtype, requires_grad=True) for w in layer]
    out = training._gru(xt, torch.tensor(lens), [ws], cell=cell, att_scores=at if need_att else None, scale_input=scale,
                        return_sequence=case.return_sequence)
    out.backward(torch.tensor(d_out, dtype=dtype))
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad      # noqa: E731
    got = {"dx": zero(xt).numpy(), "d_att": zero(at).numpy() if need_att else None}
    for k, w in zip(RG.KEYS[2:], ws):
        got[k] = zero(w).numpy()
    return got


def test_case_table_covers_what_was_agreed():
    cs = RG.CASES
    assert {c.E for c in cs} == {1, 4, 12, 16, 17, 40, 64, 49, 65} and {c.T for c in cs} == {1, 2, 6} and {c.B for c in cs} == {1, 17, 33}
    for E in RG.E_LIST:
        assert {(c.variant, c.return_sequence) for c in cs if c.E == E} == {(v, s) for v, _ in RG.VARIANTS for s in (True, False)}
    assert any(c.B == 33 and c.max_blocks == 1 for c in cs) and any(c.B == 33 and c.max_blocks == 0 for c in cs)
    assert any(c.route == "streamed" for c in cs)
    lens = RG.case_lengths(6, 33)
    assert {0, 1, 6, 9, -1} <= set(lens.tolist()) and (lens[16:32] == 0).all()
    assert RG.case_lengths(2, 17).max() == 5 and RG.case_lengths(2, 17).min() == -1


@pytest.mark.parametrize("name", IDS)
def test_oracle_matches_torch_double_autograd(name):
    case = RG.CASE_BY_NAME[name]
    G, T = RG.case_oracle(case)
    ref = _torch_grads(case, torch.float64)
    assert sorted(G) == sorted(ref) == sorted(RG.KEYS) and sorted(T) == sorted(G)
    for k in RG.KEYS:
        if G[k] is None:
            assert ref[k] is None and T[k] is None
            continue
        assert G[k].shape == ref[k].shape, k
        scale = max(np.abs(ref[k]).max(), 1e-300)
        assert np.abs(G[k] - ref[k]).max() <= 1e-9 * scale, (k, float(np.abs(G[k] - ref[k]).max() / scale))
        assert (T[k] >= np.abs(G[k]) * (1 - 1e-12)).all(), k          # the terms bound the result they were summed to


def test_oracle_matches_central_differences():
    """sum(out * d_out) of tests/ref_dien.py's forward, differentiated numerically in x, the scores and every weight."""
    case = RG.Case("fd", 3, 4, 5, "AUGRU", False, 0, None, 7)
    x, _, layer, att, d_out = RG.case_inputs(case)
    x, att, d_out = (np.asarray(v, np.float64) for v in (x, att, d_out))
    layer = [np.asarray(w, np.float64) for w in layer]
    lens = np.array([4, 2, 0, 7, 1], np.int32)
    for variant, scale in RG.VARIANTS:
        cell = RG.cell_of(variant)
        for seq in (True, False):
            d = d_out if not seq else np.random.RandomState(3).randn(5, 4, 3)
            G, _ = RG.gru_bwd(x, lens, layer, cell, att, scale, seq, d)

            def f(xv, av, ws):
                return float((ref_dien.dynamic_gru(xv, lens, [tuple(ws)], cell=cell, att_scores=av, scale_input=scale, return_sequence=seq) * d).sum())

            operands = [("dx", x), ("d_att", att)] + list(zip(RG.KEYS[2:], layer))
            for key, arr in operands:
                if G[key] is None:
                    continue
                num = np.zeros_like(arr)
                it = np.nditer(arr, flags=["multi_index"])
                for _ in it:
                    i = it.multi_index
                    old = arr[i]
                    arr[i] = old + 1e-5
                    hi = f(x, att, layer)
                    arr[i] = old - 1e-5
                    lo = f(x, att, layer)
                    arr[i] = old
                    num[i] = (hi - lo) / 2e-5
                scale_ = max(np.abs(num).max(), 1e-12)
                assert np.abs(num - G[key].reshape(num.shape)).max() <= 1e-5 * scale_, (variant, seq, key)


@pytest.mark.parametrize("name", IDS)
def test_float32_autograd_sits_inside_half_the_bar(name, capsys):
    """torch's float32 autograd of training._gru against the oracle under assert_close_terms' defaults: with the saturating factors
    split into their terms a float32 restatement stays below half the bar on every case, so the default bar stands for the kernel."""
    case = RG.CASE_BY_NAME[name]
    G, T = RG.case_oracle(case)
    got = _torch_grads(case, torch.float32)
    worst = {}
    for k in RG.KEYS:
        if G[k] is None:
            continue
        n0 = len(TERMS_REPORT)
        assert_close_terms(got[k], G[k], T[k], what="%s %s (float32 autograd)" % (name, k))
        worst[k] = TERMS_REPORT[n0][4]
    with capsys.disabled():
        print("\n[gru_bwd float32 autograd] %s: worst err / bar %.3g (%s)"
              % (name, max(worst.values()), ", ".join("%s %.2g" % kv for kv in sorted(worst.items()))))
    assert max(worst.values()) <= 0.5


# ---------------------------------------------------------------------------------------------------
# host-only entry points
# ---------------------------------------------------------------------------------------------------
def test_supported_and_workspace_for_the_table():
    from deepctr_amd import ops
    for c in RG.CASES:
        cell, scale = RG.case_options(c)
        assert ops.gru_bwd_supported(c.T, c.E, cell, scale, c.return_sequence, c.route), c.name
        assert ops.gru_bwd_workspace_bytes(c.B, c.T, c.E, cell, scale, c.return_sequence, c.route) == 0, c.name
    # the two bounds the table stands on, read from the library: the widest resident and the widest supported E
    resident = [E for E in range(1, 80) if ops.gru_bwd_supported(6, E, route="resident")]
    taken = [E for E in range(1, 80) if ops.gru_bwd_supported(6, E)]
    assert resident == list(range(1, RG.RESIDENT_MAX_E + 1)) and taken == list(range(1, RG.SUPPORT_MAX_E + 1))
    assert all(ops.gru_bwd_supported(T, 64) for T in (1, 50, 4096))
    # declined: two layers, scale_input with an attention-gated cell
    assert not ops.gru_bwd_supported(6, 8, n_layers=2)
    assert not ops.gru_bwd_supported(6, 8, "AGRU", True) and not ops.gru_bwd_supported(6, 8, "AUGRU", True)


def _bwd_args(**kw):
    from deepctr_amd import _C
    fwd = dict(batch=4, x=16, x_stride=12, x_row_stride=4, lengths=16, att_scores=16, att_stride=3, seq_len=3, dim=4, n_layers=1, cell=0,
               scale_input=0, return_sequence=1, route=0)
    top = dict(h_seq=16, h_stride=12, h_row_stride=4, d_out=16, d_out_stride=12, d_out_row_stride=4, dx=16, dx_stride=12, dx_row_stride=4,
               d_att=16, d_att_stride=3)
    for k, v in kw.items():
        (fwd if k in fwd or k == "layers" else top)[k] = v
    layers = (ctypes.c_void_p * 4)(16, 16, 16, 16)
    b = _C.gru.BwdArgs(**top)
    fwd.setdefault("layers", ctypes.cast(layers, ctypes.c_void_p))
    b.fwd = _C.gru.Args(**fwd)
    b._keep = layers
    return b


def test_argument_errors_without_a_gpu():
    """Every refusal precedes the launch: these calls carry made-up pointers and run where no GPU exists."""
    from deepctr_amd import _C
    lib = _C.lib()
    f = lambda b: lib.dctr_gru_bwd(ctypes.byref(b), None)   # noqa: E731
    assert lib.dctr_gru_bwd(None, None) == -1 and lib.dctr_gru_bwd_supported(None) == 0 and lib.dctr_gru_bwd_workspace_bytes(None) == 0
    assert f(_bwd_args(batch=0)) == 0                                # an empty batch: a no-op
    assert f(_bwd_args(d_out=None)) == -1
    assert b"gru_bwd" in lib.dctr_last_error()
    assert f(_bwd_args(x=None)) == -1 and f(_bwd_args(h_seq=None)) == -1 and f(_bwd_args(layers=None)) == -1
    assert f(_bwd_args(lengths=None)) == -1
    assert f(_bwd_args(cell=2, att_scores=None)) == -1 and f(_bwd_args(scale_input=1, att_scores=None)) == -1
    assert f(_bwd_args(dx_stride=11)) == -2 and f(_bwd_args(dx_row_stride=3)) == -2
    assert f(_bwd_args(dx=None, dx_stride=0, dx_row_stride=0, batch=0)) == 0        # ... which are read with dx only
    assert f(_bwd_args(h_stride=11)) == -2 and f(_bwd_args(x_row_stride=3)) == -2 and f(_bwd_args(d_out_stride=11)) == -2
    assert f(_bwd_args(return_sequence=0, d_out_stride=3)) == -2 and f(_bwd_args(return_sequence=0, d_out_stride=4, batch=0)) == 0
    assert f(_bwd_args(cell=1, d_att_stride=2)) == -2 and f(_bwd_args(cell=1, att_stride=2)) == -2
    assert f(_bwd_args(seq_len=0)) == -2 and f(_bwd_args(batch=-1)) == -2 and f(_bwd_args(max_blocks=-1)) == -2
    assert f(_bwd_args(cell=3)) == -4 and f(_bwd_args(accumulate=2)) == -4 and f(_bwd_args(route=3)) == -4
    assert f(_bwd_args(return_sequence=2)) == -4
    assert f(_bwd_args(n_layers=2)) == _C.E_UNSUPPORTED and f(_bwd_args(cell=1, scale_input=1)) == _C.E_UNSUPPORTED
    wide = RG.SUPPORT_MAX_E + 1
    assert f(_bwd_args(dim=wide, x_row_stride=wide, x_stride=3 * wide, h_row_stride=wide, h_stride=3 * wide, d_out_row_stride=wide,
                       d_out_stride=3 * wide, dx_row_stride=wide, dx_stride=3 * wide)) == _C.E_UNSUPPORTED
    assert f(_bwd_args(dim=49, route=1, x_row_stride=49, x_stride=147, h_row_stride=49, h_stride=147, d_out_row_stride=49,
                       d_out_stride=147, dx_row_stride=49, dx_stride=147)) == _C.E_UNSUPPORTED


def test_header_declares_the_entry_points_and_the_mirror_matches_the_c_layout(tmp_path):
    import shutil
    import subprocess
    from deepctr_amd import _C
    header = open(os.path.join(ROOT, "include", "dctr.h")).read()
    assert "#define DCTR_ABI_VERSION 13" in header and _C.ABI_VERSION == 13
    for sym, ret in (("dctr_gru_bwd", "int"), ("dctr_gru_bwd_supported", "int"), ("dctr_gru_bwd_workspace_bytes", "size_t")):
        assert re.search(r"\b%s %s\(const dctr_gru_bwd_args_t\* args" % (ret, sym), header), sym
        assert _C.SYMBOLS[sym][1][0] == ctypes.POINTER(_C.gru.BwdArgs)
    assert "gru_bwd_kernels.hip" in __import__("deepctr_amd.build", fromlist=["SOURCES"]).SOURCES
    assert "gru_bwd_kernels.hip" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    structs = (("dctr_gru_args_t", _C.gru.Args), ("dctr_gru_bwd_args_t", _C.gru.BwdArgs))
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
@pytest.mark.parametrize("name", ["E12_GRU_seq_T6_B33", "E12_AIGRU_final_T2_B1", "E17_AGRU_seq_T1_B1", "E17_AUGRU_final_T6_B17"])
def test_dynamic_gru_on_the_cpu_is_the_torch_loop(name, monkeypatch):
    from deepctr_amd import training
    case = RG.CASE_BY_NAME[name]
    x, lens, layer, att, _ = RG.case_inputs(case)
    cell, scale = RG.case_options(case)
    xt, at = torch.tensor(x, requires_grad=True), torch.tensor(att, requires_grad=True)
    ws = [torch.tensor(w, requires_grad=True) for w in layer]
    kw = dict(cell=cell, att_scores=at if (cell != "GRU" or scale) else None, scale_input=scale, return_sequence=case.return_sequence)
    want = training._gru(xt, torch.tensor(lens), [ws], **kw)
    assert training.HIP_AUTOGRAD_OPS is True
    for switch in (True, False):
        monkeypatch.setattr(training, "HIP_AUTOGRAD_OPS", switch)
        got = training.dynamic_gru(xt, torch.tensor(lens), [ws], **kw)
        assert torch.equal(got, want) and got.grad_fn is not None
        with torch.no_grad():
            assert torch.equal(training.dynamic_gru(xt, torch.tensor(lens), [ws], **kw), want)
    if cell == "GRU" and not scale:     # a stack: layer by layer, the same bits
        ws2 = [torch.tensor(w * 0.5, requires_grad=True) for w in layer]
        two = training._gru(xt, torch.tensor(lens), [ws, ws2], return_sequence=case.return_sequence)
        assert torch.equal(training.dynamic_gru(xt, torch.tensor(lens), [ws, ws2], return_sequence=case.return_sequence), two)
