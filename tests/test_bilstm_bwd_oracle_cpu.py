"""CPU: the float64 oracle of dctr_bilstm_bwd (tests/ref_bilstm_bwd.py) against torch double autograd over training._bilstm and
against central differences of tests/ref_dsin.bilstm, the room tests.util.assert_close_terms leaves a float32 implementation, what
the case table can tell apart, the host-only entry points (no launch), the C layout of the args struct, and the autograd step's
bilstm on the CPU.

Worst err / bar of float32 torch autograd of training._bilstm on the CPU against the oracle (-s prints every case): at most 0.11
(u16_D16_T1_B1_L1_r1_fw_none), so the default bar stands."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import ref_bilstm_bwd as RB
from tests import ref_dsin
from tests.util import TERMS_REPORT, assert_close_terms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [c.name for c in RB.CASES]


def flat(G):
    return [G["dx"]] + [g for layer in G["d_layers"] for g in layer]


def _torch_grads(case, dtype, monkeypatch, masks="case"):
    """[dx, the 6 L weight gradients] from torch autograd over training._bilstm on the CPU.  masks "case": _dropout hands out the
    case's masks in the order _bilstm asks for them (fw then bw, layer by layer); "seed": _bilstm draws its own under seed 7."""
    from deepctr_amd import training
    x, layers, case_masks, d_out = RB.case_inputs(case)
    xt = torch.tensor(x, dtype=dtype, requires_grad=True)
    ws = [[torch.tensor(w, dtype=dtype, requires_grad=True) for w in layer] for layer in layers]
    if masks == "case":
        queue = list(case_masks or [])

        def handout(ones, rate, training_):
            m = queue.pop(0)
            return ones if m is None else torch.tensor(m, dtype=dtype).reshape(ones.shape)
        monkeypatch.setattr(training, "_dropout", handout)
        out = training._bilstm(xt, ws, case.res, case.merge, "sigmoid", 0.2, case_masks is not None)
        assert not queue
    else:
        torch.manual_seed(7)
        out = training._bilstm(xt, ws, case.res, case.merge, "sigmoid", 0.2, True)
    if case.merge is None:
        torch.autograd.backward(out, [torch.tensor(d, dtype=dtype) for d in d_out])
    else:
        out.backward(torch.tensor(d_out, dtype=dtype))
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad      # noqa: E731
    return [zero(t).numpy() for t in [xt] + [w for layer in ws for w in layer]]


def test_case_table_covers_what_was_agreed():
    cs = RB.CASES
    assert {c.u for c in cs} == {4, 12, 16, 17, 40, RB.STREAMED_U} and {c.T for c in cs} == {1, 2, 5} and {c.B for c in cs} == {1, 17, 33}
    assert {c.L for c in cs} == {1, 2, 3} and {c.merge for c in cs} == set(RB.MERGES) and {c.masks for c in cs} == set(RB.MASK_KINDS)
    assert any(c.res == 0 for c in cs) and any(c.res == 1 < c.L for c in cs) and any(c.res == c.L > 1 for c in cs)
    assert any(c.Din > c.u for c in cs) and any(c.Din < c.u for c in cs)
    assert all(c.u <= 17 for c in cs if c.B == 1)
    assert any(c.B == 33 and c.max_blocks == 2 for c in cs) and any(c.B == 33 and c.max_blocks == 0 for c in cs)
    assert {c.route for c in cs} == {None, "streamed", "resident"}
    partial = RB.case_inputs(next(c for c in cs if c.masks == "partial" and c.L > 1))[2]
    assert any(m is None for m in partial) and any(m is not None for m in partial)
    m = RB.case_inputs(next(c for c in cs if c.masks == "all"))[2][0]
    assert set(np.unique(m).tolist()) == {0.0, 1.25}


@pytest.mark.parametrize("name", IDS)
def test_oracle_matches_torch_double_autograd(name, monkeypatch):
    case = RB.CASE_BY_NAME[name]
    G, T = RB.case_oracle(case)
    ref = _torch_grads(case, torch.float64, monkeypatch)
    for k, (g, t, r) in enumerate(zip(flat(G), flat(T), ref)):
        assert g.shape == r.shape, k
        scale = max(np.abs(r).max(), 1e-300)
        assert np.abs(g - r).max() <= 1e-9 * scale, (k, float(np.abs(g - r).max() / scale))
        assert (t >= np.abs(g) * (1 - 1e-12)).all(), k          # the terms bound the result they were summed to


def test_masks_are_reproduced_by_reseeding(monkeypatch):
    """_bilstm draws one mask [B, 1, D] per LSTM, fw then bw, layer by layer: the same draws under the same seed, handed to the
    oracle, give its own double autograd."""
    from deepctr_amd import training
    case = RB.CASE_BY_NAME["u12_D9_T2_B17_L2_r1_mul_all"]
    x, layers, _, d_out = RB.case_inputs(case)
    torch.manual_seed(7)
    masks = [training._dropout(torch.ones(case.B, 1, case.Din if l == 0 else case.u, dtype=torch.float64), 0.2, True).numpy().reshape(case.B, -1)
             for l in range(case.L) for _ in range(2)]
    assert all(set(np.unique(m).tolist()) <= {0.0, 1.25} for m in masks) and not np.array_equal(masks[0], masks[1])
    G, _ = RB.bilstm_bwd(x, layers, masks, case.res, case.merge, d_out)
    ref = _torch_grads(case, torch.float64, monkeypatch, masks="seed")
    for k, (g, r) in enumerate(zip(flat(G), ref)):
        assert np.abs(g - r).max() <= 1e-9 * max(np.abs(r).max(), 1e-300), k


def test_oracle_matches_central_differences():
    """sum(out * d_out) of tests/ref_dsin.py's forward, differentiated numerically in x and every weight.  ref_dsin.bilstm has no
    masks: a sample's masks scale the rows of ITS kernels (x m W = x (diag(m) W)), so it runs sample by sample."""
    rng = np.random.RandomState(3)
    for merge, res, L, Din in (("ave", 0, 2, 4), ("mul", 1, 2, 2), (None, 2, 2, 3), ("concat", 0, 1, 3), ("bw", 1, 1, 3)):
        case = RB.Case("fd", 3, Din if res < L else 3, 3, 2, L, res, merge, "all", None, 0, 7)
        x, layers, masks, d_out = RB.case_inputs(case)
        x = np.asarray(x, np.float64)
        layers = [[np.asarray(w, np.float64) for w in layer] for layer in layers]
        masks[1] = None
        G, _ = RB.bilstm_bwd(x, layers, masks, res, merge, d_out)

        def f():
            total = 0.0
            for b in range(case.B):
                folded = []
                for l, layer in enumerate(layers):
                    row = list(layer)
                    for d in range(2):
                        m = masks[2 * l + d]
                        if m is not None:
                            row[3 * d] = layer[3 * d] * np.asarray(m, np.float64)[b][:, None]
                    folded.append(tuple(row))
                out = ref_dsin.bilstm(x[b:b + 1], folded, res, merge)
                if merge is None:
                    total += float((out[0] * d_out[0][b:b + 1]).sum() + (out[1] * d_out[1][b:b + 1]).sum())
                else:
                    total += float((out * d_out[b:b + 1]).sum())
            return total

        for k, (arr, g) in enumerate(zip([x] + [w for layer in layers for w in layer], flat(G))):
            num = np.zeros_like(arr)
            it = np.nditer(arr, flags=["multi_index"])
            picks = set(rng.choice(arr.size, min(arr.size, 12), replace=False).tolist())
            for n, _ in enumerate(it):
                if n not in picks:
                    continue
                i = it.multi_index
                old = arr[i]
                arr[i] = old + 1e-5
                hi = f()
                arr[i] = old - 1e-5
                lo = f()
                arr[i] = old
                num[i] = (hi - lo) / 2e-5
            sel = num != 0
            scale_ = max(np.abs(g).max(), 1e-12)
            assert np.abs(num - g.reshape(num.shape))[sel].max(initial=0.0) <= 1e-5 * scale_, (merge, res, k)


@pytest.mark.parametrize("name", IDS)
def test_float32_autograd_sits_inside_half_the_bar(name, capsys, monkeypatch):
    """torch's float32 autograd of training._bilstm against the oracle under assert_close_terms' defaults: with the saturating factors
    split into their terms a float32 restatement stays below half the bar on every case, so the default bar stands for the kernel."""
    case = RB.CASE_BY_NAME[name]
    G, T = RB.case_oracle(case)
    got = _torch_grads(case, torch.float32, monkeypatch)
    worst = []
    for k, (a, g, t) in enumerate(zip(got, flat(G), flat(T))):
        n0 = len(TERMS_REPORT)
        assert_close_terms(a, g, t, what="%s output %d (float32 autograd)" % (name, k))
        worst.append(TERMS_REPORT[n0][4])
    with capsys.disabled():
        print("\n[bilstm_bwd float32 autograd] %s: worst err / bar %.3g (output %d)" % (name, max(worst), int(np.argmax(worst))))
    assert max(worst) <= 0.5


def _moved(case, **change):
    """Largest |G' - G| / bar over the outputs when the oracle is run with ``change``."""
    x, layers, masks, d_out = RB.case_inputs(case)
    G, T = RB.case_oracle(case)
    kw = dict(layers=layers, masks=masks, res_layers=case.res, merge_mode=case.merge, reverse_back=True)
    kw.update(change)
    G2, _ = RB.bilstm_bwd(x, kw["layers"], kw["masks"], kw["res_layers"], kw["merge_mode"], d_out, reverse_back=kw["reverse_back"])
    return max(float((np.abs(a - b) / (1e-4 * np.abs(b) + 2e-6 * t + 1e-30)).max()) for a, b, t in zip(flat(G2), flat(G), flat(T)))


def test_the_table_tells_the_mistakes_apart():
    """From the oracle alone: each mistake an implementation could make moves some gradient by at least 100 bars on every case that
    exercises it."""
    def swapped(layers, u):
        perm = np.concatenate([np.arange(u, 2 * u), np.arange(u), np.arange(2 * u, 4 * u)])         # i <-> f
        return [[w[..., perm] for w in layer] for layer in layers]

    for c in RB.CASES:
        layers = RB.case_inputs(c)[1]
        assert _moved(c, layers=swapped(layers, c.u)) >= 100, ("gate quarters", c.name)
        if c.merge != "fw" and c.T > 1:
            assert _moved(c, reverse_back=False) >= 100, ("reversal", c.name)
        if c.masks != "none":
            assert _moved(c, masks=None) >= 100, ("masks", c.name)
        if c.res >= 1:
            assert _moved(c, res_layers=c.res - 1) >= 100, ("residual", c.name)
        if c.merge == "ave":
            assert _moved(c, merge_mode="sum") >= 100, ("ave as sum", c.name)


@pytest.mark.parametrize("name", IDS)
def test_gates_are_off_saturation(name):
    case = RB.CASE_BY_NAME[name]
    x, layers, masks, _ = RB.case_inputs(case)
    _, state = RB.forward(x, layers, masks, case.res, case.merge)
    z = RB.gate_preactivations(state)
    assert (np.abs(z) < 4).mean() >= 0.9, float((np.abs(z) < 4).mean())


# ---------------------------------------------------------------------------------------------------
# host-only entry points
# ---------------------------------------------------------------------------------------------------
def _k_slices(k, rows=512):
    want = max(1, min(32, -(-k // rows)))
    chunk = -(-(-(-k // want)) // 32) * 32
    return -(-k // chunk)


def test_supported_workspace_and_tape_for_the_table_and_a_grid():
    from deepctr_amd import ops
    r4 = lambda n: (n + 3) // 4 * 4         # noqa: E731
    for c in RB.CASES:
        assert ops.bilstm_bwd_supported(c.T, c.Din, c.u, c.L, c.res, c.merge, route=c.route), c.name
        nd = 1 if c.merge in ("fw", "bw") else 2
        rows = c.T * c.B
        want = nd * r4(c.B * c.T * c.Din)
        for l in range(c.L):
            D = c.Din if l == 0 else c.u
            want += nd * (r4(rows * 4 * c.u) + r4(rows * (D + c.u)) + r4(_k_slices(rows) * (D + c.u + 1) * 4 * c.u))
        assert ops.bilstm_bwd_workspace_bytes(c.B, c.T, c.Din, c.u, c.L, c.res, c.merge, c.route) == 4 * want, c.name
    # the bounds the table stands on, read from the library: DSIN's own shape (T 5, two layers, Din = u)
    taken = [u for u in range(1, 100) if ops.bilstm_bwd_supported(5, u, u, 2)]
    resident = [u for u in range(1, 100) if ops.bilstm_bwd_supported(5, u, u, 2, route="resident")]
    assert taken == list(range(1, 65)) and resident == list(range(1, RB.STREAMED_U))
    assert all(ops.bilstm_bwd_supported(5, 64, 64, 2, route=r) for r in (None, "streamed"))
    assert ops.bilstm_bwd_supported(5, 16, 16, 2, route="streamed") and not ops.bilstm_bwd_supported(5, 16, 16, 2, route="workspace")
    for L in (1, 2, 3, 4):
        assert all(ops.bilstm_bwd_supported(3, 20, 24, L, res, mm) for res in range(L) for mm in RB.MERGES)
        assert ops.bilstm_bwd_supported(3, 24, 24, L, L)
    assert not ops.bilstm_bwd_supported(3, 8, 8, 5)                  # the grouped GEMM's eight groups: four layers
    assert not ops.bilstm_bwd_supported(3, 8, 8, 2, recurrent_activation="hard_sigmoid")
    assert not ops.bilstm_bwd_supported(200, 64, 64, 2) and ops.bilstm_bwd_workspace_bytes(64, 200, 64, 64, 2) == 0
    assert ops.bilstm_bwd_macs(5, 32, 32, 2) == 3 * ops.bilstm_macs(5, 32, 32, 2)


def _train_args(**kw):
    from deepctr_amd import _C
    fwd = dict(batch=4, x=16, x_stride=15, x_row_stride=5, seq_len=3, in_dim=5, units=4, n_layers=2, res_layers=0, merge_mode=4,
               recurrent_activation=0, route=0, out=16, out_stride=12, out_row_stride=4, out_bw=16, out_bw_stride=12, out_bw_row_stride=4)
    top = dict(tape=16, tape_bytes=2 * 2 * 3 * 2 * 4 * 4 * 4, d_out=16, d_out_stride=12, d_out_row_stride=4, d_out_bw=16, d_out_bw_stride=12,
               d_out_bw_row_stride=4, dx=16, dx_stride=15, dx_row_stride=5, workspace=16, workspace_bytes=1 << 30)
    for k, v in kw.items():
        (fwd if k in fwd or k == "layers" else top)[k] = v
    layers = (ctypes.c_void_p * 12)(*([16] * 12))
    t = _C.lstm.TrainArgs(**top)
    fwd.setdefault("layers", ctypes.cast(layers, ctypes.c_void_p))
    t.fwd = _C.lstm.Args(**fwd)
    t._keep = layers
    return t


def test_argument_errors_without_a_gpu():
    """Every refusal precedes the launch: these calls carry made-up pointers and run where no GPU exists."""
    from deepctr_amd import _C
    lib = _C.lib()
    b = lambda t: lib.dctr_bilstm_bwd(ctypes.byref(t), None)            # noqa: E731
    f = lambda t: lib.dctr_bilstm_train_fwd(ctypes.byref(t), None)      # noqa: E731
    assert lib.dctr_bilstm_bwd(None, None) == -1 and lib.dctr_bilstm_train_fwd(None, None) == -1
    assert lib.dctr_bilstm_bwd_supported(None) == 0 and lib.dctr_bilstm_bwd_workspace_bytes(None) == 0 and lib.dctr_bilstm_tape_bytes(None) == 0
    t = _train_args()
    assert lib.dctr_bilstm_tape_bytes(ctypes.byref(t.fwd)) == 2 * 2 * 3 * 2 * 4 * 4 * 4
    assert lib.dctr_bilstm_tape_bytes(ctypes.byref(_train_args(seq_len=0).fwd)) == 0
    for call in (b, f):
        assert call(_train_args(batch=0)) == 0                          # an empty batch: a no-op
        assert call(_train_args(x=None)) == -1 and call(_train_args(layers=None)) == -1
        assert call(_train_args(tape=None)) == -1 and call(_train_args(tape_bytes=100)) == -1
        assert call(_train_args(x_row_stride=4)) == -2 and call(_train_args(x_stride=14)) == -2
        assert call(_train_args(seq_len=0)) == -2 and call(_train_args(batch=-1)) == -2 and call(_train_args(n_layers=9)) == -2
        assert call(_train_args(res_layers=2)) == -2                    # a residual over layer 0 with in_dim != units
        assert call(_train_args(merge_mode=7)) == -4 and call(_train_args(recurrent_activation=2)) == -4 and call(_train_args(route=4)) == -4
        assert call(_train_args(route=3)) == _C.E_UNSUPPORTED
        wide = dict(units=65, in_dim=65, seq_len=5, x_row_stride=65, x_stride=325, out_row_stride=65, out_stride=325, d_out_row_stride=65,
                    d_out_stride=325, dx_row_stride=65, dx_stride=325)
        assert call(_train_args(**wide)) == _C.E_UNSUPPORTED
    assert b"bilstm_train_fwd" in lib.dctr_last_error()
    assert f(_train_args(out=None)) == -1 and f(_train_args(merge_mode=6, out_bw=None)) == -1
    assert f(_train_args(recurrent_activation=1, batch=0)) == 0         # the forward runs hard_sigmoid; the backward does not
    assert b(_train_args(recurrent_activation=1)) == _C.E_UNSUPPORTED and b(_train_args(n_layers=5)) == _C.E_UNSUPPORTED
    assert b"bilstm_bwd" in lib.dctr_last_error()
    assert b(_train_args(d_out=None)) == -1 and b(_train_args(merge_mode=6, d_out_bw=None)) == -1
    assert b(_train_args(workspace=None)) == -1 and b(_train_args(workspace_bytes=64)) == -1
    assert b(_train_args(d_out_stride=11)) == -2 and b(_train_args(d_out_row_stride=3)) == -2
    assert b(_train_args(merge_mode=5, out_row_stride=8, out_stride=24)) == -2                      # concat: d_out is [T, 2u]
    assert b(_train_args(merge_mode=6, d_out_bw_stride=11)) == -2
    assert b(_train_args(dx_stride=14)) == -2 and b(_train_args(dx_row_stride=4)) == -2
    assert b(_train_args(dx=None, dx_stride=0, dx_row_stride=0, batch=0)) == 0                      # ... which are read with dx only
    assert b(_train_args(max_blocks=-1)) == -2 and b(_train_args(accumulate=2)) == -4


def test_header_declares_the_entry_points_and_the_mirror_matches_the_c_layout(tmp_path):
    import shutil
    import subprocess
    from deepctr_amd import _C
    header = open(os.path.join(ROOT, "include", "dctr.h")).read()
    assert "#define DCTR_ABI_VERSION 13" in header and _C.ABI_VERSION == 13
    for sym, ret in (("dctr_bilstm_train_fwd", "int"), ("dctr_bilstm_bwd", "int"), ("dctr_bilstm_bwd_supported", "int"),
                     ("dctr_bilstm_bwd_workspace_bytes", "size_t")):
        assert re.search(r"\b%s %s\(const dctr_lstm_train_args_t\* args" % (ret, sym), header), sym
        assert _C.SYMBOLS[sym][1][0] == ctypes.POINTER(_C.lstm.TrainArgs)
    assert re.search(r"\bsize_t dctr_bilstm_tape_bytes\(const dctr_lstm_args_t\* args", header)
    assert "lstm_bwd_kernels.hip" in __import__("deepctr_amd.build", fromlist=["SOURCES"]).SOURCES
    assert "lstm_bwd_kernels.hip" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    structs = (("dctr_lstm_args_t", _C.lstm.Args), ("dctr_lstm_train_args_t", _C.lstm.TrainArgs))
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
@pytest.mark.parametrize("name", ["u12_D9_T2_B17_L2_r1_mul_all", "u16_D16_T5_B33_L3_r3_None_all", "u4_D7_T1_B1_L1_r0_fw_all"])
def test_bilstm_on_the_cpu_is_the_torch_loop(name, monkeypatch):
    from deepctr_amd import training
    case = RB.CASE_BY_NAME[name]
    x, layers, _, _ = RB.case_inputs(case)
    xt = torch.tensor(x, requires_grad=True)
    ws = [[torch.tensor(w, requires_grad=True) for w in layer] for layer in layers]
    assert training.HIP_AUTOGRAD_OPS is True and training.BILSTM_HIP_MIN_ROWS >= 0
    for switch in (True, False):
        monkeypatch.setattr(training, "HIP_AUTOGRAD_OPS", switch)
        for rate, train in ((0.0, False), (0.2, True)):
            torch.manual_seed(3)
            want = training._bilstm(xt, ws, case.res, case.merge, "sigmoid", rate, train)
            torch.manual_seed(3)
            got = training.bilstm(xt, ws, case.res, case.merge, "sigmoid", rate, train)
            for a, b in zip(*((got, want) if case.merge is None else ((got,), (want,)))):
                assert torch.equal(a, b) and a.grad_fn is not None
