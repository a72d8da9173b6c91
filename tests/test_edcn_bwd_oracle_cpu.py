"""The float64 oracle of dctr_edcn_bwd (tests/ref_edcn_bwd.py) against torch double autograd over _EDCN._autograd_logit's expression,
the float32 / float64 measurement that sets the GPU bar, the C layout of dctr_edcn_train_args_t, the host-only queries, every argument
error of the ABI and of ops.edcn_bwd before any launch, and the gate on the CPU.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import ref_edcn_bwd as RB
from tests.test_edcn_cpu import SWEEP, tower_case
from tests.util import load_golden, golden_meta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _torch_tower(case, F, d, bridge_type, par, act, bact):
    """_EDCN._autograd_logit's expression in float64 over the case's operands -> (leaves dict, tape [L, B, 3D], logit [B], out)."""
    t64 = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=True)       # noqa: E731
    D, L, off = F * d, len(case["dnn_kernels"]), case["off"]
    lv = dict(x=t64(case["xbuf"][:, off:off + D]), gates=[t64(g) for g in case["gates"]], cw=[t64(w) for w in case["cross_kernels"]],
              cb=[t64(b) for b in case["cross_biases"]], dw=[t64(w) for w in case["dnn_kernels"]], db=[t64(b) for b in case["dnn_biases"]],
              head=t64(case["head"]))
    if bridge_type == "concatenation":
        lv["bw"] = [t64(k) for k, _ in case["bridge_weights"]]
        lv["bb"] = [t64(b) for _, b in case["bridge_weights"]]
    f = (lambda v: torch.relu(v)) if act == "relu" else (lambda v: v)
    fb = (lambda v: torch.relu(v)) if bact == "relu" else (lambda v: v)
    x = lv["x"].reshape(-1, F, d)
    B = x.shape[0]
    gate = lambda g: torch.softmax(g * (1.0 / case["tau"]), dim=1)       # noqa: E731
    deep = (x * gate(lv["gates"][0])).reshape(B, D)
    cross = (x * gate(lv["gates"][1])).reshape(B, D)
    tape = []
    for i in range(L):
        w, b = lv["cw"][i], lv["cb"][i].reshape(-1)
        c = cross * (cross @ w) + b + cross if par == "vector" else cross * (cross @ w.t() + b) + cross
        h = f(deep @ lv["dw"][i] + lv["db"][i])
        if bridge_type == "pointwise_addition":
            br = c + h
        elif bridge_type == "hadamard_product":
            br = c * h
        else:
            br = fb(torch.cat([c, h], dim=-1) @ lv["bw"][i] + lv["bb"][i])
        tape.append(torch.cat([c, h, br], dim=-1))
        if i + 1 < L:
            b3 = br.reshape(B, F, d)
            deep = (b3 * gate(lv["gates"][2 * i + 2])).reshape(B, D)
            cross = (b3 * gate(lv["gates"][2 * i + 3])).reshape(B, D)
    out = tape[-1]
    return lv, torch.stack(tape).detach().numpy(), (out @ lv["head"]).reshape(-1), out


def _autograd(case, F, d, bridge_type, par, act, bact, d_logit, d_out):
    lv, tape, logit, out = _torch_tower(case, F, d, bridge_type, par, act, bact)
    D = F * d
    loss = 0.0
    if d_logit is not None:
        loss = loss + (logit * torch.tensor(d_logit, dtype=torch.float64)).sum()
    if d_out is not None:
        loss = loss + (out * torch.tensor(d_out[:, :3 * D], dtype=torch.float64)).sum()
    loss.backward()
    g = lambda t: None if t.grad is None else t.grad.numpy()       # noqa: E731
    res = dict(dx=g(lv["x"]), d_gates=[g(t) for t in lv["gates"]], d_cross_w=[g(t) for t in lv["cw"]], d_cross_b=[g(t) for t in lv["cb"]],
               d_dnn_w=[g(t) for t in lv["dw"]], d_dnn_b=[g(t) for t in lv["db"]], d_head_w=g(lv["head"]) if d_logit is not None else None)
    if "bw" in lv:
        res["d_bridge_w"], res["d_bridge_b"] = [g(t) for t in lv["bw"]], [g(t) for t in lv["bb"]]
    return res, tape


@pytest.mark.parametrize("seed_kind", ["d_logit", "d_out", "both"])
@pytest.mark.parametrize("act", ["relu", "linear"])
@pytest.mark.parametrize("par", ["vector", "matrix"])
@pytest.mark.parametrize("bridge_type", RB.BRIDGES_BWD)
def test_oracle_matches_torch_double_autograd(bridge_type, par, act, seed_kind):
    """1e-12 of max(result, magnitude), F in {1, 2, 3, 9}, d in {1, 4, 5}, L in {1, 3}; the magnitudes bound the result."""
    for k, (F, d, L, B) in enumerate(((1, 1, 1, 4), (2, 4, 3, 7), (3, 5, 1, 6), (9, 4, 3, 5), (9, 1, 3, 3))):
        case = tower_case(F, d, L, B, bridge_type, par, 3, 0.5 if k % 2 else 1.0, 10 * k + 1)
        dl, do = RB.seeds(case, F, d, k)
        dl, do = (dl if seed_kind != "d_out" else None), (do if seed_kind != "d_logit" else None)
        ref, tape = _autograd(case, F, d, bridge_type, par, act, act, dl, do)
        got = RB.oracle(case, F, d, tape, bridge_type, par, act, act, d_logit=dl, d_out=do)
        mag = RB.oracle(case, F, d, tape, bridge_type, par, act, act, d_logit=dl, d_out=do, absolute=True)
        names = [n for n, _ in RB.flatten(got)]
        assert names == [n for n, _ in RB.flatten(ref)] and names == [n for n, _ in RB.flatten(mag)]
        assert ("d_head_w" in names) == (dl is not None) and ("d_bridge_w[0]" in names) == (bridge_type == "concatenation")
        for (n, a), (_, r), (_, m) in zip(RB.flatten(got), RB.flatten(ref), RB.flatten(mag)):
            assert a.shape == r.shape == m.shape, n
            assert (np.abs(a - r) <= 1e-12 * np.maximum(np.abs(r), m)).all(), (n, F, d, L)
            assert (np.abs(a) <= m * (1 + 1e-12)).all(), n


def test_sweep_is_the_forward_sweep_without_the_layered_row():
    from deepctr_amd import ops
    assert RB.SWEEP_BWD == [s for s in SWEEP if s[0] * s[1] != 1024]
    F = RB.SWEEP_BWD[-1][0]
    assert RB.SWEEP_BWD[-1][1] == 16 and ops.edcn_bwd_supported(F, 16, 4) and not ops.edcn_bwd_supported(F + 1, 16, 4)


def test_float32_backward_against_float64_sets_the_bar():
    """The float32 run of the oracle against its float64 run over SWEEP_BWD x bridges x parameterizations x relu / linear, both seeds:
    the worst error as a share of the summed magnitude.  Measured 7.79e-7 (printed below); BWD_RTOL_TERMS is twice that rounded up to one
    digit, and this test holds the constant to the rule."""
    worst = 0.0
    for (F, d, L, B) in RB.SWEEP_BWD:
        for bridge_type in RB.BRIDGES_BWD:
            for par in ("vector", "matrix"):
                for act in ("relu", "linear"):
                    case = tower_case(F, d, L, B, bridge_type, par, 3, 0.5, F * 100 + d)
                    tape = RB.tower_tape(case, F, d, bridge_type, par, act, act).astype(np.float32)
                    dl, do = RB.seeds(case, F, d)
                    kw = dict(d_logit=dl, d_out=do)
                    r64 = RB.flatten(RB.oracle(case, F, d, tape, bridge_type, par, act, act, **kw))
                    r32 = RB.flatten(RB.oracle(case, F, d, tape, bridge_type, par, act, act, dtype=np.float32, **kw))
                    mag = RB.flatten(RB.oracle(case, F, d, tape, bridge_type, par, act, act, absolute=True, **kw))
                    for (n, a), (_, b), (_, m) in zip(r32, r64, mag):
                        assert a.dtype == np.float32, n
                        share = float((np.abs(a.astype(np.float64) - b) / (m + 1e-300)).max())
                        worst = max(worst, share)
    print("float32 oracle vs float64: worst error %.3g of the summed magnitude" % worst)
    digit = 10.0 ** np.floor(np.log10(2 * worst))
    assert 0 < worst and abs(RB.BWD_RTOL_TERMS - np.ceil(2 * worst / digit) * digit) <= 1e-9 * digit, "twice the measurement, one digit, rounded up"


def test_header_declares_the_train_entry_points_and_the_mirror_matches_the_c_layout(tmp_path):
    import shutil
    import subprocess
    from deepctr_amd import _C
    header = open(os.path.join(ROOT, "include", "dctr.h")).read()
    assert "#define DCTR_ABI_VERSION 13" in header and _C.ABI_VERSION == 13              # no existing struct changed
    for sym in ("dctr_edcn_train_fwd", "dctr_edcn_bwd", "dctr_edcn_bwd_supported", "dctr_edcn_bwd_workspace_bytes", "dctr_edcn_tape_bytes"):
        assert re.search(r"\b(int|size_t) %s\(const dctr_edcn_train_args_t\* args" % sym, header), sym
        assert _C.SYMBOLS[sym][1][0] == ctypes.POINTER(_C.edcn.TrainArgs), sym
    assert "edcn_bwd_kernels.hip" in __import__("deepctr_amd.build", fromlist=["SOURCES"]).SOURCES
    assert os.path.exists(os.path.join(ROOT, "deepctr_amd", "csrc", "edcn_device.h"))
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    cls, cname = _C.edcn.TrainArgs, "dctr_edcn_train_args_t"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dctr.h"', "int main(void) {",
             '    printf("sizeof %%zu\\n", sizeof(%s));' % cname]
    for fname, _ in cls._fields_:
        lines.append('    printf("%s %%zu\\n", offsetof(%s, %s));' % (fname, cname, fname))
    lines += ["    return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    seen = 0
    for line in filter(None, out):
        field, val = line.split()
        want = ctypes.sizeof(cls) if field == "sizeof" else getattr(cls, field).offset
        assert int(val) == want, "%s: C says %s, ctypes %d" % (field, val, want)
        seen += 1
    assert seen == 1 + len(cls._fields_)


def test_host_only_queries():
    from deepctr_amd import ops
    for bridge_type in RB.BRIDGES_BWD:
        for par in ("vector", "matrix"):
            for act in ("relu", "linear"):
                assert ops.edcn_bwd_supported(26, 16, 2, bridge_type, par, act, act), (bridge_type, par, act)
    assert ops.edcn_bwd_supported(1, 1) and ops.edcn_bwd_supported(39, 16, 32)
    assert not ops.edcn_bwd_supported(64, 16)                                            # D = 1024: past the LDS plan
    assert not ops.edcn_bwd_supported(40, 16) and not ops.edcn_bwd_supported(39, 16, 33)
    assert not ops.edcn_bwd_supported(26, 16, 2, "attention_pooling")
    for act in ("dice", "sigmoid", "tanh", "prelu"):
        assert not ops.edcn_bwd_supported(26, 16, 2, activation=act), act
    assert not ops.edcn_bwd_supported(26, 16, 2, "concatenation", bridge_activation="sigmoid")
    assert ops.edcn_bwd_supported(26, 16, 2, "hadamard_product", bridge_activation="sigmoid")        # (no Dense in that bridge)
    assert not ops.edcn_bwd_supported(26, 16, 2, bn=True)
    assert not ops.edcn_bwd_supported(0, 16) and not ops.edcn_bwd_supported(3, 4, 0) and not ops.edcn_bwd_supported(3, 4, 1, "sum")
    assert ops.edcn_tape_bytes(130, 26, 16, 2) == 2 * 130 * 3 * 416 * 4 and ops.edcn_tape_bytes(0, 3, 4, 2) == 0
    # the workspace: gates + 256 rows of column sums (+ the rows' operands and S slices of [D, D] partials with the weight gradients)
    D, L, B = 12, 2, 100
    r16 = lambda n: (n + 15) // 16 * 16       # noqa: E731
    small = r16(L * 2 * 3 * 4) + r16(256 * (L * 6 * D + 3 * D) * 4)
    assert ops.edcn_bwd_workspace_bytes(B, 3, 4, L, weights=False) == small
    assert ops.edcn_bwd_workspace_bytes(B, 3, 4, L) == small + r16(L * B * D * 4) + 1 * L * 1 * D * D * 4
    assert ops.edcn_bwd_workspace_bytes(B, 3, 4, L, "concatenation", "matrix", slices=3) == small + r16(L * B * 3 * D * 4) + 3 * L * 4 * D * D * 4
    assert ops.edcn_bwd_workspace_bytes(1000, 3, 4, L) == small + r16(L * 1000 * D * 4) + 4 * L * D * D * 4      # 256 rows a slice
    assert ops.edcn_bwd_workspace_bytes(B, 64, 16, L) == 0 and ops.edcn_bwd_workspace_bytes(B, 3, 4, L, "attention_pooling") == 0


def _abi(**kw):
    from deepctr_amd import _C
    fwd = dict(batch=4, x_stride=15, x_offset=3, fields=3, dim=4, cross_num=2, mode=0, bridge=1, activation=1, bridge_activation=1, inv_tau=2.0)
    top = {}
    own = set(n for n, _ in _C.edcn.TrainArgs._fields_) - {"fwd"}
    for k, v in kw.items():
        (top if k in own else fwd)[k] = v
    t = _C.edcn.TrainArgs(**top)
    t.fwd = _C.edcn.Args(**fwd)
    return t


def test_abi_argument_errors_without_a_gpu():
    from deepctr_amd import _C
    lib = _C.lib()
    f = lambda t: lib.dctr_edcn_bwd(ctypes.byref(t), None)       # noqa: E731
    ptrs = (ctypes.c_void_p * 4)(16, 16, 16, 16)
    arr = ctypes.cast(ptrs, ctypes.c_void_p)
    full = dict(x=16, gates=arr, cross_w=arr, cross_b=arr, dnn_w=arr, dnn_b=arr, head_w=16, tape=16, d_logit=16, workspace=16,
                workspace_bytes=1 << 30)
    assert lib.dctr_edcn_bwd(None, None) == -1 and lib.dctr_edcn_train_fwd(None, None) == -1
    assert lib.dctr_edcn_bwd_supported(None) == 0 and lib.dctr_edcn_bwd_workspace_bytes(None) == 0 and lib.dctr_edcn_tape_bytes(None) == 0
    assert f(_abi()) == -1 and b"edcn_bwd" in lib.dctr_last_error()                  # pointers missing
    for k, v in (("fields", 0), ("dim", 0), ("cross_num", 0), ("batch", -1), ("x_stride", 14), ("x_offset", -1), ("slices", -1), ("slices", 257)):
        assert f(_abi(**dict(full, **{k: v}))) == -2, k
    for k, v in (("mode", 2), ("bridge", 4), ("activation", 5), ("bridge_activation", -1), ("route", 3), ("accumulate", 2)):
        assert f(_abi(**dict(full, **{k: v}))) == -4, k
    assert f(_abi(**dict(full, inv_tau=float("nan")))) == -2
    for k in ("x", "gates", "cross_w", "cross_b", "dnn_w", "dnn_b", "tape", "workspace"):
        a = dict(full)
        del a[k]
        assert f(_abi(**a)) == -1, k
    assert f(_abi(**dict(full, d_logit=None))) == -1                                  # neither seed
    assert f(_abi(**dict(full, head_w=None))) == -1                                   # d_logit without head_w
    assert f(_abi(**dict(full, d_logit=None, d_out=16, d_out_stride=36, d_head_w=16))) == -1      # d_head_w without d_logit
    assert f(_abi(**dict(full, d_out=16, d_out_stride=35))) == -2                     # 3 D = 36 columns do not fit
    assert f(_abi(**dict(full, dx=16, dx_stride=11))) == -2 and f(_abi(**dict(full, dx=16, dx_stride=14, dx_offset=3))) == -2
    assert f(_abi(**dict(full, dx=16, dx_stride=12, dx_offset=-1))) == -2
    assert f(_abi(**dict(full, bridge=2))) == -1                                      # concatenation without its weights
    assert f(_abi(**dict(full, d_bridge_w=arr))) == -1                                # a bridge gradient without the Dense bridge
    assert f(_abi(**dict(full, tape=20))) == -3 and f(_abi(**dict(full, workspace=20))) == -3         # alignment
    assert f(_abi(**dict(full, workspace_bytes=64))) == -1                            # too small a workspace
    for bad in (dict(bridge=3), dict(activation=4), dict(activation=2), dict(route=2), dict(fields=64, dim=16, x_stride=1027),
                dict(cross_num=33), dict(bn_scale=arr, bn_shift=arr)):
        assert f(_abi(**dict(full, **bad))) == -5, bad
        assert lib.dctr_edcn_train_fwd(ctypes.byref(_abi(**dict(full, logit=16, **bad))), None) == -5, bad
    assert lib.dctr_edcn_train_fwd(ctypes.byref(_abi(**dict(full, logit=16, tape=None))), None) == -1
    assert lib.dctr_edcn_train_fwd(ctypes.byref(_abi(**dict(full, logit=16, tape=20))), None) == -3
    assert lib.dctr_edcn_train_fwd(ctypes.byref(_abi(**dict(full, logit=None))), None) == -1
    assert lib.dctr_edcn_train_fwd(ctypes.byref(_abi(**dict(full, logit=16, batch=0, tape=None))), None) == 0     # empty batch: a no-op
    assert f(_abi(**dict(full, batch=0, workspace=None))) == 0


def _cpu_case(bridge_type="concatenation", par="vector"):
    case = tower_case(3, 4, 2, 5, bridge_type, par, 3, 0.5, 1)
    t = lambda a: torch.from_numpy(a)       # noqa: E731
    args = [t(case["xbuf"]), 3, 4, [t(a) for a in case["gates"]], [t(a) for a in case["cross_kernels"]], [t(a) for a in case["cross_biases"]],
            [t(a) for a in case["dnn_kernels"]], [t(a) for a in case["dnn_biases"]]]
    kw = dict(bridge_type=bridge_type, parameterization=par, tau=0.5, x_offset=3, head_w=t(case["head"]))
    if bridge_type == "concatenation":
        kw["bridge_weights"] = [(t(k), t(b)) for k, b in case["bridge_weights"]]
    return args, kw


def test_ops_argument_errors_before_any_launch():
    from deepctr_amd import _C, ops
    args, kw = _cpu_case()
    tape = torch.zeros(2, 5, 36)
    dl = torch.zeros(5)
    bwd = lambda a=args, tp=tape, **more: ops.edcn_bwd(*a, tp, **dict(kw, **more))       # noqa: E731
    with pytest.raises(ValueError, match="d_logit, d_out or both"):
        bwd()
    with pytest.raises(ValueError, match="tape"):
        bwd(tp=torch.zeros(2, 5, 35), d_logit=dl)
    with pytest.raises(ValueError, match="tape"):
        bwd(tp=None, d_logit=dl)
    with pytest.raises(ValueError, match="d_logit"):
        bwd(d_logit=torch.zeros(4))
    with pytest.raises(ValueError, match="head_w"):
        bwd(d_logit=dl, head_w=None)
    with pytest.raises(ValueError, match="d_out"):
        bwd(d_out=torch.zeros(5, 35))
    with pytest.raises(ValueError, match="d_head_w needs d_logit"):
        bwd(d_out=torch.zeros(5, 36), d_head_w=True)
    with pytest.raises(ValueError, match="slices"):
        bwd(d_logit=dl, slices=257)
    with pytest.raises(ValueError, match="dx"):
        bwd(d_logit=dl, dx=torch.zeros(5, 14), dx_offset=3)
    with pytest.raises(ValueError, match="d_dnn_w takes 2 entries"):
        bwd(d_logit=dl, d_dnn_w=[torch.zeros(12, 12)])
    with pytest.raises(ValueError, match=r"d_gates\[1\]"):
        bwd(d_logit=dl, d_gates=[torch.zeros(3), torch.zeros(4), None, None])
    with pytest.raises(ValueError, match="rounds take"):
        bwd(a=args[:3] + [args[3][:3]] + args[4:], d_logit=dl)
    with pytest.raises(ValueError, match="bridge_weights"):
        bwd(d_logit=dl, bridge_weights=None)
    with pytest.raises(ValueError, match="not what dctr_edcn_bwd takes"):
        bwd(d_logit=dl, activation="sigmoid")
    with pytest.raises(ValueError, match="bridge_type"):
        bwd(d_logit=dl, bridge_type="sum")
    a2, kw2 = _cpu_case("hadamard_product")
    with pytest.raises(ValueError, match="concatenation bridge only"):
        ops.edcn_bwd(*a2, tape, d_logit=dl, d_bridge_b=True, **kw2)
    with pytest.raises(ValueError, match="tape"):
        ops.edcn_train(*args, tape=torch.zeros(2, 5, 35), **kw)
    with pytest.raises(ValueError, match="head_w"):
        ops.edcn_train(*args, logit=True, **dict(kw, head_w=None))
    # well-formed calls reach the device check: there is no CPU path
    with pytest.raises(_C.DctrExtensionError):
        bwd(d_logit=dl, dx=True, d_gates=True, d_dnn_w=True)
    with pytest.raises(_C.DctrExtensionError):
        ops.edcn_train(*args, **kw)


def test_gate_is_false_on_the_cpu_and_the_torch_ops_are_unchanged(monkeypatch):
    from deepctr_amd import ops, training as tops
    from tests.test_edcn_cpu import build_model
    g = load_golden("model_edcn_cat_vec")
    meta = golden_meta(g)
    model = build_model(meta, "cpu")
    F, d = model.n_fields, model.emb_dim
    torch.manual_seed(0)
    parts = [torch.randn(7, d) for _ in range(F)]
    assert 0 <= tops.EDCN_HIP_MIN_ROWS <= tops.EDCN_HIP_MAX_ROWS and tops.HIP_AUTOGRAD_OPS
    assert not tops._edcn_on_hip(model, torch.stack(parts, dim=1), True)
    calls = []
    monkeypatch.setattr(ops.EDCNTowerFunction, "apply", lambda *a: calls.append(a))
    got = model._autograd_logit(None, 0, 7, parts, None, True)
    monkeypatch.undo()
    # the same expression with the gate taken out of the way: the same bits
    monkeypatch.setattr(tops, "_edcn_on_hip", lambda model, x, training: False)
    again = model._autograd_logit(None, 0, 7, parts, None, True)
    assert not calls and got.shape == (7,) and torch.equal(got, again)
    lv_case = dict(xbuf=torch.stack(parts, dim=1).reshape(7, F * d).numpy(), off=0, tau=model.tau,
                   gates=[r.g.detach().numpy() for r in model.regulations],
                   cross_kernels=[c.w("kernel0").detach().numpy() for c in model.cross_layers],
                   cross_biases=[c.w("bias0").detach().numpy() for c in model.cross_layers],
                   dnn_kernels=[dn.w("kernel0").detach().numpy() for dn in model.dnn_layers],
                   dnn_biases=[dn.w("bias0").detach().numpy() for dn in model.dnn_layers],
                   bridge_weights=[tuple(t.detach().numpy() for t in b.weights_for_op()) for b in model.bridges],
                   head=model.dense.w("kernel").detach().numpy())
    _, _, logit, _ = _torch_tower(lv_case, F, d, "concatenation", "vector", model.dnn_layers[0].activation, model.bridges[0].activation)
    np.testing.assert_allclose(got.detach().numpy(), logit.detach().numpy(), rtol=1e-4, atol=1e-5)
