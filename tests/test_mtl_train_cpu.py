"""CPU: the multi-task models' HIP training step (DESIGN.md §4.15 "Training") as far as it can be checked without a GPU — the NumPy
oracle of dctr_mtl_mix_bwd / dctr_mtl_loss_grad (tests/ref_mtl_bwd.py) against torch autograd in float64 over the models' own
restatement, the float32-vs-float64 run that sets the bar of the GPU op test, the argument checks of the three entry points (no launch),
the header, what training_hip.supported answers, what HipTrainer registers, and the seeds of the GPU mini-fuzz."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import ref_mtl_bwd as RB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (B, E, H, dz, members): the sweep of tests/test_gpu_mtl_train.py::test_mix_bwd_vs_float64_oracle
MIX_SWEEP = [
    (1, 1, 1, 1, [[0]]),                                        # n_g = 1: ds is exactly 0
    (5, 3, 17, 5, [[0, 1, 2], [0, 1, 2]]),                      # an expert in several gates
    (67, 4, 70, 65, [[0, 3], [1, 3], [3]]),                     # expert 2 in no gate: zero dh columns; widths past one wave
    (130, 9, 8, 130, [[g, (g + 1) % 9, (g + 4) % 9] for g in range(9)]),      # more than eight gates: two launches, dh summed over both
    (33, 3, 64, 64, [[2, 0, 1]]),                               # a permuted member list
    (9, 10, 5, 7, [list(range(10)), [9, 3, 3, 0, 1, 2, 4, 5, 6, 7, 8]]),      # more than eight members: the kernel's two-sweep form; a repeated one
    (70, 8, 130, 3, [list(range(8))]),                          # eight members: the widest register form, H past two waves
]


def mix_case(B, E, H, dz, members, seed):
    """Seeded float32 operands of ops.mtl_mix_bwd / RB.mix_bwd: h [B, E * H], z[g] [B, dz], d_out [B, G * H], gate kernels
    N(0, 4 / dz): gate logits of standard deviation 1, a few units at most.  (A float32 softmax carries the rounding of l - max, eps * |l|,
    into every weight as a RELATIVE error: with N(0, 1) kernels the logits of the dz = 130 case reach 19 and a lone small p_j d_out term of
    dh sits 1.8e-6 of itself off in float32 NumPy too — a property of the number format at that logit scale, not of a summation order,
    and nothing the summed-magnitude term is meant to absorb.)"""
    rng = np.random.RandomState(seed)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)      # noqa: E731
    G = len(members)
    return dict(h=f32(rng.standard_normal((B, E * H))), z=[f32(rng.standard_normal((B, dz)) * 0.5) for _ in range(G)],
                gate_kernels=[f32(rng.standard_normal((dz, len(ms))) * 2.0 / np.sqrt(dz)) for ms in members], d_out=f32(rng.standard_normal((B, G * H))))


def _cols(F=5, E=8, dense=2):
    from deepctr_amd.feature_column import DenseFeat, SparseFeat, VarLenSparseFeat
    cols = []
    for k in range(F):
        if k % 3 == 2:
            cols.append(VarLenSparseFeat(SparseFeat("S%d" % k, 9 + k, E), maxlen=4, combiner=("mean", "sum")[k % 2]))
        else:
            cols.append(SparseFeat("C%d" % k, 20 + 3 * k, E))
    return cols + [DenseFeat("D%d" % k, 1) for k in range(dense)]


def _feed(rng, cols, n):
    from tests.test_gpu_mtl import _fuzz_feed
    return _fuzz_feed(rng, cols, n)


MODELS = {
    "MMOE": dict(num_experts=3, expert_dnn_hidden_units=(16, 8), gate_dnn_hidden_units=(6,), tower_dnn_hidden_units=(8,)),
    "PLE": dict(num_levels=2, shared_expert_num=1, specific_expert_num=1, expert_dnn_hidden_units=(16,), tower_dnn_hidden_units=(8,)),
    "SharedBottom": dict(bottom_dnn_hidden_units=(16, 8), tower_dnn_hidden_units=(8,), task_types=("binary", "regression")),
    "ESMM": dict(tower_dnn_hidden_units=(16, 8)),
}


def build(kind, device="cpu", seed=0, cols=None, **more):
    from deepctr_amd import models
    from tests.test_gpu_models import _randomise
    rng = np.random.RandomState(seed)
    cols = _cols() if cols is None else cols
    model = getattr(models, kind)(cols, device=device, **dict(MODELS[kind], **more))
    w = _randomise(model, rng)
    w = {k: (rng.standard_normal(v.shape).astype(np.float32) if "gate_softmax" in k else v) for k, v in w.items()}
    model.set_weights_by_name(w)
    return model, cols, w


def _staged(model, feed, n):
    from deepctr_amd import engine
    staged = engine.Staged(n)
    model._stage_inputs(feed, staged)
    model._begin()
    return staged


@pytest.mark.parametrize("kind", sorted(MODELS))
def test_loss_oracle_matches_autograd_in_float64(kind):
    """d (sum_t w_t loss_t) / d logit_t, the reported losses and the bias gradients of RB.loss_grad against autograd over
    _fit.task_losses on the model's own logits in float64 — with a row in ESMM's clipped region and one at the upper clip."""
    from deepctr_amd.models.multitask import _fit
    model, cols, _ = build(kind)
    weights = [1.0, 0.5]
    model.compile("sgd", loss_weights=weights)
    rng = np.random.RandomState(5)
    n = 40
    staged = _staged(model, _feed(rng, cols, n), n)
    with torch.no_grad():
        logits = [l.double() * 8.0 for l in model.autograd_logits(staged, 0, n)]
    logits[0][:2], logits[1][:2] = torch.tensor([-20.0, 20.0]).double(), torch.tensor([-20.0, 20.0]).double()
    leaves = [l.clone().requires_grad_(True) for l in logits]
    binary = [t == "binary" for t in model.task_types]
    ys = torch.from_numpy(np.stack([(rng.rand(n) < 0.5).astype(np.float64) if b else rng.standard_normal(n) for b in binary]))
    pairs = _fit.task_losses(model, leaves, ys)
    sum(w * l for w, (l, _) in zip(weights, pairs)).backward()
    pred = np.stack([(torch.sigmoid(l) if b else l).detach().numpy() for l, b in zip(leaves, binary)])
    dl, loss, dbias = RB.loss_grad(pred, ys.numpy(), model._compiled["loss"], binary, weights, esmm=model.esmm)
    for t in range(2):
        g = leaves[t].grad.numpy()
        assert np.abs(dl[t] - g).max() <= 1e-10 * max(1.0, float(np.abs(g).max())), (kind, t)
        assert abs(loss[t] / n - float(pairs[t][1])) <= 1e-10 * max(1.0, abs(float(pairs[t][1])))
        assert abs(dbias[t] - g.sum()) <= 1e-10
    if model.esmm:
        assert dl[1][0] == 0.0 and dl[1][1] == 0.0 and leaves[1].grad[0] == 0 and leaves[1].grad[1] == 0        # outside the clip range
        assert (np.abs(dl[1][2:]) > 0).all()


@pytest.mark.parametrize("kind", ["MMOE", "PLE"])
def test_mix_oracle_matches_autograd_in_float64(kind):
    """RB.mix_bwd against autograd over the mixture as MultiTaskModel.autograd_logits writes it, on every level of the model, from the
    model's own expert outputs, gate inputs and gate kernels in float64: dh, ds, dz and dWg to 1e-10."""
    from deepctr_amd import training as tops
    model, cols, _ = build(kind)
    rng = np.random.RandomState(6)
    n = 23
    staged = _staged(model, _feed(rng, cols, n), n)
    with torch.no_grad():
        parts, _e, _l, _f = tops.stage_forward(model.stage_plan, staged, 0, n)
        xs = [torch.cat(parts, dim=-1)]
        for lv in model.levels:
            src = lambda s: xs[s if len(xs) > 1 else 0]      # noqa: E731
            H = lv.experts[0].hidden_units[-1]
            hs = [tops.dnn_forward(d, src(s), True).double() for d, s in zip(lv.experts, lv.expert_src)]
            zs = [tops.dnn_forward(gd, src(s), True).double() for gd, s in zip(lv.gate_dnns, lv.gate_src)]
            ws = [g.w("kernel").double() for g in lv.gate_dense]
            with torch.enable_grad():
                hl, zl, wl = ([t.clone().requires_grad_(True) for t in ts] for ts in (hs, zs, ws))
                ls = [z @ w for z, w in zip(zl, wl)]
                for l in ls:
                    l.retain_grad()
                outs = [(torch.stack([hl[m] for m in ms], dim=1) * torch.softmax(l, dim=-1).unsqueeze(-1)).sum(1) for l, ms in zip(ls, lv.members)]
                d_out = torch.from_numpy(rng.standard_normal((n, len(outs) * H)))
                (torch.cat(outs, dim=-1) * d_out).sum().backward()
            ref = RB.mix_bwd(torch.cat(hs, dim=-1).numpy(), H, [z.numpy() for z in zs], [w.numpy() for w in ws], lv.members, d_out.numpy())
            close = lambda a, b: np.abs(a - b).max() <= 1e-10 * max(1.0, float(np.abs(b).max()))      # noqa: E731
            zero = torch.zeros(n, H).double()
            assert close(ref["dh"], torch.cat([zero if t.grad is None else t.grad for t in hl], dim=-1).numpy())
            assert close(ref["ds"], torch.cat([l.grad for l in ls], dim=-1).numpy())
            assert close(ref["logits"], torch.cat(ls, dim=-1).detach().numpy())
            for g in range(len(ls)):
                assert close(ref["dz"][g], zl[g].grad.numpy()) and close(ref["dWg"][g], wl[g].grad.numpy())
            xs = [o.detach().float() for o in outs]


def test_float32_oracle_against_float64_sets_the_bar():
    """The float32 NumPy run of mix_bwd against the float64 run over the GPU op test's own sweep: the worst error of dh and ds in units
    of the summed magnitude, times two (the kernel sums the wave's partial products in another order) and rounded up, is
    RB.OP_RTOL_TERMS = 1.4e-6 (6.66e-7 when the bar was set).  Asserted with room for another BLAS — the float32 run passes the bar, and
    the bar is within 4x of it — and at or below assert_close_terms' default."""
    worst = 0.0
    for i, (B, E, H, dz, members) in enumerate(MIX_SWEEP):
        case = mix_case(B, E, H, dz, members, 300 + i)
        args = (case["h"], H, case["z"], case["gate_kernels"], members, case["d_out"])
        o64, o32, mag = RB.mix_bwd(*args), RB.mix_bwd(*args, dtype=np.float32), RB.mix_bwd(*args, absolute=True)
        for k in ("dh", "ds"):
            err, m = np.abs(o32[k].astype(np.float64) - o64[k]), mag[k]
            assert (err[m == 0] == 0).all()
            worst = max(worst, float((err[m > 0] / m[m > 0]).max()))
        if len(members[0]) == 1 and len(members) == 1:
            assert (o64["ds"] == 0).all() and (o32["ds"] == 0).all()
        if E == 4:
            assert (o64["dh"][:, 2 * H:3 * H] == 0).all() and (mag["dh"][:, 2 * H:3 * H] == 0).all()
    print("float32 vs float64 mix_bwd: worst error / summed magnitude = %.3g" % worst)
    assert worst <= RB.OP_RTOL_TERMS <= 4 * worst, worst
    assert RB.OP_RTOL_TERMS <= 2e-6


def test_magnitude_mode_bounds_the_plain_run():
    B, E, H, dz, members = MIX_SWEEP[2]
    case = mix_case(B, E, H, dz, members, 9)
    args = (case["h"], H, case["z"], case["gate_kernels"], members, case["d_out"])
    o, mag = RB.mix_bwd(*args), RB.mix_bwd(*args, absolute=True)
    for k in ("dh", "ds"):
        assert (mag[k] >= np.abs(o[k])).all()
    for g in range(len(members)):
        assert (mag["dz"][g] >= np.abs(o["dz"][g])).all() and (mag["dWg"][g] >= np.abs(o["dWg"][g])).all()


def test_abi_argument_errors_without_a_gpu():
    from deepctr_amd import _C
    lib = _C.lib()
    cast = lambda p: ctypes.cast(p, ctypes.c_void_p)      # noqa: E731
    arr = cast((ctypes.c_void_p * 17)(*([16] * 17)))
    i64 = cast((ctypes.c_int64 * 17)(*([4] * 17)))
    gn, mem = (ctypes.c_int32 * 2)(2, 1), (ctypes.c_int32 * 3)(0, 1, 1)
    # (batch = 0: whatever the checks let through returns before a launch — this file also runs where a GPU is present)
    good = dict(batch=0, h=16, h_stride=6, n_experts=2, width=3, n_gates=2, z_dim=4, z=arr, z_stride=i64, gate_kernel=arr, gate_n=cast(gn),
                members=cast(mem), members_dev=16, d_out=16, d_out_stride=6, d_out_offset=0, dh=16, dh_stride=6, ds=16, ds_stride=3,
                logits=None, logits_stride=0)
    mix = lambda **kw: lib.dctr_mtl_mix_bwd(ctypes.byref(_C.mtl.MixBwdArgs(**dict(good, **kw))), None)      # noqa: E731
    assert lib.dctr_mtl_mix_bwd(None, None) == -1 and mix() == 0 and mix(logits=16, logits_stride=3) == 0
    for k in ("h", "z", "z_stride", "gate_kernel", "gate_n", "members", "members_dev", "d_out", "dh", "ds"):
        assert mix(**{k: None}) == -1, k
    assert mix(gate_n=cast((ctypes.c_int32 * 2)(2, 0))) == -2 and b"gate_n" in lib.dctr_last_error()          # n_g = 0
    assert mix(members=cast((ctypes.c_int32 * 3)(0, 2, 1))) == -2 and b"member" in lib.dctr_last_error()      # a member index >= E
    assert mix(members=cast((ctypes.c_int32 * 3)(0, -1, 1))) == -2
    assert mix(d_out_offset=-1) == -2 and mix(d_out_offset=1) == -2 and mix(d_out_stride=-6) == -2 and mix(h_stride=-6) == -2
    assert mix(dh_stride=5) == -2 and mix(ds_stride=2) == -2 and mix(logits=16, logits_stride=2) == -2 and mix(batch=-1) == -2
    assert mix(z_stride=cast((ctypes.c_int64 * 2)(4, -4))) == -2 and mix(width=0) == -2 and mix(z_dim=5) == -2
    # dctr_mtl_loss_grad
    kinds = lambda *v: cast((ctypes.c_int32 * len(v))(*v))      # noqa: E731
    w = cast((ctypes.c_float * 3)(1.0, 0.5, 2.0))
    lgood = dict(batch=0, n_tasks=2, esmm=0, pred=16, pred_stride=0, y=16, y_stride=0, loss_kind=kinds(0, 1), binary=kinds(1, 0), loss_weight=w,
                 dlogit=16, dlogit_stride=0, loss_sum=16, dbias=None)
    lg = lambda **kw: lib.dctr_mtl_loss_grad(ctypes.byref(_C.mtl.LossArgs(**dict(lgood, **kw))), None)      # noqa: E731
    assert lib.dctr_mtl_loss_grad(None, None) == -1 and lg() == 0 and lg(dbias=arr) == 0
    for k in ("pred", "y", "loss_kind", "binary", "loss_weight", "dlogit", "loss_sum"):
        assert lg(**{k: None}) == -1, k
    assert lg(loss_kind=kinds(0, 2)) == -4 and b"unknown loss kind" in lib.dctr_last_error()
    assert lg(loss_kind=kinds(-1, 1)) == -4 and lg(esmm=2) == -4
    assert lg(loss_kind=kinds(1, 1)) == -5 and lg(binary=kinds(1, 1)) == -5                   # binary + mse, regression + bce: not this kernel's
    assert lg(esmm=1) == -4 and lg(esmm=1, loss_kind=kinds(0, 0), binary=kinds(1, 1)) == 0
    assert lg(esmm=1, n_tasks=3, loss_kind=kinds(0, 0, 0), binary=kinds(1, 1, 1)) == -4       # the ESMM form takes two tasks
    assert lg(n_tasks=0) == -2 and lg(batch=-1) == -2 and lg(batch=4, pred_stride=3, y_stride=4, dlogit_stride=4) == -2
    assert lg(batch=4, pred_stride=4, y_stride=-4, dlogit_stride=4) == -2
    # dctr_mtl_sum_slots
    ss = lambda src=arr, strides=i64, n_src=2, batch=0, n=4, dst=16, dst_stride=8, dst_offset=2, acc=0: lib.dctr_mtl_sum_slots(   # noqa: E731
        src, strides, n_src, batch, n, dst, dst_stride, dst_offset, acc, None)
    assert ss() == 0 and ss(n_src=16) == 0 and ss(acc=1) == 0
    assert ss(n_src=17) == -2 and b"n_src" in lib.dctr_last_error() and ss(n_src=0) == -2                    # more than 16 sources
    assert ss(src=None) == -1 and ss(strides=None) == -1 and ss(dst=None) == -1
    assert ss(src=cast((ctypes.c_void_p * 2)(16, None))) == -1
    assert ss(dst_offset=-1) == -2 and ss(dst_offset=5) == -2 and ss(dst_stride=-8) == -2 and ss(n=0) == -2 and ss(batch=-1) == -2
    assert ss(strides=cast((ctypes.c_int64 * 2)(4, 3))) == -2 and ss(strides=cast((ctypes.c_int64 * 2)(4, -4))) == -2


def test_op_argument_errors_raise_before_any_launch():
    from deepctr_amd import _C, ops
    z = torch.zeros
    with pytest.raises(ValueError, match="members"):
        ops.mtl_mix_bwd(z(5, 6), 2, 3, [z(5, 4)], [z(4, 2)], [[0, 2]], z(5, 3), z(5, 6), z(5, 2))
    with pytest.raises(ValueError, match="mixes no expert"):
        ops.mtl_mix_bwd(z(5, 6), 2, 3, [z(5, 4)], [z(4, 0)], [[]], z(5, 3), z(5, 6), z(5, 2))
    with pytest.raises(ValueError, match="d_out must be"):
        ops.mtl_mix_bwd(z(5, 6), 2, 3, [z(5, 4)], [z(4, 2)], [[0, 1]], z(5, 3), z(5, 6), z(5, 2), d_out_offset=1)
    with pytest.raises(ValueError, match="ds must be"):
        ops.mtl_mix_bwd(z(5, 6), 2, 3, [z(5, 4)], [z(4, 2)], [[0, 1]], z(5, 3), z(5, 6), z(5, 1))
    with pytest.raises(ValueError, match="dh must be"):
        ops.mtl_mix_bwd(z(5, 6), 2, 3, [z(5, 4)], [z(4, 2)], [[0, 1]], z(5, 3), z(5, 5), z(5, 2))
    with pytest.raises(_C.DctrExtensionError):
        ops.mtl_mix_bwd(z(5, 6), 2, 3, [z(5, 4)], [z(4, 2)], [[0, 1]], z(5, 3), z(5, 6), z(5, 2))       # CPU tensors, after every check
    with pytest.raises(ValueError, match="unknown loss"):
        ops.mtl_loss_grad(z(2, 5), z(2, 5), z(2, 5), z(2), ["hinge", "mse"], [True, False])
    with pytest.raises(ValueError, match="on a regression output"):
        ops.mtl_loss_grad(z(2, 5), z(2, 5), z(2, 5), z(2), ["binary_crossentropy", "binary_crossentropy"], [True, False])
    with pytest.raises(ValueError, match="esmm takes two binary tasks"):
        ops.mtl_loss_grad(z(2, 5), z(2, 5), z(2, 5), z(2), ["binary_crossentropy", "mse"], [True, False], esmm=True)
    with pytest.raises(ValueError, match="loss_sum"):
        ops.mtl_loss_grad(z(2, 5), z(2, 5), z(2, 5), z(3), ["binary_crossentropy", "mse"], [True, False])
    with pytest.raises(ValueError, match="dlogit must be"):
        ops.mtl_loss_grad(z(2, 5), z(2, 5), z(2, 4), z(2), ["binary_crossentropy", "mse"], [True, False])
    with pytest.raises(ValueError, match="1 .. 16 sources"):
        ops.mtl_sum_slots([z(5, 4)] * 17, 4, z(5, 4))
    with pytest.raises(ValueError, match=r"srcs\[1\] must be"):
        ops.mtl_sum_slots([z(5, 4), z(5, 3)], 4, z(5, 4))
    with pytest.raises(ValueError, match="dst must be"):
        ops.mtl_sum_slots([z(5, 4)], 4, z(5, 5), dst_offset=2)
    with pytest.raises(_C.DctrExtensionError):
        ops.mtl_sum_slots([z(5, 4)], 4, z(5, 6), dst_offset=2)


def test_header_compiles_as_c_and_the_mirror_matches_the_layout(tmp_path):
    from deepctr_amd import _C
    header = open(os.path.join(ROOT, "include", "dctr.h")).read()
    assert "#define DCTR_ABI_VERSION 13" in header and _C.ABI_VERSION == 13              # new entry points only: no existing struct changed
    assert re.search(r"\bint dctr_mtl_mix_bwd\(const dctr_mtl_mix_bwd_args_t\* args", header)
    assert re.search(r"\bint dctr_mtl_loss_grad\(const dctr_mtl_loss_args_t\* args", header)
    assert re.search(r"\bint dctr_mtl_sum_slots\(const float\* const\* src", header)
    for sym in ("dctr_mtl_mix_bwd", "dctr_mtl_loss_grad", "dctr_mtl_sum_slots"):
        assert sym in _C.SYMBOLS
    assert "mtl_bwd_kernels.hip" in __import__("deepctr_amd.build", fromlist=["SOURCES"]).SOURCES
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    for cls, cname in ((_C.mtl.MixBwdArgs, "dctr_mtl_mix_bwd_args_t"), (_C.mtl.LossArgs, "dctr_mtl_loss_args_t")):
        lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dctr.h"', "int main(void) {",
                 '    printf("enums %d %d\\n", DCTR_MTL_LOSS_BCE, DCTR_MTL_LOSS_MSE);', '    printf("sizeof %%zu\\n", sizeof(%s));' % cname]
        for fname, _ in cls._fields_:
            lines.append('    printf("%s %%zu\\n", offsetof(%s, %s));' % (fname, cname, fname))
        lines += ["    return 0;", "}"]
        src = tmp_path / (cname + ".c")
        src.write_text("\n".join(lines) + "\n")
        exe = tmp_path / cname
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
        out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
        seen = 0
        for line in filter(None, out):
            field, *vals = line.split()
            if field == "enums":
                assert [int(v) for v in vals] == [_C.mtl.LOSS_BCE, _C.mtl.LOSS_MSE]
                continue
            want = ctypes.sizeof(cls) if field == "sizeof" else getattr(cls, field).offset
            assert int(vals[0]) == want, "%s: C says %s, ctypes %d" % (field, vals[0], want)
            seen += 1
        assert seen == 1 + len(cls._fields_)


def test_supported_answers_for_the_defaults_and_declines_the_rest():
    from deepctr_amd import models, training_hip
    cols = _cols()
    for kind in sorted(MODELS):
        ctor = getattr(models, kind)
        assert training_hip.supported(ctor(cols, device="cpu")), kind                    # the reference's default arguments
        for act in ("sigmoid", "tanh", "linear"):
            assert training_hip.supported(ctor(cols, dnn_activation=act, device="cpu")), (kind, act)
        for kw in (dict(dnn_use_bn=True), dict(dnn_dropout=0.3), dict(dnn_activation="dice")):
            assert not training_hip.supported(ctor(cols, device="cpu", **kw)), (kind, kw)
    m = models.MMOE(cols, task_types=("binary", "regression"), device="cpu")
    assert training_hip.supported(m)
    m.compile("adam", loss=["binary_crossentropy", "mse"])
    assert training_hip.supported(m)
    m.compile("adam", loss=["binary_crossentropy", "binary_crossentropy"])                # a regression task on binary_crossentropy
    assert not training_hip.supported(m)
    m.compile("adam", loss=["mse", "mse"])
    assert not training_hip.supported(m)
    with pytest.raises(ValueError, match="outside the HIP training step"):
        training_hip.HipTrainer(m)


@pytest.mark.parametrize("kind", sorted(MODELS))
def test_trainer_registers_every_trainable_weight_once(kind):
    from deepctr_amd import training, training_hip
    model, cols, _ = build(kind, l2_reg_dnn=0.3, l2_reg_embedding=0.2)
    tr = training_hip.HipTrainer(model, "sgd")
    names = {t.data_ptr(): n for n, t in model.named_weights()}
    got = sorted(names[p.w.data_ptr()] for p in tr.params)
    assert got == sorted(n for n, _ in model.named_weights()) and len(set(got)) == len(got)
    l2 = {names[p.w.data_ptr()]: p.l2 for p in tr.params}
    for n, v in l2.items():
        want = 0.2 if n.endswith("/embeddings") else 0.3 if re.search(r"/kernel\d+$", n) else 0.0
        assert v == want, (n, v)
    assert sorted((names[t.data_ptr()], v) for t, v in training.regularized_weights(model)) == sorted((n, v) for n, v in l2.items() if v)
    assert any("gate_softmax" in n for n in l2) == bool(model.levels) and any(n.startswith("dense") for n in l2)


def test_fit_keeps_its_rule_and_its_refusals():
    from deepctr_amd.models.multitask import _fit
    model, cols, _ = build("MMOE")
    model.compile("adam")
    assert _fit.takes_hip_step(model)
    model.hip_training = False
    assert not _fit.takes_hip_step(model)
    model.hip_training = True
    model.compile(lambda params: torch.optim.SGD(params, lr=0.1))
    assert not _fit.takes_hip_step(model)
    model.compile("nadam")
    assert not _fit.takes_hip_step(model)
    bn, _, _ = build("MMOE", dnn_use_bn=True)
    bn.compile("adam")
    assert not _fit.takes_hip_step(bn)
    rng = np.random.RandomState(0)
    feed = _feed(rng, cols, 8)
    ys = [np.zeros(8, dtype=np.float32)] * 2
    model.compile("adam")
    for opt, val in (("sample_weight", np.ones(8)), ("class_weight", {0: 1.0}), ("callbacks", [object()]), ("steps_per_epoch", 2), ("_dp", object())):
        with pytest.raises(NotImplementedError, match=r"fit\(%s=\.\.\.\) is not implemented for multi-task models" % opt):
            model.fit(feed, ys, verbose=0, **{opt: val})


# ---- the GPU mini-fuzz's configurations (tests/test_gpu_mtl_train.py::test_fuzz_fit_on_both_steps) ----------------------------------
FUZZ_SEEDS = list(range(12))


def fuzz_config(seed):
    """(kind, constructor kwargs, columns, rows, batch size, optimizer, loss weights) of a seed: the four constructors in turn over random
    widths inside the HIP step's family."""
    rng = np.random.RandomState(7000 + seed)
    kind = ("MMOE", "PLE", "SharedBottom", "ESMM")[seed % 4]
    T = 2 if kind == "ESMM" else int(rng.randint(2, 4))
    units = lambda lo=0: tuple(int(u) for u in rng.choice([3, 8, 16, 17, 32], int(rng.randint(lo, 3))))      # noqa: E731
    kw = dict(task_names=["t%d" % t for t in range(T)], tower_dnn_hidden_units=units(),
              task_types=["binary"] * T if kind == "ESMM" else [str(rng.choice(["binary", "regression"])) for _ in range(T)],
              dnn_activation=str(rng.choice(["relu", "relu", "tanh", "sigmoid"])), l2_reg_dnn=float(rng.choice([0.0, 1e-3])))
    if kind == "MMOE":
        kw.update(num_experts=int(rng.randint(2, 6)), expert_dnn_hidden_units=units(1), gate_dnn_hidden_units=units())
    elif kind == "PLE":
        kw.update(shared_expert_num=int(rng.randint(0, 3)), specific_expert_num=int(rng.randint(1, 3)), num_levels=int(rng.randint(1, 4)),
                  expert_dnn_hidden_units=units(1), gate_dnn_hidden_units=units())
    elif kind == "SharedBottom":
        kw.update(bottom_dnn_hidden_units=units())
    cols = _cols(int(rng.randint(1, 6)), int(rng.choice([4, 8, 16])), int(rng.randint(0, 3)))
    bs = [64, 100][seed % 2]
    return kind, kw, cols, 2 * bs + bs // 3, bs, "adam" if seed % 3 == 2 else "sgd", [float(w) for w in rng.choice([1.0, 0.5, 2.0], T)]


def fuzz_setup(seed, device):
    """The seed's model with its random weights, feed and labels; None where the random weights saturate an output (|logit| >= 30)."""
    from deepctr_amd import models
    from tests.test_gpu_models import _randomise
    kind, kw, cols, n, bs, opt, lw = fuzz_config(seed)
    rng = np.random.RandomState(seed)
    model = getattr(models, kind)(cols, device=device, **kw)
    w = _randomise(model, rng)
    w = {k: (rng.standard_normal(v.shape).astype(np.float32) if "gate_softmax" in k else v) for k, v in w.items()}
    feed = _feed(rng, cols, n)
    ys = [(rng.rand(n) > 0.5).astype(np.float32) if t == "binary" else rng.standard_normal(n).astype(np.float32) for t in kw["task_types"]]
    return kind, kw, cols, w, feed, ys, n, bs, opt, lw


def test_fuzz_seeds_train_on_the_autograd_step_alone():
    """At most 3 of the 12 seeds of the GPU mini-fuzz may skip (saturating or diverging random weights, tests/test_gpu_fuzz.py's
    rules): counted here on CPU-built models, on the autograd step alone."""
    from deepctr_amd import models, training_hip
    from deepctr_amd.models.multitask import _fit
    skips = 0
    for seed in FUZZ_SEEDS:
        kind, kw, cols, w, feed, ys, n, bs, opt, lw = fuzz_setup(seed, "cpu")
        model = getattr(models, kind)(cols, device="cpu", **kw)
        model.set_weights_by_name(w)
        model.compile(opt, loss_weights=lw)
        assert training_hip.supported(model), (seed, kind, kw)
        staged = _staged(model, feed, n)
        with torch.no_grad():
            lg = torch.stack(model.autograd_logits(staged, 0, n)).numpy()
        if not (np.isfinite(lg).all() and np.abs(lg).max() < 30.0):
            skips += 1
            continue
        h = _fit.fit_torch(model, staged, torch.from_numpy(np.stack(ys)), n, bs, 1, False, _fit.EpochEnd(model, None, bs, 1, 0)).history
        if not (np.isfinite(h["loss"][-1]) and h["loss"][-1] < 50.0):
            skips += 1
    assert skips <= 3, skips
