"""NumPy oracle of the multi-task models (reference deepctr/models/multitask/{sharedbottom,esmm,mmoe,ple}.py), float64 or float32, on
the shared oracle helpers (embedding groups, combined DNN input).

``level_op`` / ``towers_op`` compute what ops.mtl_level / ops.mtl_towers compute, from the same operands.  ``absolute=True`` is the
magnitude mode for tests.util.assert_close_terms: the same network on |x|, |W|, |b|, |scale|, |shift| with every activation replaced
by the identity, mixed with the TRUE gate weights (they lie in (0, 1) and sum to one): an upper bound of the magnitude every sum was
taken at.  ``uniform_gates`` / ``zero_heads``: what a model that ignored its gate kernels / its heads would answer.

The bar of the op tests: assert_close_terms with rtol = 1e-4 and rtol_terms = OP_RTOL_TERMS.  Measured on the CPU
(tests/test_mtl_cpu.py::test_float32_ops_against_float64_set_the_bar over the sweep of tests/test_gpu_mtl.py): the float32 NumPy run of
``level_op`` and ``towers_op`` sits at most 2.22e-7 of the summed magnitude off the float64 run.  Twice that, since the MFMA tile sums k
in another order than NumPy, is 4.44e-7; rounded up: 4.5e-7.  Below assert_close_terms' default 2e-6."""
import json

import numpy as np

from oracle.ref_models import _bn_name, _combined_dnn_input, _embed_groups

OP_RTOL_TERMS = 4.5e-7


def _softmax(v):
    e = np.exp(v - v.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def _act(v, activation, absolute=False):
    if absolute or activation in ("linear", None):
        return v
    if activation == "relu":
        return np.maximum(v, 0)
    if activation == "sigmoid":
        return 1.0 / (1.0 + np.exp(-v))
    if activation == "tanh":
        return np.tanh(v)
    raise ValueError(activation)


def dnn_op(x, kernels, biases, activation="relu", bn=None, dice=None, dtype=np.float64, absolute=False):
    """bn[l]: None or (scale, shift); dice[l]: (alpha, mean, variance) with activation 'dice'."""
    dt = np.dtype(dtype).type
    ab = np.abs if absolute else (lambda v: v)
    h = np.asarray(x).astype(dt)
    for l, (w, b) in enumerate(zip(kernels, biases)):
        h = h @ ab(np.asarray(w).astype(dt)) + ab(np.asarray(b).astype(dt)).reshape(-1)
        if bn is not None and bn[l] is not None:
            h = h * ab(np.asarray(bn[l][0]).astype(dt)).reshape(-1) + ab(np.asarray(bn[l][1]).astype(dt)).reshape(-1)
        if activation in ("dice", "Dice") and not absolute:
            a, mu, var = (np.asarray(t).astype(dt).reshape(-1) for t in dice[l])
            p = 1.0 / (1.0 + np.exp(-(h - mu) / np.sqrt(var + dt(1e-9))))
            h = a * (1.0 - p) * h + p * h
        else:
            h = _act(h, activation, absolute)
    return h


def level_op(xbuf, in_dim, x_offsets, expert_kernels, expert_biases, gate_kernels, members, expert_src=None, gate_src=None,
             activation="relu", expert_bn=None, expert_dice=None, gate_dnn_kernels=None, gate_dnn_biases=None, gate_bn=None, gate_dice=None,
             dtype=np.float64, absolute=False, uniform_gates=False, return_gates=False):
    """What ops.mtl_level computes -> [B, G * H]."""
    dt = np.dtype(dtype).type
    xbuf = np.asarray(xbuf)
    E, G = len(expert_kernels), len(gate_kernels)
    expert_src = [0] * E if expert_src is None else expert_src
    gate_src = [0] * G if gate_src is None else gate_src
    slot = lambda s: xbuf[:, x_offsets[s]:x_offsets[s] + in_dim].astype(dt)      # noqa: E731
    pick = lambda lst, i: None if lst is None else lst[i]      # noqa: E731
    hs = [dnn_op(np.abs(slot(expert_src[e])) if absolute else slot(expert_src[e]), expert_kernels[e], expert_biases[e], activation,
                 pick(expert_bn, e), pick(expert_dice, e), dt, absolute) for e in range(E)]
    outs, gates = [], []
    for g in range(G):
        z = slot(gate_src[g])
        if gate_dnn_kernels is not None:
            z = dnn_op(z, gate_dnn_kernels[g], gate_dnn_biases[g], activation, pick(gate_bn, g), pick(gate_dice, g), dt)
        p = _softmax(z @ np.asarray(gate_kernels[g]).astype(dt))
        if uniform_gates:
            p = np.full_like(p, dt(1.0) / dt(p.shape[1]))
        gates.append(p)
        outs.append(sum(p[:, j:j + 1] * hs[m] for j, m in enumerate(members[g])))
    out = np.concatenate(outs, axis=-1)
    return (out, gates) if return_gates else out


def towers_op(xbuf, in_dim, x_offsets, kernels, biases, head_ws, global_biases=None, binary=None, activation="relu", bn=None, dice=None,
              esmm=False, dtype=np.float64, absolute=False, zero_heads=False):
    """What ops.mtl_towers computes -> [T, B]."""
    dt = np.dtype(dtype).type
    ab = np.abs if absolute else (lambda v: v)
    xbuf = np.asarray(xbuf)
    T = len(head_ws)
    binary = [True] * T if binary is None else binary
    out = []
    for t in range(T):
        x = ab(xbuf[:, x_offsets[t]:x_offsets[t] + in_dim].astype(dt))
        h = dnn_op(x, kernels[t], biases[t], activation, None if bn is None else bn[t], None if dice is None else dice[t], dt, absolute)
        w = ab(np.asarray(head_ws[t]).astype(dt)).reshape(-1)
        l = h @ (np.zeros_like(w) if zero_heads else w)
        if global_biases is not None and global_biases[t] is not None:
            l = l + ab(np.asarray(global_biases[t]).astype(dt)).reshape(-1)[0]
        out.append(1.0 / (1.0 + np.exp(-l)) if (binary[t] and not absolute) else l)
    if esmm and not absolute:
        out[1] = out[0] * out[1]
    return np.stack(out)


class _Names(object):
    """The reference's weight names in its creation order: named and auto-named DNNs with their BatchNormalization counter."""

    def __init__(self, weights, use_bn):
        self.w, self.use_bn, self.n_bn, self.auto = weights, use_bn, 0, {}

    def auto_name(self, base):
        n = self.auto.get(base, 0)
        self.auto[base] = n + 1
        return base if n == 0 else "%s_%d" % (base, n)

    def dnn(self, name=None):
        name = self.auto_name("dnn") if name is None else name
        ks, bs, bn = [], [], []
        while "%s/kernel%d" % (name, len(ks)) in self.w:
            i = len(ks)
            ks.append(self.w["%s/kernel%d" % (name, i)])
            bs.append(self.w["%s/bias%d" % (name, i)])
            if self.use_bn:
                p = {n: np.asarray(self.w["%s/%s" % (_bn_name(self.n_bn), n)], dtype=np.float64)
                     for n in ("gamma", "beta", "moving_mean", "moving_variance")}
                self.n_bn += 1
                inv = p["gamma"] / np.sqrt(p["moving_variance"] + 1e-3)
                bn.append((inv, p["beta"] - p["moving_mean"] * inv))
        return ks, bs, (bn if self.use_bn else None)


def _towers(nm, x, in_dim, offsets, task_types, task_names, names, pred_names, activation, esmm, dt, zero_heads, logits, absolute=False):
    ks, bs, bns, heads, gbs = [], [], [], [], []
    for t, tname in enumerate(task_names):
        k, b, bn = nm.dnn(None if names is None else names[t])
        ks.append(k), bs.append(b), bns.append(bn)
        heads.append(nm.w[nm.auto_name("dense") + "/kernel"])
        gbs.append(nm.w[(pred_names[t] if pred_names[t] is not None else nm.auto_name("prediction_layer")) + "/global_bias"])
    return towers_op(x, in_dim, offsets, ks, bs, heads, gbs, [tt == "binary" and not logits for tt in task_types], activation,
                     bns if nm.use_bn else None, esmm=esmm and not logits, dtype=dt, zero_heads=zero_heads, absolute=absolute)


def model(kind, dnn_cols, weights, feed, kw, dtype=np.float32, uniform_gates=False, zero_heads=False, logits=False, return_gates=False):
    """The four constructors' forward -> [T, B, 1] (``logits``: the values before the sigmoids; ESMM's second entry the cvr logit)."""
    dt = np.dtype(dtype).type
    groups, dense = _embed_groups(dnn_cols, feed, weights, "", dt)
    x = _combined_dnn_input([e for g in groups.values() for e in g], dense).astype(dt)
    in_dim = x.shape[1]
    task_names = list(kw.get("task_names", ("ctr", "ctcvr")))
    task_types = list(kw.get("task_types", ("binary", "binary")))
    T = len(task_names)
    act = kw.get("dnn_activation", "relu")
    nm = _Names(weights, bool(kw.get("dnn_use_bn", False)))
    tower_names = ["tower_" + n for n in task_names]
    all_gates = []
    if kind == "ESMM":
        y = _towers(nm, x, in_dim, [0, 0], ["binary"] * 2, task_names, None, [task_names[0], None], act, True, dt, zero_heads, logits)
    elif kind == "SharedBottom":
        ks, bs, bn = nm.dnn()
        h = dnn_op(x, ks, bs, act, bn, dtype=dt)
        y = _towers(nm, h, h.shape[1], [0] * T, task_types, task_names, tower_names, task_names, act, False, dt, zero_heads, logits)
    else:
        offsets, first = [0], True
        if kind == "MMOE":
            plans = [("", kw.get("num_experts", 3))]
        else:
            plans = [("level_%d_" % i, None) for i in range(kw.get("num_levels", 2))]
        for li, (prefix, n_exp) in enumerate(plans):
            experts, esrc, gdnn, gk, gsrc, members = [], [], [], [], [], []
            if kind == "MMOE":
                for i in range(n_exp):
                    experts.append(nm.dnn("expert_%d" % i))
                    esrc.append(0)
                for n in task_names:
                    gdnn.append(nm.dnn("gate_" + n))
                    gk.append(weights["gate_softmax_%s/kernel" % n])
                    gsrc.append(0)
                    members.append(list(range(n_exp)))
            else:
                ns, nh = kw.get("specific_expert_num", 1), kw.get("shared_expert_num", 1)
                last = li == len(plans) - 1
                for i, n in enumerate(task_names):
                    for j in range(ns):
                        experts.append(nm.dnn("%stask_%s_expert_specific_%d" % (prefix, n, j)))
                        esrc.append(0 if first else i)
                for k in range(nh):
                    experts.append(nm.dnn("%sexpert_shared_%d" % (prefix, k)))
                    esrc.append(0 if first else T)
                for i, n in enumerate(task_names):
                    gdnn.append(nm.dnn("%sgate_specific_%s" % (prefix, n)))
                    gk.append(weights["%sgate_softmax_specific_%s/kernel" % (prefix, n)])
                    gsrc.append(0 if first else i)
                    members.append(list(range(i * ns, (i + 1) * ns)) + list(range(T * ns, T * ns + nh)))
                if not last:
                    gdnn.append(nm.dnn(prefix + "gate_shared"))
                    gk.append(weights[prefix + "gate_softmax_shared/kernel"])
                    gsrc.append(0 if first else T)
                    members.append(list(range(T * ns + nh)))
            has_gd = bool(gdnn[0][0])
            x, gates = level_op(x, in_dim, offsets, [e[0] for e in experts], [e[1] for e in experts], gk, members, esrc, gsrc, act,
                                [e[2] for e in experts] if nm.use_bn else None, None,
                                [g[0] for g in gdnn] if has_gd else None, [g[1] for g in gdnn] if has_gd else None,
                                [g[2] for g in gdnn] if (has_gd and nm.use_bn) else None, dtype=dt, uniform_gates=uniform_gates,
                                return_gates=True)
            all_gates.append(gates)
            in_dim = np.asarray(experts[0][0][-1]).shape[1]
            offsets, first = [g * in_dim for g in range(len(gk))], False
        y = _towers(nm, x, in_dim, offsets[:T], task_types, task_names, tower_names, task_names, act, False, dt, zero_heads, logits)
    y = y.reshape(T, -1, 1).astype(dt)
    return (y, all_gates) if return_gates else y


def run_fixture(g, dtype=np.float32, weights=None, **options):
    """The oracle over a tests/golden/model_{mmoe,ple,sb,esmm}_*.npz fixture -> [T, B, 1]."""
    from tests.spec import columns_from_spec
    meta = json.loads(bytes(g["meta"]).decode())
    feed = {k[5:]: v for k, v in g.items() if k.startswith("feed/")}
    if weights is None:
        weights = {k[2:]: v for k, v in g.items() if k.startswith("w/")}
    return model(meta["model"], columns_from_spec(meta["dnn"]), weights, feed, meta["kwargs"], dtype=dtype, **options)
