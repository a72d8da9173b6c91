"""NumPy oracle of EDCN (reference deepctr/models/edcn.py:18-94), RegulationModule (layers/core.py:270-321) and BridgeModule
(layers/interaction.py:1502-1565), float64 or float32, on the shared oracle helpers (embedding groups, linear logit, keras Add).

``absolute=True`` is the magnitude mode for tests.util.assert_close_terms: the same network on |x|, |W|, |b| and the gates (which are
positive already), with every activation — and the softmax weights of attention pooling, which lie in (0, 1) — replaced by the identity
on magnitudes: an upper bound of the magnitude every sum of the tower was taken at.

The bar of the tower-op tests: assert_close_terms with rtol = 1e-4 and rtol_terms = TOWER_RTOL_TERMS.  Measured on the CPU
(tests/test_edcn_cpu.py::test_float32_tower_against_float64_sets_the_bar, over the sweep of tests/test_gpu_edcn.py: the three fused
bridges x {vector, matrix} x offsets {3, 4} x relu / linear x with / without the BatchNormalization affine): the float32 NumPy run of
``tower_op`` sits at most 4.46e-7 of the summed magnitude off the float64 run (c / h / br and the logit alike).  Twice that, since the
MFMA tile sums k in another order than NumPy, is 8.9e-7; rounded up to one digit: 9e-7."""
import json

import numpy as np

from oracle import ref_numpy as R
from oracle.ref_models import _add, _embed_groups, linear_logit

TOWER_RTOL_TERMS = 9e-7
BRIDGES = ("pointwise_addition", "hadamard_product", "concatenation", "attention_pooling")


def _softmax(v, axis):
    e = np.exp(v - v.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)


def gate(g, tau, dtype=np.float64, uniform=False):
    """softmax over the fields of g / tau -> [F] (``uniform``: what a RegulationModule that ignored its weights would apply)."""
    dt = np.dtype(dtype).type
    g = np.asarray(g).astype(dt).reshape(-1)
    if uniform:
        return np.full(g.shape, dt(1.0) / dt(g.size), dtype=dt)
    return _softmax(g * dt(1.0 / tau), 0)


def regulation(x, g, tau, dtype=np.float64, uniform=False):
    """x [B, F, d] -> [B, F * d]."""
    dt = np.dtype(dtype).type
    x = np.asarray(x).astype(dt)
    return (x * gate(g, tau, dt, uniform)[None, :, None]).reshape(x.shape[0], -1)


def _act(v, activation, absolute):
    if absolute or activation in ("linear", None):
        return v
    if activation == "relu":
        return np.maximum(v, 0)
    if activation == "sigmoid":
        return 1.0 / (1.0 + np.exp(-v))
    if activation == "tanh":
        return np.tanh(v)
    raise ValueError(activation)


def bridge(x, h, bridge_type, weights=None, activation="relu", dtype=np.float64, absolute=False):
    """weights: (kernel [2D, D], bias [D]) for 'concatenation'; ((k0, b0, k1, b1), (k0, b0, k1, b1)) for 'attention_pooling'."""
    dt = np.dtype(dtype).type
    ab = np.abs if absolute else (lambda v: v)
    x, h = ab(np.asarray(x).astype(dt)), ab(np.asarray(h).astype(dt))
    if bridge_type == "pointwise_addition":
        return x + h
    if bridge_type == "hadamard_product":
        return x * h
    if bridge_type == "concatenation":
        k, b = (ab(np.asarray(t).astype(dt)) for t in weights)
        return _act(np.concatenate([x, h], axis=-1) @ k + b.reshape(-1), activation, absolute)
    if bridge_type == "attention_pooling":
        if absolute:
            return x + h
        outs = []
        for t, (k0, b0, k1, b1) in zip((x, h), weights):
            hid = _act(t @ np.asarray(k0).astype(dt) + np.asarray(b0).astype(dt).reshape(-1), activation, False)
            outs.append(_softmax(hid @ np.asarray(k1).astype(dt) + np.asarray(b1).astype(dt).reshape(-1), -1) * t)
        return outs[0] + outs[1]
    raise ValueError(bridge_type)


def dice(v, alpha, mean, var, eps=1e-9):
    p = 1.0 / (1.0 + np.exp(-(v - mean) / np.sqrt(var + eps)))
    return alpha * (1.0 - p) * v + p * v


def tower_op(xbuf, fields, dim, gates, cross_kernels, cross_biases, dnn_kernels, dnn_biases, bridge_type="hadamard_product",
             parameterization="vector", tau=1.0, activation="relu", bn=None, dice_params=None, bridge_weights=None, bridge_activation="relu",
             x_offset=0, head_w=None, add=(), global_bias=None, sigmoid_out=False, dtype=np.float64, absolute=False, uniform_gates=False):
    """What ops.edcn computes from a [B, stride] buffer -> (logit [B] or None, out [B, 3D] = [c, h, br] of the last round).
    bn: per round None or (scale, shift); dice_params: per round (alpha, mean, variance) with activation 'dice'."""
    dt = np.dtype(dtype).type
    ab = np.abs if absolute else (lambda v: v)
    F, d = int(fields), int(dim)
    D, L = F * d, len(dnn_kernels)
    A = lambda t: ab(np.asarray(t).astype(dt))       # noqa: E731
    x = A(np.asarray(xbuf)[:, x_offset:x_offset + D])
    B = x.shape[0]
    deep = regulation(x.reshape(B, F, d), gates[0], tau, dt, uniform_gates)
    cross = regulation(x.reshape(B, F, d), gates[1], tau, dt, uniform_gates)
    for i in range(L):
        w, b = A(cross_kernels[i]), A(cross_biases[i]).reshape(-1)
        if parameterization == "vector":
            c = cross * (cross @ w.reshape(D, 1)) + b + cross
        else:
            c = cross * (cross @ w.reshape(D, D).T + b) + cross
        z = deep @ A(dnn_kernels[i]).reshape(D, D) + A(dnn_biases[i]).reshape(-1)
        if bn is not None and bn[i] is not None:
            z = z * A(bn[i][0]).reshape(-1) + A(bn[i][1]).reshape(-1)
        if activation in ("dice", "Dice") and not absolute:
            h = dice(z, *(np.asarray(t).astype(dt).reshape(-1) for t in dice_params[i]))
        else:
            h = _act(z, activation, absolute)
        br = bridge(c, h, bridge_type, None if bridge_weights is None else bridge_weights[i], bridge_activation, dt, absolute)
        if i + 1 < L:
            deep = regulation(br.reshape(B, F, d), gates[2 * i + 2], tau, dt, uniform_gates)
            cross = regulation(br.reshape(B, F, d), gates[2 * i + 3], tau, dt, uniform_gates)
    out = np.concatenate([c, h, br], axis=-1)
    logit = None
    if head_w is not None:
        logit = out @ A(head_w).reshape(-1)
        for t in add:
            logit = logit + A(t).reshape(-1)
        if global_bias is not None:
            logit = logit + A(global_bias).reshape(-1)[0]
        if sigmoid_out and not absolute:
            logit = 1.0 / (1.0 + np.exp(-logit))
    return logit, out


def _name(base, k):
    return base if k == 0 else "%s_%d" % (base, k)


def tower_weights(weights, cross_num, bridge_type, dnn_use_bn=False):
    """The tower op's arguments out of a weight dict under the reference's layer names (edcn.py:67-87 creation order)."""
    per = 3 if bridge_type == "attention_pooling" else 1            # DNN layers created per round
    gates = [weights["%s/%s_field_weight" % (_name("regulation_module", k), _name("regulation_module", k))] for k in range(2 * cross_num)]
    ck = [weights[_name("cross_net", i) + "/kernel0"] for i in range(cross_num)]
    cb = [weights[_name("cross_net", i) + "/bias0"] for i in range(cross_num)]
    dk = [weights[_name("dnn", per * i) + "/kernel0"] for i in range(cross_num)]
    db = [weights[_name("dnn", per * i) + "/bias0"] for i in range(cross_num)]
    bw = bn = None
    if bridge_type == "concatenation":
        bw = [(weights[_name("dense", i) + "/kernel"], weights[_name("dense", i) + "/bias"]) for i in range(cross_num)]
    elif bridge_type == "attention_pooling":
        bw = [tuple(tuple(weights["%s/%s" % (_name("dnn", 3 * i + j), n)] for n in ("kernel0", "bias0", "kernel1", "bias1")) for j in (1, 2))
              for i in range(cross_num)]
    if dnn_use_bn:
        bn = []
        for i in range(cross_num):
            p = {n: np.asarray(weights["%s/%s" % (_name("batch_normalization", i), n)], dtype=np.float64)
                 for n in ("gamma", "beta", "moving_mean", "moving_variance")}
            inv = p["gamma"] / np.sqrt(p["moving_variance"] + 1e-3)
            bn.append((inv, p["beta"] - p["moving_mean"] * inv))
    head = weights[_name("dense", cross_num if bridge_type == "concatenation" else 0) + "/kernel"]
    return dict(gates=gates, cross_kernels=ck, cross_biases=cb, dnn_kernels=dk, dnn_biases=db, bridge_weights=bw, bn=bn), head


def edcn(linear_cols, dnn_cols, weights, feed, cross_num=2, cross_parameterization="vector", bridge_type="concatenation", tau=1.0,
         dnn_use_bn=False, dnn_activation="relu", task="binary", dtype=np.float32, absolute=False, uniform_gates=False,
         compute_bridge=None, **_):
    """``compute_bridge``: a weightless bridge type to compute with INSTEAD of ``bridge_type`` (the weights keep the names
    ``bridge_type`` gives them): what a tower with the wrong bridge would answer."""
    dt = np.dtype(dtype).type
    if absolute:
        assert not dnn_use_bn and dnn_activation in ("relu", "linear")
        weights = {k: np.abs(v) for k, v in weights.items()}
        feed = {k: (np.abs(v) if np.asarray(v).dtype.kind == "f" else v) for k, v in feed.items()}
    lin = linear_logit(linear_cols, feed, weights, dt)
    groups, dense = _embed_groups(dnn_cols, feed, weights, "", dt)
    assert not dense
    embs = [np.asarray(e) for g in groups.values() for e in g]        # [B, 1, d] each: sparse first, then the pooled sequences
    x = np.concatenate(embs, axis=1)
    B, F, d = x.shape
    tw, head = tower_weights(weights, cross_num, bridge_type, dnn_use_bn)
    if compute_bridge is not None:
        bridge_type, tw["bridge_weights"] = compute_bridge, None
    logit, _ = tower_op(x.reshape(B, F * d), F, d, parameterization=cross_parameterization, bridge_type=bridge_type, tau=tau,
                        activation=dnn_activation, head_w=head, dtype=dt, absolute=absolute, uniform_gates=uniform_gates, **tw)
    logit = logit.reshape(B, 1).astype(dt)
    bias = weights["prediction_layer/global_bias"].astype(dt)
    if absolute:
        return _add(lin, logit) + np.abs(bias)
    return R.prediction_layer(_add(lin, logit), bias, task)


def run_fixture(g, dtype=np.float32, task=None, weights=None, absolute=False, **override):
    """The oracle over a tests/golden/model_edcn_*.npz fixture (task='regression': the logit; ``weights`` overrides the fixture's;
    further keywords override the fixture's constructor arguments, e.g. bridge_type)."""
    from tests.spec import columns_from_spec
    meta = json.loads(bytes(g["meta"]).decode())
    feed = {k[5:]: v for k, v in g.items() if k.startswith("feed/")}
    if weights is None:
        weights = {k[2:]: v for k, v in g.items() if k.startswith("w/")}
    kw = dict(meta["kwargs"])
    kw.update(override)
    if task is not None:
        kw["task"] = task
    return edcn(columns_from_spec(meta["linear"]), columns_from_spec(meta["dnn"]), weights, feed, dtype=dtype, absolute=absolute, **kw)
