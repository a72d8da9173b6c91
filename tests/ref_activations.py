"""float64 NumPy oracle of the eight tf.keras 2.x activation functions the DNN kernels take beside relu / sigmoid / tanh / linear / Dice
(deepctr_amd/csrc/act_device.h), shared by tests/test_activations_cpu.py (which pins it without TensorFlow: known values, torch's
float64 functions, central differences) and tests/test_gpu_activations.py.

Definitions: tf.keras 2.x ``keras/activations.py`` — the functions ``tf.keras.layers.Activation(name)`` resolves, which is what the
reference's ``activation_layer`` builds for a string (deepctr/layers/activation.py:75-85).
    elu(z)          = z > 0 ? z : alpha (exp(z) - 1), alpha = 1                      (activations.elu -> backend.elu)
    selu(z)         = scale * elu(z, alpha), scale = 1.0507009873554805, alpha = 1.6732632423543772    (activations.selu / tf.nn.selu)
    softplus(z)     = log(exp(z) + 1)                                                 (activations.softplus -> tf.math.softplus)
    softsign(z)     = z / (|z| + 1)                                                   (activations.softsign -> tf.math.softsign)
    exponential(z)  = exp(z)                                                          (activations.exponential)
    hard_sigmoid(z) = 0 for z < -2.5, 1 for z > 2.5, else 0.2 z + 0.5                 (activations.hard_sigmoid, Keras 2; Keras 3 and torch
                                                                                       use relu6(z + 3) / 6, another function)
    swish(z)        = z sigmoid(z), alias silu                                        (activations.swish -> tf.nn.silu)
    gelu(z)         = 0.5 z (1 + erf(z / sqrt 2))                                     (activations.gelu, approximate=False)
Each comes with its derivative in two forms: from the pre-activation z (all eight), and from the OUTPUT h = f(z) for the six where the
kernels of dctr_mlp_bwd's chained form take it from there (FROM_OUTPUT)."""
import math

import numpy as np

SELU_SCALE = 1.0507009873554805
SELU_ALPHA = 1.6732632423543772
NAMES = ("elu", "selu", "softplus", "softsign", "exponential", "hard_sigmoid", "swish", "gelu")
ALIASES = {"silu": "swish"}
FROM_OUTPUT = ("elu", "selu", "softplus", "softsign", "exponential", "hard_sigmoid")       # act' can be written in h
FROM_Z = ("swish", "gelu")                                                               # act' needs z
CODES = {"elu": 5, "selu": 6, "softplus": 7, "softsign": 8, "exponential": 9, "hard_sigmoid": 10, "swish": 11, "gelu": 12}   # DCTR_ACT_*
KINKS = {"elu": (0.0,), "selu": (0.0,), "softsign": (0.0,), "hard_sigmoid": (-2.5, 2.5)}   # where f' jumps (elu, softsign: f'' only)

_erf = np.vectorize(math.erf, otypes=[np.float64])
_erfc = np.vectorize(math.erfc, otypes=[np.float64])


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _sigmoid(z):
    """sigmoid(z) without overflow or cancellation on either side."""
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def value(name, z):
    name, z = ALIASES.get(name, name), _f64(z)
    if name == "elu":
        return np.where(z > 0, z, np.expm1(np.minimum(z, 0.0)))
    if name == "selu":
        return SELU_SCALE * np.where(z > 0, z, SELU_ALPHA * np.expm1(np.minimum(z, 0.0)))
    if name == "softplus":
        return np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z)))
    if name == "softsign":
        return z / (1.0 + np.abs(z))
    if name == "exponential":
        return np.exp(z)
    if name == "hard_sigmoid":
        return np.clip(0.2 * z + 0.5, 0.0, 1.0)
    if name == "swish":
        return z * _sigmoid(z)
    assert name == "gelu", name
    return 0.5 * z * _erfc(-z / math.sqrt(2.0))           # = 0.5 z (1 + erf(z / sqrt 2)), exact in the negative tail too


def deriv_from_z(name, z):
    name, z = ALIASES.get(name, name), _f64(z)
    if name == "elu":
        return np.where(z > 0, 1.0, np.exp(np.minimum(z, 0.0)))
    if name == "selu":
        return SELU_SCALE * np.where(z > 0, 1.0, SELU_ALPHA * np.exp(np.minimum(z, 0.0)))
    if name == "softplus":
        return _sigmoid(z)
    if name == "softsign":
        return 1.0 / (1.0 + np.abs(z)) ** 2
    if name == "exponential":
        return np.exp(z)
    if name == "hard_sigmoid":
        return np.where((z > -2.5) & (z < 2.5), 0.2, 0.0)
    if name == "swish":
        s = _sigmoid(z)
        return s * (1.0 + z * _sigmoid(-z))
    assert name == "gelu", name
    return 0.5 * _erfc(-z / math.sqrt(2.0)) + z * np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def deriv_from_output(name, h):
    """act' in terms of h = f(z), as the kernels of the chained dctr_mlp_bwd define it (include/dctr.h)."""
    name, h = ALIASES.get(name, name), _f64(h)
    if name == "elu":
        return np.where(h > 0, 1.0, h + 1.0)
    if name == "selu":
        return np.where(h > 0, SELU_SCALE, h + SELU_SCALE * SELU_ALPHA)
    if name == "softplus":
        return -np.expm1(-h)
    if name == "softsign":
        return (1.0 - np.abs(h)) ** 2
    if name == "exponential":
        return h
    assert name == "hard_sigmoid", name
    return np.where((h > 0) & (h < 1), 0.2, 0.0)


def _lipschitz(name, z, tz):
    """An upper bound of |f'| around z: the largest of |f'| at z and at z -+ 1e-3 of the magnitude z was summed at (far more than fp32
    moves z, so a kink or a steep stretch next to z is inside)."""
    d = 1e-3 * tz
    return np.maximum(np.abs(deriv_from_z(name, z)), np.maximum(np.abs(deriv_from_z(name, z - d)), np.abs(deriv_from_z(name, z + d))))


def dnn(x, kernels, biases, name, bn=None):
    """DNN.call in float64: z_l = h_{l-1} W_l + b_l (then z_l * scale_l + shift_l with ``bn`` = [(scale, shift)]), h_l = f(z_l).
    Returns (zs, hs, terms): per layer the pre-activations the function sees, the outputs, and for tests.util.assert_close_terms the
    magnitude every output was summed at, carried through the function to first order: T_z = T_{h, l-1} |W| + |b| (times |scale|,
    plus |shift|), T_h = sup|f'| T_z + |h| — an error of delta T_z in z is an error of |f'| delta T_z in h."""
    h = _f64(x)
    th = np.abs(h)
    zs, hs, ts = [], [], []
    for l, (w, b) in enumerate(zip(kernels, biases)):
        w, b = _f64(w), _f64(b)
        z, tz = h @ w + b, th @ np.abs(w) + np.abs(b)
        if bn is not None and bn[l] is not None:
            sc, sh = _f64(bn[l][0]), _f64(bn[l][1])
            z, tz = z * sc + sh, tz * np.abs(sc) + np.abs(sh)
        h = value(name, z)
        th = _lipschitz(name, z, tz) * tz + np.abs(h)
        zs.append(z)
        hs.append(h)
        ts.append(th)
    return zs, hs, ts


def head(h, th, head_w, add=(), global_bias=None, sigmoid_out=False):
    """Dense(1, use_bias=False) + add + global bias (+ sigmoid) on the last layer's outputs; (y, terms)."""
    hw = _f64(head_w).reshape(-1)
    y, t = h @ hw, th @ np.abs(hw)
    for a in add:
        y, t = y + _f64(a), t + np.abs(_f64(a))
    if global_bias is not None:
        y, t = y + float(global_bias), t + abs(float(global_bias))
    if sigmoid_out:
        p = _sigmoid(y)
        return p, p * (1.0 - p) * t + p
    return y, t


def mlp_bwd(x, kernels, biases, acts, name, head_w=None, dlogit=None, d_out=None):
    """The contract of dctr_mlp_bwd for these functions, in float64, with ``terms`` as tests/ref_mlp_bwd.py::mlp_bwd computes them.
    acts = the forward's SAVED (float32) outputs.  act' comes from them for FROM_OUTPUT and from z_l = X_l W_l + b_l (X_l = the saved
    input of the layer) for FROM_Z."""
    name = ALIASES.get(name, name)
    x, kernels, acts = _f64(x), [_f64(k) for k in kernels], [_f64(a) for a in acts]
    L = len(kernels)
    g = {"dW": [None] * L, "db": [None] * L, "d_head_w": None}
    t = {"dW": [None] * L, "db": [None] * L, "d_head_w": None}
    if head_w is not None:
        head_w, dlogit = _f64(head_w).reshape(-1), _f64(dlogit).reshape(-1)
        dh = dlogit[:, None] * head_w[None, :]
        th = np.abs(dh)
        g["d_head_w"], t["d_head_w"] = acts[-1].T @ dlogit, np.abs(acts[-1]).T @ np.abs(dlogit)
    else:
        dh = _f64(d_out)
        th = np.abs(dh)
    for l in range(L - 1, -1, -1):
        xl = x if l == 0 else acts[l - 1]
        d = deriv_from_output(name, acts[l]) if name in FROM_OUTPUT else deriv_from_z(name, xl @ kernels[l] + _f64(biases[l]))
        dz, tz = dh * d, th * np.abs(d)
        g["dW"][l], t["dW"][l] = xl.T @ dz, np.abs(xl).T @ tz
        g["db"][l], t["db"][l] = dz.sum(0), tz.sum(0)
        dh, th = dz @ kernels[l].T, tz @ np.abs(kernels[l]).T
    g["dx"], t["dx"] = dh, th
    return g, t


def make_dnn(seed, batch, in_dim, units, name, bn=False):
    """Inputs of a forward / backward case (float32): x [B, in_dim + 3] (row stride > in_dim), kernels, biases, (scale, shift) per
    layer or None.  Pre-activations of O(1.5) spread over both sides of 0 and of +-2.5, and a few at +-30:
      * layer 0: input column in_dim - 2 is 0 except +-30 in rows 1 and 2, and feeds unit units[0] - 2 alone with weight 1 and
        bias 0 — that unit sees z = +-30 there (0 elsewhere) and feeds nothing on (exp(30) would overflow the next layer);
      * last layer (of two or more): input column in_dim - 1 is 0 except 2 in rows 3 and 4, and feeds unit units[0] - 1 alone; that unit
        feeds the even units of the next layer with +30 / (f(2) - f(0)) and the odd ones with the negative, their biases take f(0)
        times that out again: rows 3 and 4 see z of about +-30 in every unit of layer 1, the other rows nothing."""
    rng = np.random.RandomState(seed)
    dims = [in_dim] + list(units)
    x = (rng.standard_normal((batch, in_dim + 3)) * 1.2).astype(np.float32)
    ks = [(rng.standard_normal((k, n)) * (1.5 / np.sqrt(k))).astype(np.float32) for k, n in zip(dims[:-1], dims[1:])]
    bs = [(rng.standard_normal(n) * 0.5).astype(np.float32) for n in units]
    bnp = [((rng.rand(n) + 0.5).astype(np.float32), (rng.standard_normal(n) * 0.2).astype(np.float32)) for n in units] if bn else None
    assert batch >= 5 and in_dim >= 4 and units[0] >= 4
    c0, c1, u0, u1 = in_dim - 2, in_dim - 1, units[0] - 2, units[0] - 1
    x[:, c0], x[:, c1] = 0.0, 0.0
    x[1, c0], x[2, c0], x[3, c1], x[4, c1] = 30.0, -30.0, 2.0, 2.0
    for c, u in ((c0, u0), (c1, u1)):
        ks[0][:, u], ks[0][c, :] = 0.0, 0.0
        ks[0][c, u], bs[0][u] = 1.0, 0.0
        if bn:
            bnp[0][0][u], bnp[0][1][u] = 1.0, 0.0
    if len(units) > 1:
        ks[1][u0, :], ks[1][u1, :] = 0.0, 0.0
    for l in range(1, len(units)):
        # (an unbounded function — exponential — feeds the next layer values of any size: every later kernel is scaled so that its
        #  pre-activations have a standard deviation of 1.5 again)
        hprev = dnn(x[:, :in_dim], ks[:l], bs[:l], name, None if bnp is None else bnp[:l])[1][-1]
        ks[l] = (ks[l] * (1.5 / max(float((hprev @ _f64(ks[l])).std()), 1e-6))).astype(np.float32)
    if len(units) > 1:
        f0, f2 = float(value(name, 0.0)), float(value(name, 2.0))
        ks[1][u1, :] = (30.0 / (f2 - f0)) * np.where(np.arange(units[1]) % 2 == 0, 1.0, -1.0)
        bs[1] = (bs[1] - f0 * ks[1][u1, :]).astype(np.float32)
    else:
        ks[0][c1, u1] = 0.0
    return x, ks, bs, bnp
