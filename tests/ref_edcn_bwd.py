"""NumPy oracle of dctr_edcn_bwd (include/dctr.h), closed form, no autograd: a function of (x, weights, tape, d_logit, d_out).  Per
round i, in reverse, with c / h / br of the round FROM THE TAPE IT IS HANDED, xin = x (round 0) or br of round i-1 from the tape,
gd / gc the field softmaxes of the round's two gates spread over the columns, deep = xin gd, cross = xin gc:

    bridge   c + h: dc += dbr, dh += dbr  |  c * h: dc += dbr h, dh += dbr c
             Dense: dz = dbr [br > 0] (relu; identity for linear), dWb = [c, h]^T dz, dbb = sum dz, dc += dz Wb[0:D]^T, dh += dz Wb[D:2D]^T
    DNN      dz = dh [h > 0], dWd = deep^T dz, dbd = sum dz, ddeep = dz Wd^T
    cross    vector, s = cross . w:      dcross = dc (s + 1) + w (dc . cross), dw = sum_b (dc . cross)_b cross_b, db = sum dc
             matrix, u = W cross + b:    dcross = dc * (u + 1) + W^T (dc * cross), dW = (dc * cross)^T cross, db = sum dc * cross
    gates    dxin = ddeep gd + dcross gc;  dG[f] = sum_{b, e} d . xin;  d_gate = (1 / tau) g * (dG - sum_f g dG)

The seed of the last round is d_out + d_logit * head_w; d_head_w = sum_b d_logit[b] [c, h, br]_last[b].  The relu masks come from the
tape (h > 0, br > 0): a float32 / float64 sign flip of a pre-activation cannot make the op and the oracle differ.

``absolute=True`` returns, per output element, the sum of the magnitudes of its summands (the ``terms`` of
tests.util.assert_close_terms): the same expressions on |x|, |W|, |b|, |tape|, |d_logit|, |d_out| with the masks kept (a masked summand
is an exact zero on both sides), the gates as they are (positive already) and the one difference (dG - sum g dG) taken as a sum.

The bar of the op tests: assert_close_terms with rtol = 1e-4 and rtol_terms = BWD_RTOL_TERMS.  Measured on the CPU
(tests/test_edcn_bwd_oracle_cpu.py::test_float32_backward_against_float64_sets_the_bar, over SWEEP_BWD x the three bridges x {vector,
matrix} x relu / linear, d_logit and d_out both given, every output): the float32 NumPy run of this oracle sits at most 7.79e-7 of
the summed magnitude off the float64 run.  Twice that, since the MFMA tiles and the slice sums add in another order than NumPy, is
1.56e-6; rounded up to one digit: 2e-6."""
import numpy as np

from tests import ref_edcn as RE

BWD_RTOL_TERMS = 2e-6
BRIDGES_BWD = ("pointwise_addition", "hadamard_product", "concatenation")
OUTPUTS = ("dx", "d_gates", "d_cross_w", "d_cross_b", "d_dnn_w", "d_dnn_b", "d_bridge_w", "d_bridge_b", "d_head_w")

# (F, d, cross_num, B): tests.test_edcn_cpu.SWEEP without its D = 1024 row (the layered route has no HIP backward); the last row is the
# largest D the backward's LDS plan accepts at d = 16 (tests/test_edcn_bwd_oracle_cpu.py checks both statements)
SWEEP_BWD = [
    (1, 1, 1, 5),
    (2, 3, 2, 17),
    (3, 4, 1, 65),
    (9, 4, 3, 33),
    (5, 17, 2, 40),
    (26, 16, 2, 130),
    (39, 16, 4, 20),
]


def tower_tape(case, F, d, bridge_type, parameterization, activation="relu", bridge_activation="relu", dtype=np.float64, absolute=False):
    """[L, B, 3D]: c, h, br of every round, RE.tower_op run round by round (the first i + 1 rounds give round i's out); ``absolute``:
    the magnitudes they were summed at."""
    L = len(case["dnn_kernels"])
    outs = []
    for i in range(L):
        bw = None if case["bridge_weights"] is None else case["bridge_weights"][:i + 1]
        _, out = RE.tower_op(case["xbuf"], F, d, case["gates"][:2 * i + 2], case["cross_kernels"][:i + 1], case["cross_biases"][:i + 1],
                             case["dnn_kernels"][:i + 1], case["dnn_biases"][:i + 1], bridge_type=bridge_type,
                             parameterization=parameterization, tau=case["tau"], activation=activation, bridge_weights=bw,
                             bridge_activation=bridge_activation, x_offset=case["off"], dtype=dtype, absolute=absolute)
        outs.append(out)
    return np.stack(outs)


def tower_bwd(xbuf, fields, dim, gates, cross_kernels, cross_biases, dnn_kernels, dnn_biases, tape, d_logit=None, d_out=None,
              bridge_type="hadamard_product", parameterization="vector", tau=1.0, activation="relu", bridge_weights=None,
              bridge_activation="relu", x_offset=0, head_w=None, dtype=np.float64, absolute=False, tape_terms=None):
    """-> dict over OUTPUTS: dx [B, D], the per-round lists in the weights' own shapes (d_bridge_* None without the Dense bridge),
    d_head_w in head_w's shape (None without d_logit).  ``tape_terms`` (with ``absolute``): the magnitudes c / h / br were SUMMED at
    (RE.tower_op's magnitude mode, round by round) in place of |tape| — the terms of an end-to-end comparison, in which the tape is an
    intermediate and not an operand; the masks still come from ``tape``."""
    dt = np.dtype(dtype).type
    pos = np.abs if absolute else (lambda v: v)
    A = lambda t: pos(np.asarray(t).astype(dt))       # noqa: E731
    sub = (lambda a, b: a + b) if absolute else (lambda a, b: a - b)
    F, d = int(fields), int(dim)
    D, L = F * d, len(dnn_kernels)
    x = A(np.asarray(xbuf)[:, x_offset:x_offset + D])
    B = x.shape[0]
    raw = np.asarray(tape).reshape(L, B, 3 * D)
    T = A(raw) if tape_terms is None or not absolute else np.asarray(tape_terms).astype(dt).reshape(L, B, 3 * D)
    inv_tau = pos(dt(1.0 / tau))
    dc, dh, dbr = (np.zeros((B, D), dtype=dt) for _ in range(3))
    d_head = None
    if d_out is not None:
        o = A(np.asarray(d_out)[:, :3 * D])
        dc, dh, dbr = dc + o[:, :D], dh + o[:, D:2 * D], dbr + o[:, 2 * D:]
    if d_logit is not None:
        dl, hw = A(d_logit).reshape(B, 1), A(head_w).reshape(-1)
        dc, dh, dbr = dc + dl * hw[:D], dh + dl * hw[D:2 * D], dbr + dl * hw[2 * D:]
        d_head = (dl * T[L - 1]).sum(0).reshape(np.asarray(head_w).shape)
    concat = bridge_type == "concatenation"
    res = dict(d_gates=[None] * (2 * L), d_cross_w=[None] * L, d_cross_b=[None] * L, d_dnn_w=[None] * L, d_dnn_b=[None] * L,
               d_bridge_w=[None] * L if concat else None, d_bridge_b=[None] * L if concat else None, d_head_w=d_head)
    for i in range(L - 1, -1, -1):
        c, h = T[i][:, :D], T[i][:, D:2 * D]
        xin = x if i == 0 else T[i - 1][:, 2 * D:]
        gd, gc = (RE.gate(gates[2 * i + j], tau, dt) for j in range(2))
        gdc, gcc = np.repeat(gd, d)[None, :], np.repeat(gc, d)[None, :]
        deep, cross = xin * gdc, xin * gcc
        if concat:
            dz = dbr * (raw[i][:, 2 * D:] > 0) if bridge_activation == "relu" else dbr
            Wb = A(bridge_weights[i][0]).reshape(2 * D, D)
            res["d_bridge_w"][i] = (np.concatenate([c, h], axis=1).T @ dz).reshape(np.asarray(bridge_weights[i][0]).shape)
            res["d_bridge_b"][i] = dz.sum(0).reshape(np.asarray(bridge_weights[i][1]).shape)
            dc, dh = dc + dz @ Wb[:D].T, dh + dz @ Wb[D:].T
        elif bridge_type == "pointwise_addition":
            dc, dh = dc + dbr, dh + dbr
        elif bridge_type == "hadamard_product":
            dc, dh = dc + dbr * h, dh + dbr * c
        else:
            raise ValueError(bridge_type)
        dz = dh * (raw[i][:, D:2 * D] > 0) if activation == "relu" else dh
        Wd = A(dnn_kernels[i]).reshape(D, D)
        res["d_dnn_w"][i] = (deep.T @ dz).reshape(np.asarray(dnn_kernels[i]).shape)
        res["d_dnn_b"][i] = dz.sum(0).reshape(np.asarray(dnn_biases[i]).shape)
        ddeep = dz @ Wd.T
        if parameterization == "vector":
            w = A(cross_kernels[i]).reshape(D)
            s, t = cross @ w, (dc * cross).sum(1)
            dcross = dc * (s + dt(1))[:, None] + w[None, :] * t[:, None]
            res["d_cross_w"][i] = (t[:, None] * cross).sum(0).reshape(np.asarray(cross_kernels[i]).shape)
            res["d_cross_b"][i] = dc.sum(0).reshape(np.asarray(cross_biases[i]).shape)
        else:
            W = A(cross_kernels[i]).reshape(D, D)
            u = cross @ W.T + A(cross_biases[i]).reshape(-1)
            q = dc * cross
            dcross = dc * (u + dt(1)) + q @ W
            res["d_cross_w"][i] = (q.T @ cross).reshape(np.asarray(cross_kernels[i]).shape)
            res["d_cross_b"][i] = q.sum(0).reshape(np.asarray(cross_biases[i]).shape)
        for j, (g, dv) in enumerate(((gd, ddeep), (gc, dcross))):
            dG = (dv * xin).reshape(B, F, d).sum(axis=(0, 2))
            res["d_gates"][2 * i + j] = (inv_tau * g * sub(dG, (g * dG).sum())).reshape(np.asarray(gates[2 * i + j]).shape)
        dbr = ddeep * gdc + dcross * gcc
        dc, dh = np.zeros((B, D), dtype=dt), np.zeros((B, D), dtype=dt)
    res["dx"] = dbr
    return res


def seeds(case, F, d, seed=0):
    """Seeded float32 (d_logit [B], d_out [B, 3D + 5]: five columns wider than what is read)."""
    B, D = case["xbuf"].shape[0], F * d
    rng = np.random.RandomState(1000 + seed)
    return (rng.standard_normal(B) * 0.5).astype(np.float32), (rng.standard_normal((B, 3 * D + 5)) * 0.5).astype(np.float32)


def oracle(case, F, d, tape, bridge_type, parameterization, activation="relu", bridge_activation="relu", d_logit=None, d_out=None, **kw):
    return tower_bwd(case["xbuf"], F, d, case["gates"], case["cross_kernels"], case["cross_biases"], case["dnn_kernels"], case["dnn_biases"],
                     tape, d_logit=d_logit, d_out=d_out, bridge_type=bridge_type, parameterization=parameterization, tau=case["tau"],
                     activation=activation, bridge_weights=case["bridge_weights"], bridge_activation=bridge_activation, x_offset=case["off"],
                     head_w=case["head"], **kw)


def flatten(res):
    """[(name, array)] of every output a result dict holds."""
    flat = []
    for name in OUTPUTS:
        v = res.get(name)
        if v is None:
            continue
        if isinstance(v, (list, tuple)):
            flat += [("%s[%d]" % (name, i), np.asarray(t)) for i, t in enumerate(v) if t is not None]
        else:
            flat.append((name, np.asarray(v)))
    return flat
