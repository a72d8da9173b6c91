"""Float64 oracle of dctr_gru_bwd (include/dctr.h): backpropagation through time of one DynamicGRU layer, written from the equations
of the header and checked against torch's double autograd over training._gru (tests/test_gru_bwd_oracle_cpu.py).

    gru_bwd(x, lengths, layer, cell, att, scale_input, return_sequence, d_out) -> (G, T)

G holds dx, d_att (None where the variant has no scores) and the four weight gradients; T holds, per element, the sum of |summands|
from the same recursion run on absolute values, in which the saturating factors are split into their terms — 1 - c^2 counts as
1 + c^2, r (1 - r) as r + r^2, 1 - u' as 1 + |u'|, 1 - a as 1 + |a| and h - c as |h| + |c| — so that a float32 implementation is
given room where those factors cancel to nearly nothing (tests.util.assert_close_terms).

The case table below is read by the CPU and the GPU tests."""
import collections

import numpy as np

from tests import ref_dien

KEYS = ("dx", "d_att", "d_gate_kernel", "d_gate_bias", "d_candidate_kernel", "d_candidate_bias")
VARIANTS = (("GRU", False), ("AIGRU", True), ("AGRU", False), ("AUGRU", False))      # (name, scale_input); AIGRU is GRU + scale_input
RESIDENT_MAX_E = 48         # the widest E whose weights stay in LDS; the next one streams them (the CPU test asks the library)
SUPPORT_MAX_E = 65          # the widest E dctr_gru_bwd takes; the next one is refused


def cell_of(variant):
    return "GRU" if variant == "AIGRU" else variant


def gru_bwd(x, lengths, layer, cell, att, scale_input, return_sequence, d_out):
    x = np.asarray(x, np.float64)
    B, T, E = x.shape
    wg, bg, wc, bc = (np.asarray(v, np.float64).reshape(s) for v, s in zip(layer, ((2 * E, 2 * E), (2 * E,), (2 * E, E), (E,))))
    lens = np.clip(np.asarray(lengths).reshape(-1), 0, T)
    need_att = cell != "GRU" or scale_input
    a_all = np.asarray(att, np.float64).reshape(B, T) if need_att else np.zeros((B, T))
    d_out = np.asarray(d_out, np.float64)
    xs = x * a_all[:, :, None] if scale_input else x
    # the forward, every step's operands kept
    h = np.zeros((B, E))
    steps = []
    for t in range(T):
        ru = ref_dien.sigmoid(np.concatenate([xs[:, t], h], 1) @ wg + bg)
        r, u = ru[:, :E], ru[:, E:]
        c = np.tanh(np.concatenate([xs[:, t], r * h], 1) @ wc + bc)
        a = a_all[:, t:t + 1]
        if cell == "AGRU":
            hn = (1 - a) * h + a * c
        else:
            up = (1 - a) * u if cell == "AUGRU" else u
            hn = up * h + (1 - up) * c
        steps.append((h, r, u, c))
        h = np.where((t < lens)[:, None], hn, h)
    out = []
    for terms in (False, True):
        ab = np.abs if terms else (lambda v: v)
        one_minus = (lambda v: 1 + np.abs(v)) if terms else (lambda v: 1 - v)
        W_g, W_c, X, XR, A = ab(wg), ab(wc), ab(xs), ab(x), ab(a_all)
        D = ab(d_out)
        g = dict(dx=np.zeros((B, T, E)), d_att=np.zeros((B, T)), d_gate_kernel=np.zeros((2 * E, 2 * E)), d_gate_bias=np.zeros(2 * E),
                 d_candidate_kernel=np.zeros((2 * E, E)), d_candidate_bias=np.zeros(E))
        dh = np.zeros((B, E))
        for t in range(T - 1, -1, -1):
            hp, r, u, c = steps[t]
            live = (t < lens)[:, None]
            if return_sequence:
                dh = dh + np.where(live, D[:, t], 0)
            else:
                dh = dh + np.where((t == lens - 1)[:, None], D, 0)
            H, C, a = ab(hp), ab(c), A[:, t:t + 1]
            h_minus_c = (H + C) if terms else (hp - c)
            da = np.zeros((B, 1))
            if cell == "AGRU":
                dc = dh * a
                dhp = dh * one_minus(a)
                da = (dh * h_minus_c).sum(1, keepdims=True) if terms else (dh * (c - hp)).sum(1, keepdims=True)
                du = np.zeros((B, E))
            else:
                up = one_minus(a) * u if cell == "AUGRU" else u
                dc = dh * one_minus(up)
                dup = dh * h_minus_c
                dhp = dh * up
                if cell == "AUGRU":
                    du = dup * one_minus(a)
                    da = (dup * u).sum(1, keepdims=True) * (1 if terms else -1)
                else:
                    du = dup
            dzc = np.where(live, dc * ((1 + c * c) if terms else (1 - c * c)), 0)
            du = np.where(live, du, 0)
            da = np.where(live, da, 0)
            d_in = dzc @ W_c.T
            dxt, drh = d_in[:, :E], d_in[:, E:]
            g["d_candidate_kernel"] += np.concatenate([X[:, t], r * H], 1).T @ dzc
            g["d_candidate_bias"] += dzc.sum(0)
            dr = drh * H
            dzg = np.concatenate([dr * ((r + r * r) if terms else r * (1 - r)), du * ((u + u * u) if terms else u * (1 - u))], 1)
            d_in = dzg @ W_g.T
            g["d_gate_kernel"] += np.concatenate([X[:, t], H], 1).T @ dzg
            g["d_gate_bias"] += dzg.sum(0)
            dxt = dxt + d_in[:, :E]
            if scale_input:
                da = da + (dxt * XR[:, t]).sum(1, keepdims=True)
                dxt = dxt * a
            g["dx"][:, t] = dxt
            g["d_att"][:, t] = da[:, 0]
            dh = np.where(live, dhp + drh * r + d_in[:, E:], dh)
        if not need_att:
            g["d_att"] = None
        out.append(g)
    return out[0], out[1]


# ---------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name E T B variant return_sequence max_blocks route seed")
E_LIST = (1, 4, 12, 16, 17, 40, 64, RESIDENT_MAX_E + 1, SUPPORT_MAX_E)
T_LIST = (1, 2, 6)
B_LIST = (1, 17, 33)


def _table():
    cases = []
    for i, E in enumerate(E_LIST):
        for v, (variant, _) in enumerate(VARIANTS):
            for s, seq in enumerate((True, False)):
                # One row alone goes with E <= 17.  Its weight gradients are the outer product of a single row, so the bar has no
                # magnitude summed over rows to lean on, and the forward's own rounding passes straight into them: a pre-activation
                # that cancels over its 2E products to z carries 1e-7 sum|products| / |z| relative error into c and h, which are
                # factors of the gradient and which the terms take at their magnitude.  That grows with the reduction's length
                # (float32 autograd on the CPU reaches 0.64 of the bar at E 65 with one row, 0.1 at E 12); the partial tile and
                # the K padding are exercised at the narrow widths all the same, and the wide ones take 17 and 33 rows.
                T, B = T_LIST[(i + v + s) % 3], B_LIST[(i + v) % 3] if E <= 17 else B_LIST[1 + (i + v) % 2]
                # 33 rows on one workgroup: it walks three tiles and sums the weight gradients across them
                cases.append(Case("E%d_%s_%s_T%d_B%d" % (E, variant, "seq" if seq else "final", T, B), E, T, B, variant, seq,
                                  1 if B == 33 else 0, None, len(cases)))
    # three tiles on three workgroups (their atomics meet), and small shapes forced onto the streamed weights
    for variant, seq in (("GRU", True), ("AUGRU", False)):
        cases.append(Case("E17_%s_%s_T6_B33_wide" % (variant, "seq" if seq else "final"), 17, 6, 33, variant, seq, 0, None, len(cases)))
    for variant, seq in (("AIGRU", True), ("AGRU", False)):
        cases.append(Case("E12_%s_%s_T6_B33_streamed" % (variant, "seq" if seq else "final"), 12, 6, 33, variant, seq, 0, "streamed",
                          len(cases)))
    return cases


CASES = _table()
CASE_BY_NAME = {c.name: c for c in CASES}


def case_lengths(T, B):
    """<= 0, 1, T, T + 3 and what lies between, cycled over the rows; with 33 rows the second tile of 16 is all zeros.  One row alone
    runs every step."""
    if B == 1:
        return np.array([T], np.int32)
    pattern = [T, 1, 0, T + 3, -1, max(T - 1, 1), T, 2]
    lens = np.array([pattern[i % len(pattern)] for i in range(B)], np.int32)
    if B > 32:
        lens[16:32] = 0
    return lens


def case_inputs(case):
    """(x [B,T,E], lengths, layer, att [B,T], d_out) in float32: weights N(0, 1/2E), gate bias 1 + 0.3 N, candidate bias 0.3 N, as the
    GRU fixtures; scores in (0, 1)."""
    rng = np.random.RandomState(1000 + case.seed)
    E, T, B = case.E, case.T, case.B
    f = np.float32
    x = rng.randn(B, T, E).astype(f)
    s = np.sqrt(0.5 / E)
    layer = [(rng.randn(2 * E, 2 * E) * s).astype(f), (1 + 0.3 * rng.randn(2 * E)).astype(f), (rng.randn(2 * E, E) * s).astype(f),
             (0.3 * rng.randn(E)).astype(f)]
    att = rng.rand(B, T).astype(f)
    d_out = rng.randn(*((B, T, E) if case.return_sequence else (B, E))).astype(f)
    return x, case_lengths(T, B), layer, att, d_out


def case_options(case):
    """(cell, scale_input) of the case's variant."""
    return cell_of(case.variant), dict(VARIANTS)[case.variant]


_ORACLE = {}


def case_oracle(case):
    """(G, T) of the case, computed once and shared (callers do not write into it)."""
    if case.name not in _ORACLE:
        x, lens, layer, att, d_out = case_inputs(case)
        cell, scale = case_options(case)
        _ORACLE[case.name] = gru_bwd(x, lens, layer, cell, att, scale, case.return_sequence, d_out)
    return _ORACLE[case.name]
