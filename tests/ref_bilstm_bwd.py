"""Float64 oracle of dctr_bilstm_train_fwd / dctr_bilstm_bwd (include/dctr.h): BiLSTM with per-LSTM input dropout masks and
backpropagation through time of both stacks, written from the equations of the header and checked against torch's double autograd
over training._bilstm and central differences of tests/ref_dsin.bilstm (tests/test_bilstm_bwd_oracle_cpu.py).

    forward(x, layers, masks, res_layers, merge_mode) -> (out, state)          out: a pair for merge_mode None
    bilstm_bwd(x, layers, masks, res_layers, merge_mode, d_out) -> (G, T)

G holds dx and d_layers (per layer the six weight gradients in ops.LSTM_WEIGHTS' order; zeros for a stack the merge never reads); T
holds, per element, the sum of |summands| from the same recursion run on absolute values, in which the saturating factors are split
into their terms — 1 - tanh(c)^2 counts as 1 + tanh(c)^2, 1 - g^2 as 1 + g^2 and i (1 - i) as i + i^2 — so that a float32
implementation is given room where those factors cancel to nearly nothing (tests.util.assert_close_terms).

``masks``: None, or 2 x n_layers entries (fw layer 0, bw layer 0, fw layer 1, ...), each None or [B, D_l].  ``reverse_back`` False
leaves every backward layer's output in the order it was produced (the dropped reversal the table must tell apart).

The case table below is read by the CPU and the GPU tests."""
import collections

import numpy as np

MERGES = ("fw", "bw", "sum", "mul", "ave", "concat", None)
STREAMED_U = 52             # the narrowest u (Din = u, T 5, two layers) whose weights stream; the CPU test asks the library


def sigmoid(z):
    return 1.0 / (1.0 + np.exp(-z))


def _masks(masks, L):
    return [None] * (2 * L) if masks is None else list(masks)


def _stack(x, layers, masks, res_layers, d, reverse_back):
    """One direction's forward; per layer (input, mask, W, U, b, steps), steps[t] = (i, f, g, o, c_prev, c, h_prev, z)."""
    L = len(layers)
    B, T, _ = x.shape
    inp = x
    state = []
    for l, layer in enumerate(layers):
        W, U, b = (np.asarray(v, np.float64) for v in layer[3 * d:3 * d + 3])
        u = U.shape[0]
        m = masks[2 * l + d]
        m = np.ones((B, inp.shape[2])) if m is None else np.asarray(m, np.float64).reshape(B, -1)
        h, c = np.zeros((B, u)), np.zeros((B, u))
        steps = [None] * T
        rows = np.zeros((B, T, u))
        for t in (range(T - 1, -1, -1) if d else range(T)):
            z = (inp[:, t] * m) @ W + h @ U + b
            i, f, g, o = sigmoid(z[:, :u]), sigmoid(z[:, u:2 * u]), np.tanh(z[:, 2 * u:3 * u]), sigmoid(z[:, 3 * u:])
            cn = f * c + i * g
            steps[t] = (i, f, g, o, c, cn, h, z)
            h, c = o * np.tanh(cn), cn
            rows[:, t] = h
        if d and not reverse_back:
            rows = rows[:, ::-1]
        state.append((inp, m, W, U, b, steps))
        inp = rows + inp if l >= L - res_layers else rows
    return inp, state


def forward(x, layers, masks, res_layers, merge_mode, reverse_back=True):
    x = np.asarray(x, np.float64)
    masks = _masks(masks, len(layers))
    res_layers = min(int(res_layers), len(layers))
    fw, sf = _stack(x, layers, masks, res_layers, 0, reverse_back) if merge_mode != "bw" else (None, None)
    bw, sb = _stack(x, layers, masks, res_layers, 1, reverse_back) if merge_mode != "fw" else (None, None)
    if merge_mode == "fw":
        out = fw
    elif merge_mode == "bw":
        out = bw
    elif merge_mode is None:
        out = (fw, bw)
    elif merge_mode == "sum":
        out = fw + bw
    elif merge_mode == "mul":
        out = fw * bw
    elif merge_mode == "ave":
        out = (fw + bw) / 2
    elif merge_mode == "concat":
        out = np.concatenate([fw, bw], -1)
    return out, (fw, bw, sf, sb)


def gate_preactivations(state):
    """Every gate pre-activation of the forward, flat."""
    return np.concatenate([s[7].reshape(-1) for st in state[2:] if st is not None for layer in st for s in layer[5]])


def bilstm_bwd(x, layers, masks, res_layers, merge_mode, d_out, reverse_back=True):
    x = np.asarray(x, np.float64)
    B, T, Din = x.shape
    L = len(layers)
    res_layers = min(int(res_layers), L)
    _, (fw, bw, sf, sb) = forward(x, layers, masks, res_layers, merge_mode, reverse_back)
    u = np.asarray(layers[0][1]).shape[0]
    out = []
    for terms in (False, True):
        ab = np.abs if terms else (lambda v: v)
        one_minus_sq = (lambda v: 1 + v * v) if terms else (lambda v: 1 - v * v)
        sig_prime = (lambda v: v + v * v) if terms else (lambda v: v * (1 - v))
        if merge_mode is None:
            dys = [ab(np.asarray(d_out[0], np.float64)), ab(np.asarray(d_out[1], np.float64))]
        else:
            D = ab(np.asarray(d_out, np.float64))
            dys = {"fw": [D, None], "bw": [None, D], "sum": [D, D], "ave": [D / 2, D / 2], "concat": [D[..., :u], D[..., u:]]}.get(merge_mode)
            if merge_mode == "mul":
                dys = [D * ab(bw), D * ab(fw)]
        g = dict(dx=np.zeros((B, T, Din)),
                 d_layers=[[np.zeros(np.asarray(w).shape) for w in layer] for layer in layers])
        for d, (dy, st) in enumerate(zip(dys, (sf, sb))):
            if dy is None:
                continue
            for l in range(L - 1, -1, -1):
                inp, m, W, U, b, steps = st[l]
                d_res = dy
                if d and not reverse_back:
                    dy = dy[:, ::-1]
                WU = ab(np.concatenate([W, U], 0))
                M, IN = ab(m), ab(inp * m[:, None])
                dW, dU, db = g["d_layers"][l][3 * d:3 * d + 3]
                d_in = np.zeros(inp.shape)
                dh, dc = np.zeros((B, u)), np.zeros((B, u))
                for t in (range(T) if d else range(T - 1, -1, -1)):
                    i, f, gg, o, cp, cn, hp, _ = steps[t]
                    gg, cp, hp, tc = ab(gg), ab(cp), ab(hp), ab(np.tanh(cn))
                    dh = dh + dy[:, t]
                    do = dh * tc
                    dc = dc + dh * o * one_minus_sq(tc)
                    dz = np.concatenate([dc * gg * sig_prime(i), dc * cp * sig_prime(f), dc * i * one_minus_sq(gg), do * sig_prime(o)], 1)
                    da = dz @ WU.T
                    D_l = inp.shape[2]
                    dW += IN[:, t].T @ dz
                    dU += hp.T @ dz
                    db += dz.sum(0)
                    d_in[:, t] = da[:, :D_l] * M + (d_res[:, t] if l >= L - res_layers else 0)
                    dh, dc = da[:, D_l:], dc * f
                dy = d_in
            g["dx"] += dy
        out.append(g)
    return out[0], out[1]


# ---------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name u Din T B L res merge masks route max_blocks seed")
U_LIST = (4, 12, 16, 17, 40, STREAMED_U)
T_LIST = (1, 2, 5)
B_LIST = (1, 17, 33)
MASK_KINDS = ("all", "none", "partial")


def _name(u, Din, T, B, L, res, merge, masks, tag=""):
    return "u%d_D%d_T%d_B%d_L%d_r%d_%s_%s%s" % (u, Din, T, B, L, res, merge, masks, tag)


def _table():
    cases = []

    def add(u, Din, T, B, L, res, merge, masks, route=None, max_blocks=0, tag=""):
        cases.append(Case(_name(u, Din, T, B, L, res, merge, masks, tag), u, Din, T, B, L, res, merge, masks, route, max_blocks, len(cases)))

    k = 0
    for i, u in enumerate(U_LIST):
        for j in range(3):
            merge = MERGES[k % len(MERGES)]
            L = 1 + (i + j) % 3
            res = (0, 1, L)[(i + 2 * j) % 3]
            # a residual over layer 0 needs Din = u; the others alternate a wider and a narrower input
            Din = u if res >= L else (u + 3 if k % 2 == 0 else max(u - 3, 1))
            T = T_LIST[(i + j) % 3]
            # One row alone goes with u <= 17: its weight gradients are the outer product of a single row, so the bar has no
            # magnitude summed over rows to lean on and the forward's own rounding passes straight into them; that grows with the
            # reduction's length (tests/ref_gru_bwd.py has the figures).  The wide ones take 17 and 33 rows.
            B = B_LIST[(i + j) % 3] if u <= 17 else B_LIST[1 + (i + j) % 2]
            # 33 rows on two workgroups: each walks two or three (tile, direction) items
            add(u, Din, T, B, L, res, merge, MASK_KINDS[k % 3], max_blocks=2 if B == 33 and j == 1 else 0)
            k += 1
    # every merge mode once more at DSIN's own options (two layers, no residual, dropout on both), on a narrow odd width
    for merge in MERGES:
        add(12, 12, 5, 17, 2, 0, merge, "all", tag="_dsin")
    # a small shape forced onto streamed weights, and three layers, all residual, forced onto resident ones
    add(12, 9, 5, 33, 2, 1, "ave", "partial", route="streamed", tag="_streamed")
    add(16, 16, 2, 33, 3, 3, None, "all", route="resident", tag="_resident")
    return cases


CASES = _table()
CASE_BY_NAME = {c.name: c for c in CASES}


def case_inputs(case):
    """(x [B,T,Din], layers, masks, d_out) in float32: kernels N(0, 1 / (D + u)), biases 0.3 N (forget gate + 1, keras'
    unit_forget_bias), masks 0 or 1.25 (rate 0.2); d_out a pair for merge_mode None."""
    rng = np.random.RandomState(2000 + case.seed)
    f = np.float32
    u, Din, T, B, L = case.u, case.Din, case.T, case.B, case.L
    x = rng.randn(B, T, Din).astype(f)
    layers = []
    for l in range(L):
        D = Din if l == 0 else u
        s = np.sqrt(1.0 / (D + u))
        layer = []
        for _ in range(2):
            bias = 0.3 * rng.randn(4 * u)
            bias[u:2 * u] += 1.0
            layer += [(rng.randn(D, 4 * u) * s).astype(f), (rng.randn(u, 4 * u) * s).astype(f), bias.astype(f)]
        layers.append(layer)
    masks = []
    for l in range(L):
        for d in range(2):
            m = ((rng.rand(B, Din if l == 0 else u) >= 0.2) / 0.8).astype(f)
            keep = case.masks == "all" or (case.masks == "partial" and (l + d) % 2 == 0)
            masks.append(m if keep else None)
    if case.masks == "none":
        masks = None
    w = 2 * u if case.merge == "concat" else u
    d_out = rng.randn(B, T, w).astype(f)
    if case.merge is None:
        d_out = (d_out, rng.randn(B, T, u).astype(f))
    return x, layers, masks, d_out


_ORACLE = {}


def case_oracle(case):
    """(G, T) of the case, computed once and shared (callers do not write into it)."""
    if case.name not in _ORACLE:
        x, layers, masks, d_out = case_inputs(case)
        _ORACLE[case.name] = bilstm_bwd(x, layers, masks, case.res, case.merge, d_out)
    return _ORACLE[case.name]
