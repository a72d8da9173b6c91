"""NumPy oracle of the backward of the field-axis conv / pool stack (tests/ref_fieldconv.py is the forward's; the stack has no HIP
backward yet: this is the reference one will be held to), closed form, no autograd: a function of (x, kernels, tape, d_out,
d_stage_outs).  The tape is, per stage s, (P_s, sel_s): the pooled map [B, rout, E, C_out] and, in the same shape, the row of the stage's
conv output every pooled element came from.  Per stage, last to first, with X_s = x (stage 0) or P_{s-1} FROM THE TAPE IT IS HANDED,
pb = (w - 1) // 2:

    dP_s  = (s last ? d_out : dX_{s+1}) + d_stage_outs[s]
    dZ_s[b, sel_s[b,r',e,co], e, co] = dP_s[b,r',e,co] (1 - P_s[b,r',e,co]^2)         every other dZ_s is 0
    dbias_s[co]    = sum_{b,r,e} dZ_s[b,r,e,co]
    dK_s[d,ci,co]  = sum_{b,r,e} Xpad_s[b,r+d,e,ci] dZ_s[b,r,e,co]
    dX_s[b,r,e,ci] = sum_{d,co} dZ_s[b,r+pb-d,e,co] K_s[d,ci,co]                      rows outside the map contribute 0

The selection is an INPUT: a float32 / float64 difference in which row wins a near-tie cannot arise inside the oracle.  ``forward_tape``
is the float64 (or float32) forward that produces a tape: k-max by a stable argsort of -value (ties to the lower row, tf.nn.top_k's
order), max pooling by the first maximum of the window.

``absolute=True`` returns, per output element, the sum of the magnitudes of its summands (the ``terms`` of
tests.util.assert_close_terms): the same expressions on |x|, |K|, |d_out|, |d_stage_outs| with 1 + P^2 for 1 - P^2.

Near-ties.  Two forwards that both meet the forward's bar, 1e-4 |v| + 2e-6 max|v of the sample| per value, cannot order two values
differently when the values are further apart than twice that, which is at most GAP = 2 (1e-4 + 2e-6) = 2.04e-4 because |tanh| <= 1.
``min_selection_gap`` returns per stage and per pooled line (b, e, c) the smallest gap that decides a selection; comparisons of a
selection made by two implementations leave out the lines at or under GAP, and the table below keeps them under a quarter of every case
(tests/test_fieldconv_bwd_oracle_cpu.py).

The bar for a float32 implementation: assert_close_terms with rtol = 1e-4 and rtol_terms = BWD_RTOL_TERMS.  Measured on the CPU
(tests/test_fieldconv_bwd_oracle_cpu.py::test_float32_backward_against_float64_sets_the_bar, every case of CASES, every output, the
float64 tape handed to both): the float32 NumPy run of this oracle sits at most 1.46e-7 of the summed magnitude off the float64 run.
Twice that is 2.9e-7 (3e-7 to one digit), below assert_close_terms' default 2e-6: the default is kept."""
import collections
import functools

import numpy as np

from tests import ref_fieldconv as RF

BWD_RTOL_TERMS = 2e-6
GAP = 2.0 * (1e-4 + 2e-6)
GAP_SHARE_MAX = 0.25

# max_blocks: 0, or the cap on workgroups an implementation is asked to run the case with (16 columns (b, e) to a tile: with 2 or 3
# workgroups a workgroup walks several tiles)
Case = collections.namedtuple("Case", "name B F E chans widths pools d_out dso max_blocks seed")


def _case(i, F, E, B, chans, max_blocks=0, seed=None):
    """Case i of the table: widths from {1, 2, 6, 7, F + 3}, k from {1, 3, rows}, p from {1, 2, 3}, the kinds alternating."""
    wset = (1, 2, 6, 7, F + 3)
    rows, widths, pools = F, [], []
    for s in range(len(chans) - 1):
        widths.append(wset[(i + 2 * s) % 5])
        pick = (i // 2 + s) % 3
        if (i + s) % 2 == 0:
            arg = min((1, 3, rows)[pick], rows)
            pools.append(("kmax", arg))
            rows = arg
        else:
            arg = min((1, 2, 3)[pick], rows)
            pools.append(("max", arg))
            rows //= arg
    L = len(chans) - 1
    dso = (None, "all", "some")[i % 3] if L > 1 or i % 2 else None
    d_out = not (dso == "all" and i % 6 == 1)
    name = "c%02d_F%d_E%d_B%d_%s_%s" % (i, F, E, B, "x".join(str(c) for c in chans),
                                        "_".join("w%d%s%d" % (w, k[0], a) for w, (k, a) in zip(widths, pools)))
    return Case(name, B, F, E, tuple(chans), tuple(widths), tuple(pools), d_out, dso, max_blocks, 100 + i if seed is None else seed)


def _table():
    Fs, Es, Bs = (1, 2, 5, 7, 13), (1, 4, 5, 17), (1, 17, 33)
    chains = ((1, 3), (1, 16, 17), (4, 20, 1), (1, 3, 17, 2, 5))
    out = []
    for i in range(38):
        out.append(_case(i, Fs[i % 5], Es[(i // 5 + i) % 4], Bs[(i + i // 3) % 3], chains[(i + i // 4) % 4]))
    # a workgroup walks several tiles: 33 x 5 = 165 columns are 11 tiles over 2 workgroups; and 33 x 17 columns over 3
    out.append(_case(38, 13, 5, 33, (1, 16, 17), max_blocks=2))
    out.append(_case(39, 7, 17, 33, (4, 20, 1), max_blocks=3))
    # rows % p != 0 with a window of 3 over 13 and then over 4 rows, every stage's map seeded
    out.append(_case(41, 13, 4, 17, (1, 3, 17, 2, 5)))
    return out


CASES = _table()
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)


def stage_rows(case):
    rows, out = case.F, []
    for kind, arg in case.pools:
        rows = arg if kind == "kmax" else rows // arg
        out.append(rows)
    return out


@functools.lru_cache(maxsize=None)
def case_inputs(case):
    """(x [B,F,E] or [B,F,E,C_0], kernels, biases, d_out or None, d_stage_outs or None), float32, never modified."""
    rng = np.random.RandomState(case.seed)
    B, F, E, ch = case.B, case.F, case.E, case.chans
    x = rng.standard_normal((B, F, E) if ch[0] == 1 else (B, F, E, ch[0])).astype(np.float32)
    kernels, biases = [], []
    for s, w in enumerate(case.widths):
        kernels.append((rng.standard_normal((w, ch[s], ch[s + 1])) * (0.9 / np.sqrt(min(w, F) * ch[s]))).astype(np.float32))
        biases.append((rng.standard_normal(ch[s + 1]) * 0.3).astype(np.float32))
    rows = stage_rows(case)
    shapes = [(B, r, E, c) for r, c in zip(rows, ch[1:])]
    d_out = rng.standard_normal(shapes[-1]).astype(np.float32) if case.d_out else None
    dso = None
    if case.dso:
        dso = [rng.standard_normal(sh).astype(np.float32) if case.dso == "all" or s % 2 == 0 else None for s, sh in enumerate(shapes)]
    for a in [x, d_out] + kernels + biases + [d for d in (dso or []) if d is not None]:
        if a is not None:
            a.setflags(write=False)
    return x, kernels, biases, d_out, dso


def _x4(x, dtype):
    x = np.asarray(x).astype(dtype)
    return x[..., None] if x.ndim == 3 else x


def _k3(kern, dtype):
    kern = np.asarray(kern).astype(dtype)
    return kern[:, 0] if kern.ndim == 4 else kern


def select(y, kind, arg):
    """The rows of y [B,R,E,C] a pooling picks, [B,rout,E,C] int32: k-max: a stable argsort of -value (ties to the lower row); max
    pooling: the first maximum of every window of ``arg`` rows (the trailing rows % arg are never picked)."""
    if kind == "kmax":
        return np.argsort(-y, axis=1, kind="stable")[:, :arg].astype(np.int32)
    B, R, E, C = y.shape
    n = R // arg
    win = y[:, :n * arg].reshape(B, n, arg, E, C)
    return (win.argmax(axis=2) + (np.arange(n) * arg)[None, :, None, None]).astype(np.int32)


def forward_tape(x, kernels, biases, pools, dtype=np.float64):
    """The forward with its selection: [(P_s, sel_s)] per stage."""
    h = _x4(x, dtype)
    tape = []
    for kern, bias, (kind, arg) in zip(kernels, biases, pools):
        y = RF.conv_same(h, kern, bias)
        sel = select(y, kind, int(arg))
        h = np.take_along_axis(y, sel.astype(np.int64), axis=1)
        tape.append((h, sel))
    return tape


def min_selection_gap(x, kernels, biases, pools):
    """Per stage an array [B,E,C]: the smallest gap that decides a selection on the line (b, e, c), from the float64 forward.  k-max:
    between neighbours of the sorted top k + 1 (the k-th against the first one left out included); max pooling: between the maximum
    and the runner-up of every window.  inf where nothing is decided (one row; windows of one)."""
    h = _x4(x, np.float64)
    gaps = []
    for kern, bias, (kind, arg) in zip(kernels, biases, pools):
        y = RF.conv_same(h, kern, bias)
        B, R, E, C = y.shape
        arg = int(arg)
        if kind == "kmax":
            top = -np.sort(-y, axis=1)[:, :min(arg + 1, R)]
            g = (top[:, :-1] - top[:, 1:]).min(axis=1) if top.shape[1] > 1 else np.full((B, E, C), np.inf)
        else:
            n = R // arg
            win = -np.sort(-y[:, :n * arg].reshape(B, n, arg, E, C), axis=2)
            g = (win[:, :, 0] - win[:, :, 1]).min(axis=1) if arg > 1 else np.full((B, E, C), np.inf)
        gaps.append(g)
        h = np.take_along_axis(y, select(y, kind, arg).astype(np.int64), axis=1)
    return gaps


def field_conv_bwd(x, kernels, tape, d_out=None, d_stage_outs=None, dtype=np.float64, absolute=False):
    """The equations of the module docstring.  Returns {'dx': x's shape, 'd_kernels': [L] in [w, C_in, C_out], 'd_biases': [L]}."""
    A = np.abs if absolute else (lambda v: v)
    L = len(kernels)
    x4 = _x4(x, dtype)
    dK, dB, dX = [None] * L, [None] * L, None
    for s in range(L - 1, -1, -1):
        P, sel = tape[s]
        P = np.asarray(P).astype(dtype)
        K = _k3(kernels[s], dtype)
        w = K.shape[0]
        pb = (w - 1) // 2
        X = x4 if s == 0 else np.asarray(tape[s - 1][0]).astype(dtype)
        rin = X.shape[1]
        dP = np.zeros_like(P)
        if s == L - 1:
            if d_out is not None:
                dP = dP + A(np.asarray(d_out).astype(dtype).reshape(P.shape))
        else:
            dP = dP + dX
        if d_stage_outs is not None and d_stage_outs[s] is not None:
            dP = dP + A(np.asarray(d_stage_outs[s]).astype(dtype).reshape(P.shape))
        one = np.dtype(dtype).type(1)
        g = dP * ((one + P * P) if absolute else (one - P * P))
        dZ = np.zeros((P.shape[0], rin) + P.shape[2:], dtype)
        np.put_along_axis(dZ, np.asarray(sel).astype(np.int64), g, axis=1)
        dB[s] = dZ.sum(axis=(0, 1, 2))
        Xp = np.pad(A(X), ((0, 0), (pb, w - 1 - pb), (0, 0), (0, 0)))
        dK[s] = np.stack([np.einsum("brei,breo->io", Xp[:, d:d + rin], dZ) for d in range(w)])
        dZp = np.pad(dZ, ((0, 0), (w - 1 - pb, pb), (0, 0), (0, 0)))
        dX = np.zeros(X.shape, dtype)
        for d in range(w):
            dX = dX + dZp[:, w - 1 - d:w - 1 - d + rin] @ A(K[d]).T
    return {"dx": dX.reshape(np.asarray(x).shape), "d_kernels": dK, "d_biases": dB}


def outputs(G):
    """[(name, array)] of a result of field_conv_bwd, in a fixed order."""
    out = [("dx", G["dx"])]
    for s, (k, b) in enumerate(zip(G["d_kernels"], G["d_biases"])):
        out += [("d_kernel[%d]" % s, k), ("d_bias[%d]" % s, b)]
    return out


@functools.lru_cache(maxsize=None)
def case_tape(case):
    """The float64 tape of a case."""
    x, kernels, biases, d_out, dso = case_inputs(case)
    return forward_tape(x, kernels, biases, case.pools, np.float64)


def torch_stack(x, kernels, biases, sels):
    """The stack in torch ops with pooling as ``gather`` with the tape's selection: differentiable, and unable to select differently.
    x [B,R,E] or [B,R,E,C_0]; kernels [w, C_in, C_out]; sels per stage an integer tensor [B,rout,E,C].  Returns every stage's map."""
    import torch
    h = x.unsqueeze(-1) if x.dim() == 3 else x
    maps = []
    for kern, bias, sel in zip(kernels, biases, sels):
        if kern.dim() == 4:
            kern = kern[:, 0]
        w, rows = kern.shape[0], h.shape[1]
        pb = (w - 1) // 2
        hp = torch.nn.functional.pad(h, (0, 0, 0, 0, pb, w - 1 - pb))
        z = bias + sum(hp[:, d:d + rows] @ kern[d] for d in range(w))
        h = torch.gather(torch.tanh(z), 1, sel.long())
        maps.append(h)
    return maps
