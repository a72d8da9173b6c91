"""What tests/test_gpu_bilinear_bwd.py and tests/test_bilinear_bwd_oracle_cpu.py share:
  1. a float64 NumPy oracle, closed form and without autograd, of dctr_bilinear_bwd (deepctr_amd/csrc/bilinear_bwd_kernels.hip): the
     backward of SENETLayer.call + BilinearInteraction.call as FiBiNET wires them, restated from the contract in include/dctr.h;
  2. the table of cases both tests run, each with what it is there for, and their inputs.
The CPU test pins 1 against torch double autograd over training._bilinear and the SENET lines of FiBiNET's autograd step.

The oracle returns (grads, terms) in the convention of tests/ref_fieldpair_bwd.py.  ``terms`` is the input of
tests.util.assert_close_terms: the same backward over absolute values, under the gates of the float64 forward, an upper bound of the
magnitude each output element was summed at."""
import collections
import zlib

import numpy as np

TYPES = ("all", "each", "interaction")
MODES = ("model", "senet", "layer")
WRONG = ("da2", "dxj")          # planted errors: the dA2 path dropped; the dx_j half of every pair dropped


def _f64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


def pair_indices(F):
    """(ii, jj): the pairs i < j of F fields in itertools.combinations order."""
    ii, jj = np.triu_indices(F, 1)
    return ii, jj


def weight_count(bilinear_type, F):
    return {"all": 1, "each": F - 1, "interaction": F * (F - 1) // 2}[bilinear_type]


def weight_index(bilinear_type, F):
    """The matrix of each pair."""
    ii, _ = pair_indices(F)
    return {"all": np.zeros(len(ii), dtype=np.int64), "each": ii, "interaction": np.arange(len(ii))}[bilinear_type]


def width(F, E, mode, dense_cols=0):
    P = F * (F - 1) // 2
    return {"model": 2 * P * E + dense_cols, "senet": F * E, "layer": P * E}[mode]


def _pairs(x, g, coef, W, idx, wrong):
    """One bilinear layer: x [B,F,E], g [B,P,E], coef [B,P] (1 or A2[i] A2[j]), W [nW,E,E], idx [P] -> dx [B,F,E], dW [nW,E,E],
    q [B,P] = <g, (x_i W) (.) x_j>."""
    ii, jj = pair_indices(x.shape[1])
    Wp = W[idx]
    xi, xj = x[:, ii], x[:, jj]
    U = np.einsum("bpe,ped->bpd", xi, Wp)
    gc = g * coef[:, :, None]
    dx = np.zeros_like(x)
    np.add.at(dx, (slice(None), ii), np.einsum("bpd,ped->bpe", gc * xj, Wp))
    if wrong != "dxj":
        np.add.at(dx, (slice(None), jj), gc * U)
    dW = np.zeros_like(W)
    np.add.at(dW, idx, np.einsum("bpe,bpd->ped", xi, gc * xj))
    return dx, dW, (g * U * xj).sum(-1)


def _run(x, d_out, w1, w2, Ws, Wr, bilinear_type, mode, dense_cols, gates, wrong):
    B, F, E = x.shape
    P = F * (F - 1) // 2
    ii, jj = pair_indices(F)
    idx = weight_index(bilinear_type, F)
    out = {}
    dx = np.zeros_like(x)
    if mode != "layer":
        Z = x.mean(-1)
        P1 = Z @ w1
        if gates is None:
            gates = [P1 > 0, None]
        A1 = P1 * gates[0]
        P2 = A1 @ w2
        if gates[1] is None:
            gates[1] = P2 > 0
        A2 = P2 * gates[1]
    if mode == "model":
        g = d_out[:, :2 * P * E].reshape(B, P, 2, E)
        dxs, out["dws"], q = _pairs(x, g[:, :, 0], A2[:, ii] * A2[:, jj], Ws, idx, wrong)
        dxr, out["dwr"], _ = _pairs(x, g[:, :, 1], np.ones((B, P)), Wr, idx, wrong)
        dx += dxs + dxr
        dA2 = np.zeros_like(A2)
        np.add.at(dA2, (slice(None), ii), A2[:, jj] * q)
        np.add.at(dA2, (slice(None), jj), A2[:, ii] * q)
        if dense_cols:
            out["d_dense"] = d_out[:, 2 * P * E:2 * P * E + dense_cols].copy()
    elif mode == "senet":
        g = d_out[:, :F * E].reshape(B, F, E)
        dx += A2[:, :, None] * g
        dA2 = (g * x).sum(-1)
    else:
        dxr, out["dwr"], _ = _pairs(x, d_out[:, :P * E].reshape(B, P, E), np.ones((B, P)), Wr, idx, wrong)
        dx += dxr
    if mode != "layer":
        if wrong == "da2":
            dA2 = np.zeros_like(dA2)
        dP2 = dA2 * gates[1]                    # relu'(0) = 0
        out["dw2"] = A1.T @ dP2
        dP1 = (dP2 @ w2.T) * gates[0]
        out["dw1"] = Z.T @ dP1
        dx += ((dP1 @ w1.T) / E)[:, :, None]
    out["dx"] = dx
    return out, gates


def bilinear_bwd(x, d_out, w1=None, w2=None, Ws=None, Wr=None, bilinear_type="interaction", mode="model", dense_cols=0, wrong=None):
    """dctr_bilinear_bwd (include/dctr.h) in float64.  x [B,F,E]; d_out [B, width]; w1 [F,r], w2 [r,F] (modes model, senet); Ws / Wr: the
    nW matrices [E,E] of the SENET-side / raw-side layer (model: both; layer: Wr).  Returns grads / terms with the keys dx [B,F,E] and,
    as the mode has them, dw1, dw2, dws [nW,E,E], dwr [nW,E,E], d_dense [B,dense_cols]."""
    assert mode in MODES and wrong in (None,) + WRONG
    x, d_out = _f64(x), _f64(d_out)
    w1, w2 = (None if w is None else _f64(w) for w in (w1, w2))
    Ws, Wr = (None if W is None else _f64(np.stack([np.asarray(m) for m in W])) for W in (Ws, Wr))
    ab = lambda a: None if a is None else np.abs(a)     # noqa: E731
    G, gates = _run(x, d_out, w1, w2, Ws, Wr, bilinear_type, mode, dense_cols, None, wrong)
    T, _ = _run(ab(x), ab(d_out), ab(w1), ab(w2), ab(Ws), ab(Wr), bilinear_type, mode, dense_cols, gates, None)
    return G, T


def preactivations(x, w1, w2):
    """(P1 [B,r], its summed magnitude, P2 [B,F], its summed magnitude) of the SENET forward in float64."""
    x, w1, w2 = _f64(x), _f64(w1), _f64(w2)
    Z = x.mean(-1)
    P1 = Z @ w1
    A1 = np.maximum(P1, 0)
    return P1, np.abs(Z) @ np.abs(w1), A1 @ w2, A1 @ np.abs(w2)


GATE_MARGIN = 1e-3


# ---------------------------------------------------------------------------------------------------
# the cases: (F, E, B), max_blocks, the route they are there for, what they exercise
# ---------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name shape max_blocks route why")
CASES = [
    Case("smallest", (2, 1, 5), 0, "lds", "one pair, E = 1, r = 1"),
    Case("ragged", (3, 4, 33), 0, "lds", "a ragged last tile, E below 16"),
    Case("e17", (13, 17, 40), 0, "lds", "E > 16 and not a multiple of 4: column tiles, weight gradients added per tile"),
    Case("criteo", (26, 16, 70), 0, "lds", "the default shape, r = 8: five walks of the tiles"),
    Case("e32", (7, 32, 21), 0, "lds", "two column tiles"),
    Case("f60", (60, 16, 6), 0, "workspace", "1,770 pairs: many pair chunks and walks; three dx-sized buffers pass the LDS"),
    Case("many_tiles", (6, 12, 8200), 0, "lds", "many workgroups' atomics"),
    Case("general", (200, 4, 5), 0, "workspace", "a tile past the LDS: the general route, workspace required (the forward's own example)"),
    Case("walk", (26, 16, 1001), 2, "lds", "2 workgroups carry their weight sums across 63 tiles"),
]
CASE_BY_NAME = {c.name: c for c in CASES}
DENSE = 3                       # dense columns of the runs that have them
_INPUTS = {}


def reduction_size(F):
    return max(1, F // 3)


Inputs = collections.namedtuple("Inputs", "x w1 w2 Ws Wr d_model d_senet d_layer")


def case_inputs(case, r=None):
    """The inputs of a case, float32 values, the same at every call: x [B,F,E], W_1 [F,r], W_2 [r,F], the P matrices of each layer (a
    bilinear_type takes its first nW), and d_out for the three modes (d_model with DENSE columns behind its 2*P*E).  Every SENET
    pre-activation stays GATE_MARGIN of its summed magnitude away from zero: samples that violate it are drawn again."""
    F, E, B = case.shape
    r = reduction_size(F) if r is None else r
    key = (case.name, r)
    if key in _INPUTS:
        return _INPUTS[key]
    P = F * (F - 1) // 2
    rng = np.random.RandomState(zlib.crc32(("%s/%d" % key).encode()) % (2 ** 31))
    for _ in range(100):
        # (with r = 1 the sign pattern of W_2 alone decides which fields can be active: drawn until a quarter of the samples have
        # two active fields, or the SENET side of every pair would be zero)
        w1 = (rng.randn(F, r) / np.sqrt(F)).astype(np.float32)
        w2 = (rng.randn(r, F) / np.sqrt(r)).astype(np.float32)
        x = rng.randn(B, F, E).astype(np.float32)
        for _ in range(100):
            P1, M1, P2, M2 = preactivations(x, w1, w2)
            bad = (np.abs(P1) < 2 * GATE_MARGIN * M1).any(1) | (np.abs(P2) < 2 * GATE_MARGIN * M2).any(1)
            if not bad.any():
                break
            x[bad] = rng.randn(int(bad.sum()), F, E).astype(np.float32)
        else:
            raise AssertionError("%s: no draw keeps the SENET pre-activations off zero" % case.name)
        mixed = all((Q > 0).any() and (Q < 0).any() for Q in (P1, P2))     # both layers have active and inactive units
        if ((P2 > 0).sum(1) >= 2).mean() >= 0.25 and (mixed or F < 3):
            break
    else:
        raise AssertionError("%s: no draw of the SENET weights leaves two fields active" % case.name)
    Ws = list((rng.randn(P, E, E) / np.sqrt(E)).astype(np.float32))
    Wr = list((rng.randn(P, E, E) / np.sqrt(E)).astype(np.float32))
    d_model = rng.randn(B, 2 * P * E + DENSE).astype(np.float32)
    d_senet = rng.randn(B, F * E).astype(np.float32)
    d_layer = rng.randn(B, P * E).astype(np.float32)
    for a in [x, w1, w2, d_model, d_senet, d_layer] + Ws + Wr:
        a.setflags(write=False)
    _INPUTS[key] = Inputs(x, w1, w2, Ws, Wr, d_model, d_senet, d_layer)
    return _INPUTS[key]


def run_operands(case, bilinear_type, mode, dense_cols=0, r=None, rows=None):
    """(x, d_out, w1, w2, Ws, Wr) a run hands the op or the oracle (None where the mode has none); ``rows``: the first samples only."""
    inp = case_inputs(case, r)
    F, E, _ = case.shape
    nW = weight_count(bilinear_type, F)
    sl = slice(None) if rows is None else slice(0, rows)
    if mode == "model":
        P = F * (F - 1) // 2
        return inp.x[sl], inp.d_model[sl, :2 * P * E + dense_cols], inp.w1, inp.w2, inp.Ws[:nW], inp.Wr[:nW]
    if mode == "senet":
        return inp.x[sl], inp.d_senet[sl], inp.w1, inp.w2, None, None
    return inp.x[sl], inp.d_layer[sl], None, None, None, inp.Wr[:nW]


_ORACLE = {}


def oracle(case, bilinear_type, mode, dense_cols=0, r=None, rows=None):
    """bilinear_bwd of a run, computed once and shared (read-only)."""
    key = (case.name, bilinear_type, mode, dense_cols, r, rows)
    if key not in _ORACLE:
        x, d_out, w1, w2, Ws, Wr = run_operands(case, bilinear_type, mode, dense_cols, r, rows)
        G, T = bilinear_bwd(x, d_out, w1, w2, Ws, Wr, bilinear_type, mode, dense_cols)
        for a in list(G.values()) + list(T.values()):
            a.setflags(write=False)
        _ORACLE[key] = (G, T)
    return _ORACLE[key]
