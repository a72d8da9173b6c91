"""What tests/test_gpu_fieldpair_bwd.py and tests/test_fieldpair_bwd_oracle_cpu.py share:
  1. a float64 NumPy oracle, closed form and without autograd, of dctr_fieldpair_bwd (deepctr_amd/csrc/fieldpair_bwd_kernels.hip): the
     backward of FEFMLayer.call / FwFMLayer.call, restated from the contract in include/dctr.h;
  2. the table of cases both tests run, each with what it is there for, and their inputs.
The CPU test pins 1 against torch double autograd over training._fefm and the FwFM einsum.

The oracle returns (grads, terms) in the convention of tests/ref_interacting_bwd.py.  ``terms`` is the input of
tests.util.assert_close_terms: the same backward over absolute values, an upper bound of the magnitude each output element was summed
at."""
import collections
import zlib

import numpy as np


def _f64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


def pair_indices(F):
    """(ii, jj): the pairs i < j of F fields in itertools.combinations order."""
    ii, jj = np.triu_indices(F, 1)
    return ii, jj


def _fefm(x, W, g, wrong=False):
    """x [B,F,E], W [P,E,E], g [B,P] -> dx [B,F,E], dW [P,E,E].  dx_i = sum_{j != i} g_ij S_ij x_j, dW = A + A^T with
    A = sum_b g x_i x_j^T.  ``wrong``: the A^T half of dW is dropped."""
    ii, jj = pair_indices(x.shape[1])
    S = W + W.transpose(0, 2, 1)
    xi, xj = x[:, ii], x[:, jj]                                   # [B,P,E]
    dx = np.zeros_like(x)
    np.add.at(dx, (slice(None), ii), g[:, :, None] * np.einsum("pcd,bpd->bpc", S, xj))
    np.add.at(dx, (slice(None), jj), g[:, :, None] * np.einsum("pcd,bpd->bpc", S, xi))
    A = np.einsum("bp,bpe,bpd->ped", g, xi, xj)
    return dx, (A if wrong else A + A.transpose(0, 2, 1))


def _fwfm(x, r, dl, wrong=False):
    """x [B,F,E], r [F,F], dl [B] -> dx [B,F,E], dr [F,F] (the strict upper triangle; zero elsewhere).  ``wrong``: r' without its
    mirrored half."""
    up = np.triu(r, 1)
    rp = up if wrong else up + up.T
    dx = dl[:, None, None] * np.einsum("ij,bje->bie", rp, x)
    dr = np.triu(np.einsum("b,bie,bje->ij", dl, x, x), 1)
    return dx, dr


def fieldpair_bwd(x, weights, kind, d_pairs=None, d_logit=None, wrong=False):
    """dctr_fieldpair_bwd (include/dctr.h) in float64.  x [B,F,E]; weights: the P matrices [E,E] (``fefm``) or [F,F] (``fwfm``);
    d_pairs [B,P] and / or d_logit [B], converted to float64 BEFORE they are added.  Returns grads / terms with the keys dx [B,F,E]
    and dw ([P,E,E] or [F,F], the latter zero outside the strict upper triangle)."""
    x = _f64(x)
    B, F, _ = x.shape
    if kind == "fefm":
        W = _f64(np.stack([np.asarray(w) for w in weights]))
        g, t = np.zeros((B, F * (F - 1) // 2)), np.zeros((B, F * (F - 1) // 2))
        if d_pairs is not None:
            g, t = g + _f64(d_pairs), t + np.abs(_f64(d_pairs))
        if d_logit is not None:
            g, t = g + _f64(d_logit)[:, None], t + np.abs(_f64(d_logit))[:, None]
        dx, dw = _fefm(x, W, g, wrong)
        tx, tw = _fefm(np.abs(x), np.abs(W), t)
    else:
        assert d_pairs is None
        dx, dw = _fwfm(x, _f64(weights), _f64(d_logit), wrong)
        tx, tw = _fwfm(np.abs(x), np.abs(_f64(weights)), np.abs(_f64(d_logit)))
    return {"dx": dx, "dw": dw}, {"dx": tx, "dw": tw}


# ---------------------------------------------------------------------------------------------------
# the cases: (F, E, B), max_blocks, the route they are there for, what they exercise
# ---------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name shape max_blocks route why")
CASES = [
    Case("smallest", (2, 1, 5), 0, "lds", "one pair, E = 1"),
    Case("ragged", (3, 4, 33), 0, "lds", "a ragged last tile, E below 16"),
    Case("e17", (13, 17, 40), 0, "lds", "E > 16 and not a multiple of 4: column tiles, 4-B weight loads"),
    Case("criteo", (26, 16, 70), 0, "lds", "the Criteo shape: 325 pairs in one chunk"),
    Case("e32", (7, 32, 21), 0, "lds", "two column tiles"),
    Case("f60", (60, 16, 6), 0, "lds", "1,770 pairs: several pair chunks, g of the dx product read from HBM"),
    Case("two_subtiles", (6, 12, 8200), 0, "lds", "two 16-sample sub-tiles per workgroup, many workgroups' atomics"),
    Case("general", (200, 16, 5), 0, "workspace", "a tile past the LDS: the general route, workspace required"),
    Case("walk", (26, 16, 1001), 2, "lds", "2 workgroups walk 63 tiles and carry their dW sums across them"),
]
CASE_BY_NAME = {c.name: c for c in CASES}
KINDS = ("fefm", "fwfm")
# which upstream gradients a run hands the op: FEFM takes the three combinations, FwFM has the logit only
COMBOS = {"fefm": ("pairs", "logit", "both"), "fwfm": ("logit",)}
_INPUTS = {}


def case_inputs(case, kind):
    """(x [B,F,E], weights, d_pairs [B,P] or None, d_logit [B]) of a case and kind, float32 values, the same at every call.  FEFM
    weights: a list of P [E,E] matrices of unit row scale; FwFM: [F,F], every cell drawn (the kernel must ignore the diagonal and the
    lower triangle)."""
    key = (case.name, kind)
    if key in _INPUTS:
        return _INPUTS[key]
    F, E, B = case.shape
    P = F * (F - 1) // 2
    rng = np.random.RandomState(zlib.crc32(("%s/%s" % key).encode()) % (2 ** 31))
    x = rng.randn(B, F, E).astype(np.float32)
    d_logit = rng.randn(B).astype(np.float32)
    if kind == "fefm":
        weights = list((rng.randn(P, E, E) / np.sqrt(E)).astype(np.float32))
        d_pairs = rng.randn(B, P).astype(np.float32)
    else:
        weights = rng.randn(F, F).astype(np.float32)
        d_pairs = None
    for a in [x, d_logit] + ([d_pairs] + weights if kind == "fefm" else [weights]):
        a.setflags(write=False)
    _INPUTS[key] = (x, weights, d_pairs, d_logit)
    return _INPUTS[key]


def combo_grads(combo, d_pairs, d_logit):
    """The (d_pairs, d_logit) a gradient combination hands the op."""
    return (d_pairs if combo in ("pairs", "both") else None), (d_logit if combo in ("logit", "both") else None)


_ORACLE = {}


def oracle(case, kind, combo):
    """fieldpair_bwd of a case, computed once and shared (read-only)."""
    key = (case.name, kind, combo)
    if key not in _ORACLE:
        x, weights, d_pairs, d_logit = case_inputs(case, kind)
        dp, dl = combo_grads(combo, d_pairs, d_logit)
        G, T = fieldpair_bwd(x, weights, kind, dp, dl)
        for a in list(G.values()) + list(T.values()):
            a.setflags(write=False)
        _ORACLE[key] = (G, T)
    return _ORACLE[key]
