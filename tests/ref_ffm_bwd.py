"""What tests/test_gpu_ffm_bwd.py and tests/test_ffm_bwd_oracle_cpu.py share:
  1. a float64 NumPy oracle, closed form and without autograd, of dctr_ffm_bwd (deepctr_amd/csrc/ffm_bwd_kernels.hip): the backward of
     ONN's field-aware pair products, restated from the contract in include/dctr.h;
  2. the table of cases both tests run, each with what it is there for, and their inputs.
The CPU test pins 1 against torch double autograd over the products of _ONN._autograd_logit.

The oracle returns (grads, terms): per field the gradient of its fused table [V_j, F-1, d] (a pre-pooled field: of its rows
[B, F-1, d]; a frozen field: None), and the same sums over absolute values — the input of tests.util.assert_close_terms."""
import collections
import itertools
import zlib

import numpy as np

from tests.ref_onn import slot


def ffm_bwd(ids, masters, g, reduce_sum=False, pooled=None, frozen=(), wrong=False):
    """ids [F, B]; masters[j] [V_j, F-1, d]; g [B, P*d] ([B, P] with reduce_sum); ``pooled`` {j: [B, (F-1)*d]}; ``frozen``: fields that
    get no gradient.  An id outside [0, V_j) gets no gradient and enters its partners' as a row of zeros.  ``wrong``: the partner's row
    is read at the field's OWN slot index (right only where the two agree)."""
    F = len(masters)
    ids = np.asarray(ids)
    B = ids.shape[1]
    pooled = pooled or {}
    g = np.asarray(g, dtype=np.float64)
    rows, valid = [], []
    for j in range(F):
        if j in pooled:
            r = np.asarray(pooled[j], dtype=np.float64)
            d = r.shape[1] // (F - 1)
            rows.append(r[:B, :(F - 1) * d].reshape(B, F - 1, d))
            valid.append(np.ones(B, dtype=bool))
        else:
            m = np.asarray(masters[j], dtype=np.float64)
            idx = ids[j].astype(np.int64)
            ok = (idx >= 0) & (idx < m.shape[0])
            r = np.zeros((B,) + m.shape[1:])
            r[ok] = m[idx[ok]]
            rows.append(r)
            valid.append(ok)
    d = rows[0].shape[2]
    out = []
    for rr, gg in ((rows, g), ([np.abs(r) for r in rows], np.abs(g))):
        drow = [np.zeros_like(r) for r in rr]
        for p, (i, j) in enumerate(itertools.combinations(range(F), 2)):
            gp = gg[:, p:p + 1] if reduce_sum else gg[:, p * d:(p + 1) * d]
            drow[i][:, slot(i, j)] = gp * rr[j][:, slot(i, j) if wrong else slot(j, i)]
            drow[j][:, slot(j, i)] = gp * rr[i][:, slot(j, i) if wrong else slot(i, j)]
        res = []
        for j in range(F):
            if j in frozen:
                res.append(None)
            elif j in pooled:
                res.append(drow[j])
            else:
                G = np.zeros(np.asarray(masters[j]).shape)
                ok = valid[j]
                np.add.at(G, ids[j].astype(np.int64)[ok], drow[j][ok])
                res.append(G)
        out.append(res)
    return out[0], out[1]


# ---------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name shape vocab pooled frozen max_blocks route why")
CASES = [
    Case("smallest", (2, 1, 1), (1, 1), (), (), (0,), "lds", "one pair, d = 1, one sample, vocabularies of one row"),
    Case("ragged", (3, 5, 33), None, (), (), (0,), "lds", "d not a multiple of 4: the scalar gather"),
    Case("vec", (4, 4, 3), None, (), (), (0,), "lds", "d % 4 == 0: the 16-B gather"),
    Case("dup", (3, 8, 300), (1, 2, 40), (), (), (0,), "lds", "every atomic of a field lands on one or two rows"),
    Case("tiles", (9, 8, 700), None, (), (), (0, 1), "lds", "many tiles; with max_blocks = 1 one workgroup walks them all"),
    Case("pooled", (5, 8, 70), None, (2, 4), (), (0,), "lds", "a middle and the last field pre-pooled, in buffers with a padded row pitch"),
    Case("frozen", (3, 5, 33), None, (), (1,), (0,), "lds", "ragged with field 1 frozen: a NULL gradient pointer"),
    Case("criteo4", (26, 4, 130), None, (), (), (0,), "lds", "the Criteo shape at the reference's default embedding_dim"),
    Case("criteo16", (26, 16, 67), None, (), (), (0,), "lds", "the Criteo shape at d = 16: one sample per tile"),
    Case("direct", (60, 16, 6), None, (), (), (0,), "direct", "226 KB of rows per sample: past the LDS"),
]
CASE_BY_NAME = {c.name: c for c in CASES}
# (case, forced route, reduce_sum, max_blocks): every LDS case also with the direct route forced, each with reduce_sum off and on
RUNS = [(c.name, route, reduce_sum, mb) for c in CASES for route in ((None, "direct") if c.route == "lds" else (None,))
        for reduce_sum in (False, True) for mb in c.max_blocks]
RUN_IDS = ["%s-%s-%s-mb%d" % (n, r or "auto", "sum" if s else "cat", mb) for n, r, s, mb in RUNS]
PAD = 5             # extra columns behind a pre-pooled field's (F-1)*d
_INPUTS = {}
_ORACLE = {}


def case_vocab(case):
    F = case.shape[0]
    return list(case.vocab) if case.vocab else [37 + 3 * j for j in range(F)]


def ids_dtype(case):
    """int32 / int64 alternate from case to case."""
    return np.int64 if [c.name for c in CASES].index(case.name) % 2 else np.int32


def case_inputs(case, reduce_sum):
    """(ids [F, B], masters, g [B, W], pooled {j: [B, (F-1)*d + PAD]}) of a case, float32 values, the same at every call."""
    key = (case.name, bool(reduce_sum))
    if key in _INPUTS:
        return _INPUTS[key]
    F, d, B = case.shape
    P, R = F * (F - 1) // 2, (F - 1) * d
    vocab = case_vocab(case)
    rng = np.random.RandomState(zlib.crc32(("ffm_bwd/%s" % case.name).encode()) % (2 ** 31))
    masters = [rng.standard_normal((vocab[j], F - 1, d)).astype(np.float32) for j in range(F)]
    ids = np.stack([rng.randint(0, vocab[j], B) for j in range(F)]).astype(ids_dtype(case))
    pooled = {j: rng.standard_normal((B, R + PAD)).astype(np.float32) for j in case.pooled}
    g = rng.standard_normal((B, P * d)).astype(np.float32)
    if reduce_sum:
        g = np.ascontiguousarray(g[:, :P])
    for a in masters + [ids, g] + list(pooled.values()):
        a.setflags(write=False)
    _INPUTS[key] = (ids, masters, g, pooled)
    return _INPUTS[key]


def oracle(case, reduce_sum):
    """ffm_bwd of a case, computed once and shared (read-only)."""
    key = (case.name, bool(reduce_sum))
    if key not in _ORACLE:
        ids, masters, g, pooled = case_inputs(case, reduce_sum)
        R = (case.shape[0] - 1) * case.shape[1]
        G, T = ffm_bwd(ids, masters, g, reduce_sum, {j: v[:, :R] for j, v in pooled.items()}, case.frozen)
        for a in G + T:
            if a is not None:
                a.setflags(write=False)
        _ORACLE[key] = (G, T)
    return _ORACLE[key]
