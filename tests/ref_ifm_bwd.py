"""Float64 NumPy oracle of dctr_ifm_bwd (include/dctr.h), closed form, no autograd.  Per sample, with e [F, d] the embeddings, m the
factor THE CALLER HANDS OVER (the float32 factor_out of the forward: the op does not project or exponentiate again, so neither does
the oracle), t the first-order terms and g = d_out[b]:

    S[c]    = sum_f m[f] e[f,c]              u[f,c] = S[c] - m[f] e[f,c]
    dm[f]   = sum_c e[f,c] u[f,c] + t[f]
    dx[f,c] = g m[f] u[f,c]                  dterms[f] = g m[f]
    dm'[f]  = softmax ? g m[f] (dm[f] - (1/F) sum_h m[h] dm[h]) : g dm[f]
    dact_s  = dm' kernel_s^T                 dkernel_s = act_s^T dm'

``absolute=True`` returns, per output element, the sum of the magnitudes of its summands (the ``terms`` of
tests.util.assert_close_terms): every product by the product of the magnitudes, every sum and difference by the sum of the magnitudes —
u is formed as S - m e, so its magnitude holds both."""
import numpy as np


def ifm_bwd(x, fields, dim, m, d_out, sources=(), terms=None, softmax=False, absolute=False):
    """x [B, >= F*d], m [B, F], d_out [B], sources [(act [B,K], kernel [K,F])], terms [B,F] or None ->
    dict(dx [B,F,d], dterms [B,F], dmprime [B,F], dact [per source [B,K]], dkernel [per source [K,F]])."""
    F, d = int(fields), int(dim)
    f64 = lambda a: np.asarray(a, dtype=np.float64)       # noqa: E731
    pos = np.abs if absolute else (lambda a: a)
    B = x.shape[0]
    e = pos(f64(x)[:, :F * d].reshape(B, F, d))
    m = pos(f64(m)[:, :F])
    g = pos(f64(d_out).reshape(B))
    t = np.zeros((B, F)) if terms is None else pos(f64(terms)[:, :F])
    me = m[:, :, None] * e
    S = me.sum(1, keepdims=True)
    u = S + me if absolute else S - me
    dm = (e * u).sum(-1) + t
    gm = g[:, None] * m
    out = dict(dx=gm[:, :, None] * u, dterms=gm)
    if softmax:
        mean = (m * dm).sum(-1, keepdims=True) / F
        dmp = gm * (dm + mean if absolute else dm - mean)
    else:
        dmp = g[:, None] * dm
    out["dmprime"] = dmp
    out["dact"] = [dmp @ pos(f64(kernel)).T for _, kernel in sources]
    out["dkernel"] = [pos(f64(act)).T @ dmp for act, _ in sources]
    return out


def factor(mprime, sources, softmax, F):
    """float64: m' = mprime + sum_s act_s kernel_s; m = F * softmax(m') or m'."""
    mp = np.zeros((sources[0][0].shape[0] if sources else mprime.shape[0], F)) if mprime is None else np.asarray(mprime, np.float64)[:, :F]
    for act, kernel in sources:
        mp = mp + np.asarray(act, np.float64) @ np.asarray(kernel, np.float64)
    if not softmax:
        return mp
    ex = np.exp(mp - mp.max(axis=1, keepdims=True))
    return F * ex / ex.sum(axis=1, keepdims=True)


# F, d, B, K per source, dmprime wanted (m' handed over in the forward), first-order terms, extra columns behind every matrix
SWEEP = [
    (1, 1, 5, (3,), False, True, 0), (2, 3, 17, (), True, True, 3), (3, 5, 33, (7, 21), False, False, 5), (5, 2, 64, (64,), True, True, 0),
    (13, 17, 40, (65, 130), False, True, 7), (16, 16, 129, (16,), False, True, 0), (7, 64, 21, (100,), False, True, 1),
    (5, 33, 9, (19,), False, True, 3), (3, 130, 6, (8,), False, True, 2), (64, 1, 70, (5,), False, True, 0),
    (65, 3, 66, (33, 31), False, False, 1), (600, 2, 19, (40,), False, True, 1), (39, 4, 1001, (64,), False, True, 0),
    (39, 4, 257, (2496, 64), False, True, 0),
]


def case(F, d, B, Ks, mprime, terms, pad, softmax, seed=None):
    """Random float32 operands of one call, each matrix ``pad`` columns wider than what is read: dict(x, m, d_out, sources, terms,
    mprime) — m is the float32 factor of the float64 m' of these operands, as the forward would have saved it."""
    rng = np.random.RandomState(F * 1000 + d if seed is None else seed)
    x = (rng.standard_normal((B, F * d + pad)) * 0.5).astype(np.float32)
    sources = []
    for K in Ks:
        act = rng.standard_normal((B, K + pad)).astype(np.float32)
        w = (rng.standard_normal((K, F)) / np.sqrt(K)).astype(np.float32)
        sources.append((act, w))
    mp = rng.standard_normal((B, F)).astype(np.float32) if (mprime or not Ks) else None
    m = np.zeros((B, F + pad), dtype=np.float32)
    m[:, :F] = factor(mp, [(a[:, :a.shape[1] - pad], w) for a, w in sources], softmax, F)
    t = None
    if terms:
        t = (rng.standard_normal((B, F + pad)) * 0.3).astype(np.float32)
    d_out = (rng.standard_normal(B) * 0.5).astype(np.float32)
    return dict(x=x, m=m, d_out=d_out, sources=sources, terms=t, mprime=mp, pad=pad)


def oracle(c, F, d, softmax, absolute=False):
    pad = c["pad"]
    srcs = [(a[:, :a.shape[1] - pad], w) for a, w in c["sources"]]
    return ifm_bwd(c["x"], F, d, c["m"], c["d_out"], srcs, c["terms"], softmax, absolute)
