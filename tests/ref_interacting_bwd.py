"""What tests/test_gpu_interacting_bwd.py and tests/test_interacting_bwd_oracle_cpu.py share:
  1. a float64 NumPy oracle, closed form and without autograd, of dctr_interacting_bwd (deepctr_amd/csrc/interacting_bwd_kernels.hip):
     the backward of the InteractingLayer stack of AutoInt / DIFM, restated from the contract in include/dctr.h;
  2. a restatement of the host arithmetic that sizes a workgroup's tile, picks the route and sizes the workspace;
  3. the table of cases the GPU test runs, each with what it is there for, and their inputs.
The CPU test pins 1 against torch double autograd over training._interacting and 2 and 3 against the library's host-only calls.

The oracle returns (grads, terms) in the convention of tests/ref_interaction_bwd.py.  ``terms`` is the input of
tests.util.assert_close_terms: the same backward over absolute values, an upper bound of the magnitude each output element was summed
at.  The forward's own intermediates (X_l, Q, K, V, the softmax P and the ReLU mask) enter it as |true float64 value|."""
import collections
import zlib

import numpy as np


def _f64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


class Layer(object):
    """What training._interacting reads of an InteractingLayer: the options and w(name)."""

    def __init__(self, weights, d, H, use_res, scaling):
        self.att_embedding_size, self.head_num, self.use_res, self.scaling = d, H, use_res, scaling
        self._w = dict(zip(("query", "key", "value", "res"), weights))

    def w(self, name):
        return self._w[name]

    @property
    def weights_qkvr(self):
        return (self._w["query"], self._w["key"], self._w["value"], self._w.get("res") if self.use_res else None)


def forward(x, weights, d, H, use_res, scaling):
    """The stack in float64.  x [B, F, E]; weights: per layer (query, key, value, res) [E_l, d*H].  Returns one dict per layer: X (the
    input), Q, K, V [B, F, H, d], P [B, H, F, F], Z [B, F, d*H] (the pre-activation), tZ (the magnitude Z was summed at: P (|X| |W_v|) +
    |X| |W_res|) — and the last layer's output."""
    X = _f64(x)
    B, F = X.shape[:2]
    s = 1.0 / np.sqrt(d) if scaling else 1.0
    out = []
    for W in weights:
        Wq, Wk, Wv = (_f64(w) for w in W[:3])
        Q, K, V = ((X @ w).reshape(B, F, H, d) for w in (Wq, Wk, Wv))
        S = np.einsum("bihc,bjhc->bhij", Q, K) * s
        e = np.exp(S - S.max(-1, keepdims=True))
        P = e / e.sum(-1, keepdims=True)
        Z = np.einsum("bhij,bjhc->bihc", P, V).reshape(B, F, H * d)
        tZ = np.einsum("bhij,bjhc->bihc", P, (np.abs(X) @ np.abs(Wv)).reshape(B, F, H, d)).reshape(B, F, H * d)
        if use_res:
            Z = Z + X @ _f64(W[3])
            tZ = tZ + np.abs(X) @ np.abs(_f64(W[3]))
        out.append(dict(X=X, Q=Q, K=K, V=V, P=P, Z=Z, tZ=tZ))
        X = np.maximum(Z, 0.0)
    return out, X


def interacting_bwd(x, weights, d, H, use_res, scaling, dy, drop_delta=False):
    """dctr_interacting_bwd (include/dctr.h).  Per layer, last to first, with s = 1 / sqrt(d) when scaling else 1:
        dZ = dY [Z > 0];  dV_h = P_h^T dZ_h;  dP = dZ_h V_h^T;  delta_i = sum_j P_ij dP_ij;  dS = s P (dP - delta)
        dQ_h = dS K_h;  dK_h = dS^T Q_h;  dX = dQ W_q^T + dK W_k^T + dV W_v^T (+ dZ W_res^T);  dW_m = sum_b X^T dM
    x [B, F, E], dy [B, F * d*H].  Returns grads / terms with the keys dx [B, F, E] and d{query,key,value,res}{l}.
    ``drop_delta``: the softmax backward without its row term — the wrong restatement of the CPU test."""
    layers, _ = forward(x, weights, d, H, use_res, scaling)
    B, F = layers[0]["X"].shape[:2]
    dH = d * H
    s = 1.0 / np.sqrt(d) if scaling else 1.0
    g = _f64(dy).reshape(B, F, dH)
    t = np.abs(g)
    G, T = {}, {}
    for l in range(len(weights) - 1, -1, -1):
        c = layers[l]
        X, Q, K, V, P = c["X"], c["Q"], c["K"], c["V"], c["P"]
        aX, aQ, aK, aV = np.abs(X), np.abs(Q), np.abs(K), np.abs(V)
        mask = (c["Z"] > 0).astype(np.float64)
        dZ, tdZ = g * mask, t * mask
        dZh, tdZh = dZ.reshape(B, F, H, d), tdZ.reshape(B, F, H, d)
        dV, tdV = np.einsum("bhij,bihc->bjhc", P, dZh), np.einsum("bhij,bihc->bjhc", P, tdZh)
        dP, tdP = np.einsum("bihc,bjhc->bhij", dZh, V), np.einsum("bihc,bjhc->bhij", tdZh, aV)
        delta, tdelta = (P * dP).sum(-1, keepdims=True), (P * tdP).sum(-1, keepdims=True)
        if drop_delta:
            delta = 0.0 * delta
        dS, tdS = s * P * (dP - delta), s * P * (tdP + tdelta)
        dQ, tdQ = np.einsum("bhij,bjhc->bihc", dS, K), np.einsum("bhij,bjhc->bihc", tdS, aK)
        dK, tdK = np.einsum("bhij,bihc->bjhc", dS, Q), np.einsum("bhij,bihc->bjhc", tdS, aQ)
        parts = [("query", dQ.reshape(B, F, dH), tdQ.reshape(B, F, dH)), ("key", dK.reshape(B, F, dH), tdK.reshape(B, F, dH)),
                 ("value", dV.reshape(B, F, dH), tdV.reshape(B, F, dH))]
        if use_res:
            parts.append(("res", dZ, tdZ))
        g, t = 0.0, 0.0
        for m, (name, dM, tdM) in enumerate(parts):
            W = _f64(weights[l][m])
            G["d%s%d" % (name, l)] = np.einsum("bfe,bfc->ec", X, dM)
            T["d%s%d" % (name, l)] = np.einsum("bfe,bfc->ec", aX, tdM)
            g = g + dM @ W.T
            t = t + tdM @ np.abs(W).T
    G["dx"], T["dx"] = g, t
    return G, T


def relu_margin(x, weights, d, H, use_res, scaling):
    """The smallest |Z| / (the magnitude Z was summed at) over every layer and element: an fp32 kernel recomputes Z and an element
    within rounding of zero could take the other ReLU branch than the oracle.  An element whose summed magnitude is exactly zero (every
    field of the sample came out of the ReLU below as zero, and there is no residual: d1_h1 has such samples) is zero in any arithmetic
    and on the same branch in both; it counts as infinitely far."""
    return float(sample_margins(x, weights, d, H, use_res, scaling).min())


def sample_margins(x, weights, d, H, use_res, scaling):
    """relu_margin per sample [B] (a sample's Z depends on no other sample)."""
    layers, _ = forward(x, weights, d, H, use_res, scaling)
    worst = np.full(layers[0]["X"].shape[0], np.inf)
    for c in layers:
        live = c["tZ"] > 0
        assert (c["Z"][~live] == 0).all()
        ratio = np.where(live, np.abs(c["Z"]) / np.where(live, c["tZ"], 1.0), np.inf)
        worst = np.minimum(worst, ratio.min((1, 2)))
    return worst


# ---------------------------------------------------------------------------------------------------
# the host's plan (interacting_bwd_kernels.hip: ib_plan)
# ---------------------------------------------------------------------------------------------------
LDS_TARGET, LDS_MAX = 80 * 1024, 160 * 1024
GLOBAL_WGS, GLOBAL_MAX = 256, 256 << 20
MAX_LAYERS, MAX_S = 32, 16

Plan = collections.namedtuple("Plan", "supported route S tile_bytes workspace_bytes")


def _align(v, a):
    return (v + a - 1) // a * a


def plan(F, E, d, H, L, use_res):
    """A workgroup's buffers: the inputs of the L layers and dZ, dQ, dK, dV ([rows padded to 16, ldx] each), Q, K, V ([S*F, ldq]), three
    softmax statistics per (row, head), and the sums of every weight gradient.  The largest S <= 16 within 80 KiB; S = 1 up to 160 KiB;
    beyond that S = 1 in a per-workgroup slice of the workspace (<= 256 slices, <= 256 MiB unless one slice is larger)."""
    if L > MAX_LAYERS:
        return Plan(False, None, 0, 0, 0)
    dH = d * H
    ldx, ldq, nb = _align(max(E, dH), 16) + 4, dH | 1, 4 if use_res else 3
    acc = _align(nb * (E + (L - 1) * dH) * dH, 4)

    def tile(S):
        sf = S * F
        return (_align((L + 4) * _align(sf, 16) * ldx + 3 * sf * ldq + 3 * sf * H, 4) + acc) * 4
    S = MAX_S
    while S > 1 and tile(S) > LDS_TARGET:
        S -= 1
    tb = tile(S)
    if tb <= LDS_MAX:
        return Plan(True, "lds", S, tb, 0)
    slices = min(max(GLOBAL_MAX // tb, 1), GLOBAL_WGS)
    return Plan(True, "workspace", 1, tb, tb * slices)


# ---------------------------------------------------------------------------------------------------
# the cases: (F, E, d, H, L, use_res, scaling, B), max_blocks, the route they are there for, what they exercise
# ---------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name shape max_blocks route why")
CASES = [
    Case("one_field", (1, 3, 8, 2, 1, True, False, 5), 0, "lds", "a single field"),
    Case("d1_h1", (2, 4, 1, 1, 2, False, True, 33), 0, "lds", "d = 1 and H = 1, scaling, three tiles"),
    Case("three_layers", (4, 3, 8, 2, 3, True, True, 5), 0, "lds", "three layers, scaling with the residual"),
    Case("d17", (5, 6, 17, 3, 2, True, False, 40), 0, "lds", "d past 16 (two passes per head), odd d*H"),
    Case("criteo", (26, 16, 8, 2, 3, True, False, 70), 0, "lds", "the Criteo shape, a ragged last tile"),
    Case("criteo_walk", (26, 16, 8, 2, 3, True, False, 300), 3, "lds", "3 workgroups walk the tiles and sum weight gradients across them"),
    Case("no_res", (39, 32, 16, 4, 2, False, False, 19), 0, "workspace",
         "no residual, four column tiles; 72 KiB of weight-gradient sums push one sample's buffers past 160 KiB"),
    Case("past_lds", (200, 32, 16, 4, 1, True, False, 6), 0, "workspace", "a sample past the LDS: buffers in the workspace"),
]
CASE_BY_NAME = {c.name: c for c in CASES}
RELU_MARGIN = 1e-5
_INPUTS = {}


def case_inputs(case):
    """(x [B, F, E], weights per layer, dy [B, F * d*H]) of a case, float32 values, the same at every call.  Weights of unit row scale
    keep the softmax away from uniform, dy is of order one.  With 10^5 .. 10^6 pre-activations a draw nearly always holds a few within
    RELU_MARGIN of zero: the samples that do are drawn again (from the same seeded stream, a sample's Z depends on no other sample)
    until none is left, so the condition of relu_margin holds for every element of what is returned."""
    if case.name in _INPUTS:
        return _INPUTS[case.name]
    F, E, d, H, L, use_res, scaling, B = case.shape
    rng = np.random.RandomState(zlib.crc32(case.name.encode()) % (2 ** 31))
    dH = d * H
    weights, K = [], E
    for _ in range(L):
        weights.append([(rng.randn(K, dH) * (1.2 / np.sqrt(K))).astype(np.float32) for _ in range(4 if use_res else 3)])
        K = dH
    dy = rng.randn(B, F * dH).astype(np.float32)
    x = rng.randn(B, F, E).astype(np.float32)
    for _ in range(64):
        bad = np.nonzero(sample_margins(x, weights, d, H, use_res, scaling) <= 2 * RELU_MARGIN)[0]
        if not len(bad):
            break
        x[bad] = rng.randn(len(bad), F, E).astype(np.float32)
    for a in [x, dy] + [w for layer in weights for w in layer]:
        a.setflags(write=False)
    _INPUTS[case.name] = (x, weights, dy)
    return _INPUTS[case.name]
