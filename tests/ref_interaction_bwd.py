"""What tests/test_gpu_interaction_bwd.py and tests/test_interaction_bwd_oracle_cpu.py share:
  1. float64 NumPy oracles, closed form and without autograd, of the backward ops between dctr_mlp_bwd and the embedding scatter of NFM,
     PNN, AFM, DCN and DCNMix: dctr_bi_interaction_bwd, dctr_inner_product_bwd, dctr_afm_bwd (deepctr_amd/csrc/interaction_bwd_kernels.hip),
     dctr_crossnet_bwd (vector and matrix) and dctr_crossnet_mix_bwd (deepctr_amd/csrc/crossnet_bwd_kernels.hip);
  2. a restatement of the host arithmetic that picks each op's route and sizes its workspace;
  3. the table of cases the GPU test runs, each with the route it is there for.
The CPU test pins 1 against torch double autograd and 2 and 3 against the library's host-only calls.

Every oracle restates the CONTRACT in the header comment of its kernels and returns (grads, terms).  ``terms`` is the input of
tests.util.assert_close_terms: the same backward over absolute values, an upper bound of the magnitude each output element was summed
at.  The forward's own intermediates (x_l, s_l, u_l, v1, v2, p; AFM's alpha, t, y and ReLU mask) enter it as |true float64 value|: a
forward recurrence run over absolute values would grow to 10^3 .. 10^4 x |ref| at d >= 1000 and the bar would mean nothing."""
import collections
import zlib

import numpy as np


def _f64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


def pair_indices(F):
    """Pairs (i, j), i < j, ordered by i then j (itertools.combinations), as the kernels number them."""
    ii = [i for i in range(F - 1) for _ in range(i + 1, F)]
    jj = [j for i in range(F - 1) for j in range(i + 1, F)]
    return np.asarray(ii, dtype=np.int64), np.asarray(jj, dtype=np.int64)


# ---------------------------------------------------------------------------------------------------
# the oracles
# ---------------------------------------------------------------------------------------------------
def bi_interaction_bwd(x, dy):
    """BiInteractionPooling, y[b, e] = 0.5 ((sum_f x)^2 - sum_f x^2)  (interaction_bwd_kernels.hip:15):
        dx[b, f, e] = dy[b, e] (sum_f' x[b, f', e] - x[b, f, e])
    x [B, F, E], dy [B, E].  The contract IS the difference (at F = 1 it is an exact zero): its terms are |dy| (sum_f' |x| + |x_f|)."""
    x, dy = _f64(x), _f64(dy)
    s, a = x.sum(1, keepdims=True), np.abs(x)
    return {"dx": dy[:, None, :] * (s - x)}, {"dx": np.abs(dy)[:, None, :] * (a.sum(1, keepdims=True) + a)}


def inner_product_bwd(x, dy):
    """InnerProductLayer(reduce_sum), y[b, p(i, j)] = <x_i, x_j>  (interaction_bwd_kernels.hip:37):
        dx[b, i, e] = sum_{j != i} dy[b, p(min(i, j), max(i, j))] x[b, j, e]
    x [B, F, E], dy [B, F (F - 1) / 2]."""
    x, dy = _f64(x), _f64(dy)
    B, F, E = x.shape
    ii, jj = pair_indices(F)
    G = np.zeros((B, F, F))
    G[:, ii, jj] = dy
    G[:, jj, ii] = dy
    return {"dx": np.einsum("bij,bje->bie", G, x)}, {"dx": np.einsum("bij,bje->bie", np.abs(G), np.abs(x))}


def afm_forward(x, W, b, h, p):
    """AFMLayer.call (reference layers/interaction.py:116-146) in float64: bi [B, P, E], pre [B, P, A], alpha [B, P], t [B, P], y [B]."""
    x, W, b, h, p = _f64(x), _f64(W), _f64(b).reshape(-1), _f64(h).reshape(-1), _f64(p).reshape(-1)
    ii, jj = pair_indices(x.shape[1])
    bi = x[:, ii] * x[:, jj]
    pre = bi @ W + b
    s = np.maximum(pre, 0.0) @ h
    e = np.exp(s - s.max(1, keepdims=True))
    alpha = e / e.sum(1, keepdims=True)
    t = bi @ p
    return bi, pre, alpha, t, (alpha * t).sum(1)


def afm_bwd(x, W, b, h, p, dy, drop_last_pair=False):
    """AFMLayer backward (interaction_bwd_kernels.hip:59-64; reference layers/interaction.py:116-146).  With bi_p = x_i .* x_j,
    pre_pa = b_a + sum_e bi_pe W_ea, s_p = sum_a relu(pre_pa) h_a, alpha = softmax_p(s), t_p = bi_p . proj_p, y = sum_p alpha_p t_p, g = dy:
        ds_p = alpha_p (g t_p - g y);  d pre_pa = ds_p h_a [pre_pa > 0];  d bi_pe = g alpha_p proj_p[e] + sum_a d pre_pa W_ea
        d x_i += d bi_p .* x_j;  d x_j += d bi_p .* x_i
        d proj_p[e] = sum_{b, p} g alpha_p bi_pe;  d proj_h[a] = sum ds_p relu(pre_pa);  d b[a] = sum d pre_pa;  d W[e, a] = sum bi_pe d pre_pa
    x [B, F, E], W [E, A], b [A], h [A], p [E], dy [B].  ``drop_last_pair``: the last pair contributes to no sum of the backward (the
    forward is whole) — the wrong restatement of the CPU test."""
    x, W, h, p, dy = _f64(x), _f64(W), _f64(h).reshape(-1), _f64(p).reshape(-1), _f64(dy).reshape(-1)
    B, F, E = x.shape
    ii, jj = pair_indices(F)
    bi, pre, alpha, t, y = afm_forward(x, W, b, h, p)
    mask = (pre > 0).astype(np.float64)
    g = dy[:, None]
    live = np.ones(len(ii))
    if drop_last_pair:
        live[-1] = 0.0
    ax, abi, aW, ah, ap, ag = np.abs(x), np.abs(bi), np.abs(W), np.abs(h), np.abs(p), np.abs(g)
    ds = alpha * g * (t - y[:, None]) * live
    tds = alpha * ag * (np.abs(t) + np.abs(y)[:, None]) * live
    ga, tga = g * alpha * live, ag * alpha * live
    dpre, tdpre = ds[:, :, None] * h * mask, tds[:, :, None] * ah * mask
    dbi, tdbi = ga[:, :, None] * p + dpre @ W.T, tga[:, :, None] * ap + tdpre @ aW.T
    G = {"dp": np.einsum("bp,bpe->e", ga, bi), "dh": np.einsum("bp,bpa->a", ds, np.maximum(pre, 0.0)), "db": dpre.sum((0, 1)),
         "dW": np.einsum("bpe,bpa->ea", bi, dpre), "dx": np.zeros((B, F, E))}
    T = {"dp": np.einsum("bp,bpe->e", tga, abi), "dh": np.einsum("bp,bpa->a", tds, np.maximum(pre, 0.0)), "db": tdpre.sum((0, 1)),
         "dW": np.einsum("bpe,bpa->ea", abi, tdpre), "dx": np.zeros((B, F, E))}
    for k in range(len(ii)):                                        # (np.add.at over [B, P, E] is slower than this walk)
        i, j = ii[k], jj[k]
        G["dx"][:, i] += dbi[:, k] * x[:, j]
        G["dx"][:, j] += dbi[:, k] * x[:, i]
        T["dx"][:, i] += tdbi[:, k] * ax[:, j]
        T["dx"][:, j] += tdbi[:, k] * ax[:, i]
    return G, T


def afm_kink_margin(x, W, b):
    """Per sample, the smallest |pre| in float32 ulp (2^-23) of its summed magnitude |bi| . |W| + |b|: the kernel recomputes pre in
    float32, an element within rounding of zero could take the other ReLU branch than the oracle."""
    x, W, b = _f64(x), _f64(W), _f64(b).reshape(-1)
    ii, jj = pair_indices(x.shape[1])
    bi = x[:, ii] * x[:, jj]
    return (np.abs(bi @ W + b) / ((np.abs(bi) @ np.abs(W) + np.abs(b)) * 2.0 ** -23 + 1e-300)).min((1, 2))


def crossnet_forward(x, kernels, bias, mode):
    """CrossNet.call (reference layers/interaction.py:405-424) in float64.  vector: s_l = x_l . w_l, x_{l+1} = x0 s_l + b_l + x_l;
    matrix: u_l = x_l W_l^T, x_{l+1} = x0 .* (u_l + b_l) + x_l.  Returns (xs [x_0 .. x_L], s or u per layer)."""
    x0 = _f64(x)
    xs, mids = [x0], []
    for l in range(0 if kernels is None else len(kernels)):
        w, b = _f64(kernels[l]), _f64(bias[l])
        if mode == "vector":
            m = xs[-1] @ w                                          # [B]
            xs.append(x0 * m[:, None] + b + xs[-1])
        else:
            m = xs[-1] @ w.T                                        # [B, d]
            xs.append(x0 * (m + b) + xs[-1])
        mids.append(m)
    return xs, mids


def crossnet_bwd(x, kernels, bias, mode, dy, corrupt=None):
    """CrossNet backward (crossnet_bwd_kernels.hip: the "CrossNet backward" comment block above cross_vector_bwd_kernel and the comment of
    cross_matrix_bwd_elem_kernel; reference layers/interaction.py:405-424), g = dy, l = L - 1 .. 0:
      vector: ds = g . x0;  d b_l += sum_b g;  d w_l += sum_b ds x_l;  d x0 += g s_l;  g += ds w_l
      matrix: du = g .* x0;  d x0 += g .* (u_l + b_l);  d b_l += sum_b du;  d W_l[n, k] += sum_b du[b, n] x_l[b, k];  g += du W_l
    and d x0 += g at the end (x_0 is the first x_l too).  x [B, d], kernels [L, d] or [L, d, d], bias [L, d], dy [B, d].
    ``corrupt``: "ds_col" — the last layer's ds (vector) / g W step (matrix) leaves out column d - 1;  "dw_row" — d kernels of layer 0
    leaves out batch row B - 1: the wrong restatements of the CPU test."""
    x0, dy = _f64(x), _f64(dy)
    L = 0 if kernels is None else len(kernels)
    xs, mids = crossnet_forward(x0, kernels, bias, mode)
    a0 = np.abs(x0)
    g, tg = dy.copy(), np.abs(dy)
    dx0, tdx0 = np.zeros_like(x0), np.zeros_like(x0)
    dk, tk, db, tb = [None] * L, [None] * L, [None] * L, [None] * L
    for l in range(L - 1, -1, -1):
        w, aw, xl, axl, m = _f64(kernels[l]), np.abs(_f64(kernels[l])), xs[l], np.abs(xs[l]), mids[l]
        rows = slice(0, x0.shape[0] - 1) if corrupt == "dw_row" and l == 0 else slice(None)
        cols = slice(0, x0.shape[1] - 1) if corrupt == "ds_col" and l == L - 1 else slice(None)
        if mode == "vector":
            ds, tds = (g[:, cols] * x0[:, cols]).sum(1), (tg[:, cols] * a0[:, cols]).sum(1)
            db[l], tb[l] = g.sum(0), tg.sum(0)
            dk[l], tk[l] = ds[rows] @ xl[rows], tds[rows] @ axl[rows]
            dx0 += g * m[:, None]
            tdx0 += tg * np.abs(m)[:, None]
            g, tg = g + ds[:, None] * w, tg + tds[:, None] * aw
        else:
            b = _f64(bias[l])
            du, tdu = g * x0, tg * a0
            dx0 += g * (m + b)
            tdx0 += tg * (np.abs(m) + np.abs(b))
            db[l], tb[l] = du.sum(0), tdu.sum(0)
            dk[l], tk[l] = du[rows].T @ xl[rows], tdu[rows].T @ axl[rows]
            g, tg = g.copy(), tg.copy()
            g[:, cols] += (du @ w)[:, cols]
            tg[:, cols] += (tdu @ aw)[:, cols]
    G = {"dx": dx0 + g, "dk": np.stack(dk) if L else None, "db": np.stack(db) if L else None}
    T = {"dx": tdx0 + tg, "dk": np.stack(tk) if L else None, "db": np.stack(tb) if L else None}
    return G, T


def mix_forward(x, U, V, C, G, bias):
    """CrossNetMix.call (reference layers/interaction.py:511-549) in float64.  U, V [L, ne, d, r], C [L, ne, r, r], G [ne, d], bias [L, d].
    Returns xs [x_0 .. x_L] and per layer (v1 [ne, B, r], v2 [ne, B, r], uv [ne, B, d], p [B, ne])."""
    x0 = _f64(x)
    U, V, C, G, bias = _f64(U), _f64(V), _f64(C), _f64(G), _f64(bias)
    xs, mids = [x0], []
    for l in range(U.shape[0]):
        xl = xs[-1]
        v1 = np.tanh(np.einsum("bi,eij->ebj", xl, V[l]))
        v2 = np.tanh(np.einsum("ebk,ejk->ebj", v1, C[l]))
        uv = np.einsum("ebj,eij->ebi", v2, U[l])
        s = xl @ G.T
        e = np.exp(s - s.max(1, keepdims=True))
        p = e / e.sum(1, keepdims=True)
        xs.append(np.einsum("be,ebi->bi", p, x0[None] * (uv + bias[l])) + xl)
        mids.append((v1, v2, uv, p))
    return xs, mids


def crossnet_mix_bwd(x, U, V, C, G, bias, dy, corrupt=None):
    """CrossNetMix backward (crossnet_bwd_kernels.hip: the "CrossNetMix backward" comment block above mix_copy_rows_kernel; reference
    layers/interaction.py:511-549).  Per layer l and expert e, with
    v1 = tanh(x_l V_e), v2 = tanh(v1 C_e^T), uv_e = v2 U_e^T, out_e = x_0 .* (uv_e + b_l), p = softmax_e(x_l . g_e), g the gradient of x_{l+1}:
        dp_e = g . out_e;  ds_e = p_e (dp_e - sum_e' p_e' dp_e');  t_e = p_e g .* x_0
        d b_l += sum_b g .* x_0;  d U_e += t_e^T v2;  d v2 = t_e U_e;  a2 = d v2 .* (1 - v2^2);  d C_e += a2^T v1
        d v1 = a2 C_e;  a1 = d v1 .* (1 - v1^2);  d V_e += x_l^T a1;  d g_e += x_l^T ds_e
        d x_l = g + sum_e (ds_e (x) g_e + a1 V_e^T);  d x_0 += sum_e p_e g .* (uv_e + b_l)
    ``corrupt``: "gate_col" — the last layer's dp_e leaves out column d - 1;  "dw_row" — d V of layer 0 leaves out batch row B - 1."""
    x0, dy = _f64(x), _f64(dy)
    U, V, C, G, bias = _f64(U), _f64(V), _f64(C), _f64(G), _f64(bias)
    L = U.shape[0]
    xs, mids = mix_forward(x0, U, V, C, G, bias)
    a0, aU, aV, aC, aG = np.abs(x0), np.abs(U), np.abs(V), np.abs(C), np.abs(G)
    g, tg = dy.copy(), np.abs(dy)
    dx0, tdx0 = np.zeros_like(x0), np.zeros_like(x0)
    out = {k: np.zeros_like(a) for k, a in (("dU", U), ("dV", V), ("dC", C), ("dG", G), ("db", bias))}
    trm = {k: np.zeros_like(a) for k, a in out.items()}
    for l in range(L - 1, -1, -1):
        xl, axl = xs[l], np.abs(xs[l])
        v1, v2, uv, p = mids[l]
        av1, av2 = np.abs(v1), np.abs(v2)
        cols = slice(0, x0.shape[1] - 1) if corrupt == "gate_col" and l == L - 1 else slice(None)
        rows = slice(0, x0.shape[0] - 1) if corrupt == "dw_row" and l == 0 else slice(None)
        oute, aoute = x0[None] * (uv + bias[l]), a0[None] * (np.abs(uv) + np.abs(bias[l]))
        dp, tdp = np.einsum("bi,ebi->be", g[:, cols], oute[:, :, cols]), np.einsum("bi,ebi->be", tg[:, cols], aoute[:, :, cols])
        ds, tds = p * (dp - (p * dp).sum(1, keepdims=True)), p * (tdp + (p * tdp).sum(1, keepdims=True))
        t, tt = p.T[:, :, None] * (g * x0)[None], p.T[:, :, None] * (tg * a0)[None]                   # [ne, B, d]
        out["db"][l], trm["db"][l] = (g * x0).sum(0), (tg * a0).sum(0)
        out["dU"][l], trm["dU"][l] = np.einsum("ebi,ebj->eij", t, v2), np.einsum("ebi,ebj->eij", tt, av2)
        a2, ta2 = np.einsum("ebi,eij->ebj", t, U[l]) * (1 - v2 * v2), np.einsum("ebi,eij->ebj", tt, aU[l]) * (1 - v2 * v2)
        out["dC"][l], trm["dC"][l] = np.einsum("ebj,ebk->ejk", a2, v1), np.einsum("ebj,ebk->ejk", ta2, av1)
        a1, ta1 = np.einsum("ebj,ejk->ebk", a2, C[l]) * (1 - v1 * v1), np.einsum("ebj,ejk->ebk", ta2, aC[l]) * (1 - v1 * v1)
        out["dV"][l], trm["dV"][l] = np.einsum("bi,ebj->eij", xl[rows], a1[:, rows]), np.einsum("bi,ebj->eij", axl[rows], ta1[:, rows])
        out["dG"] += ds.T @ xl
        trm["dG"] += tds.T @ axl
        dx0 += np.einsum("be,ebi->bi", p, g[None] * (uv + bias[l]))
        tdx0 += np.einsum("be,ebi->bi", p, tg[None] * (np.abs(uv) + np.abs(bias[l])))
        g, tg = g + ds @ G + np.einsum("ebj,eij->bi", a1, V[l]), tg + tds @ aG + np.einsum("ebj,eij->bi", ta1, aV[l])
    out["dx"], trm["dx"] = dx0 + g, tdx0 + tg
    return out, trm


# ---------------------------------------------------------------------------------------------------
# the host arithmetic of the routes and workspace sizes, restated
# ---------------------------------------------------------------------------------------------------
LDS_SOFT, LDS_MAX = 64 * 1024, 160 * 1024          # dynamic LDS a kernel gets without asking / with hipFuncSetAttribute
CAP = {"bi": 8192, "ip": 16384, "vec": 4096, "mat": 4096, "mix": 8192}          # workgroups (of 256) of the elementwise grid-stride loops
MIX_MAX_EXPERTS = 16


def _ceil_div(a, b):
    return -(-a // b)


def _al4(n):
    return (n + 3) // 4 * 4


def afm_bwd_lds_bytes(F, E, A):
    """dctr_afm_bwd: the weights and their gradients once per workgroup, per wave (4) a sample tile, its gradient and the pair scores."""
    nw = E * A + 2 * A + E
    return (2 * nw + 4 * (2 * F * E + F * (F - 1) // 2)) * 4


def cross_vector_lds_bytes(d, L):
    """cross_vector_bwd_kernel: per wave (4) x_l, d w and d b accumulators [L, d] each and s_l [L]."""
    return 4 * (3 * L * d + L) * 4


def cross_vector_bwd_on_chip(d, L):
    return d <= 2048 and cross_vector_lds_bytes(d, L) <= LDS_MAX


def mlp_dw_parts(batch, out_elems):
    """train_common.h:38 — row slices of a dW whose reduction is the batch: 512 rows each from 1024 rows on, lowered until the count
    divides the batch."""
    if batch < 1024:
        return 1
    tiles = max(out_elems // 4096, 1)
    cap = min(max(1024 // tiles, 32), 128)
    parts = min(batch // 512, cap)
    while parts > 1 and batch % parts != 0:
        parts -= 1
    return parts


def k_slices(k, rows_per_slice):
    """gemm_kernels.hip: dctr_gemm::k_slices."""
    if k <= 0:
        return 1
    want = min(max(_ceil_div(k, rows_per_slice if rows_per_slice > 0 else k), 1), 32)
    chunk = _ceil_div(_ceil_div(k, want), 32) * 32
    return _ceil_div(k, chunk)


def mix_k_slices(B):
    """(slices, rows of the last one) of the weight-gradient GEMMs of dctr_crossnet_mix_bwd: k_slices(B, 256), at most 16."""
    ks = min(k_slices(B, 256), 16)
    n = k_slices(B, _ceil_div(B, ks))
    chunk = _ceil_div(_ceil_div(B, n), 32) * 32
    return n, B - (n - 1) * chunk


def crossnet_ws_bytes(mode, B, d, L):
    """dctr_crossnet_bwd_workspace_bytes.  vector, layered: x_1 .. x_{L-1}, g, d x0 [B, d], s_0 .. s_{L-1}, ds [B]; matrix: x_1 .. x_{L-1},
    u_0 .. u_{L-1}, g, du, d x0 [B, d] and the dW slices."""
    if B <= 0 or L <= 0:
        return 0
    if mode == "vector":
        return 0 if cross_vector_bwd_on_chip(d, L) else ((L + 1) * B * d + (L + 1) * B) * 4
    parts = mlp_dw_parts(B, d * d)
    return ((2 * L + 2) * B * d + (parts * d * d if parts > 1 else 0)) * 4


def mix_ws_bytes(B, d, L, ne, r):
    """mix_plan, every piece 4-float aligned: X | V1 | V2 | UV | P | G | GX | T | DX0 | DV2 | DV1 | DS.  L = 0: the wrapper's B d floats."""
    if L == 0:
        return B * d * 4
    return 4 * sum(_al4(n) for n in (L * B * d, L * ne * B * r, L * ne * B * r, L * ne * B * d, L * B * ne, B * d, B * d, ne * B * d, B * d,
                                      ne * B * r, ne * B * r, B * ne))


def library_crossnet_ws_bytes(mode, B, d, L):
    """dctr_crossnet_bwd_workspace_bytes of the library: host arithmetic, no device needed."""
    import ctypes
    from deepctr_amd import _C
    a = _C.CrossBwdArgs(batch=B, dim=d, layers=L, mode=_C.CROSS_VECTOR if mode == "vector" else _C.CROSS_MATRIX, x_stride=d, dy_stride=d,
                        dx_stride=d)
    return int(_C.lib().dctr_crossnet_bwd_workspace_bytes(ctypes.byref(a)))


def library_mix_ws_bytes(B, d, L, ne, r):
    import ctypes
    from deepctr_amd import _C
    a = _C.CrossMixBwdArgs(batch=B, dim=d, layers=L, experts=ne, low_rank=r, x_stride=d, dy_stride=d, dx_stride=d)
    return int(_C.lib().dctr_crossnet_mix_bwd_workspace_bytes(ctypes.byref(a)))


# ---------------------------------------------------------------------------------------------------
# the cases: one table, run by tests/test_gpu_interaction_bwd.py, routes pinned by the CPU test
# ---------------------------------------------------------------------------------------------------
# op: bi (B, F, E) | ip (B, F, E) | afm (B, F, E, A) | vec / mat (B, d, L) | mix (B, d, L, experts, r);  data: "signed" (standard normal
# draws, weights scaled 1 / sqrt(d)) or "nonneg" (|the same draws|, CrossNet weights scaled 1 / d: nothing cancels, terms == |ref| and the
# comparison is the literal 1e-4 relative bar);  route: what resolve() must find, else the case no longer reaches what it was made for
# and the tests FAIL;  cap2: the elementwise grid-stride loops take a second trip (more elements than CAP[op] * 256);  scale: factor on x
Case = collections.namedtuple("Case", "id op shape data route cap2 scale why")

ROUTES = {"bi": ("elem",), "ip": ("elem",), "afm": ("lds64", "lds160", "refused"), "vec": ("L0", "vec_chip64", "vec_chip160", "vec_layered"),
          "mat": ("parts1", "sliced"), "mix": ("L0", "ks1", "ks2", "ks5", "refused")}


def _cases():
    out = []

    def add(op, shape, route, cap2=False, data=("signed",), scale=1.0, why=""):
        for kind in data:
            out.append(Case("%s-%s-%s" % (op, "x".join(str(s) for s in shape), kind), op, tuple(shape), kind, route, cap2, scale, why))
    both = ("signed", "nonneg")
    for shape in ((1, 1, 1), (5, 2, 4), (257, 7, 5), (70, 26, 16)):
        add("bi", shape, "elem", data=both)
    add("bi", (140000, 2, 16), "elem", cap2=True, data=both, why="B E > 8192 * 256: the loop's second trip")
    for shape in ((1, 2, 1), (9, 3, 5), (70, 26, 16), (3, 64, 8)):
        add("ip", shape, "elem", data=both)
    add("ip", (66000, 4, 16), "elem", cap2=True, data=both, why="B F E > 16384 * 256")
    add("afm", (1, 2, 4, 1), "lds64", why="one pair: softmax over one score")
    add("afm", (5, 7, 5, 3), "lds64", why="B = 4k + 1: three invalid waves in the last workgroup")
    add("afm", (7, 4, 3, 2), "lds64", why="B = 4k + 3: one invalid wave")
    add("afm", (70, 26, 16, 8), "lds64", why="325 pairs: six trips of the pair loop, the last with five lanes")
    add("afm", (6, 12, 8, 16), "lds64", why="66 pairs: two lanes take two pairs, the others one")
    add("afm", (9, 30, 64, 4), "lds160", scale=0.6, why="71,024 B: the raised-LDS launch")
    add("afm", (5, 62, 64, 8), "lds160", scale=0.5, why="161,968 B: the last shape accepted; 1,891 pairs")
    add("afm", (5, 63, 64, 8), "refused", scale=0.5, why="165,008 B: DCTR_E_UNSUPPORTED, outputs untouched")
    add("vec", (5, 7, 0), "L0", data=both)
    for shape in ((1, 7, 1), (15, 63, 2), (16, 64, 1), (17, 65, 3), (70, 429, 2)):
        add("vec", shape, "vec_chip64", data=both)
    add("vec", (33, 1100, 2), "vec_chip160", data=both)
    add("vec", (21, 2048, 1), "vec_chip160", data=both, why="all 32 register chunks full")
    add("vec", (21, 2047, 1), "vec_chip160", data=both, why="the last chunk one lane short")
    add("vec", (19, 1137, 3), "vec_chip160", data=both, why="163,776 B: the last on-chip shape")
    add("vec", (19, 1138, 3), "vec_layered", data=both, why="163,920 B: the hand-over by LDS")
    add("vec", (9, 2049, 1), "vec_layered", data=both, why="the hand-over by width")
    add("vec", (37, 1677, 3), "vec_layered", data=both)
    add("vec", (520, 2100, 2), "vec_layered", cap2=True, data=both, why="B d > 4096 * 256; 9 row slices of the column sums, the last short")
    for shape in ((1, 1, 1), (37, 45, 2), (130, 300, 3)):
        add("mat", shape, "parts1", data=both)
    add("mat", (1031, 12, 2), "parts1", data=both, why="a prime batch past 1024: the slice count falls back to 1")
    add("mat", (1030, 12, 2), "sliced", data=both, why="2 slices of 515 rows")
    add("mat", (2048, 45, 1), "sliced", data=both, why="4 slices")
    add("mat", (1030, 1024, 1), "sliced", cap2=True, data=both, why="B d > 4096 * 256")
    add("mix", (5, 7, 1, 1, 3), "ks1", why="one expert: the gate is 1")
    add("mix", (9, 6, 0, 2, 2), "L0")
    add("mix", (70, 45, 3, 2, 4), "ks1")
    add("mix", (33, 64, 2, 16, 1), "ks1", why="16 experts, rank 1")
    add("mix", (1100, 70, 2, 3, 5), "ks5", why="5 k-slices, the last 204 rows")
    add("mix", (1100, 128, 1, 16, 4), "ks5", cap2=True, why="experts B d > 8192 * 256")
    add("mix", (300, 429, 2, 4, 32), "ks2")
    add("mix", (5, 7, 1, 17, 2), "refused", why="17 experts: DCTR_E_DIM, outputs untouched")
    return out


CASES = _cases()
CASE_IDS = [c.id for c in CASES]
MATRIX_MODES = ("recompute", "saved")       # every matrix case runs both (the GPU test); L = 1 saved: saved_x = None


def elements(case):
    """Elements of the op's largest elementwise grid-stride loop."""
    s = case.shape
    if case.op == "bi":
        return s[0] * s[2]
    if case.op == "ip":
        return s[0] * s[1] * s[2]
    if case.op in ("vec", "mat"):
        return s[0] * s[1]
    if case.op == "mix":
        return s[3] * s[0] * s[1]
    return 0


def resolve(case):
    """What the restated host arithmetic finds for a case — dict(route, cap2, and per op lds / parts / slices / last_rows / ws_bytes) —
    after asserting that it is what the table names."""
    s, info = case.shape, {}
    if case.op in ("bi", "ip"):
        route = "elem"
    elif case.op == "afm":
        info["lds"] = lds = afm_bwd_lds_bytes(*s[1:])
        route = "lds64" if lds <= LDS_SOFT else "lds160" if lds <= LDS_MAX else "refused"
    elif case.op == "vec":
        B, d, L = s
        info["lds"], info["ws_bytes"] = cross_vector_lds_bytes(d, L), crossnet_ws_bytes("vector", B, d, L)
        route = ("L0" if L == 0 else "vec_layered" if not cross_vector_bwd_on_chip(d, L) else
                 "vec_chip64" if info["lds"] <= LDS_SOFT else "vec_chip160")
        if route == "vec_layered":
            info["slices"] = min(_ceil_div(B, 64), 64)
            per = _ceil_div(B, info["slices"])
            info["last_rows"] = B - (info["slices"] - 1) * per
    elif case.op == "mat":
        B, d, L = s
        info["parts"], info["ws_bytes"] = mlp_dw_parts(B, d * d), crossnet_ws_bytes("matrix", B, d, L)
        route = "sliced" if info["parts"] > 1 else "parts1"
    else:
        B, d, L, ne, r = s
        info["slices"], info["last_rows"] = mix_k_slices(B)
        info["ws_bytes"] = mix_ws_bytes(B, d, L, ne, r)
        route = "refused" if ne > MIX_MAX_EXPERTS else "L0" if L == 0 else "ks%d" % info["slices"]
    cap2 = case.op in CAP and elements(case) > CAP[case.op] * 256
    assert route == case.route and cap2 == case.cap2, "%s no longer reaches its route: %s cap2=%s %r" % (case.id, route, cap2, info)
    info["route"], info["cap2"] = route, cap2
    return info


# ---------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------
KINK_ULP = 64               # AFM: no |pre| within this many float32 ulp of its summed magnitude
KINK_REDRAWS = 8


def _seed(case, *more):
    key = "%s-%s" % (case.op, "x".join(str(s) for s in case.shape))           # signed and nonneg: the same draws
    return zlib.crc32(("/".join([key] + [str(m) for m in more])).encode()) & 0x7fffffff


def make_data(case):
    """Deterministic float32 inputs of a case, unpadded (the GPU test puts x / dy / dx on wider row strides).
      bi, ip: x [B, F, E], dy;  afm: x, W, b, h, p, dy, and ``redrawn`` (rows redrawn for the ReLU margin);  vec / mat: x [B, d],
      kernels, bias (None at L = 0), dy;  mix: x, U, V, C, G, bias, dy."""
    rng = np.random.RandomState(_seed(case))
    nonneg = case.data == "nonneg"
    f32 = lambda a: (np.abs(a) if nonneg else a).astype(np.float32)           # noqa: E731
    draw = lambda *shape: rng.standard_normal(shape)                           # noqa: E731
    s = case.shape
    if case.op in ("bi", "ip"):
        B, F, E = s
        return dict(x=f32(draw(B, F, E) * case.scale), dy=f32(draw(B, E if case.op == "bi" else F * (F - 1) // 2)))
    if case.op == "afm":
        B, F, E, A = s
        d = dict(x=f32(draw(B, F, E) * 0.7 * case.scale), W=f32(draw(E, A) * 0.5), b=f32(draw(A) * 0.2), h=f32(draw(A, 1) * 0.7),
                 p=f32(draw(E, 1) * 0.7), dy=f32(draw(B)))
        redrawn = []
        for row in np.nonzero(afm_kink_margin(d["x"], d["W"], d["b"]) < KINK_ULP)[0]:
            for attempt in range(1, KINK_REDRAWS + 1):
                d["x"][row] = (np.random.RandomState(_seed(case, row, attempt)).standard_normal((F, E)) * 0.7 * case.scale).astype(np.float32)
                if afm_kink_margin(d["x"][row:row + 1], d["W"], d["b"])[0] >= KINK_ULP:
                    break
            else:
                raise AssertionError("%s: row %d keeps a pre-activation within %d ulp of zero after %d redraws" % (case.id, row, KINK_ULP, KINK_REDRAWS))
            redrawn.append(int(row))
        d["redrawn"] = redrawn
        return d
    if case.op in ("vec", "mat"):
        B, d, L = s
        x = f32(draw(B, d) * case.scale)
        ks = draw(*((L, d) if case.op == "vec" else (L, d, d))) / (d if nonneg else np.sqrt(d))
        bs, dy = draw(L, d) * 0.1, draw(B, d)
        return dict(x=x, kernels=f32(ks) if L else None, bias=f32(bs) if L else None, dy=f32(dy))
    B, d, L, ne, r = s
    return dict(x=f32(draw(B, d) * 0.7 * case.scale), U=f32(draw(L, ne, d, r) / np.sqrt(r)), V=f32(draw(L, ne, d, r) / np.sqrt(d)),
                C=f32(draw(L, ne, r, r) / np.sqrt(r)), G=f32(draw(ne, d) / np.sqrt(d)), bias=f32(draw(L, d) * 0.1), dy=f32(draw(B, d)))


def oracle(case, d, corrupt=None):
    """(grads, terms) of a case's data."""
    if case.op == "bi":
        return bi_interaction_bwd(d["x"], d["dy"])
    if case.op == "ip":
        return inner_product_bwd(d["x"], d["dy"])
    if case.op == "afm":
        return afm_bwd(d["x"], d["W"], d["b"], d["h"], d["p"], d["dy"], drop_last_pair=corrupt == "last_pair")
    if case.op in ("vec", "mat"):
        return crossnet_bwd(d["x"], d["kernels"], d["bias"], "vector" if case.op == "vec" else "matrix", d["dy"], corrupt=corrupt)
    return crossnet_mix_bwd(d["x"], d["U"], d["V"], d["C"], d["G"], d["bias"], d["dy"], corrupt=corrupt)


WEIGHT_GRADS = {"bi": (), "ip": (), "afm": ("dW", "db", "dh", "dp"), "vec": ("dk", "db"), "mat": ("dk", "db"),
                "mix": ("dU", "dV", "dC", "dG", "db")}


def saved_for_matrix(d):
    """saved_u [L, B, d] / saved_x [max(L - 1, 1), B, d] of a matrix case: the oracle's own float64 u_l / x_l rounded to float32, so the
    backward is tested by itself and not through the forward kernel."""
    xs, us = crossnet_forward(d["x"], d["kernels"], d["bias"], "matrix")
    su = np.stack(us).astype(np.float32)
    sx = np.stack(xs[1:-1]).astype(np.float32) if len(us) > 1 else None
    return su, sx
