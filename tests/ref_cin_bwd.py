"""Three things that tests/test_gpu_cin_bwd.py and tests/test_cin_bwd_oracle_cpu.py share, which is why they live in one module:
  1. the float64 NumPy oracle of dctr_cin_bwd (deepctr_amd/csrc/cin_layered_kernels.hip, deepctr_amd/csrc/cin_bwd_kernels.hip) for relu /
     sigmoid / tanh / linear;
  2. a restatement of the host arithmetic that decides, per layer, whether the z-free MFMA kernels run, which template instance, how
     the rows are sliced and how large the workspace is;
  3. the table of cases the GPU test runs, each with the routes it is there for.
The CPU test pins 1 against torch double autograd and 2 and 3 against dctr_cin_bwd_workspace_bytes.

The oracle restates the op's CONTRACT, not autograd: rows r = (sample, embedding dimension) are independent, act' is taken from the
forward's SAVED layer outputs (float32 values) exactly as cin_dpre_kernel defines it — relu: y > 0, sigmoid: y (1 - y), tanh: 1 - y^2,
linear: 1 — and the next layer's x_k is the saved output too.  Besides every gradient it returns ``terms``: the same computation over
absolute values, an upper bound of the magnitude each output element was summed at (tests.util.assert_close_terms)."""
import collections
import zlib

import numpy as np

ACTS = ("relu", "sigmoid", "tanh", "linear")
CHUNK = 1024                    # rows per step of the oracle: z = x_0 (outer) x_k is formed for one chunk at a time, never whole


def _f64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


def act_fwd(z, act):
    if act == "relu":
        return np.maximum(z, 0.0)
    if act == "sigmoid":
        return 1.0 / (1.0 + np.exp(-z))
    if act == "tanh":
        return np.tanh(z)
    assert act == "linear", act
    return z


def act_deriv(y, act):
    """act' from the activation's OUTPUT y, as cin_dpre_kernel defines it."""
    if act == "relu":
        return (y > 0).astype(np.float64)
    if act == "sigmoid":
        return y * (1.0 - y)
    if act == "tanh":
        return 1.0 - y * y
    assert act == "linear", act
    return np.ones_like(y)


def layer_plan(F0, layer_size, split):
    """Per layer (Fk, H, Hn, d0, off): x_k columns, maps, maps handed to the next layer, first direct map, offset of the direct maps in
    the op's output — CinPlan of cin_layered_kernels.hip.  Also returns out_dim."""
    out, fk, off, L = [], F0, 0, len(layer_size)
    for k, H in enumerate(layer_size):
        last = k == L - 1
        Hn = 0 if last else (H // 2 if split else H)
        d0 = (0 if last else H // 2) if split else 0
        out.append((fk, H, Hn, d0, off))
        off += H - d0
        fk = Hn
    return out, off


def to_rows(x, F0, D):
    """x [B, >= F0*D] -> X0t [B*D, F0] (cin_to_rows_kernel)."""
    B = x.shape[0]
    return _f64(np.asarray(x)[:, :F0 * D].reshape(B, F0, D).transpose(0, 2, 1).reshape(B * D, F0))


def from_rows(dx0t, B, F0, D):
    """[B*D, F0] -> [B, F0*D] (cin_from_rows_kernel)."""
    return _f64(dx0t.reshape(B, D, F0).transpose(0, 2, 1).reshape(B, F0 * D))


def forward(x0t, filters, biases, layer_size, split, act, round32=True):
    """The saved layer outputs y_k [R, H_k]: a float64 forward, every layer's output rounded to float32 (and fed on rounded, as the
    next layer reads it).  ``round32`` False keeps the float64 values (the autograd pin of the CPU test).  Returns (ys, pres)."""
    x0t = _f64(x0t)
    plan, _ = layer_plan(x0t.shape[1], layer_size, split)
    xk, ys, pres = x0t, [], []
    for k, (fk, H, Hn, d0, off) in enumerate(plan):
        W, pre = _f64(filters[k]).reshape(-1, H), np.empty((x0t.shape[0], H))
        for r in range(0, x0t.shape[0], CHUNK):
            z = (x0t[r:r + CHUNK, :, None] * xk[r:r + CHUNK, None, :fk]).reshape(-1, x0t.shape[1] * fk)
            pre[r:r + CHUNK] = z @ W + _f64(biases[k])
        y = act_fwd(pre, act)
        if round32:
            y = y.astype(np.float32)
        ys.append(y)
        pres.append(pre)
        xk = _f64(y)
    return ys, pres


def cin_bwd(x0t, filters, ys, layer_size, split, act, d_out, D, corrupt=None):
    """x0t [R, F0] (R = B*D), filters[k] [F0*Fk, H_k], ys[k] [R, H_k] the saved outputs, d_out [B, out_dim].  Returns (grads, terms):
    dicts with dpre / db / dW / dxk (lists per layer), dx0 [R, F0] (first factor, all layers) and dx [R, F0] = dx0 + layer 0's dxk.
        g_k[r, h] = [h < Hn] dxk_{k+1}[r, h] + [h >= d0] d_out[r / D, off + h - d0];   dpre_k = g_k .* act'(y_k);   db_k = colsum(dpre_k)
        dW_k[i Fk + j, h] = sum_r x0[r, i] xk[r, j] dpre_k[r, h];   T = dpre_k W_k^T
        dxk_k[r, j] = sum_i x0[r, i] T[r, i Fk + j];   dx0[r, i] += sum_j xk[r, j] T[r, i Fk + j]
    terms: the same over |.|.  ``corrupt(k, dpre)``: what the two MFMA kernels see in place of dpre_k (db keeps the clean one) — the
    staging-hole emulation of the CPU test."""
    x0t, d_out = _f64(x0t), _f64(d_out)
    R, F0 = x0t.shape
    plan, out_dim = layer_plan(F0, layer_size, split)
    assert d_out.shape[1] == out_dim and R == d_out.shape[0] * D
    ax0, L = np.abs(x0t), len(plan)
    g = {"dpre": [None] * L, "db": [None] * L, "dW": [None] * L, "dxk": [None] * L, "dx0": np.zeros((R, F0))}
    t = {"dpre": [None] * L, "db": [None] * L, "dW": [None] * L, "dxk": [None] * L, "dx0": np.zeros((R, F0))}
    brow = np.arange(R) // D
    dxn = txn = None
    for k in range(L - 1, -1, -1):
        fk, H, Hn, d0, off = plan[k]
        y, W = _f64(ys[k]), _f64(filters[k]).reshape(F0 * fk, H)
        xk = x0t if k == 0 else _f64(ys[k - 1])[:, :fk]
        axk, aW = np.abs(xk), np.abs(W)
        gk, tk = np.zeros((R, H)), np.zeros((R, H))
        if dxn is not None:
            gk[:, :Hn] += dxn
            tk[:, :Hn] += txn
        gk[:, d0:] += d_out[brow, off:off + H - d0]
        tk[:, d0:] += np.abs(d_out[brow, off:off + H - d0])
        d = act_deriv(y, act)
        dpre, tpre = gk * d, tk * np.abs(d)
        g["dpre"][k], t["dpre"][k] = dpre, tpre
        g["db"][k], t["db"][k] = dpre.sum(0), tpre.sum(0)
        if corrupt is not None:
            dpre = corrupt(k, dpre)
        dW, tW = np.zeros((F0 * fk, H)), np.zeros((F0 * fk, H))
        dxk, txk = np.empty((R, fk)), np.empty((R, fk))
        for r in range(0, R, CHUNK):
            s = slice(r, r + CHUNK)
            z = (x0t[s, :, None] * xk[s, None, :]).reshape(-1, F0 * fk)
            az = np.abs(z)
            dW += z.T @ dpre[s]
            tW += az.T @ tpre[s]
            T, aT = (dpre[s] @ W.T).reshape(-1, F0, fk), (tpre[s] @ aW.T).reshape(-1, F0, fk)
            dxk[s], txk[s] = np.einsum("ri,rij->rj", x0t[s], T), np.einsum("ri,rij->rj", ax0[s], aT)
            g["dx0"][s] += np.einsum("rj,rij->ri", xk[s], T)
            t["dx0"][s] += np.einsum("rj,rij->ri", axk[s], aT)
        g["dW"][k], t["dW"][k], g["dxk"][k], t["dxk"][k] = dW, tW, dxk, txk
        dxn, txn = dxk, txk
    g["dx"], t["dx"] = g["dx0"] + g["dxk"][0], t["dx0"] + t["dxk"][0]
    return g, t


# ---------------------------------------------------------------------------------------------------
# host arithmetic of the routes (deepctr_amd/csrc/cin_bwd_kernels.hip: fused_shape_ok, lds_bytes, dw_lds_bytes, dw_split,
# launch_dw_fused; deepctr_amd/csrc/cin_layered_kernels.hip: cin_plan, the `parts` of dctr_cin_bwd), restated
# ---------------------------------------------------------------------------------------------------
RB = 64                 # rows per workgroup of the dz kernel = rows per staged tile of the dW kernel
DW_TW = 2               # (i, j-block) tiles per wave of the dW kernel
DEFAULT_CUS = 256       # what dctr_n_cus() falls back to without a device


def _ceil_div(a, b):
    return -(-a // b)


def _al4(n):
    return (n + 3) // 4 * 4


def fused_shape_ok(F0, Fk, H):
    """Shapes both z-free kernels take: H = 16 KS <= 128, F0 <= 32 (eight staging registers), Fk <= 32 or (Fk % 4 == 0 and Fk <= 64)
    (sixteen), the dz kernel's LDS within 160 KiB and the dW kernel's within 80 KiB."""
    dz_lds = RB * ((H + 4) + 2 * (F0 | 1) + (Fk | 1)) * 4
    dw_lds = RB * ((H + 4) + (F0 | 1) + (_ceil_div(Fk, 16) * 16 + 4)) * 4
    return (H % 16 == 0 and 16 <= H <= 128 and 1 <= F0 <= 32 and Fk >= 1 and (Fk <= 32 or (Fk % 4 == 0 and Fk <= 64))
            and dz_lds <= 160 * 1024 and dw_lds <= 80 * 1024)


def dw_split(F0, Fk, rows, cus=DEFAULT_CUS):
    """(n_chunks, rows_per_split, splits) of the dW kernel: ~4 workgroups per CU, every slice a multiple of the 64-row tile."""
    nt = _ceil_div(Fk, 16) * F0
    n_chunks = _ceil_div(nt, 4 * DW_TW)
    splits = max(1, min(_ceil_div(4 * cus, n_chunks), _ceil_div(rows, RB)))
    rps = _ceil_div(_ceil_div(rows, splits), RB) * RB
    return n_chunks, rps, _ceil_div(rows, rps)


def gemm_parts(rows, H):
    """Row slices of the non-fused dW: the partial products must fit the dz buffer (rows / H of them), at most 32, lowered until the
    count divides the rows.  1: a single GEMM with beta = 1 straight into d_filters."""
    parts = min(32, rows // H)
    while parts > 1 and rows % parts != 0:
        parts -= 1
    return max(parts, 1)


Route = collections.namedtuple("Route", "fused Fk H ldk KS TPI XK4 n_chunks rps splits tiles last_rows parts")


def routes(F0, layer_size, split, rows, cus=DEFAULT_CUS):
    """Per layer: fused or not; fused: KS = H / 16 (the template instance of both kernels), TPI = 16-column blocks of x_k, XK4 (16-B
    loads of x_k: Fk % 4 == 0 and row pitch % 4 == 0 — every x_k the op reads starts 16-B aligned, and its pitch is Fk or, under
    split-half where the layer sizes are even, 2 Fk: XK4 is Fk % 4 == 0 in every call the op accepts), the dW kernel's slices, tiles per
    slice and rows of the last slice;  non-fused: ``parts`` of the dW GEMM."""
    plan, _ = layer_plan(F0, layer_size, split)
    out = []
    for k, (fk, H, Hn, d0, off) in enumerate(plan):
        ldk = F0 if k == 0 else layer_size[k - 1]
        if fused_shape_ok(F0, fk, H):
            n_chunks, rps, splits = dw_split(F0, fk, rows, cus)
            out.append(Route(True, fk, H, ldk, H // 16, _ceil_div(fk, 16), fk % 4 == 0 and ldk % 4 == 0, n_chunks, rps, splits,
                             rps // RB, rows - (splits - 1) * rps, None))
        else:
            out.append(Route(False, fk, H, ldk, None, None, None, None, None, None, None, None, gemm_parts(rows, H)))
    return out


def workspace_floats(B, F0, D, layer_size, split, fwd_ws_bytes, cus=DEFAULT_CUS):
    """cin_plan's carving, every piece 4-float aligned: X0t | per layer y_k and (non-fused) z_k | the re-run forward's output | dpre
    [R, widest] | dz (largest non-fused z) | the dW kernel's partial products (most slices) | dX0t | two dxk [R, widest x_k] | the
    re-run forward's own workspace (``fwd_ws_bytes``: dctr_cin_workspace_bytes, another function of the library)."""
    R = B * D
    plan, out_dim = layer_plan(F0, layer_size, split)
    n = _al4(R * F0)
    zmax = pmax = 0
    for fk, H, Hn, d0, off in plan:
        n += _al4(R * H)
        if fused_shape_ok(F0, fk, H):
            pmax = max(pmax, dw_split(F0, fk, R, cus)[2] * F0 * fk * H)
        else:
            n += _al4(R * F0 * fk)
            zmax = max(zmax, R * F0 * fk)
    hmax, fkmax = max(layer_size), max(p[0] for p in plan)
    n += _al4(B * out_dim) + _al4(R * hmax) + _al4(zmax) + _al4(pmax) + _al4(R * F0) + 2 * _al4(R * fkmax) + _al4((fwd_ws_bytes + 3) // 4)
    return n


def library_bytes(B, F0, D, layers, split):
    """(dctr_cin_bwd_workspace_bytes, dctr_cin_workspace_bytes) of the library for these shapes: host arithmetic, no device needed."""
    import ctypes
    from deepctr_amd import _C
    lib = _C.lib()
    lib.dctr_cin_bwd_workspace_bytes.restype = ctypes.c_size_t
    lib.dctr_cin_workspace_bytes.restype = ctypes.c_size_t
    n = len(layers)
    ls = (ctypes.c_int32 * n)(*layers)
    fp, bp = (ctypes.c_void_p * n)(), (ctypes.c_void_p * n)()
    f = _C.CinArgs(x=None, batch=B, x_stride=F0 * D + 5, fields=F0, dim=D, n_layers=n, split_half=int(split), activation=1,
                   layer_size=ctypes.cast(ls, ctypes.c_void_p), filters=ctypes.cast(fp, ctypes.c_void_p),
                   bias=ctypes.cast(bp, ctypes.c_void_p), out=None, workspace=None, workspace_bytes=0)
    a = _C.CinBwdArgs(fwd=ctypes.pointer(f), d_out=None, out_dim=layer_plan(F0, layers, split)[1], dx_accumulate=0, d_filters=None,
                      d_bias=None, dx=None, dx_stride=0)
    return int(lib.dctr_cin_bwd_workspace_bytes(ctypes.byref(a))), int(lib.dctr_cin_workspace_bytes(ctypes.byref(f)))


def old_dpre_stage_map(H):
    """The dpre tile staging both kernels had before the flat index: thread t stages float4 column t % H4 of rows t / H4 + u * (256 / H4),
    u < H / 16 (H4 = H / 4).  Returns the boolean [64, H4] map of what it writes — all of the tile only where 256 % H4 == 0."""
    H4, KS = H // 4, H // 16
    drows, m = 256 // H4, np.zeros((RB, H4), dtype=bool)
    for tid in range(256):
        for u in range(KS):
            assert tid // H4 + u * drows < RB
            m[tid // H4 + u * drows, tid % H4] = True
    return m


def dpre_stage_map(H):
    """The flat staging: element u of thread t is float4 idx = t + 256 u of the tile's 64 * H4 contiguous ones: row idx / H4, column idx % H4.
    Returns how often each [row, column] is written."""
    H4, KS = H // 4, H // 16
    m = np.zeros((RB, H4), dtype=int)
    for tid in range(256):
        for u in range(KS):
            idx = tid + 256 * u
            m[idx // H4, idx % H4] += 1
    return m


def hole_emulation(H, mode):
    """``corrupt`` for cin_bwd: in every 64-row block the dpre entries old_dpre_stage_map leaves unstaged become zeros (mode "zero") or
    the previous block's values (mode "stale"; the first block: zeros) — what a workgroup of the unfixed kernels could find in LDS."""
    hole = np.repeat(~old_dpre_stage_map(H), 4, axis=1)                 # [64, H]

    def corrupt(k, dpre):
        out = dpre.copy()
        for r in range(0, dpre.shape[0], RB):
            n = min(RB, dpre.shape[0] - r)
            prev = np.zeros((RB, dpre.shape[1]))
            if mode == "stale" and r > 0:
                prev = dpre[r - RB:r]
            out[r:r + n][hole[:n]] = prev[:n][hole[:n]]
        return out
    return corrupt


# ---------------------------------------------------------------------------------------------------
# the GPU cases: one table, run by tests/test_gpu_cin_bwd.py, routes pinned by the CPU test
# ---------------------------------------------------------------------------------------------------
# B x D rows of F0 fields;  layers / split / act: the CIN;  tags: the branches the case is there for (see BRANCHES);  expect: a check of
# the restated routes the case must pass, else it no longer reaches what it was made for (the tests FAIL then, they do not skip);
# slices: B is chosen from the device's CU count so that layer 1 of the dW kernel walks that many tiles per slice (B is then None)
Case = collections.namedtuple("Case", "id B F0 D layers split act tags expect slices why")

BRANCHES = {
    "hole-H48": "dpre staging, 256 % (H/4) != 0", "hole-H80": "same", "hole-H96": "same", "hole-H112": "same",
    "ks-1": "template instance KS / NH", "ks-2": "", "ks-3": "", "ks-4": "", "ks-5": "", "ks-6": "", "ks-7": "", "ks-8": "",
    "tpi-1": "16-column blocks of x_k", "tpi-2": "", "tpi-3": "", "tpi-4": "",
    "F0-1": "waves without an i of their own at TPI = 1", "F0-2": "", "F0-3": "", "F0-32": "the staging-register limit",
    "Fk-4": "kw = 1 of the XK4 staging", "Fk-17": "one live column in the second block",
    "xk-prev-scalar": "x_k from a previous layer with ldk % 4 != 0: scalar staging",
    "mixed-nf-f": "non-fused layer behind a fused one in the backward order (dxnext hand-over)", "mixed-f-nf": "the other order",
    "tanh": "cin_dpre_kernel's tanh", "tiles-2": "the dW kernel's pipeline: a second tile in a slice", "tiles-3": "and a third",
    "dw-fused": "dW ending: fused kernel + sum_parts", "dw-batched": "batched partial GEMMs + sum_parts", "dw-gemm1": "one GEMM, beta = 1",
    "rows-1": "", "rows-15": "", "rows-63": "", "rows-64": "", "rows-65": "",
}


def _tags_of(F0, layers, split, rows):
    """Tags that follow from the restated routes (at DEFAULT_CUS; the slices-* cases get theirs by hand)."""
    rt = routes(F0, layers, split, rows)
    tags = set()
    for k, r in enumerate(rt):
        if r.fused:
            tags |= {"ks-%d" % r.KS, "tpi-%d" % r.TPI, "dw-fused"}
            if F0 in (1, 2, 3, 32):
                tags.add("F0-%d" % F0)
            if r.Fk in (4, 17):
                tags.add("Fk-%d" % r.Fk)
            if r.H in (48, 80, 96, 112) and rows >= RB:
                tags.add("hole-H%d" % r.H)
            if k > 0 and not r.XK4 and r.ldk % 4 != 0:
                tags.add("xk-prev-scalar")
            if k > 0 and not rt[k - 1].fused:
                tags.add("mixed-f-nf")            # backward order: the fused layer k runs first, its dxk feeds the non-fused k - 1
            if k + 1 < len(rt) and not rt[k + 1].fused:
                tags.add("mixed-nf-f")
        else:
            tags.add("dw-batched" if r.parts > 1 else "dw-gemm1")
    return tags


def _case(id, B, F0, D, layers, split=False, act="relu", tags=(), expect=None, slices=None, why=""):
    layers = tuple(layers)
    t = set(tags)
    if B is not None:
        t |= _tags_of(F0, layers, split, B * D)
    if act == "tanh":
        t.add("tanh")
    return Case(id, B, F0, D, layers, bool(split), act, frozenset(t), expect, slices, why)


def _cases():
    out = []
    # the staging hole: one fused layer, row 63 of a full block (128 rows) and a ragged second block (135 rows) both live
    for H in (48, 80, 96, 112):
        for B, D in ((8, 16), (9, 15)):
            for F0 in (3, 26):
                out.append(_case("hole-H%d-ks%d-R%d-F%d" % (H, H // 16, B * D, F0), B, F0, D, (H,),
                                 expect=lambda rt, H=H: rt[0].fused and rt[0].H == H, why="rows the old dpre staging left out"))
    for ks in (1, 2, 4, 8):
        out.append(_case("ks-%d" % ks, 9, 26, 15, (16 * ks,), expect=lambda rt, ks=ks: rt[0].fused and rt[0].KS == ks,
                         why="template instance; 256 % (H/4) == 0: the staging never had a hole here"))
    # second-layer Fk x F0: through split-half and not; the second layer's H walks the KS values
    first = {4: ((8,), (4,)), 12: ((24,), (12,)), 16: ((32,), (16,)), 17: ((34,), (17,)), 26: ((52,), (26,)), 32: ((64,), (32,)),
             36: ((72,), (36,)), 48: ((96,), (48,)), 64: ((128,), (64,))}
    n = 0
    for fk in sorted(first):
        for F0 in (1, 2, 3, 5, 32):
            for split in (True, False):
                h2 = 16 * (1 + n % 8)
                n += 1
                out.append(_case("tpi-%d-Fk%d-F%d-%s" % (_ceil_div(fk, 16), fk, F0, "split" if split else "whole"), 9, F0, 15,
                                 first[fk][0 if split else 1] + (h2,), split=split,
                                 expect=lambda rt, fk=fk: rt[1].fused and rt[1].Fk == fk and rt[1].TPI == _ceil_div(fk, 16),
                                 why="second layer x_k of %d columns, H = %d" % (fk, h2)))
    out.append(_case("mixed-nf-f-f", 9, 7, 15, (12, 32, 16), split=True,
                     expect=lambda rt: [r.fused for r in rt] == [False, True, True], why="non-fused, then fused layers"))
    out.append(_case("mixed-f-nf-f", 9, 7, 15, (32, 10, 16), split=False,
                     expect=lambda rt: [r.fused for r in rt] == [True, False, True], why="a non-fused layer between fused ones"))
    for B, D in ((1, 1), (3, 5), (9, 7), (8, 8), (5, 13)):
        out.append(_case("rows-%d" % (B * D), B, 5, D, (96, 32), split=True, tags=("rows-%d" % (B * D),),
                         expect=lambda rt: rt[0].fused and rt[1].fused, why="row edges of the 64-row tile"))
    out.append(_case("nonfused-R131-gemm1", 131, 5, 1, (10, 6), expect=lambda rt: not rt[0].fused and rt[0].parts == 1 and rt[1].parts == 1,
                     why="a prime row count: one dW GEMM with beta = 1"))
    out.append(_case("nonfused-R135-batched", 9, 5, 15, (10, 6), expect=lambda rt: not rt[0].fused and rt[0].parts > 1 and rt[1].parts > 1,
                     why="batched partial dW GEMMs + sum_parts"))
    for tiles in (2, 3):
        out.append(_case("slices-%d" % tiles, None, 32, 3, (64, 48), tags=("tiles-%d" % tiles, "F0-32", "tpi-4", "tpi-2", "ks-3", "ks-4", "dw-fused", "hole-H48"),
                         slices=tiles, expect=lambda rt, tiles=tiles: rt[1].fused and rt[1].tiles == tiles and rt[1].last_rows % RB != 0,
                         why="layer 1 of the dW kernel walks %d tiles per slice, the last slice ragged" % tiles))
    # shapes at which every sum of the op has a fixed order (bit_reproducible below): the repeated-call test asserts equal bits there
    out.append(_case("det-tpi2", 4, 20, 15, (32, 32), expect=lambda rt: all(r.fused and r.TPI == 2 for r in rt),
                     why="two LDS atomics per dx element: any order gives the same bits"))
    out.append(_case("det-F2", 4, 2, 15, (16, 16), expect=lambda rt: all(r.fused and r.TPI == 1 for r in rt),
                     why="TPI = 1 with two fields: two waves own an i each"))
    for act in ACTS:
        out.append(_case("act-%s-fused" % act, 9, 7, 15, (48, 32), split=True, act=act, expect=lambda rt: rt[0].fused and rt[1].fused))
        out.append(_case("act-%s-nonfused" % act, 9, 7, 15, (12, 10), split=True, act=act, expect=lambda rt: not rt[0].fused and not rt[1].fused))
    return out


CASES = _cases()
CASE_IDS = [c.id for c in CASES]


def bit_reproducible(F0, rt, rows):
    """(dx, db, dW): which results of two identical calls from the same start have equal BITS (db, dW: per layer), from reading the
    kernels' sums.
      dxk / dx0 of a layer: cin_dz_fused_kernel adds to its LDS tiles with float atomics from several waves — dx0[r, i] once per
          16-column block of x_k (TPI adds), dxk[r, j] once per wave that shares the block (4 / TPI waves at TPI < 4, those with an i of
          their own: at most F0).  Two adds onto zero commute; three or more round differently in another order.  The non-fused route
          goes through dctr_gemm, which may split K over workgroups that add with float atomics: not claimed.
      Every result of layer k is computed from dpre_k, i.e. from the dxk of the layer above: it can only be reproducible where all
          layers above are.
      db: launch_act_bwd_colsum sums in a fixed order within a workgroup and leaves with one float atomic per column and workgroup onto
          d_bias: equal bits with ONE workgroup — H % 4 == 0 and rows <= 4 * (256 / (H / 4)).
      dW: the fused kernel stores each slice's partial product (no atomics) and sum_parts_kernel adds the slices in index order, four
          interleaved chains, onto d_filters: a fixed order.  Non-fused (dctr_gemm): not claimed."""
    own = [r.fused and r.TPI <= 2 and (r.TPI == 2 or min(4, F0) <= 2) for r in rt]
    above = [all(own[k + 1:]) for k in range(len(rt))]
    db = [above[k] and r.H % 4 == 0 and rows <= 4 * (256 // (r.H // 4)) for k, r in enumerate(rt)]
    dW = [above[k] and r.fused for k, r in enumerate(rt)]
    return all(own), db, dW


def slices_batch(case, cus):
    """Smallest B for which layer 1's dW slices hold exactly ``case.slices`` tiles and the last slice is ragged (rows = B * D)."""
    for B in range(1, 1 << 16):
        r = routes(case.F0, case.layers, case.split, B * case.D, cus)[1]
        if r.tiles == case.slices and r.last_rows % RB != 0:
            return B
        if r.tiles > case.slices:
            break
    raise AssertionError("%s: no row count gives %d tiles per slice at %d CUs" % (case.id, case.slices, cus))


def resolve(case, cus=DEFAULT_CUS):
    """The case with its batch filled in (slices-*: from the CU count) and its routes; raises when it no longer reaches them."""
    if case.B is None:
        case = case._replace(B=slices_batch(case, cus))
    rt = routes(case.F0, case.layers, case.split, case.B * case.D, cus)
    assert case.expect is None or case.expect(rt), "%s no longer reaches its route: %r" % (case.id, rt)
    return case, rt


def make_data(case):
    """Deterministic inputs of a resolved case (float32 NumPy): x [B, F0*D + 5] (row stride > F0*D), filters, biases, d_out, and the
    saved outputs ys of a float64 forward rounded to float32.  relu: every layer holds exact zeros and positive values.  (The GPU test
    hands the oracle the forward KERNEL's saved outputs instead, which the op reads: a unit within an ulp of zero then cannot flip
    between the checker and the kernels.)"""
    plan, out_dim = layer_plan(case.F0, case.layers, case.split)
    rng = np.random.RandomState(zlib.crc32(case.id.encode()) & 0x7fffffff)
    x = rng.standard_normal((case.B, case.F0 * case.D + 5)).astype(np.float32)
    fs = [(rng.standard_normal((case.F0 * fk, H)) / np.sqrt(case.F0 * fk)).astype(np.float32) for fk, H, _, _, _ in plan]
    bs = [(rng.standard_normal(H) * 0.1).astype(np.float32) for _, H, _, _, _ in plan]
    d_out = rng.standard_normal((case.B, out_dim)).astype(np.float32)
    ys, _ = forward(to_rows(x, case.F0, case.D), fs, bs, case.layers, case.split, case.act)
    if case.act == "relu" and case.B * case.D >= 15:
        assert all((y == 0).any() and (y > 0).any() for y in ys), case.id
    return dict(x=x, filters=fs, biases=bs, d_out=d_out, ys=ys)


def oracle(case, data, corrupt=None, ys=None):
    """(grads, terms) of a resolved case's data; dx as [B, F0*D].  ``ys``: saved outputs to use in place of data["ys"]."""
    g, t = cin_bwd(to_rows(data["x"], case.F0, case.D), data["filters"], data["ys"] if ys is None else ys, case.layers, case.split, case.act, data["d_out"],
                   case.D, corrupt=corrupt)
    g["dx"], t["dx"] = from_rows(g["dx"], case.B, case.F0, case.D), from_rows(t["dx"], case.B, case.F0, case.D)
    return g, t
