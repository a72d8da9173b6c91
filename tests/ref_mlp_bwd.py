"""Three things that tests/test_gpu_mlp_bwd.py and tests/test_mlp_bwd_oracle_cpu.py share, which is why they live in one module:
  1. the float64 NumPy oracle of dctr_mlp_bwd (deepctr_amd/csrc/dnn_train_kernels.hip, deepctr_amd/csrc/mlp_bwd_kernels.hip) for relu /
     sigmoid / tanh / linear;
  2. a restatement of the host arithmetic that decides which of the op's two forms a shape takes and how large its workspace is;
  3. the table of cases the GPU test runs, each with the form it must take.
The CPU test pins 1 against torch double autograd and 2 and 3 against dctr_mlp_bwd_workspace_bytes.

The oracle restates the op's CONTRACT, not autograd: act' is taken from the forward's SAVED outputs (float32 values) exactly as the
kernels define it — relu: h > 0, sigmoid: h (1 - h), tanh: 1 - h^2, linear: 1 — so a unit within an ulp of zero cannot flip between
the checker and the kernel.  Besides every gradient it returns ``terms``: the same computation over absolute values, an upper bound
of the magnitude each output element was summed at (tests.util.assert_close_terms)."""
import collections
import zlib

import numpy as np

ACTS = ("relu", "sigmoid", "tanh", "linear")


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


def act_deriv(h, act):
    """act' from the activation's OUTPUT h, as head_bwd_kernel / act_bwd_colsum_kernel / the backward chain's epilogue define it."""
    if act == "relu":
        return (h > 0).astype(np.float64)
    if act == "sigmoid":
        return h * (1.0 - h)
    if act == "tanh":
        return 1.0 - h * h
    assert act == "linear", act
    return np.ones_like(h)


def saved_acts(x, kernels, biases, act, round32=True):
    """The forward's saved layer outputs: a float64 forward, every layer's output rounded to float32 (and fed on rounded, as the
    next layer of the kernel reads it).  ``round32`` False keeps the float64 values (the autograd pin of the CPU test).
    relu: every layer must hold exact zeros AND positive values, else act' = (h > 0) is not exercised."""
    h = _f64(x)
    out = []
    for l, (w, b) in enumerate(zip(kernels, biases)):
        h = act_fwd(h @ _f64(w) + _f64(b), act)
        if round32:
            h = h.astype(np.float32)
        if act == "relu":
            assert (h == 0).any() and (h > 0).any(), "relu layer %d of %d rows: needs exact zeros and positive values" % (l, h.shape[0])
        out.append(h)
        h = _f64(h)
    return out


def mlp_bwd(x, kernels, acts, act, head_w=None, dlogit=None, d_out=None):
    """x [B, in_dim], kernels[l] [K_l, N_l], acts[l] [B, N_l] (the saved outputs), and either (head_w [N_last], dlogit [B]) or
    d_out [B, N_last] = d(loss)/d(acts[-1]).  Returns (grads, terms): dicts with dx [B, in_dim], dW / db (lists), d_head_w (None
    when headless), float64.
        dZ_last = (dlogit (x) head_w | d_out) .* act'(h_last);   d_head_w = h_last^T dlogit
        dW_l = X_l^T dZ_l;   db_l = colsum(dZ_l);   dZ_{l-1} = (dZ_l W_l^T) .* act'(h_{l-1});   dx = dZ_0 W_0^T
    terms: T_{l-1} = (T_l |W_l|^T) .* |act'|, dW terms |X_l|^T T_l, db terms colsum(T_l), head terms |h|^T |dlogit|."""
    x, kernels, acts = _f64(x), [_f64(k) for k in kernels], [_f64(a) for a in acts]
    L = len(kernels)
    g = {"dW": [None] * L, "db": [None] * L, "d_head_w": None}
    t = {"dW": [None] * L, "db": [None] * L, "d_head_w": None}
    if head_w is not None:
        head_w, dlogit = _f64(head_w).reshape(-1), _f64(dlogit).reshape(-1)
        dh = dlogit[:, None] * head_w[None, :]
        th = np.abs(dlogit)[:, None] * np.abs(head_w)[None, :]
        g["d_head_w"] = acts[-1].T @ dlogit
        t["d_head_w"] = np.abs(acts[-1]).T @ np.abs(dlogit)
    else:
        dh = _f64(d_out)
        th = np.abs(dh)
    for l in range(L - 1, -1, -1):
        d = act_deriv(acts[l], act)
        dz, tz = dh * d, th * np.abs(d)
        xl = x if l == 0 else acts[l - 1]
        g["dW"][l], t["dW"][l] = _f64(xl.T) @ dz, _f64(np.abs(xl).T) @ tz
        g["db"][l], t["db"][l] = dz.sum(0), tz.sum(0)
        dh, th = dz @ _f64(kernels[l].T), tz @ _f64(np.abs(kernels[l]).T)
    g["dx"], t["dx"] = dh, th
    return g, t


# ---------------------------------------------------------------------------------------------------
# host arithmetic of the two forms (deepctr_amd/csrc/dnn_train_kernels.hip: mlp_bwd_chained, mlp_bwd_chain_floats, mlp_bwd_main_floats;
# deepctr_amd/csrc/train_common.h: mlp_dw_parts; deepctr_amd/csrc/gemm_kernels.hip: k_slices; deepctr_amd/csrc/mlp_bwd_kernels.hip: chain_lda, bwd_chain_fits), restated
# ---------------------------------------------------------------------------------------------------
MAX_LAYERS = 8
CHAIN_DW_ROWS = 256


def _ceil_div(a, b):
    return -(-a // b)


def _al4(n):
    return (n + 3) // 4 * 4


def chain_lda(widths):
    """Row pitch (floats) of the backward chain's LDS tiles: pad64(widest of in_dim and the layers) + 4."""
    return _ceil_div(max(widths), 64) * 64 + 4


def is_chained(widths):
    """The chained form: two 16-row tiles of the widest layer within 160 KiB of LDS, i.e. pad64(widest) + 4 <= 1280, widest <= 1216."""
    return 1 <= len(widths) - 1 <= MAX_LAYERS and 2 * 16 * chain_lda(widths) * 4 <= 160 * 1024


def k_slices(k, rows=CHAIN_DW_ROWS):
    """Row slices of the chained form's dW GEMM: at most 32, each a multiple of 32 rows."""
    if k <= 0:
        return 1
    want = max(1, min(32, _ceil_div(k, rows)))
    return _ceil_div(k, _ceil_div(_ceil_div(k, want), 32) * 32)


def chain_rt(batch, widths):
    """16-row tiles per workgroup of the backward chain (launch_bwd_chain in deepctr_amd/csrc/mlp_bwd_kernels.hip), restated by reading: the library
    exposes rt nowhere, so unlike the sizes above this one cannot be pinned from the CPU."""
    rt = 4 if batch > 65536 else (2 if batch > 16 * 2 * 256 else 1)
    while rt > 1 and 2 * 16 * rt * chain_lda(widths) * 4 > 160 * 1024:
        rt >>= 1
    return rt


def dw_parts(batch, out_elems):
    """Row slices of the layered form's dW: 1 below 1024 rows, else batch / 512 capped, lowered until it divides the batch."""
    if batch < 1024:
        return 1
    cap = min(128, max(32, 1024 // max(1, out_elems // 4096)))
    parts = min(cap, batch // 512)
    while parts > 1 and batch % parts != 0:
        parts -= 1
    return parts


def chained_floats(batch, widths):
    """dZ_l [B, N_l] | W_l^T [K_l N_l] | dW slices [slices (K_l + 1) N_l] per layer, each 4-float aligned."""
    s = k_slices(batch)
    return sum(_al4(batch * n) + _al4(k * n) + _al4(s * (k + 1) * n) for k, n in zip(widths[:-1], widths[1:]))


def layered_floats(batch, widths, dice=False):
    """Two ping-pong buffers [B, widest] (Dice: three, + 2 x widest column sums), 4-float aligned, + the largest layer's dW slices."""
    w = max(widths)
    main = _al4((3 if dice else 2) * batch * w + (2 * w if dice else 0))
    parts = [dw_parts(batch, k * n) * k * n for k, n in zip(widths[:-1], widths[1:]) if dw_parts(batch, k * n) > 1]
    return main + max(parts, default=0)


def workspace_bytes(batch, widths, dice=False):
    """What dctr_mlp_bwd_workspace_bytes returns: the larger of the layered layout and, where the chained form runs, its layout."""
    if batch <= 0:
        return 0
    chained = chained_floats(batch, widths) if (not dice and is_chained(widths)) else 0
    return 4 * max(layered_floats(batch, widths, dice), chained)


# ---------------------------------------------------------------------------------------------------
# the GPU cases: one table, run by tests/test_gpu_mlp_bwd.py (with every activation), routes pinned by the CPU test
# ---------------------------------------------------------------------------------------------------
# widths = [in_dim, units...];  route: the form the shape must take;  head: Dense(1) head (else d_out, 2 columns wider than the last
# layer);  dx: input gradient wanted;  bias: per layer, False = a NULL entry in d_biases;  head_offset: head_w a view one float into a
# buffer (not 16-B aligned);  why: the branch the case is there for
Case = collections.namedtuple("Case", "id batch widths route head dx bias head_offset why")


def _case(id, batch, widths, route, head=True, dx=True, bias=None, head_offset=False, why=""):
    bias = tuple(bias) if bias is not None else (True,) * (len(widths) - 1)
    assert len(bias) == len(widths) - 1
    return Case(id, batch, tuple(widths), route, head, dx, bias, head_offset, why)


def _cases():
    out = []
    # chained form: row tiles of the chain and slice arithmetic of dW
    why = {1: "one row", 15: "a partial 16-row tile", 16: "one whole tile", 17: "one row into the second tile", 33: "k chunk of 64",
           256: "one whole slice", 257: "two slices, the last of 97 rows", 513: "three slices", 4097: "17 slices, the last of one row",
           8193: "rt = 2; 32 slices wanted, 29 made"}
    for b in (1, 15, 16, 17, 33, 256, 257, 513, 4097, 8193):
        out.append(_case("chain-B%d" % b, b, [13, 8, 5], "chained", why=why[b]))
    out.append(_case("chain-tight-B257", 257, [200, 200, 8], "chained", why="two slices AND a chained layout larger than the layered one: "
                     "the workspace guard of the GPU test starts where the sliced carving ends"))
    out.append(_case("chain-rt4", 65600, [12, 8, 4], "chained", why="rt = 4 of the backward chain"))
    out.append(_case("chain-pad64", 37, [63, 64, 65, 12], "chained", why="pad64 edges; head N = 12: 256 / (N/4) not integral"))
    out.append(_case("chain-N1028", 37, [16, 1028], "chained", why="N > 1024: scalar head, gridDim.y = 5"))
    out.append(_case("chain-N1024", 37, [8, 1024], "chained", why="one row lane of the 16-B head"))
    out.append(_case("chain-N1020", 37, [8, 1020], "chained", why="one row lane, 255 of 256 threads"))
    out.append(_case("chain-widest", 37, [1216, 8], "chained", why="widest layer the chain takes"))
    out.append(_case("chain-8layers", 37, [11, 9, 12, 7, 8, 6, 10, 5, 4], "chained", why="MAX_LAYERS"))
    # layered form: a layer wider than 1216
    for b, w in ((33, "below 1024 rows: dW with beta = 1"), (1024, "2 parts"), (1031, "prime: the parts fall back to 1"), (1536, "3 parts")):
        out.append(_case("layer-B%d" % b, b, [1217, 8, 5], "layered", why=w))
    for b in (37, 1024):
        out.append(_case("layer-N1300-B%d" % b, b, [24, 1300, 8], "layered", why="scalar act' kernel with h, gridDim.y = 6; sum_parts_kernel"))
    # operand forms on both routes, one small and one sliced batch each
    for route, k0, batches in (("chained", 13, (37, 513)), ("layered", 1217, (33, 1024))):
        for b in batches:
            tag = "%s-B%d" % (route[:5], b)
            out.append(_case("headless2-" + tag, b, [k0, 8, 5], route, head=False, why="d_out strided, two layers"))
            out.append(_case("headless3-" + tag, b, [k0, 8, 6, 5], route, head=False, why="d_out strided, three layers"))
            out.append(_case("nodx1-" + tag, b, [k0, 8], route, dx=False, why="dx = NULL, one layer: no chain launch at all"))
            out.append(_case("nodx3-" + tag, b, [k0, 8, 6, 5], route, dx=False, why="dx = NULL: l_first = 1"))
            out.append(_case("nobias-first-" + tag, b, [k0, 8, 5], route, bias=(False, True), why="NULL d_biases[0]: no ones_last column"))
            out.append(_case("nobias-last-" + tag, b, [k0, 8, 5], route, bias=(True, False), why="NULL d_biases[1]"))
            out.append(_case("nobias-all-" + tag, b, [k0, 8, 5], route, bias=(False, False), why="no bias gradient"))
            out.append(_case("headoff-" + tag, b, [k0, 12, 8], route, head_offset=True, why="misaligned head_w: scalar head at N % 4 == 0"))
    return out


CASES = _cases()
CASE_IDS = [c.id for c in CASES]


def make_data(case, act):
    """Deterministic inputs of a case (float32 NumPy): x [B, in_dim + 3] (row stride > in_dim), kernels, biases, the saved outputs,
    head_w / dlogit or d_out [B, N_last + 2].  The biases of units 0 and 1 of every layer are set so that row 0 has a pre-activation
    of -0.5 and one of +0.5: relu keeps zeros and positive values in every layer at every batch size."""
    rng = np.random.RandomState(zlib.crc32(("%s/%s" % (case.id, act)).encode()) & 0x7fffffff)
    B, w = case.batch, case.widths
    x = rng.standard_normal((B, w[0] + 3)).astype(np.float32)
    ks = [(rng.standard_normal((k, n)) / np.sqrt(k)).astype(np.float32) for k, n in zip(w[:-1], w[1:])]
    bs = [(rng.standard_normal(n) * 0.1).astype(np.float32) for n in w[1:]]
    h = _f64(x[:, :w[0]])
    for l in range(len(ks)):
        z0 = h[0] @ _f64(ks[l])
        bs[l][0], bs[l][1] = np.float32(-0.5 - z0[0]), np.float32(0.5 - z0[1])
        h = _f64(act_fwd(h @ _f64(ks[l]) + _f64(bs[l]), act).astype(np.float32))
    acts = saved_acts(x[:, :w[0]], ks, bs, act)
    d = dict(x=x, kernels=ks, biases=bs, acts=acts, head_w=None, dlogit=None, d_out=None)
    if case.head:
        d["head_w"] = (rng.standard_normal(w[-1]) * 0.3).astype(np.float32)
        d["dlogit"] = rng.standard_normal(B).astype(np.float32)
    else:
        d["d_out"] = rng.standard_normal((B, w[-1] + 2)).astype(np.float32)
    return d


def oracle(case, data, act):
    """(grads, terms) of a case's data."""
    w = case.widths
    return mlp_bwd(data["x"][:, :w[0]], data["kernels"], data["acts"], act, head_w=data["head_w"], dlogit=data["dlogit"],
                   d_out=None if data["d_out"] is None else data["d_out"][:, :w[-1]])
