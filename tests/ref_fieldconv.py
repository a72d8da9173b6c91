"""NumPy oracle of the field-axis conv / pool stack (keras Conv2D((w, 1), 'same', tanh), KMaxPooling, MaxPooling2D((p, 1))), FGCNNLayer
(reference deepctr/layers/interaction.py:937-1064), CCPM (deepctr/models/ccpm.py) and FGCNN (deepctr/models/fgcnn.py), written from
the equations, float64 or float32, on the shared oracle helpers (embedding groups, linear logit, DNN, keras Add).

  y[b, r, e, co] = tanh(bias[co] + sum_{d, ci} xpad[b, r + d, e, ci] K[d, ci, co]);  'same': (w - 1) // 2 zero rows before, the rest after
  k-max: the k largest along the axis in descending order of value (tf.nn.top_k(sorted=True))
  max pooling: windows of p rows at stride p, 'valid': rows // p windows, the trailing rows dropped

Each ``mutate`` name is a deliberately WRONG variant the fixtures must be able to tell from the right one (scripts/make_golden_ccpm_fgcnn.py):
'pad_side', 'keep_order', 'flip', 'channel_first', 'pool_pad', 'recombine_ew', 'swap_fg'."""
import json

import numpy as np

from oracle import ref_numpy as R
from oracle.ref_models import _add, _dnn, _embed_groups, linear_logit

MUTATIONS = ("pad_side", "keep_order", "flip", "channel_first", "pool_pad", "recombine_ew", "swap_fg")


def conv_same(x, kernel, bias, mutate=(), stats=None):
    """x [B, R, E, C_in], kernel [w, C_in, C_out] (or keras' [w, 1, C_in, C_out]), bias [C_out] -> tanh(conv) [B, R, E, C_out]."""
    dt = x.dtype
    kernel = np.asarray(kernel).astype(dt)
    if kernel.ndim == 4:
        kernel = kernel[:, 0]
    w = kernel.shape[0]
    before = (w - 1) // 2
    after = w - 1 - before
    if "pad_side" in mutate:
        before, after = after, before
    if "flip" in mutate:
        kernel = kernel[::-1]
    rows = x.shape[1]
    xp = np.pad(x, ((0, 0), (before, after), (0, 0), (0, 0)))
    z = np.zeros(x.shape[:3] + (kernel.shape[2],), dt) + np.asarray(bias).astype(dt)
    for d in range(w):
        z = z + xp[:, d:d + rows] @ kernel[d]
    if stats is not None:
        stats.append(np.abs(z).reshape(-1))
    return np.tanh(z)


def kmax(x, k, axis=1, mutate=()):
    """The k largest along ``axis`` in descending order of value."""
    x = np.asarray(x)
    if "keep_order" in mutate:          # the paper's order-preserving variant
        idx = np.sort(np.argsort(-x, axis=axis, kind="stable").take(range(k), axis=axis), axis=axis)
        return np.take_along_axis(x, idx, axis=axis)
    return (-np.sort(-x, axis=axis)).take(range(k), axis=axis)


def max_pool(x, p, mutate=()):
    """x [B, R, E, C] -> [B, R // p, E, C]."""
    rows = x.shape[1]
    n = rows // p
    if "pool_pad" in mutate and rows % p:
        # a STAND-IN for "pads the trailing rows instead of dropping them": the honest variant has one window more, which changes the
        # width of the recombination Dense's input and cannot run on the fixture's weights.  Here the tail is padded into a short window
        # of its own and the surplus window leaves at the front, so the map keeps its rows // p rows while every window moves
        x = np.concatenate([x, np.full((x.shape[0], p - rows % p) + x.shape[2:], -np.inf, x.dtype)], axis=1)[:, p:]
    return x[:, :n * p].reshape(x.shape[0], n, p, x.shape[2], x.shape[3]).max(axis=2)


def field_conv(x, kernels, biases, pools, dtype=np.float64, mutate=(), stats=None):
    """x [B, F, E] or [B, F, E, C_0]; pools: per stage ('kmax', k) or ('max', p).  Returns (the last pooled map, every stage's pooled
    map), each [B, rows, E, C]."""
    h = np.asarray(x).astype(dtype)
    if h.ndim == 3:
        h = h[..., None]
    maps = []
    for kern, bias, (kind, arg) in zip(kernels, biases, pools):
        h = conv_same(h, kern, bias, mutate, stats)
        h = kmax(h, arg, 1, mutate) if kind == "kmax" else max_pool(h, arg, mutate)
        maps.append(h)
    return h, maps


def _flatten(x, mutate=()):
    if "channel_first" in mutate:
        x = np.moveaxis(x, -1, 1)
    return x.reshape(x.shape[0], -1)


def conv_names(n, what="conv2d"):
    return [what if i == 0 else "%s_%d" % (what, i) for i in range(n)]


def fgcnn_layer(x, weights, filters, kernel_width, new_maps, pooling_width, dtype=np.float64, mutate=(), stats=None, conv_prefix="conv2d",
                dense_prefix="dense"):
    """FGCNNLayer.call: x [B, F, E] -> the new features [B, sum rows_i new_maps_i, E]."""
    dt = np.dtype(dtype).type
    n = len(filters)
    x = np.asarray(x).astype(dt)
    B, _, E = x.shape
    kernels = [weights[c + "/kernel"] for c in conv_names(n, conv_prefix)]
    biases = [weights[c + "/bias"] for c in conv_names(n, conv_prefix)]
    _, maps = field_conv(x, kernels, biases, [("max", p) for p in pooling_width], dt, mutate, stats)
    out = []
    for m, dn, new in zip(maps, conv_names(n, dense_prefix), new_maps):
        z = _flatten(m, mutate) @ weights[dn + "/kernel"].astype(dt) + weights[dn + "/bias"].astype(dt)
        if stats is not None:
            stats.append(np.abs(z).reshape(-1))
        y = np.tanh(z)
        if "recombine_ew" in mutate:
            y = np.swapaxes(y.reshape(B, E, m.shape[1] * new), 1, 2)
        else:
            y = y.reshape(B, m.shape[1] * new, E)
        out.append(y)
    return np.concatenate(out, axis=1)


def ccpm_k(i, l, n):      # noqa: E741
    """The reference's own expression for stage i of l over n fields (deepctr/models/ccpm.py:65)."""
    return max(1, int((1 - pow(i / l, l - i)) * n)) if i < l else 3


def ccpm(linear_cols, dnn_cols, weights, feed, conv_kernel_width=(6, 5), conv_filters=(4, 4), dnn_hidden_units=(128, 64), task="binary",
         dtype=np.float32, mutate=(), stats=None, **_):
    dt = np.dtype(dtype).type
    lin = linear_logit(linear_cols, feed, weights, dt)
    groups, _dense = _embed_groups(dnn_cols, feed, weights, "", dt)
    x = np.concatenate([e for g in groups.values() for e in g], axis=1)       # [B, F, E]
    n, l = x.shape[1], len(conv_filters)                                      # noqa: E741
    h = x[..., None]
    if l:
        pools, rows = [], n
        for i in range(1, l + 1):
            rows = min(ccpm_k(i, l, n), rows)
            pools.append(("kmax", rows))
        names = conv_names(l)
        h, _maps = field_conv(x, [weights[c + "/kernel"] for c in names], [weights[c + "/bias"] for c in names], pools, dt, mutate, stats)
    h = _flatten(h, mutate)
    if len(dnn_hidden_units) > 0:
        h = _dnn("dnn", h, weights, dt, "relu")
    final = _add(h @ weights["dense/kernel"].astype(dt), lin)
    return R.prediction_layer(final, weights["prediction_layer/global_bias"].astype(dt), task)


def fgcnn(linear_cols, dnn_cols, weights, feed, conv_kernel_width=(7, 7, 7, 7), conv_filters=(14, 16, 18, 20), new_maps=(3, 3, 3, 3),
          pooling_width=(2, 2, 2, 2), dnn_hidden_units=(256, 128, 64), task="binary", dtype=np.float32, mutate=(), stats=None, **_):
    dt = np.dtype(dtype).type
    lin = linear_logit(linear_cols, feed, weights, dt)
    groups, _dense = _embed_groups(dnn_cols, feed, weights, "", dt)
    origin = np.concatenate([e for g in groups.values() for e in g], axis=1)
    fg_groups, _dense = _embed_groups(dnn_cols, feed, weights, "fg", dt)
    fg = np.concatenate([e for g in fg_groups.values() for e in g], axis=1)
    if "swap_fg" in mutate:
        origin, fg = fg, origin
    n = len(conv_filters)
    combined = origin
    if n > 0:
        new = fgcnn_layer(fg, weights, conv_filters, conv_kernel_width, new_maps, pooling_width, dt, mutate, stats)
        combined = np.concatenate([origin, new], axis=1)
    B, Fc = combined.shape[:2]
    inner = R.inner_product([combined[:, i:i + 1] for i in range(Fc)], reduce_sum=True).reshape(B, -1) if Fc > 1 else np.zeros((B, 0), dt)
    h = np.concatenate([combined.reshape(B, -1), inner], axis=1)
    if len(dnn_hidden_units) > 0:
        h = _dnn("dnn", h, weights, dt, "relu")
    head = "dense" if n == 0 else "dense_%d" % n
    final = _add(h @ weights[head + "/kernel"].astype(dt), lin)
    return R.prediction_layer(final, weights["prediction_layer/global_bias"].astype(dt), task)


def applicable(meta):
    """The mutations that mean something for a fixture's configuration."""
    kw, model = meta["kwargs"], meta["model"]
    widths = list(kw.get("conv_kernel_width", (6, 5) if model == "CCPM" else (7, 7, 7, 7)))
    if not widths:
        return []
    out = ["flip", "channel_first"]
    if any(w % 2 == 0 for w in widths):
        out.append("pad_side")
    if model == "CCPM":
        out.append("keep_order")
    else:
        out += ["recombine_ew", "swap_fg"]
        rows = sum(1 for d in meta["dnn"] if d["type"] != "dense")
        for p in kw.get("pooling_width", (2, 2, 2, 2)):
            if rows % p:
                out.append("pool_pad")
                break
            rows //= p
    return out


def run_fixture(g, dtype=np.float32, task=None, weights=None, mutate=(), stats=None):
    """The oracle over a tests/golden/model_ccpm_*.npz / model_fgcnn_*.npz fixture (task='regression': the logit)."""
    from tests.spec import columns_from_spec
    meta = json.loads(bytes(g["meta"]).decode())
    feed = {k[5:]: v for k, v in g.items() if k.startswith("feed/")}
    if weights is None:
        weights = {k[2:]: v for k, v in g.items() if k.startswith("w/")}
    kw = dict(meta["kwargs"])
    if task is not None:
        kw["task"] = task
    fn = ccpm if meta["model"] == "CCPM" else fgcnn
    return fn(columns_from_spec(meta["linear"]), columns_from_spec(meta["dnn"]), weights, feed, dtype=dtype, mutate=mutate, stats=stats, **kw)
