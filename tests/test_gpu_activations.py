"""GPU: the tf.keras 2.x activation names of the DNN — elu, selu, softplus, softsign, exponential, hard_sigmoid, swish (silu), gelu
(deepctr_amd/csrc/act_device.h) — through every layer that takes them, against the float64 oracle of tests/ref_activations.py (pinned
on the CPU by tests/test_activations_cpu.py).
  1. ops.mlp on every route of dctr_mlp_fwd, with / without head + sigmoid + two add vectors, with / without the BatchNormalization
     affine, save_acts checked;  2. ops.mlp_bwd on its forms;  3. ops.dnn_train_layer against autograd over the same mask;
  4. DeepFM's logits against a float64 forward, fused and through dnn_in;  5. fit on the HIP step against the autograd step;
  6. AutoInt on the autograd step;  7. the ops that keep refusing.
Inputs (RA.make_dnn) put pre-activations on both sides of 0 and of +-2.5 and a few at +-30.  Bars: tests.util.assert_close_terms'
defaults at op level (1e-4 of the result + 2e-6 of the magnitude it was summed at, carried through the function to first order by the
oracle), the project's model bar (rtol 1e-4, atol 2e-5) on logits, tests/test_gpu_train_reg.py's on the training-mode layer and
tests/test_gpu_optimizers.py's on the two fits."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import ref_activations as RA
from tests import ref_mlp_bwd as RM
from tests.util import assert_close, assert_close_terms

pytestmark = pytest.mark.gpu

GUARD = 4096
SENTINEL = -123.25


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


# ---- 1. forward ------------------------------------------------------------------------------------------------------------------------
# route -> (rows, in_dim, units, tile_rows whose results must be bit-identical): the smallest shapes that reach each kernel
#   tile     16 / 32 / 64-row workgroups of mlp_kernel (33 rows: a ragged last tile at every height; units no multiple of 16)
#   ring     tile_rows 16 with every width a multiple of 16: mlp_ring_kernel — the same bits as the 32-row tile kernel
#   ksplit   a 500-wide input: layer 0 in two K-halves at every height (the epilogue behind the persistent accumulators)
#   wide     a 2,561-wide input: no LDS tile holds it even in halves — mlp_wide_kernel
#   layered  one layer of 1,300 units: layer by layer through the workspace, the head through the no-hidden-layer launch
ROUTES = {"tile": (33, 20, (24, 8), (16, 32, 64)), "ring": (33, 20, (32, 16), (16, 32)), "ksplit": (33, 500, (24, 8), (16, 32, 64)),
          "wide": (33, 2561, (24, 8), (0,)), "layered": (65, 20, (1300,), (0,))}


@functools.lru_cache(maxsize=None)
def _fwd_reference(route, name, bn):
    B, in_dim, units, _ = ROUTES[route]
    x, ks, bs, bnp = RA.make_dnn(len(route) + 7 * len(name), B, in_dim, units, name, bn)
    rng = np.random.RandomState(3)
    hw = (rng.standard_normal(units[-1]) * 0.3).astype(np.float32)
    add = [rng.standard_normal(B).astype(np.float32) for _ in range(2)]
    zs, hs, ts = RA.dnn(x[:, :in_dim], ks, bs, name, bnp)
    for z in zs[-1:]:                                                      # the spread the docstring promises, in the layer the output shows
        assert (z < -2.5).any() and ((z > -2.5) & (z < 0)).any() and ((z > 0) & (z < 2.5)).any() and (z > 2.5).any()
    assert (np.abs(zs[0]) >= 29).sum() >= 2 and (len(units) == 1 or ((zs[1] > 14).any() and (zs[1] < -14).any()))
    assert all(np.isfinite(h).all() for h in hs)
    head = RA.head(hs[-1], ts[-1], hw, add, 0.3, sigmoid_out=True)
    return x, ks, bs, bnp, hw, add, hs, ts, head


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("name", RA.NAMES + ("silu",))
def test_mlp_forward_matches_the_float64_oracle_on_every_route(device, name, route):
    from deepctr_amd import ops
    B, in_dim, units, heights = ROUTES[route]
    gb = dev(np.array([0.3], np.float32), device)
    for bn in (False, True):
        x, ks, bs, bnp, hw, add, hs, ts, (yref, yterms) = _fwd_reference(route, RA.ALIASES.get(name, name), bn)
        xd, kd, bd = dev(x, device), [dev(k, device) for k in ks], [dev(b, device) for b in bs]
        bnd = None if bnp is None else [tuple(dev(t, device) for t in p) for p in bnp]
        for with_head in (False, True):
            kw = dict(head_w=dev(hw, device), add=[dev(a, device) for a in add], global_bias=gb, sigmoid_out=True) if with_head else {}
            first = None
            for tile in heights:
                save = [torch.full((B, n), float("nan"), dtype=torch.float32, device=device) for n in units]
                y = ops.mlp(xd, kd, bd, name, bn=bnd, in_dim=in_dim, tile_rows=tile, save_acts=save, **kw)
                torch.cuda.synchronize()
                what = "%s %s bn=%s head=%s tile_rows=%d" % (name, route, bn, with_head, tile)
                got = y.cpu().numpy().astype(np.float64)
                assert np.isfinite(got).all(), what
                if with_head:
                    assert_close_terms(got, yref, yterms, what=what + ": head")
                else:
                    assert_close_terms(got, hs[-1], ts[-1], what=what + ": output")
                for l, sv in enumerate(save):
                    assert_close_terms(sv.cpu().numpy(), hs[l], ts[l], what=what + ": save_acts[%d]" % l)
                if first is None:
                    first = (y, save)
                else:
                    assert (bits(y) == bits(first[0])).all() and all((bits(a) == bits(b)).all() for a, b in zip(save, first[1])), \
                        what + ": not the bits of tile_rows=%d" % heights[0]


# ---- 2. backward -----------------------------------------------------------------------------------------------------------------------
# form -> (rows, widths, head): the chained form at one and at three dW slices, its headless form, and the layered form (a 1,300-unit layer)
BWD = {"chain-B33": (33, (20, 24, 8), True), "chain-B513": (513, (20, 24, 8), True), "headless-B33": (33, (20, 24, 8), False),
       "layered-B33": (33, (20, 1300, 8), True)}


def _bwd_workspace_bytes(B, widths, name):
    """dctr_mlp_bwd_workspace_bytes (pinned by tests/test_activations_cpu.py): swish / gelu take the layered form with a third buffer."""
    if name in RA.FROM_Z:
        assert B < 1024                                        # (no dW row slices below 1,024 rows)
        return 4 * ((3 * B * max(widths) + 3) // 4 * 4)
    return RM.workspace_bytes(B, list(widths))


@functools.lru_cache(maxsize=None)
def _bwd_reference(form, name):
    B, w, head = BWD[form]
    x, ks, bs, _ = RA.make_dnn(11 + len(form) + 5 * len(name), B, w[0], w[1:], name)
    rng = np.random.RandomState(B + len(name))
    zs, hs, _ = RA.dnn(x[:, :w[0]], ks, bs, name)
    # the forward's saved outputs and pre-activations: float64 values rounded to float32, every layer fed the rounded outputs
    acts, pre, h = [], [], x[:, :w[0]].astype(np.float64)
    for k, b in zip(ks, bs):
        z = h @ k.astype(np.float64) + b
        pre.append(z.astype(np.float32))
        acts.append(RA.value(name, z).astype(np.float32))
        h = acts[-1].astype(np.float64)
    d = dict(x=x, ks=ks, bs=bs, acts=acts, pre=pre, hw=None, dl=None, dout=None)
    if head:
        d["hw"], d["dl"] = (rng.standard_normal(w[-1]) * 0.3).astype(np.float32), rng.standard_normal(B).astype(np.float32)
    else:
        d["dout"] = rng.standard_normal((B, w[-1] + 2)).astype(np.float32)
    g, t = RA.mlp_bwd(x[:, :w[0]], ks, bs, acts, name, head_w=d["hw"], dlogit=d["dl"], d_out=None if head else d["dout"][:, :w[-1]])

    def g0_like(ref):
        return (rng.standard_normal(ref.shape) * max(float(np.sqrt(np.mean(np.square(ref)))), 1e-3)).astype(np.float32)
    g0 = {"dW": [g0_like(a) for a in g["dW"]], "db": [g0_like(a) for a in g["db"]], "d_head_w": g0_like(g["d_head_w"]) if head else None}
    return d, g, t, g0


def _run_bwd(device, form, name, saved_z):
    from deepctr_amd import ops
    B, w, head = BWD[form]
    d, g, t, g0 = _bwd_reference(form, RA.ALIASES.get(name, name))
    x = dev(d["x"], device)
    x_before = bits(x)
    ks, acts = [dev(k, device) for k in d["ks"]], [dev(a, device) for a in d["acts"]]
    hw = dl = dout = dhw = None
    if head:
        hw, dl, dhw = dev(d["hw"], device), dev(d["dl"], device), dev(g0["d_head_w"], device)
    else:
        dout = dev(d["dout"], device)[:, :w[-1]]
    dk, db = [dev(a, device) for a in g0["dW"]], [dev(a, device) for a in g0["db"]]
    dx = torch.full((B, w[0] + 2), SENTINEL, device=device)
    need = _bwd_workspace_bytes(B, w, RA.ALIASES.get(name, name))
    ws = torch.full((need // 4 + GUARD,), float("nan"), device=device)
    guard_before = bits(ws[need // 4:])
    holder = {"ws": ws}
    extra = {}
    if RA.ALIASES.get(name, name) in RA.FROM_Z:
        extra = dict(biases=[dev(b, device) for b in d["bs"]])
        if saved_z:
            extra["saved_z"] = [dev(z, device) for z in d["pre"]]
    ops.mlp_bwd(x, w[0], ks, acts, name, hw, dl, dk, db, dhw, dx=dx, d_out=dout, workspace=holder, **extra)
    torch.cuda.synchronize()
    tag = "%s %s saved_z=%s" % (form, name, saved_z)
    assert holder["ws"] is ws, tag + ": the op replaced a workspace that was large enough"
    assert (bits(ws[need // 4:]) == guard_before).all(), tag + ": the op wrote past dctr_mlp_bwd_workspace_bytes()"
    assert (bits(x) == x_before).all(), tag + ": x changed"

    def acc(got, start, ref, terms, what):
        got, start = got.cpu().numpy().astype(np.float64), start.astype(np.float64)
        assert np.isfinite(got).all(), "%s %s: not finite" % (what, tag)
        assert_close_terms(got - start, ref, terms + np.abs(start), what="%s %s" % (what, tag))
    for l in range(len(w) - 1):
        acc(dk[l], g0["dW"][l], g["dW"][l], t["dW"][l], "dW%d" % l)
        acc(db[l], g0["db"][l], g["db"][l], t["db"][l], "db%d" % l)
    if head:
        acc(dhw, g0["d_head_w"], g["d_head_w"], t["d_head_w"], "d_head_w")
    got = dx[:, :w[0]].cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all(), "dx %s: not finite" % tag
    assert_close_terms(got, g["dx"], t["dx"], what="dx " + tag)
    assert (bits(dx[:, w[0]:]) == bits(torch.full((B, 2), SENTINEL))).all(), "dx %s: columns past in_dim changed" % tag


@pytest.mark.parametrize("form", sorted(BWD))
@pytest.mark.parametrize("name", RA.NAMES + ("silu",))
def test_mlp_bwd_matches_the_float64_oracle(device, name, form):
    """The six functions whose derivative is written in the output ride the chained form (and the layered one behind a 1,300-unit
    layer); swish / gelu take act' from z — the forward's saved pre-activations, and the recompute GEMM without them."""
    if RA.ALIASES.get(name, name) in RA.FROM_Z:
        _run_bwd(device, form, name, saved_z=True)
        _run_bwd(device, form, name, saved_z=False)
    else:
        assert RM.is_chained(list(BWD[form][1])) == (not form.startswith("layered"))
        _run_bwd(device, form, name, saved_z=False)


# ---- 3. the training-mode layer --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_bn,rate", [(True, 0.0), (False, 0.3), (True, 0.3)])
@pytest.mark.parametrize("name", RA.NAMES + ("silu",))
def test_dnn_train_layer_matches_autograd(device, name, use_bn, rate):
    """tests/test_gpu_train_reg.py::test_dnn_train_layer_matches_autograd's method and bars: autograd over the restatement
    (training._ACTS) with the kernel's own dropout mask."""
    from deepctr_amd import ops, training
    from tests.test_gpu_train_reg import _mask_scale
    R, n = 33, 20
    rng = np.random.RandomState(R + n + int(100 * rate) + len(name))
    z0 = rng.standard_normal((R, n)).astype(np.float32) * 2.0 + 0.3
    z0[1, 3], z0[2, 5], z0[4, 7], z0[5, 11] = 30.0, -30.0, 30.0, -30.0
    assert (z0 < -2.5).any() and (z0 > 2.5).any()
    z = dev(z0, device)
    gamma = dev(1.0 + 0.3 * rng.standard_normal(n).astype(np.float32), device)
    beta = dev(0.2 * rng.standard_normal(n).astype(np.float32), device)
    mm, mv = dev(rng.standard_normal(n).astype(np.float32), device), dev(rng.rand(n).astype(np.float32) + 0.5, device)
    seed = 4321 + n
    bn = dict(gamma=gamma, beta=beta, moving_mean=mm, moving_var=mv, eps=1e-3, momentum=0.99,
              batch_mean=torch.empty(n, device=device), batch_var=torch.empty(n, device=device)) if use_bn else None
    hbuf = torch.zeros(R, n + 5, dtype=torch.float32, device=device)
    h = ops.dnn_train_layer(z, name, h=hbuf[:, 2:2 + n], bn=bn, dropout_rate=rate, dropout_seed=seed)
    ms = _mask_scale(R, n, rate, seed, device) if rate > 0 else torch.ones(R, n, device=device)
    zt = z.clone().requires_grad_(True)
    gt, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y = zt
    if use_bn:
        bm, bv = zt.mean(0), zt.var(0, unbiased=False)
        y = (zt - bm) * torch.rsqrt(bv + 1e-3) * gt + bt
    href = training._ACTS[name](y) * ms
    assert bool(torch.isfinite(h).all())
    assert_close(h.cpu().numpy(), href.detach().cpu().numpy(), rtol=2e-5, atol=2e-6, what="forward %s" % name)
    assert float(hbuf[:, :2].abs().max()) == 0.0 and float(hbuf[:, 2 + n:].abs().max()) == 0.0
    dh = dev(rng.standard_normal((R, n + 3)).astype(np.float32), device)[:, 1:1 + n]
    gz, gg, gb = torch.autograd.grad((href * dh).sum(), [zt, gt, bt], allow_unused=True)
    dz = torch.empty(R, n, dtype=torch.float32, device=device)
    d_gamma, d_beta = torch.full((n,), 0.5, device=device), torch.full((n,), -0.25, device=device)
    ops.dnn_train_layer(z, name, bn=bn, dropout_rate=rate, dropout_seed=seed, dh=dh, dz=dz, d_gamma=d_gamma, d_beta=d_beta)
    assert_close(dz.cpu().numpy(), gz.cpu().numpy(), rtol=3e-4, atol=3e-6, what="dz %s" % name)
    if use_bn:
        assert_close((d_gamma - 0.5).cpu().numpy(), gg.cpu().numpy(), rtol=3e-4, atol=2e-5, what="d_gamma %s" % name)
        assert_close((d_beta + 0.25).cpu().numpy(), gb.cpu().numpy(), rtol=3e-4, atol=2e-5, what="d_beta %s" % name)


# ---- 4. model level ---------------------------------------------------------------------------------------------------------------------
def _deepfm_cols(E=8, hashed=True, **kw):
    from deepctr_amd.feature_column import DenseFeat, SparseFeat
    return [SparseFeat("a", 50, E, **kw), SparseFeat("b", 47, E, use_hash=hashed, **kw), SparseFeat("c", 9, E, **kw), DenseFeat("d", 1)]


def _feed(rng, cols, n):
    from tests.test_gpu_train import _feed as base
    return base(rng, cols, n)


def _deepfm_float64_logits(cols, w, feed, name, n_layers=2):
    """float64: the oracle's lookup / linear / FM pieces, the new DNN oracle, Dense(1), the global bias.  First every DNN kernel in
    ``w`` is scaled (in place) so that its layer's pre-activations have a standard deviation of 1.5 on this feed: behind embeddings of
    0.05 they would stay within +-0.1, where all eight functions are straight lines, and behind an unbounded function they would not
    stay finite."""
    from oracle import ref_models as OM
    from oracle import ref_numpy as R
    dt = np.float64
    lin = OM.linear_logit(cols, feed, w, dt)
    groups, dense = OM._embed_groups(cols, feed, w, "", dt)
    fm = R.fm(np.concatenate(groups["default_group"], axis=1))
    dnn_in = OM._combined_dnn_input([e for g in groups.values() for e in g], dense)
    h = dnn_in
    for i in range(n_layers):
        k = "dnn/kernel%d" % i
        w[k] = (w[k] * (1.5 / float((h @ w[k].astype(dt)).std()))).astype(np.float32)
        h = RA.dnn(h, [w[k]], [w["dnn/bias%d" % i]], name)[1][-1]
    ks, bs = [w["dnn/kernel%d" % i].astype(dt) for i in range(n_layers)], [w["dnn/bias%d" % i].astype(dt) for i in range(n_layers)]
    zs, hs, _ = RA.dnn(dnn_in, ks, bs, name)
    assert min(float(np.abs(z).max()) for z in zs) > 2.5 and np.isfinite(hs[-1]).all()
    return (OM._add(lin, hs[-1] @ w["dense/kernel"].astype(dt), fm) + w["prediction_layer/global_bias"].astype(dt)).reshape(-1)


@pytest.mark.parametrize("name", RA.NAMES + ("silu",))
def test_deepfm_logits_match_a_float64_forward(device, name):
    """3 sparse + 1 dense feature, 70 rows, units (16, 8).  (A DNN this narrow leaves the gather's partial sums no room in the second
    LDS tile: the model takes the route through dnn_in; the one-launch route has the test below.)"""
    from deepctr_amd.models import DeepFM
    from tests.test_gpu_models import _randomise
    rng = np.random.RandomState(40 + len(name))
    cols, n = _deepfm_cols(), 70
    model = DeepFM(cols, cols, dnn_hidden_units=(16, 8), dnn_activation=name, device=device)
    w = _randomise(model, rng)
    feed = _feed(rng, cols, n)
    ref = _deepfm_float64_logits(cols, w, feed, name)
    model.set_weights_by_name(w)
    got = model.predict_logits(feed, batch_size=64).reshape(-1)
    assert_close(got, ref, rtol=1e-4, atol=2e-5, what="DeepFM %s logits" % name)


@pytest.mark.parametrize("name", RA.NAMES + ("silu",))
def test_deepfm_one_launch_route_and_dnn_in_route_agree(device, name):
    """The one-launch route (dctr_embed_mlp_fwd: the row-chained and streaming kernels decline the code, the tile kernels take it) needs
    a DNN input wide enough for the gather's partial sums: 9 sparse features of 16 + 1 dense = 145 columns.  Both routes against the
    float64 forward and against each other, at the model bar."""
    from deepctr_amd.feature_column import DenseFeat, SparseFeat
    from deepctr_amd.models import DeepFM
    from tests.test_gpu_models import _randomise
    rng = np.random.RandomState(50 + len(name))
    cols = [SparseFeat("s%d" % i, 30 + i, 16, use_hash=(i == 1)) for i in range(9)] + [DenseFeat("d", 1)]
    n = 70
    model = DeepFM(cols, cols, dnn_hidden_units=(16, 8), dnn_activation=name, device=device)
    w = _randomise(model, rng)
    feed = _feed(rng, cols, n)
    ref = _deepfm_float64_logits(cols, w, feed, name)
    model.set_weights_by_name(w)
    assert model.stage_plan.fusable and model.fused
    calls = []
    from deepctr_amd import ops
    real = ops.mlp
    try:
        ops.mlp = lambda *a, **k: calls.append(k.get("gather") is not None) or real(*a, **k)
        fused = model.predict_logits(feed, batch_size=64).reshape(-1)
        assert calls and all(calls) and not model._declined, "the one-launch route was not taken: %r / %r" % (calls, model._declined)
        del calls[:]
        model.fused = False
        plain = model.predict_logits(feed, batch_size=64).reshape(-1)
        assert calls and not any(calls), "the route through dnn_in was not taken: %r" % (calls,)
    finally:
        ops.mlp = real
    assert_close(fused, ref, rtol=1e-4, atol=2e-5, what="DeepFM %s logits, one launch" % name)
    assert_close(plain, ref, rtol=1e-4, atol=2e-5, what="DeepFM %s logits, through dnn_in" % name)
    assert_close(fused, plain, rtol=1e-4, atol=2e-5, what="DeepFM %s: the two routes" % name)


# ---- 5. fit: the HIP step against the autograd step ---------------------------------------------------------------------------------
FIT_KINDS = ("DeepFM", "xDeepFM", "DIN", "DeepFM-reg")
FIT_ROWS, FIT_BATCH = 70, 30                    # three batches, the last of 10 rows
FIT_LR = 0.005                                  # plain SGD; exponential's first steps overshoot at rates of 0.03 and more


def fit_case(kind, name, device, seed=0):
    """(make, feed, y) of a fit comparison: the layers' default initialisers, labels computed from the features.  Shared with
    tests/test_activations_cpu.py, which checks on the CPU that the autograd step's losses stay finite and decrease.  The embedding
    tables alone get RandomNormal(0, 0.1) in place of the feature columns' default RandomNormal(0, 1e-4): behind tables of 1e-4 the CIN
    filters and the attention unit see gradients whose three updates stay below an ulp of the weights, and the per-tensor rule of
    tests/test_gpu_optimizers.py asks that every tensor moves."""
    from deepctr_amd import models
    from deepctr_amd.initializers import RandomNormal
    rng = np.random.RandomState(seed)
    n = FIT_ROWS
    init = dict(embeddings_initializer=RandomNormal(mean=0.0, stddev=0.1, seed=2020))
    if kind == "DIN":
        from deepctr_amd.feature_column import DenseFeat, SparseFeat, VarLenSparseFeat
        E, T = 8, 6
        cols = [SparseFeat("user", 50, E, **init), SparseFeat("gender", 2, E, **init), SparseFeat("item_id", 31, E, **init),
                SparseFeat("cate_id", 11, E, **init), DenseFeat("pay_score", 1),
                VarLenSparseFeat(SparseFeat("hist_item_id", 31, E, embedding_name="item_id", **init), maxlen=T),
                VarLenSparseFeat(SparseFeat("hist_cate_id", 11, E, embedding_name="cate_id", **init), maxlen=T),
                VarLenSparseFeat(SparseFeat("other_seq", 9, E, **init), maxlen=4, combiner="mean")]
        make = lambda: models.DIN(cols, ["item_id", "cate_id"], dnn_activation=name, dnn_hidden_units=(16, 8), att_hidden_size=(12, 6),   # noqa: E731
                                  device=device)
        lens = rng.randint(0, T + 1, n)                    # (rows with an empty history among them)
        pad = np.arange(T)[None, :] >= lens[:, None]
        hi_, hc_ = rng.randint(1, 31, (n, T)).astype(np.int32), rng.randint(1, 11, (n, T)).astype(np.int32)
        hi_[pad], hc_[pad] = 0, 0
        feed = {"user": rng.randint(0, 50, n).astype(np.int32), "gender": rng.randint(0, 2, n).astype(np.int32),
                "item_id": rng.randint(1, 31, n).astype(np.int32), "cate_id": rng.randint(1, 11, n).astype(np.int32),
                "pay_score": rng.rand(n).astype(np.float32), "hist_item_id": hi_, "hist_cate_id": hc_,
                "other_seq": rng.randint(0, 9, (n, 4)).astype(np.int32)}
        y = ((feed["user"] % 3 == 0) ^ (feed["pay_score"] > 0.5)).astype(np.float32)
        return make, feed, y
    cols = _deepfm_cols(hashed=False, **init)              # (hashing is a device op: the CPU check of these cases runs without it)
    kw = dict(dnn_hidden_units=(16, 8), dnn_activation=name, device=device)
    if kind == "xDeepFM":
        make = lambda: models.xDeepFM(cols, cols, cin_layer_size=(8, 8), **kw)                   # noqa: E731
    elif kind == "DeepFM-reg":
        make = lambda: models.DeepFM(cols, cols, dnn_dropout=0.3, dnn_use_bn=True, **kw)         # noqa: E731
    else:
        make = lambda: models.DeepFM(cols, cols, **kw)                                           # noqa: E731
    feed = _feed(rng, cols, n)
    y = ((feed["a"] % 3 == 0) ^ (feed["d"] > 0.5)).astype(np.float32)
    return make, feed, y


@pytest.mark.parametrize("kind", FIT_KINDS)
@pytest.mark.parametrize("name", RA.NAMES)
def test_fit_on_the_hip_step_matches_the_autograd_step(device, name, kind, monkeypatch):
    """SGD, three batches (the last ragged) from the same weights: the epoch loss at tests/test_gpu_optimizers.py's bar for the two
    steps (rtol 2e-5, atol 1e-7) and the weights by its per-tensor rule (_weights_close).  With dropout the autograd step multiplies by
    the masks the HIP step's kernel drew (tests/test_gpu_train_reg.py's method): the two generators are different ones."""
    from deepctr_amd import training
    from deepctr_amd.optimizers import SGD
    from deepctr_amd.training_hip import HipTrainer
    from tests.test_gpu_optimizers import _weights_close
    from tests.test_gpu_train_reg import _mask_scale
    make, feed, y = fit_case(kind, name, device)
    w0 = make().get_weights_by_name()
    out, seeds = {}, []
    real_seed = HipTrainer.dropout_seed
    for hip in (True, False):
        model = make()
        model.set_weights_by_name(w0)
        model.hip_training = hip
        model.compile(SGD(FIT_LR), "binary_crossentropy")
        if kind == "DeepFM-reg":
            L, rate = len(model.dnn.kernels), 0.3
            if hip:
                monkeypatch.setattr(HipTrainer, "dropout_seed", lambda tr, layer: seeds.append(real_seed(tr, layer)) or seeds[-1])
            else:
                # per step the HIP step asked for its L forward seeds, then the same L again in its backward
                fwd = iter([s for i in range(0, len(seeds), 2 * L) for s in seeds[i:i + L]])
                monkeypatch.setattr(training, "_dropout", lambda x, r, t: x * _mask_scale(x.shape[0], x.shape[1], rate, next(fwd), device)
                                    if (t and r and r > 0) else x)
        h = model.fit(feed, y, batch_size=FIT_BATCH, epochs=1, verbose=0, shuffle=False)
        monkeypatch.undo()
        assert (getattr(model, "_hip_trainer", None) is not None) == hip, "fit() took the wrong step"
        if hip:
            tr = model._hip_trainer
            assert tr.zact_dnn == (name in RA.FROM_Z) and tr.slow_dnn == (kind == "DeepFM-reg")
        out[hip] = (h.history["loss"], model.get_weights_by_name())
    what = "%s %s" % (kind, name)
    assert len(seeds) == (3 * 2 * 2 if kind == "DeepFM-reg" else 0)
    assert np.isfinite(out[True][0]).all() and np.isfinite(out[False][0]).all()
    print("%s: fit loss %r (HIP step) %r (autograd step)" % (what, out[True][0], out[False][0]))
    assert_close(np.array(out[True][0]), np.array(out[False][0]), rtol=2e-5, atol=1e-7, what=what + ": fit loss, HIP step vs autograd step")
    _weights_close(what, w0, out[True][1], out[False][1])


# ---- 6. a model of the autograd step ----------------------------------------------------------------------------------------------------
def test_autoint_with_gelu_trains_on_the_autograd_step(device):
    from deepctr_amd import engine, training, training_hip
    from deepctr_amd.models import AutoInt
    rng = np.random.RandomState(6)
    cols, n = _deepfm_cols(), 512
    model = AutoInt(cols, cols, att_layer_num=1, att_embedding_size=4, att_head_num=2, dnn_hidden_units=(16, 8), dnn_activation="gelu", device=device)
    assert not training_hip.supported(model)
    feed = _feed(rng, cols, n)
    y = ((feed["a"] % 3 == 0) ^ (feed["d"] > 0.5)).astype(np.float32)
    model.compile("adam", "binary_crossentropy")
    h = model.fit(feed, y, batch_size=128, epochs=6, verbose=0)
    assert getattr(model, "_hip_trainer", None) is None
    assert np.isfinite(h.history["loss"]).all() and h.history["loss"][-1] < h.history["loss"][0]
    got = model.predict_logits(feed, batch_size=256).reshape(-1)
    staged = engine.Staged(n)
    model._stage_inputs(feed, staged)
    model._begin()
    with torch.no_grad():
        ref = training.model_logits(model, staged, 0, n).double().cpu().numpy().reshape(-1)
    assert_close(got, ref, rtol=1e-4, atol=2e-5, what="AutoInt gelu: predict_logits vs training.model_logits")


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------
def test_the_other_kernels_still_refuse(device):
    from deepctr_amd import _C, ops
    F, E = 3, 4
    D = F * E
    x = torch.zeros(4, D, device=device)
    z = lambda *shape: torch.zeros(*shape, device=device)          # noqa: E731
    with pytest.raises(ValueError, match="unknown activation"):
        ops.edcn(x, F, E, [z(1, F, 1), z(1, F, 1)], [z(D, 1)], [z(D, 1)], [z(D, D)], [z(D)], activation="selu")
    with pytest.raises(ValueError, match="unknown activation"):
        ops.edcn(x, F, E, [z(1, F, 1), z(1, F, 1)], [z(D, 1)], [z(D, 1)], [z(D, D)], [z(D)], bridge_activation="gelu")
    # DIN's attention kernels: code 5 is an enum error, nothing is written
    B, T, E = 3, 4, 4
    q, k = torch.zeros(B, E, device=device), torch.zeros(B, T, E, device=device)
    mask, out = torch.ones(B, T, dtype=torch.uint8, device=device), torch.full((B, E), SENTINEL, device=device)
    W, b = [torch.zeros(4 * E, 4, device=device)], [torch.zeros(4, device=device)]
    units = (ctypes.c_int32 * 1)(4)
    kp, bp = (ctypes.c_void_p * 1)(W[0].data_ptr()), (ctypes.c_void_p * 1)(b[0].data_ptr())
    ok, ob = torch.zeros(4, 1, device=device), torch.zeros(1, device=device)
    a = _C.DinAttnArgs(query=q.data_ptr(), keys=k.data_ptr(), key_mask=mask.data_ptr(), batch=B, maxlen=T, dim=E, n_layers=1, activation=5,
                       units=ctypes.cast(units, ctypes.c_void_p), kernels=ctypes.cast(kp, ctypes.c_void_p), biases=ctypes.cast(bp, ctypes.c_void_p),
                       out_kernel=ok.data_ptr(), out_bias=ob.data_ptr(), out=out.data_ptr(), out_stride=E)
    assert _C.lib().dctr_din_attn_pool_fwd(ctypes.byref(a), _C.stream_ptr()) == -4          # DCTR_E_ENUM
    torch.cuda.synchronize()
    assert float((out - SENTINEL).abs().max()) == 0.0
