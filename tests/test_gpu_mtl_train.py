"""GPU: the multi-task models' HIP training step (DESIGN.md §4.15 "Training") — ops.mtl_mix_bwd and ops.mtl_loss_grad against the float64
oracle (tests/ref_mtl_bwd.py), ops.mtl_sum_slots against the same float32 sum in torch, one HipTrainer.step against autograd over the
models' restatement, fit() on the HIP step against fit() on the autograd step from the same weights, and a seeded mini-fuzz over the
four constructors."""
import numpy as np
import pytest
import torch

from tests import ref_mtl_bwd as RB
from tests.test_gpu_flen import _normalised
from tests.test_mtl_train_cpu import FUZZ_SEEDS, MIX_SWEEP, MODELS, fuzz_setup, mix_case
from tests.util import assert_close, assert_close_terms

pytestmark = pytest.mark.gpu
NAN = float("nan")


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)


def _inside(device, a, left, right, fill=None):
    """``a`` as the columns [left, left + width) of a wider buffer (random, or ``fill``, around it): (buffer, the view)."""
    a = np.asarray(a, dtype=np.float32)
    buf = np.random.RandomState(a.shape[1] + left).standard_normal((a.shape[0], left + a.shape[1] + right)).astype(np.float32)
    if fill is not None:
        buf[:] = fill
    buf[:, left:left + a.shape[1]] = a
    t = dev(buf, device)
    return t, t[:, left:left + a.shape[1]]


@pytest.mark.parametrize("i", range(len(MIX_SWEEP)))
def test_mix_bwd_vs_float64_oracle(device, i):
    from deepctr_amd import ops
    B, E, H, dz, members = MIX_SWEEP[i]
    G, n_all = len(members), sum(len(ms) for ms in members)
    case = mix_case(B, E, H, dz, members, 300 + i)
    args = (case["h"], H, case["z"], case["gate_kernels"], members, case["d_out"])
    ref, mag = RB.mix_bwd(*args), RB.mix_bwd(*args, absolute=True)
    what = "B=%d E=%d H=%d dz=%d members=%s: " % (B, E, H, dz, members)
    # every operand is a view with a column offset inside a wider buffer; the outputs sit between NaN sentinels
    _, h = _inside(device, case["h"], 2, 3)
    zs = [_inside(device, z, 1 + g % 2, 2)[1] for g, z in enumerate(case["z"])]
    gk = [dev(w, device) for w in case["gate_kernels"]]
    dbuf, _ = _inside(device, case["d_out"], 3, 1)
    nan = lambda cols: _inside(device, np.full((B, cols), NAN), 4, 3, fill=NAN)      # noqa: E731
    (dh_buf, dh), (ds_buf, ds), (lg_buf, lg) = nan(E * H), nan(n_all), nan(n_all)
    run = lambda dh_, ds_, lg_: ops.mtl_mix_bwd(h, E, H, zs, gk, members, dbuf, dh_, ds_, d_out_offset=3, logits=lg_)      # noqa: E731
    run(dh, ds, lg)
    for buf, cols in ((dh_buf, E * H), (ds_buf, n_all), (lg_buf, n_all)):
        assert torch.isnan(buf[:, :4]).all() and torch.isnan(buf[:, 4 + cols:]).all() and torch.isfinite(buf[:, 4:4 + cols]).all(), what
    bar = dict(rtol=1e-4, rtol_terms=RB.OP_RTOL_TERMS)
    assert_close_terms(dh.cpu().numpy(), ref["dh"], mag["dh"], what=what + "dh", **bar)
    assert_close_terms(ds.cpu().numpy(), ref["ds"], mag["ds"], what=what + "ds", **bar)
    lmag = np.concatenate([np.abs(z).astype(np.float64) @ np.abs(w).astype(np.float64) for z, w in zip(case["z"], case["gate_kernels"])], axis=1)
    assert_close_terms(lg.cpu().numpy(), ref["logits"], lmag, what=what + "logits", **bar)
    if n_all == 1:
        assert (ds == 0).all()                              # a gate of one member: p = 1, ds exactly 0
    for e in range(E):
        if not any(e in ms for ms in members):
            assert (dh[:, e * H:(e + 1) * H] == 0).all()    # an expert no gate mixes
    (_, dh2), (_, ds2), (_, lg2) = nan(E * H), nan(n_all), nan(n_all)
    run(dh2, ds2, lg2)
    assert torch.equal(dh2, dh) and torch.equal(ds2, ds) and torch.equal(lg2, lg)              # the same bits on a second call
    dh3, ds3 = torch.empty(B, E * H, device=device), torch.empty(B, n_all, device=device)
    ops.mtl_mix_bwd(h, E, H, zs, gk, members, dbuf, dh3, ds3, d_out_offset=3)                  # without the logits, dense outputs
    assert torch.equal(dh3, dh) and torch.equal(ds3, ds)
    # the rest of the gate's backward is a bias-free linear layer's: dWg = z^T ds, dz = ds Wg^T through ops.mlp_bwd
    first = 0
    for g, ms in enumerate(members):
        n = len(ms)
        dW, dzg = torch.full((dz, n), 0.5, device=device), torch.full((B, dz + 2), NAN, device=device)
        ops.mlp_bwd(zs[g], dz, [gk[g]], [lg[:, first:first + n]], "linear", None, None, [dW], [None], None, dx=dzg[:, 1:1 + dz],
                    d_out=ds[:, first:first + n])
        assert torch.isnan(dzg[:, 0]).all() and torch.isnan(dzg[:, 1 + dz:]).all()
        assert_close_terms(dzg[:, 1:1 + dz].cpu().numpy(), ref["dz"][g], mag["dz"][g], what=what + "dz of gate %d" % g)
        assert_close_terms((dW - 0.5).cpu().numpy(), ref["dWg"][g], mag["dWg"][g] + 0.5, what=what + "dWg of gate %d" % g)
        first += n


LOSS_TYPES = {1: ["binary"], 2: ["binary", "regression"], 3: ["regression", "binary", "binary"]}


def _loss_case(device, types, B, seed, esmm=False):
    rng = np.random.RandomState(seed)
    T = len(types)
    logits = rng.uniform(-4, 4, (T, B)) if esmm else rng.standard_normal((T, B)) * 2.0
    if esmm:
        logits[:, 0], logits[:, 1] = -20.0, 20.0            # the clipped region; 1 - pc at the clip
    y = np.stack([(rng.rand(B) < 0.5).astype(np.float64) if t == "binary" else rng.standard_normal(B) for t in types])
    lt = dev(logits, device)
    pred = torch.stack([torch.sigmoid(lt[t]) if types[t] == "binary" else lt[t] for t in range(T)])
    return pred, dev(y, device)


def _run_loss(device, pred, y, types, weights, esmm):
    from deepctr_amd import ops
    T, B = pred.shape
    pb, yb, db = (torch.full((T, B + 3), NAN, device=device) for _ in range(3))
    pb[:, 1:1 + B], yb[:, 2:2 + B] = pred, y
    loss_sum = torch.full((T,), 0.5, device=device)
    dbias = [torch.full((1,), 0.5, device=device) for _ in range(T)]
    losses = ["binary_crossentropy" if t == "binary" else "mse" for t in types]
    ops.mtl_loss_grad(pb[:, 1:1 + B], yb[:, 2:2 + B], db[:, 1:1 + B], loss_sum, losses, [t == "binary" for t in types], weights, esmm=esmm,
                      dbias=dbias)
    assert torch.isnan(db[:, 0]).all() and torch.isnan(db[:, 1 + B:]).all()
    return db[:, 1:1 + B], loss_sum, torch.cat(dbias)


def _check_loss(device, types, B, weights, seed, esmm=False):
    pred, y = _loss_case(device, types, B, seed, esmm)
    dl, loss_sum, dbias = _run_loss(device, pred, y, types, weights, esmm)
    losses = ["binary_crossentropy" if t == "binary" else "mse" for t in types]
    # the oracle reads the float32 outputs the kernel reads, with the clip bound a float32 computation holds (1 - 2^-23)
    rdl, rloss, rdb = RB.loss_grad(pred.cpu().numpy(), y.cpu().numpy(), losses, [t == "binary" for t in types], weights, esmm=esmm, hi=RB.HI32)
    what = "T=%d B=%d esmm=%d: " % (len(types), B, esmm)
    assert_close(dl.cpu().numpy().astype(np.float64) * B, rdl * B, rtol=1e-5, atol=1e-7, what=what + "dlogit * B")
    # (added to 0.5 in float32: half an ulp of the sum per addition on top of the relative bar)
    assert_close((loss_sum.cpu().numpy().astype(np.float64) - 0.5), rloss, rtol=1e-5, atol=1e-6, what=what + "loss_sum")
    # (dbias is a cancelling sum: 8 ulp of the magnitude it was summed at — a 512-leaf tree is 9 additions deep, half an ulp each, twice)
    terms = 0.5 + float(np.abs(rdl).sum(-1).max())
    assert_close((dbias.cpu().numpy().astype(np.float64) - 0.5), rdb, rtol=1e-5, atol=8 * 2.0 ** -23 * terms, what=what + "dbias")
    dl2, loss2, db2 = _run_loss(device, pred, y, types, weights, esmm)
    assert torch.equal(dl2, dl) and torch.equal(loss2, loss_sum) and torch.equal(db2, dbias)
    return dl, y


@pytest.mark.parametrize("B", [1, 63, 300])
@pytest.mark.parametrize("T", [1, 2, 3])
def test_loss_grad_vs_oracle(device, T, B):
    _check_loss(device, LOSS_TYPES[T], B, [1.0, 0.5, 2.0][:T], 40 + 7 * T + B)


def test_loss_grad_esmm_vs_oracle(device):
    for B in (2, 63, 300):
        dl, y = _check_loss(device, ["binary", "binary"], B, [1.0, 0.5], 90 + B, esmm=True)
        assert (dl[1, :2] == 0).all()                       # p1 outside [1e-7, 1 - 1e-7]: torch's clamp passes no gradient
        if B > 2:
            assert (dl[1, 2:] != 0).all()


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("n_src,n", [(1, 13), (5, 13), (16, 13), (3, 64)])
def test_sum_slots_is_the_same_float32_sum(device, n_src, n, accumulate):
    from deepctr_amd import ops
    B = 37
    rng = np.random.RandomState(n_src + n)
    srcs = [dev(rng.standard_normal((B, n + 3 + k % 2)), device)[:, k % 3:k % 3 + n] for k in range(n_src)]
    base = dev(rng.standard_normal((B, n + 6)), device) if accumulate else torch.full((B, n + 6), NAN, device=device)
    dst = base.clone()
    assert ops.mtl_sum_slots(srcs, n, dst, dst_offset=2, accumulate=accumulate) is dst
    want = base[:, 2:2 + n] + srcs[0] if accumulate else srcs[0].clone()
    for s in srcs[1:]:
        want = want + s
    assert torch.equal(dst[:, 2:2 + n], want)
    keep = torch.ones(n + 6, dtype=torch.bool, device=device)
    keep[2:2 + n] = False
    assert torch.equal(torch.nan_to_num(dst[:, keep], nan=7.0), torch.nan_to_num(base[:, keep], nan=7.0))      # nothing else is touched
    again = base.clone()
    ops.mtl_sum_slots(srcs, n, again, dst_offset=2, accumulate=accumulate)
    assert torch.equal(torch.nan_to_num(again, nan=7.0), torch.nan_to_num(dst, nan=7.0))


def _step_cols():
    """F 5, E 8, one hashed feature, two pooled sequences, 2 dense (tests/test_gpu_mtl.py::_cols with the hash fixed)."""
    from deepctr_amd.feature_column import DenseFeat, SparseFeat, VarLenSparseFeat
    cols = []
    for k in range(5):
        if k in (2, 4):
            cols.append(VarLenSparseFeat(SparseFeat("S%d" % k, 9 + k, 8), maxlen=4, combiner=("mean", "sum")[k % 4 // 2 % 2]))
        else:
            cols.append(SparseFeat("C%d" % k, 20 + 3 * k, 8, use_hash=k == 1))
    return cols + [DenseFeat("D%d" % k, 1 + k) for k in range(2)]


def _build(kind, device, seed, cols, **kw):
    from deepctr_amd import models
    from tests.test_gpu_models import _randomise
    rng = np.random.RandomState(seed)
    model = getattr(models, kind)(cols, device=device, **kw)
    w = _randomise(model, rng)
    w = {k: (rng.standard_normal(v.shape).astype(np.float32) if "gate_softmax" in k else v) for k, v in w.items()}
    model.set_weights_by_name(w)
    return model, w


def _labels(rng, types, n):
    return [(rng.rand(n) > 0.5).astype(np.float32) if t == "binary" else rng.standard_normal(n).astype(np.float32) for t in types]


STEP_CASES = {
    "mmoe": ("MMOE", dict(num_experts=3, expert_dnn_hidden_units=(16, 8), gate_dnn_hidden_units=(), tower_dnn_hidden_units=(8,))),
    "mmoe_gate_dnn": ("MMOE", dict(num_experts=3, expert_dnn_hidden_units=(16, 8), gate_dnn_hidden_units=(6,), tower_dnn_hidden_units=(8,))),
    "ple_1_1": ("PLE", dict(num_levels=2, shared_expert_num=1, specific_expert_num=1, expert_dnn_hidden_units=(16,), tower_dnn_hidden_units=(8,))),
    "ple_2_2": ("PLE", dict(num_levels=2, shared_expert_num=2, specific_expert_num=2, expert_dnn_hidden_units=(16,), tower_dnn_hidden_units=(8,),
                            gate_dnn_hidden_units=(5,))),
    "sb": ("SharedBottom", dict(bottom_dnn_hidden_units=(16, 8), tower_dnn_hidden_units=(8,))),
    "sb_no_tower": ("SharedBottom", dict(bottom_dnn_hidden_units=(16, 8), tower_dnn_hidden_units=())),
    "esmm": ("ESMM", dict(tower_dnn_hidden_units=(16, 8))),
    "mmoe_regression": ("MMOE", dict(num_experts=3, expert_dnn_hidden_units=(16, 8), tower_dnn_hidden_units=(8,),
                                     task_types=("binary", "regression"))),
}


@pytest.mark.parametrize("case", sorted(STEP_CASES))
def test_hip_step_matches_autograd(device, case):
    """One HipTrainer.step(apply=False) on 211 rows against autograd over autograd_logits / _fit.task_losses (the method of
    tests/test_gpu_flen.py::_step_vs_autograd): the total loss, and every parameter gradient at the normalised bar."""
    from deepctr_amd.models.multitask import _fit
    from deepctr_amd.training_hip import HipTrainer, supported
    from tests.test_gpu_mtl import _fuzz_feed
    kind, kw = STEP_CASES[case]
    cols, n = _step_cols(), 211
    model, _ = _build(kind, device, 31, cols, l2_reg_dnn=1e-3, l2_reg_embedding=1e-3, **kw)
    weights = [1.0, 0.3] if case == "mmoe_regression" else [1.0, 0.5]
    model.compile("adam", loss_weights=weights)
    assert supported(model)
    rng = np.random.RandomState(77)
    feed = _fuzz_feed(rng, cols, n)
    yt = dev(np.stack(_labels(rng, model.task_types, n)), device)
    staged = model.stage(feed)
    model._begin()
    tr = HipTrainer(model)
    names = {t.data_ptr(): k for k, t in model.named_weights()}
    assert sorted(names[p.w.data_ptr()] for p in tr.params) == sorted(names.values())
    loss = tr.step(staged, 0, n, yt, apply=False)
    assert tuple(loss.shape) == (2,)
    params = [p.w for p in tr.params]
    for t in params:
        t.requires_grad_(True)
    try:
        model._begin()
        pairs = _fit.task_losses(model, model.autograd_logits(staged, 0, n, training=True), yt)
        grads = torch.autograd.grad(sum(w * l for w, (l, _) in zip(weights, pairs)), params, allow_unused=True)
    finally:
        for t in params:
            t.requires_grad_(False)
    for t in range(2):
        assert_close(loss[t:t + 1].cpu().numpy(), [float(pairs[t][1])], rtol=1e-4, atol=1e-6, what="%s: loss of task %d" % (case, t))
    total = float(sum(w * float(l) for w, l in zip(weights, loss.cpu().numpy())))
    assert_close([total], [float(sum(w * float(s) for w, (_, s) in zip(weights, pairs)))], rtol=1e-4, atol=1e-6, what=case + ": total loss")
    assert all(g is not None for g in grads)
    gmax = max(float(g.abs().max()) for g in grads)
    for p, gref in zip(tr.params, grads):
        assert float(gref.abs().max()) > 0, names[p.w.data_ptr()]
        _normalised(p.g.cpu().numpy(), gref.cpu().numpy(), gmax, "%s: grad of %s" % (case, names[p.w.data_ptr()]))


def _fit_both(kind, kw, cols, w, feed, ys, bs, optimizer, device, loss_weights=None):
    from deepctr_amd import models
    out = []
    for hip in (True, False):
        model = getattr(models, kind)(cols, device=device, **kw)
        model.set_weights_by_name(w)
        model.hip_training = hip
        model.compile(optimizer, loss_weights=loss_weights)
        h = model.fit(feed, ys, batch_size=bs, epochs=1, verbose=0, shuffle=False).history
        assert (getattr(model, "_hip_trainer", None) is not None) == hip, "fit() took the wrong step"
        out.append((model, h))
    return out


def _check_updates(what, optimizer, w, m_hip, m_ref):
    """tests/test_gpu_fuzz.py::_check_fit's bars on the updated weights."""
    w_hip, w_ref = m_hip.get_weights_by_name(), m_ref.get_weights_by_name()
    for k in w_ref:
        d_hip, d_ref = (w_hip[k] - w[k]).astype(np.float64), (w_ref[k] - w[k]).astype(np.float64)
        moved = float(np.abs(d_ref).max())
        err = np.abs(d_hip - d_ref) / max(moved, 1e-6)
        if optimizer == "sgd":
            assert float(err.max()) < 2e-2, "%s: update of %s (largest %.3g): off by %.3g of it" % (what, k, moved, float(err.max()))
        elif moved >= 3e-4:
            bad = float((err > 0.1).mean())
            assert bad < 1e-2, "%s: update of %s (largest %.3g): %.2f %% of the elements differ by > 10 %% of it" % (what, k, moved, 100 * bad)


@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
@pytest.mark.parametrize("kind", sorted(MODELS))
def test_fit_takes_the_hip_step_and_matches_the_autograd_step(device, kind, optimizer):
    """fit() on both steps from the same weights, three batches with the last one ragged: the same losses, the same updated weights, and
    predict() afterwards scores with the moved weights."""
    from tests.test_gpu_mtl import _fuzz_feed
    cols, bs = _step_cols(), 64
    n = 2 * bs + 21
    kw = dict(MODELS[kind], l2_reg_dnn=1e-3, l2_reg_embedding=1e-3)
    probe, w = _build(kind, device, 11, cols, **kw)
    rng = np.random.RandomState(12)
    feed = _fuzz_feed(rng, cols, n)
    ys = _labels(rng, probe.task_types, n)
    (m_hip, h_hip), (m_ref, h_ref) = _fit_both(kind, kw, cols, w, feed, ys, bs, optimizer, device, loss_weights=[1.0, 0.5])
    what = "%s %s" % (kind, optimizer)
    assert list(h_hip) == list(h_ref) == ["loss"] + ["%s_loss" % t for t in probe.task_names]
    for k in h_ref:
        assert_close(h_hip[k], h_ref[k], rtol=1e-3, atol=1e-6, what="%s: %s" % (what, k))
    if optimizer == "sgd":                      # with l2 penalties in the loss: tests/test_gpu_fit.py's bar
        assert_close(h_hip["loss"], h_ref["loss"], rtol=2e-5, atol=1e-7, what=what + ": loss with l2 penalties")
    _check_updates(what, optimizer, w, m_hip, m_ref)
    # the derived inference buffers follow the raw-pointer updates
    logits = m_hip.predict_logits(feed, batch_size=64)
    staged = m_hip.stage(feed)
    m_hip._begin()
    with torch.no_grad():
        ref = m_hip.autograd_logits(staged, 0, n)
    for t in range(2):
        assert_close(logits[t].reshape(-1), ref[t].cpu().numpy(), rtol=1e-4, atol=2e-5, what="%s: logit %d after fit" % (what, t))
    assert all(np.abs(v - w[k]).max() > 0 for k, v in m_hip.get_weights_by_name().items())
    # train_on_batch and a second fit continue on the same trainer
    tr = m_hip._hip_trainer
    steps = tr.t
    assert np.isfinite(m_hip.train_on_batch(feed, ys)) and m_hip._hip_trainer is tr and tr.t == steps + 1


def test_fit_reports_the_compiled_metrics_from_the_steps_outputs(device):
    from tests.test_gpu_mtl import _fuzz_feed
    cols, n = _step_cols(), 150
    for kind in ("ESMM", "MMOE"):
        probe, w = _build(kind, device, 3, cols, **MODELS[kind])
        rng = np.random.RandomState(4)
        feed, ys = _fuzz_feed(rng, cols, n), _labels(rng, probe.task_types, n)
        hists = []
        for hip in (True, False):
            model, _ = _build(kind, device, 3, cols, **MODELS[kind])
            model.hip_training = hip
            model.compile("sgd", metrics=["binary_crossentropy", "mse"])
            hists.append(model.fit(feed, ys, batch_size=64, epochs=2, verbose=0, shuffle=False, validation_split=0.2).history)
            assert (getattr(model, "_hip_trainer", None) is not None) == hip
        assert list(hists[0]) == list(hists[1]) and "val_ctcvr_mse" in hists[0] and "ctcvr_binary_crossentropy" in hists[0]
        for k in hists[1]:
            assert_close(hists[0][k], hists[1][k], rtol=1e-3, atol=1e-6, what="%s: %s" % (kind, k))


def test_a_declined_model_fits_on_the_autograd_step(device):
    from deepctr_amd import training_hip
    from tests.test_gpu_mtl import _fuzz_feed
    cols, n = _step_cols(), 150
    model, _ = _build("MMOE", device, 5, cols, dnn_use_bn=True, **MODELS["MMOE"])
    assert not training_hip.supported(model)
    rng = np.random.RandomState(6)
    feed, ys = _fuzz_feed(rng, cols, n), _labels(rng, model.task_types, n)
    model.compile("adam")
    h = model.fit(feed, ys, batch_size=64, epochs=1, verbose=0).history
    assert getattr(model, "_hip_trainer", None) is None and np.isfinite(h["loss"]).all()


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_fuzz_fit_on_both_steps(device, seed):
    """tests/test_gpu_fuzz.py::_check_fit over the four constructors: the skip rules (saturating or diverging random weights) and the bars
    are its; tests/test_mtl_train_cpu.py counts the seeds that skip."""
    kind, kw, cols, w, feed, ys, n, bs, opt, lw = fuzz_setup(seed, device)
    from deepctr_amd import models
    probe = getattr(models, kind)(cols, device=device, **kw)
    probe.set_weights_by_name(w)
    lg = np.stack(probe.predict_logits(feed, batch_size=4096))
    if not (np.isfinite(lg).all() and np.abs(lg).max() < 30.0):
        pytest.skip("fit fuzz %d %s: the random weights saturate the output (|logit| up to %.3g)" % (seed, kind, float(np.abs(lg).max())))
    (m_hip, h_hip), (m_ref, h_ref) = _fit_both(kind, kw, cols, w, feed, ys, bs, opt, device, loss_weights=lw)
    what = "fit fuzz %d %s %s %s bs=%d" % (seed, kind, kw, opt, bs)
    if not (np.isfinite(h_ref["loss"][-1]) and h_ref["loss"][-1] < 50.0):
        pytest.skip("%s: the random weights diverge under this optimizer (loss %.3g)" % (what, h_ref["loss"][-1]))
    for k in h_ref:
        assert_close(h_hip[k], h_ref[k], rtol=1e-3, atol=1e-6, what="%s: %s" % (what, k))
    _check_updates(what, opt, w, m_hip, m_ref)
