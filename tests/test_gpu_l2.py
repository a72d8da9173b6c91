"""GPU: which weight gets which l2 on the HIP training step, for every model kind it trains, against tests/ref_l2.py.

The l2 term never appears in a gradient buffer (the optimizer launch adds 2 l2 w to each segment's gradient and sums l2 sum(w^2) into the
loss fit() reports), so it is isolated exactly: every model trains three steps with a data gradient of exactly zero, and what is left is
closed-form (ref_l2.decayed, ref_l2.epoch_loss).  Method per kind:
  single-task kinds (DeepFM ... FLEN): fit(..., sample_weight=zeros) — dctr_bce_grad_w gives dlogit = w (p - y) / B = 0;
  multi-task kinds (SharedBottom, ESMM, MMOE, PLE): compile(loss_weights=[0, 0]) — dctr_mtl_loss_grad multiplies every task's
  dlogit by its weight, ESMM's product form included; the zero-gradient method, not the differential one.
That the data gradient is exactly zero is itself asserted: every unregularised weight keeps its bits.  No BatchNormalization, dropout or
Dice in these models: their statistics move whatever the gradient is."""
import math
import os
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_l2 as RL  # noqa: E402
import ref_optimizers as RO  # noqa: E402

pytestmark = pytest.mark.gpu

STEPS = len(RL.BATCH_ROWS)
SGD_LR = {"sgd_name": 0.01, "sgd_object": 0.1}            # ("sgd" by name: tf.keras' default rate, dctr_opt_multi; SGD(0.1): dctr_opt_apply)


class _Path(object):
    """What fit() ran: every optimizer launch's (penalty accumulator present, rows it scales the penalties by), and the ``pen_acc``
    training._fit_hip handed to its epochs (None = the two-ends fallback)."""

    def __init__(self, monkeypatch):
        from deepctr_amd import training
        from deepctr_amd.training_hip import HipTrainer
        self.launches, self.pen_acc = [], []
        real_update, real_epochs = HipTrainer.apply_update, training._fit_hip_epochs

        def apply_update(tr):
            self.launches.append((tr.penalty_acc is not None, int(tr.penalty_rows)))
            return real_update(tr)

        def epochs(model, tr, staged, yt, wt, cursor, dp, n_epochs, initial_epoch, epoch_end, pen_acc, penalty, pen0):
            self.pen_acc.append(pen_acc)
            return real_epochs(model, tr, staged, yt, wt, cursor, dp, n_epochs, initial_epoch, epoch_end, pen_acc, penalty, pen0)
        monkeypatch.setattr(HipTrainer, "apply_update", apply_update)
        monkeypatch.setattr(training, "_fit_hip_epochs", epochs)


def _fit(kind, device, optimizer, monkeypatch, frozen=False):
    """Three updates with a zero data gradient from random weights; returns (model, w0, w after, history, _Path)."""
    from deepctr_amd import training_hip
    rng = np.random.RandomState(zlib.crc32(kind.encode()) % 1000)
    model = RL.make_model(kind, device, frozen=frozen)
    w0 = RL.random_weights(model, rng)
    model.set_weights_by_name(w0)
    got0 = model.get_weights_by_name()
    assert all(np.array_equal(got0[k], w0[k]) for k in w0)
    feed = RL.make_feed(kind, rng)
    assert training_hip.supported(model), "%s is meant to train on the HIP step" % kind
    path = _Path(monkeypatch)
    fit_kw = dict(batch_size=RL.BATCH, epochs=1, verbose=0, shuffle=False)
    if kind in RL.MULTI:
        model.compile(optimizer, loss_weights=[0.0] * model.num_tasks)
        ys = [(rng.rand(RL.N_ROWS) > 0.5).astype(np.float32) for _ in range(model.num_tasks)]
        h = model.fit(feed, ys, **fit_kw)
    else:
        model.compile(optimizer, "binary_crossentropy")
        h = model.fit(feed, (rng.rand(RL.N_ROWS) > 0.5).astype(np.float32), sample_weight=np.zeros(RL.N_ROWS, dtype=np.float32), **fit_kw)
    assert getattr(model, "_hip_trainer", None) is not None, "%s: fit() took the autograd step" % kind
    # the exact path: every launch summed the penalties of the weights it was about to update, scaled by its batch's rows
    if kind in RL.SINGLE:
        assert len(path.pen_acc) == 1 and path.pen_acc[0] is not None, "%s: the trainer's segments do not carry the model's regularisers" % kind
    assert path.launches == [(True, r) for r in RL.BATCH_ROWS], (kind, path.launches)
    return model, w0, model.get_weights_by_name(), h.history, path


def _check_sgd(kind, model, w0, w1, l2s, lr, loss):
    moved = 0
    for k in w0:
        l = l2s[k]
        if l == 0.0:
            assert np.array_equal(w1[k], w0[k]), "%s: %s has no regulariser (and the data gradient is zero) but moved" % (kind, k)
            continue
        moved += 1
        want = RL.decayed(w0[k], l, lr, STEPS)
        err, bar = np.abs(w1[k].astype(np.float64) - want), RL.sgd_bar(w0[k], l, lr, STEPS)
        assert np.all(err <= bar), "%s: %s (l2 %g): %.3g x the bar off w0 (1 - 2 lr l)^%d; the step moved it by %.3g of itself, the rule says %.3g" % (
            kind, k, l, float((err / bar).max()), STEPS, float(np.abs(w1[k] / w0[k] - 1).max()), 1 - (1 - 2 * lr * l) ** STEPS)
        # every element decays, whole tables included: the ids are drawn below 8, so all rows from 8 on (of a hashed table: all but
        # eight at most) are rows no batch touched, and a shared table would stand 2 lr l |w| — thousands of bars — off had it decayed twice
        assert not np.any(w1[k] == w0[k]), k
    assert moved >= 3
    if loss is None:
        return
    # history["loss"] = the rows-weighted mean of sum l sum(w_s^2) at each step's weights (the data loss is exactly 0).  Bar, relative:
    # a thread of the optimizer launch adds at most ceil(n_max / 256) squares in float32 (n_max: the launch's largest segment), which
    # with the float32 l2 bounds the float32 part of the sum by (ceil(n_max / 256) + 2) 2^-24 (tests/test_gpu_optimizers.py::_penalty_bar);
    # the weights step s squares are the float32 trajectory, which ref_l2.sgd_bar holds within one spacing (<= 2^-23 relative) per step
    # taken of the closed form: s 2^-23 on w, 4 s 2^-24 on w^2, and s <= t - 1 for every step of the mean.
    # Together (ceil(n_max / 256) + 4 t + 2) 2^-24.
    n_max = model._hip_trainer.max_n
    want = RL.epoch_loss(w0, l2s, lr, RL.BATCH_ROWS)
    rel = (math.ceil(n_max / 256) + 4 * STEPS + 2) * 2.0 ** -24
    print("%s: loss %.9g, closed form %.9g, off by %.3g relative, bar %.3g" % (kind, loss, want, abs(loss - want) / want, rel))
    assert want > 1e-3 and abs(loss - want) <= rel * want, (kind, loss, want, abs(loss - want) / want, rel)


@pytest.mark.parametrize("opt", sorted(SGD_LR))
@pytest.mark.parametrize("kind", RL.KINDS)
def test_sgd_decays_each_weight_by_its_own_regulariser(device, kind, opt, monkeypatch):
    from deepctr_amd import optimizers
    lr = SGD_LR[opt]
    model, w0, w1, hist, _ = _fit(kind, device, "sgd" if opt == "sgd_name" else optimizers.SGD(lr), monkeypatch)
    tr = model._hip_trainer
    assert (tr.opt is None) == (opt == "sgd_name")         # the name launches dctr_opt_multi, the object dctr_opt_apply
    l2s = RL.l2_by_name(kind, list(w0))
    assert len(hist["loss"]) == 1
    _check_sgd(kind, model, w0, w1, l2s, lr, hist["loss"][0])


@pytest.mark.parametrize("kind", RL.KINDS)
def test_adam_by_name_sees_each_weights_regulariser(device, kind, monkeypatch):
    """compile("adam"), the default of every example: three updates against the float64 oracle fed g_raw = 0 and the rule's l2 per
    weight, at test_opt_apply_matches_the_float64_oracle's bar (4 x the float32 torch restatement's error + one float32 spacing)."""
    from deepctr_amd import optimizers, training
    model, w0, w1, _, _ = _fit(kind, device, "adam", monkeypatch)
    names = list(w0)
    l2s = RL.l2_by_name(kind, names)
    want = [w0[k].astype(np.float64) for k in names]
    zeros = [np.zeros_like(w) for w in want]
    oracle = RO.Oracle("adam")
    params = [torch.tensor(w0[k]) for k in names]
    ko = training.KerasOptimizer(params, optimizers.Adam())
    for _ in range(STEPS):
        oracle.update(want, zeros, [l2s[k] for k in names], 1e-3)
        for p, k in zip(params, names):
            p.grad = (2.0 * l2s[k]) * p.detach()
        ko.step()
    e_torch = max(float(np.abs(p.detach().numpy().astype(np.float64) - b).max()) for p, b in zip(params, want))
    worst = 0.0
    for k, b in zip(names, want):
        if l2s[k] == 0.0:
            assert np.array_equal(w1[k], w0[k]) and np.array_equal(b, w0[k].astype(np.float64)), "%s: %s moved" % (kind, k)
            continue
        err = np.abs(w1[k].astype(np.float64) - b)
        bar = 4.0 * e_torch + np.spacing(np.abs(b).astype(np.float32)).astype(np.float64)
        worst = max(worst, float(err.max()))
        assert np.all(np.abs(b - w0[k]) > 1e-3), k        # (three Adam updates of ~lr each, whatever the regulariser's size)
        assert np.all(err <= bar), "%s: %s off by %.3g, torch float32 by %.3g" % (kind, k, float(err.max()), e_torch)
    print("%s adam: largest error %.3g, torch float32 %.3g" % (kind, worst, e_torch))


@pytest.mark.parametrize("kind", sorted(RL.FROZEN))
def test_a_frozen_table_keeps_its_bits_beside_decaying_ones(device, kind, monkeypatch):
    """SparseFeat(trainable=False): its table (and its linear table) stay bit-identical, everything else follows the rule.  (Whether a
    frozen table's penalty belongs in the reported loss is not pinned: no loss check here.)"""
    from deepctr_amd import optimizers
    lr = SGD_LR["sgd_object"]
    model, w0, w1, _, _ = _fit(kind, device, optimizers.SGD(lr), monkeypatch, frozen=True)
    e = RL.FROZEN[kind]
    l2s = RL.l2_by_name(kind, list(w0), frozen=[e])
    frozen = [k for k in w0 if k.endswith("emb_%s/embeddings" % e)]
    assert len(frozen) == (2 if kind == "DeepFM" else 1) and all(np.array_equal(w1[k], w0[k]) for k in frozen)
    _check_sgd(kind, model, w0, w1, l2s, lr, None)
