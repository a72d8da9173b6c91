"""fit() of the multi-output models: the loop of training.fit_model over T labelled outputs.
loss = sum_t w_t * mean_b(loss_t) + l2 penalties; a binary task that has a logit takes its gradient from the logit form and reports the
value from probabilities clipped to [1e-7, 1 - 1e-7], as training._fit_torch does; ESMM's ctcvr output has no logit and takes the
clipped-probability form for both.  Two steps compute it (DESIGN.md §4.15 "Training"): the HIP step (``fit_hip``: training_hip.HipTrainer
with MultiTaskModel._hip_forward_backward, no autograd and no torch optimizer) where the model, the losses and the optimizer allow it, under
the rule of training.fit_model, and the torch-autograd step (``fit_torch``) for everything else."""
import numpy as np
import torch

from ... import training as tops

_UNSUPPORTED = ("sample_weight", "class_weight", "callbacks", "steps_per_epoch", "validation_steps", "validation_batch_size",
                "validation_freq", "initial_epoch", "_dp", "distributed", "group")
_IGNORED = ("workers", "use_multiprocessing", "max_queue_size")
_BCE = ("binary_crossentropy", "logloss", "bce")


def task_losses(model, logits, ys):
    """Per task (differentiable mean loss, reported mean loss) from autograd_logits' values and the labels ys [T, B]."""
    outs, has_logit = model.autograd_outputs(logits)
    pairs = []
    for t, name in enumerate(model._compiled["loss"]):
        y = ys[t]
        if name in _BCE:
            pc = outs[t].clamp(1e-7, 1.0 - 1e-7)
            clipped = -(y * torch.log(pc) + (1.0 - y) * torch.log(1.0 - pc))
            if has_logit[t] and model.task_types[t] == "binary":
                loss = torch.nn.functional.binary_cross_entropy_with_logits(logits[t], y, reduction="none")
            else:
                loss = clipped
            shown = clipped.detach()
        else:
            loss = torch.nn.functional.mse_loss(outs[t], y, reduction="none")
            shown = loss.detach()
        pairs.append((loss.mean(), shown.mean()))
    return pairs


class EpochEnd(object):
    """After every epoch: the History record with tf.keras' keys (loss, <task>_loss, <task>_<metric>, and their val_ forms from
    evaluate() on the validation rows), the verbose line."""

    def __init__(self, model, val, bs, epochs, verbose):
        self.model, self.val, self.bs, self.epochs, self.verbose = model, val, bs, epochs, verbose
        self.hist = tops.History()
        self.hist.model = model
        model.stop_training = False

    def __call__(self, ep, logs):
        h = self.hist
        h.epoch.append(ep)
        if self.val is not None:
            for k, v in self.model.evaluate(self.val[0], self.val[1], batch_size=self.bs, return_dict=True).items():
                logs["val_" + k] = v
        for k, v in logs.items():
            h.history.setdefault(k, []).append(v)
        if self.verbose:
            print("Epoch %d/%d - %s" % (ep + 1, self.epochs, " - ".join("%s: %.4f" % kv for kv in logs.items())))
        return bool(getattr(self.model, "stop_training", False))

    def finish(self):
        return self.hist


def fit_torch(model, staged, yt, n_tr, bs, epochs, shuffle, epoch_end):
    """The epochs over staged rows and labels yt [T, n_tr] (device-agnostic torch code: the CPU suite drives it on CPU-built models)."""
    c = model._compiled
    frozen = tops.frozen_weights(model)
    params = [t for name, t in model.named_weights() if "moving_" not in name and t.data_ptr() not in frozen]
    for t in params:
        t.requires_grad_(True)
    opt = tops.torch_optimizer(model, params)
    regs = [(t, l2) for t, l2 in tops.regularized_weights(model) if t.data_ptr() not in frozen]
    yrows = yt.t().contiguous()         # [n_tr, T]: permute_staged_ permutes dimension 0

    def permute():
        tops.permute_staged_(staged, yrows, torch.from_numpy(np.random.permutation(n_tr)).to(yrows.device))
    cursor = tops._BatchCursor(n_tr, bs, None, permute if shuffle else None)
    names = model.task_names
    metrics = list(c["metrics"])
    try:
        for ep in range(epochs):
            tot = np.zeros(1 + model.num_tasks)
            cnt = 0
            preds = [[] for _ in names]
            labels = [[] for _ in names]
            for lo, hi in cursor.epoch():
                model._begin()
                logits = model.autograd_logits(staged, int(lo), int(hi), training=True)
                ys = yrows[lo:hi].t()
                pairs = task_losses(model, logits, ys)
                loss = sum(w * l for w, (l, _) in zip(c["loss_weights"], pairs))
                shown = sum(w * s for w, (_, s) in zip(c["loss_weights"], pairs))
                for t, l2 in regs:                                  # keras adds the regularisation losses to the loss
                    pen = l2 * (t * t).sum()
                    loss = loss + pen
                    shown = shown + pen.detach()
                opt.zero_grad(set_to_none=True)
                loss.backward()
                opt.step()
                tot += np.array([float(shown.item())] + [float(s.item()) for _, s in pairs]) * (hi - lo)
                cnt += hi - lo
                if metrics:
                    with torch.no_grad():
                        outs, _ = model.autograd_outputs([l.detach() for l in logits])
                    for t in range(model.num_tasks):
                        preds[t].append(outs[t].cpu().numpy().astype(np.float64))
                        labels[t].append(ys[t].cpu().numpy().astype(np.float64))
            for t in params:
                t.requires_grad_(False)
            mean = tot / max(cnt, 1)
            logs = dict([("loss", float(mean[0]))] + [("%s_loss" % n, float(v)) for n, v in zip(names, mean[1:])])
            for t, n in enumerate(names):
                for m in metrics:
                    logs["%s_%s" % (n, model._metric_name(m))] = model._metric(m, np.concatenate(preds[t]), np.concatenate(labels[t]))
            stop = epoch_end(ep, logs)
            for t in params:
                t.requires_grad_(True)
            if stop:
                break
    finally:
        for t in params:
            t.requires_grad_(False)
    return epoch_end.finish()


def fit_hip(model, staged, yt, n_tr, bs, epochs, shuffle, epoch_end):
    """The epochs on the HIP training step.  The trainer (optimizer moments, step count) lives on the model as ``_hip_trainer``, so
    train_on_batch and a second fit() continue the same optimisation.  Per epoch ONE device matrix [steps, T] takes every step's summed
    task losses (dctr_mtl_loss_grad adds into its row), the l2 penalties ride the optimizer launch (HipTrainer.penalty_acc, as
    training._fit_hip), and the steps' outputs are gathered on the device for the compiled metrics: one copy to the host per epoch."""
    from ...training_hip import trainer_for
    c = model._compiled
    tr = trainer_for(model)
    T, names, metrics, w = model.num_tasks, model.task_names, list(c["metrics"]), np.asarray(c["loss_weights"], dtype=np.float64)
    yrows = yt.t().contiguous()         # [n_tr, T]: permute_staged_ permutes dimension 0

    def permute():
        tops.permute_staged_(staged, yrows, torch.from_numpy(np.random.permutation(n_tr)).to(yrows.device))
    cursor = tops._BatchCursor(n_tr, bs, None, permute if shuffle else None)
    pen_acc = torch.zeros(1, dtype=torch.float64, device=model.device)
    tr.penalty_acc = pen_acc
    try:
        for ep in range(epochs):
            tot = torch.zeros(max(cursor.steps, 1), T, dtype=torch.float32, device=model.device)
            pen_acc.zero_()
            rows = 0
            preds = torch.empty(T, n_tr, dtype=torch.float32, device=model.device) if metrics else None
            seen = torch.empty(T, n_tr, dtype=torch.float32, device=model.device) if metrics else None
            for i, (lo, hi) in enumerate(cursor.epoch()):
                lo, hi = int(lo), int(hi)
                ys = yrows[lo:hi].t().contiguous()
                tr.penalty_rows = hi - lo
                tr.step(staged, lo, hi, ys, loss_acc=tot[i])
                if metrics:
                    preds[:, rows:rows + hi - lo].copy_(tr._buffers(hi - lo)["pred"])
                    seen[:, rows:rows + hi - lo].copy_(ys)
                rows += hi - lo
            model._check_status()
            per = tot.double().sum(0).cpu().numpy() / max(rows, 1)
            total = float((w * per).sum()) + float(pen_acc.item()) / max(rows, 1)
            logs = dict([("loss", total)] + [("%s_loss" % n, float(v)) for n, v in zip(names, per)])
            if metrics:
                if model.esmm:
                    preds[1, :rows].mul_(preds[0, :rows])       # (the step keeps sigmoid(l_cvr): the output is the product)
                p, yy = preds[:, :rows].cpu().numpy().astype(np.float64), seen[:, :rows].cpu().numpy().astype(np.float64)
                for t, n in enumerate(names):
                    for mt in metrics:
                        logs["%s_%s" % (n, model._metric_name(mt))] = model._metric(mt, p[t], yy[t])
            if epoch_end(ep, logs):
                break
    finally:
        tr.penalty_acc, tr.penalty_rows = None, 0
    return epoch_end.finish()


def takes_hip_step(model):
    """The rule of training.fit_model: ``model.hip_training`` (default True), an optimizer given by a name the HIP step has or as an
    ``optimizers`` object, and a model / loss combination it covers (training_hip.supported -> MultiTaskModel._hip_supported)."""
    from ... import training_hip
    return bool(getattr(model, "hip_training", True) and training_hip.takes_optimizer(model) and training_hip.supported(model))


def fit_multitask(model, x, y, batch_size=256, epochs=1, verbose=1, validation_split=0.0, shuffle=True, validation_data=None, **kwargs):
    from ... import _C
    if model._compiled is None:
        raise RuntimeError("You must compile your model before training/testing. Use `model.compile(optimizer, loss)`.")
    for k, v in kwargs.items():
        if k in _IGNORED:
            continue
        if k in _UNSUPPORTED:
            if v is None:
                continue
            raise NotImplementedError("fit(%s=...) is not implemented for multi-task models (it would silently train on a different "
                                      "objective if ignored)" % k)
        raise TypeError("fit() got an unexpected keyword argument %r" % k)
    _C.require_device()
    feed = model._as_feed(x)
    n = model._num_rows(feed)
    ys = model._labels(y, n)
    val = None
    n_val = 0
    if validation_data is not None:
        if len(validation_data) != 2:
            raise NotImplementedError("fit(validation_data=...) takes (x_val, y_val); sample weights are not supported")
        val = (validation_data[0], validation_data[1])
    else:
        n_val = int(n * validation_split)
    n_tr = n - n_val
    if n_val:
        val = ({k: np.asarray(v)[n_tr:] for k, v in feed.items()}, [row[n_tr:] for row in ys])
    staged = model.stage({k: np.asarray(v)[:n_tr] for k, v in feed.items()})
    yt = torch.from_numpy(np.ascontiguousarray(ys[:, :n_tr])).to(model.device)
    bs = int(batch_size) if batch_size else n_tr
    fit = fit_hip if takes_hip_step(model) else fit_torch
    return fit(model, staged, yt, n_tr, bs, epochs, shuffle, EpochEnd(model, val, bs, epochs, verbose))
