"""fit() of the multi-output models on the torch-autograd step: the loop of training._fit_torch over T labelled outputs.
loss = sum_t w_t * mean_b(loss_t) + l2 penalties; a binary task that has a logit takes its gradient from the logit form and reports the
value from probabilities clipped to [1e-7, 1 - 1e-7], as training._fit_torch does; ESMM's ctcvr output has no logit and takes the
clipped-probability form for both.  A HIP training step for these models does not exist yet."""
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
    opt = c["optimizer"]
    if isinstance(opt, str):
        if opt.lower() not in tops._OPTS:
            raise ValueError("optimizer %r not supported (adam, adagrad, sgd, rmsprop or a torch.optim factory)" % opt)
        opt = tops._OPTS[opt.lower()](params)
    elif callable(opt):
        opt = opt(params)
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
    return fit_torch(model, staged, yt, n_tr, bs, epochs, shuffle, EpochEnd(model, val, bs, epochs, verbose))
