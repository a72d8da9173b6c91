"""What scripts/bench_bst.py and scripts/bench_dsin.py share for --train-rows: dctr_transformer_train_fwd and dctr_transformer_bwd alone on
a tensor of the model's own shape beside the backward's f32-MFMA bound (arithmetic: ops.transformer_bwd_flops at 157.3 TFLOP/s), and the
autograd step (model_logits in training mode, the loss, torch.autograd.grad over every trainable weight) under several settings of
the training switches, alternating window by window; medians of device-event timings after warm-up of every shape."""
import numpy as np
import torch

MFMA_F32_TFLOPS = 157.3


def _window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def time_alternating(fns, iters, windows):
    """Medians (ms per call) of ``windows`` windows of each function, alternating a, b, c, a, b, c ..."""
    for _ in range(3):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(windows):
        for t, fn in zip(ts, fns):
            t.append(_window(fn, iters))
    return [float(np.median(t)) for t in ts]


def kernels(r, layers, head_num, x, masks, output_type, iters, windows):
    """``layers``: Transformer layers of one stack; x [B, T, E]; ``masks``: the mask keywords of ops.transformer_train."""
    from deepctr_amd import ops
    B, T, E = x.shape
    L = len(layers)
    flags = layers[0].flags()
    ws = [l.operands() for l in layers]
    kw = dict(output_type=output_type, **masks, **flags)
    out, tape = ops.transformer_train(x, ws, head_num, **kw)
    d_out, dx = torch.randn_like(out), torch.empty_like(x)
    live = flags["use_feed_forward"] and flags["use_res"]
    gw = [torch.zeros_like(w[n]) if n in w and (live or n not in ("fw1", "fw2")) else None for w in ws for n in ops.TRANSFORMER_WEIGHTS]
    ms_f, ms_b = time_alternating([lambda: ops.transformer_train(x, ws, head_num, out=out, tape=tape, **kw),
                                   lambda: ops.transformer_bwd(x, ws, head_num, tape, d_out, dx=dx, d_weights=gw, **kw)], iters, windows)
    flops = float(B) * ops.transformer_bwd_flops(T, E, L, flags["use_feed_forward"])
    bound = flops / (MFMA_F32_TFLOPS * 1e12) * 1e3
    opts = {k: v for k, v in flags.items() if k != "ln_eps"}
    r.update(transformer_train_fwd_ms=round(ms_f, 4), transformer_bwd_ms=round(ms_b, 4), transformer_bwd_bound_ms=round(bound, 5),
             transformer_bwd_share_of_bound=round(bound / ms_b, 4), transformer_bwd_flops_per_sample=ops.transformer_bwd_flops(T, E, L),
             transformer_bwd_workspace_bytes=ops.transformer_bwd_workspace_bytes(B, T, E, head_num, L, output_type=output_type, **opts))


def steps(r, model, staged, n, train_rows, settings, iters, windows):
    """r["autograd_step_ms"][rows] = {name: ms} for every (name, {attribute of deepctr_amd.training: value}) of ``settings``."""
    from deepctr_amd import training
    frozen = training.frozen_weights(model)
    params = [t for k, t in model.named_weights() if "moving_" not in k and t.data_ptr() not in frozen]
    y = torch.randint(0, 2, (n,), device=params[0].device).float()
    names = sorted({k for _, s in settings for k in s})
    saved = {k: getattr(training, k) for k in names}
    table = r["autograd_step_ms"] = {}
    try:
        for t in params:
            t.requires_grad_(True)
        for rows in train_rows:
            rows = min(rows, n)

            def step():
                model._begin()
                logit = training.model_logits(model, staged, 0, rows, training=True)
                loss = torch.nn.functional.binary_cross_entropy_with_logits(logit, y[:rows])
                torch.autograd.grad(loss, params, allow_unused=True)

            def under(setting):
                def run():
                    for k in names:
                        setattr(training, k, setting.get(k, saved[k]))
                    step()
                return run
            ms = time_alternating([under(s) for _, s in settings], max(2, iters // 5), windows)
            table[str(rows)] = {name + "_ms": round(v, 3) for (name, _), v in zip(settings, ms)}
    finally:
        for k, v in saved.items():
            setattr(training, k, v)
        for t in params:
            t.requires_grad_(False)
