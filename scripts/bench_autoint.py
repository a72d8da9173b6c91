"""AutoInt at the reference defaults on Criteo-shaped input (26 sparse fields of vocabulary 1e5, embedding_dim 16, 13 dense; 3
InteractingLayers of d 8, H 2; DNN 256-128-64): samples/s of the whole forward (staged ids -> probabilities: gather, interacting
kernel, DNN kernel) beside the same model's torch-ops forward (training.model_logits under no_grad), device-event timing after
warm-up, and the interacting kernel alone.  ``--train`` adds one step of fit()'s autograd path with the attention stack in torch ops
and on HIP (training.HIP_AUTOGRAD_OPS off / on, alternating in the same process) and dctr_interacting_bwd alone
(profiles/autoint_interacting_bwd.txt).  Prints one JSON line.

    python scripts/bench_autoint.py [--rows 4096,65536] [--iters 20] [--train]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

F32_MFMA_PEAK_TF = 157.3


def _time(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def _median_spread(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2], xs[-1] - xs[0]


def train_leg(model, staged, n, iters, rounds=5):
    """One step of fit()'s autograd path (model_logits(training=True), BCE, backward over every trainable weight; no optimizer) with
    training.HIP_AUTOGRAD_OPS off and on, the two alternating in ``rounds`` windows of ``iters`` steps each; and dctr_interacting_bwd
    alone beside its FLOP count (the forward again + twice the forward for the gradients)."""
    from deepctr_amd import ops, training
    from deepctr_amd.models.autoint import interacting_flops
    device = model.device
    y = (torch.rand(n, device=device) > 0.5).float()
    frozen = training.frozen_weights(model)
    params = [t for name, t in model.named_weights() if "moving_" not in name and t.data_ptr() not in frozen]

    def step():
        model._begin()
        logit = training.model_logits(model, staged, 0, n, training=True)
        loss = torch.nn.functional.binary_cross_entropy_with_logits(logit, y)
        for t in params:
            t.grad = None
        loss.backward()
        return loss

    ms = {False: [], True: []}
    losses = {}
    try:
        for t in params:
            t.requires_grad_(True)
        for _ in range(rounds):
            for switch in (False, True):
                training.HIP_AUTOGRAD_OPS = switch
                ms[switch].append(_time(step, iters))
                losses[switch] = float(step().detach())
    finally:
        training.HIP_AUTOGRAD_OPS = True
        for t in params:
            t.requires_grad_(False)
            t.grad = None
    off, off_spread = _median_spread(ms[False])
    on, on_spread = _median_spread(ms[True])
    ws = model.stage_plan.run(staged, 0, n)
    weights = model._att_weights()
    dy = torch.randn(n, model.att_out_dim, device=device)
    dx = torch.empty(n, 26 * 16, device=device)
    gd = [[None if w is None else torch.zeros_like(w) for w in layer] for layer in weights]

    def bwd():
        ops.interacting_bwd(ws["dnn_in"], weights, 8, 2, True, False, dy, fields=26, dim=16, dx=dx, d_weights=gd)
    ms_bwd = _time(bwd, iters)
    flops = 3 * interacting_flops(26, 16, 8, 2, 3, True)
    tf = flops * n / (ms_bwd * 1e-3) / 1e12
    return {"step_ms_switch_off": round(off, 4), "step_ms_switch_off_spread": round(off_spread, 4), "step_ms_switch_on": round(on, 4),
            "step_ms_switch_on_spread": round(on_spread, 4), "step_speedup": round(off / on, 3), "windows": rounds, "steps_per_window": iters,
            "loss_switch_off": losses[False], "loss_switch_on": losses[True], "interacting_bwd_call_ms": round(ms_bwd, 4),
            "interacting_bwd_flop_per_sample": flops, "interacting_bwd_tflops": round(tf, 2),
            "interacting_bwd_share_of_f32_mfma_peak": round(tf / F32_MFMA_PEAK_TF, 3)}


def main():
    from deepctr_amd import engine, ops, training
    from deepctr_amd.feature_column import DenseFeat, SparseFeat
    from deepctr_amd.models import AutoInt
    from deepctr_amd.models.autoint import interacting_flops
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="4096,65536")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--train", action="store_true", help="add the training-step leg (autograd step, attention stack off / on HIP)")
    args = ap.parse_args()
    device = torch.device("cuda:0")
    rng = np.random.RandomState(0)
    V = 100000
    cols = [SparseFeat("C%d" % i, V, 16) for i in range(26)] + [DenseFeat("I%d" % i, 1) for i in range(13)]
    model = AutoInt(cols, cols, device=device)
    model.set_weights_by_name({k: (rng.standard_normal(v.shape) * (0.05 if k.endswith("embeddings") else 0.1)).astype(np.float32)
                               for k, v in model.get_weights_by_name().items()})
    flops = interacting_flops(26, 16, 8, 2, 3, True)
    res = {"model": "AutoInt", "fields": 26, "embedding_dim": 16, "att_layers": 3, "d": 8, "heads": 2,
           "interacting_flop_per_sample": flops, "rows": {}}
    for n in [int(r) for r in args.rows.split(",")]:
        feed = {"C%d" % i: rng.randint(0, V, n).astype(np.int32) for i in range(26)}
        feed.update({"I%d" % i: rng.rand(n).astype(np.float32) for i in range(13)})
        staged = engine.Staged(n)
        model._stage_inputs(feed, staged)
        out = torch.empty(n, dtype=torch.float32, device=device)

        def hip():
            model._begin()
            model._forward(staged, 0, n, out)

        def torch_ops():
            with torch.no_grad():
                training.model_logits(model, staged, 0, n)
        ms_hip = _time(hip, args.iters)
        ms_torch = _time(torch_ops, max(3, args.iters // 4))
        ws = model.stage_plan.run(staged, 0, n)
        logit = torch.empty(n, dtype=torch.float32, device=device)
        kern = model.dense.w("kernel")[:model.att_out_dim]

        def att():
            ops.interacting(ws["dnn_in"], model._att_weights(), 8, 2, True, False, fields=26, dim=16, head_w=kern, logit=logit)
        ms_att = _time(att, args.iters)
        tf = flops * n / (ms_att * 1e-3) / 1e12
        res["rows"][str(n)] = {"forward_ms": round(ms_hip, 4), "samples_per_s": round(n / (ms_hip * 1e-3)),
                               "torch_ops_ms": round(ms_torch, 4), "torch_ops_samples_per_s": round(n / (ms_torch * 1e-3)),
                               "speedup_vs_torch_ops": round(ms_torch / ms_hip, 2), "interacting_call_ms": round(ms_att, 4),
                               "interacting_tflops": round(tf, 2), "interacting_share_of_f32_mfma_peak": round(tf / F32_MFMA_PEAK_TF, 3)}
        if args.train:
            res["rows"][str(n)]["train"] = train_leg(model, staged, n, args.iters)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
