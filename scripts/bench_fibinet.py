"""FiBiNET at the reference defaults on Criteo-shaped input (26 sparse fields of vocabulary 1e5, embedding_dim 16, 13 dense;
bilinear_type 'interaction', reduction_ratio 3, DNN 256-128-64 over 2*325*16 + 13 = 10,413 columns): samples/s of the whole forward
(staged ids -> probabilities: gather, bilinear kernel, DNN kernel) beside the same model's torch-ops forward (training.model_logits
under no_grad), device-event timing after warm-up, then the bilinear kernel and the DNN kernel alone.  ``--train`` adds one step of
fit()'s autograd path with the DNN input in torch ops and on HIP (training.HIP_AUTOGRAD_OPS off / on, alternating in the same process)
and dctr_bilinear_bwd alone beside its bound (profiles/fibinet_bilinear_bwd.txt).  Prints one JSON line.

    python scripts/bench_fibinet.py [--rows 4096,65536] [--iters 20] [--train]"""
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
STORE_TBPS = 6.0             # plain-store HBM rate the cost model uses
F32_MFMA_TF = 155.0          # measured f32-MFMA rate the cost model uses
READ_TBPS = 5.5              # gather / read rate the cost model uses


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


def bilinear_bwd_flops(F, E):
    """MFMA FLOP per sample of dctr_bilinear_bwd, 'interaction': per pair and layer x_i W, (g (.) x_j) W^T and the outer product
    x_i^T (g (.) x_j) over the tile's samples, 2 E^2 each."""
    return F * (F - 1) // 2 * 2 * 3 * 2 * E * E


def train_leg(model, staged, n, iters, F, E, D, rounds=5):
    """One step of fit()'s autograd path (model_logits(training=True), BCE, backward over every trainable weight; no optimizer) with
    training.HIP_AUTOGRAD_OPS off (the torch ops: the baseline) and on, the two alternating in ``rounds`` windows of ``iters`` steps
    each; and dctr_bilinear_bwd alone (dx and the four weight gradients) beside its bound: the larger of the HBM time of its d_out
    read and the f32-MFMA time of its FLOP."""
    from deepctr_amd import ops, training
    device = model.device
    P = F * (F - 1) // 2
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
    min_rows = training.FIBINET_HIP_MIN_ROWS
    try:
        training.FIBINET_HIP_MIN_ROWS = 0       # the HIP route is timed at every row count: a threshold is read off this table
        for t in params:
            t.requires_grad_(True)
        for _ in range(rounds):
            for switch in (False, True):
                training.HIP_AUTOGRAD_OPS = switch
                ms[switch].append(_time(step, iters))
                losses[switch] = float(step().detach())
    finally:
        training.HIP_AUTOGRAD_OPS = True
        training.FIBINET_HIP_MIN_ROWS = min_rows
        for t in params:
            t.requires_grad_(False)
            t.grad = None
    off, off_spread = _median_spread(ms[False])
    on, on_spread = _median_spread(ms[True])
    ws = model.stage_plan.run(staged, 0, n)
    width = 2 * P * E + D
    d_out = torch.randn(n, width, device=device)
    dx = torch.empty(n, F * E + D, device=device)
    r = model.senet.weights_w12[0].shape[1]
    g12 = (torch.zeros(F, r, device=device), torch.zeros(r, F, device=device))
    gs, gr = torch.zeros(P, E, E, device=device), torch.zeros(P, E, E, device=device)

    def bwd():
        ops.senet_bilinear_bwd(ws["dnn_in"], d_out, senet_w=model.senet.weights_w12, senet_bilinear_w=model.senet_bilinear.matrices,
                               bilinear_w=model.bilinear.matrices, bilinear_type="interaction", fields=F, dim=E, dense_cols=D, dx=dx,
                               d_senet_w=g12, d_senet_bilinear_w=gs, d_bilinear_w=gr)
    ms_bwd = _time(bwd, iters)
    read_ms = 4 * width * n / (READ_TBPS * 1e12) * 1e3
    mfma_ms = bilinear_bwd_flops(F, E) * n / (F32_MFMA_TF * 1e12) * 1e3
    bound_ms = max(read_ms, mfma_ms)
    return {"step_ms_switch_off": round(off, 4), "step_ms_switch_off_spread": round(off_spread, 4), "step_ms_switch_on": round(on, 4),
            "step_ms_switch_on_spread": round(on_spread, 4), "step_speedup": round(off / on, 3), "windows": rounds, "steps_per_window": iters,
            "loss_switch_off": losses[False], "loss_switch_on": losses[True], "bilinear_bwd_call_ms": round(ms_bwd, 4),
            "bilinear_bwd_d_out_read_ms": round(read_ms, 4), "bilinear_bwd_mfma_ms": round(mfma_ms, 4),
            "bilinear_bwd_flop_per_sample": bilinear_bwd_flops(F, E), "bilinear_bwd_bound_ms": round(bound_ms, 4),
            "bilinear_bwd_share_of_bound": round(bound_ms / ms_bwd, 3)}


def main():
    from deepctr_amd import engine, ops, training
    from deepctr_amd.feature_column import DenseFeat, SparseFeat
    from deepctr_amd.models import FiBiNET
    from deepctr_amd.models.fibinet import bilinear_flops
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="4096,65536")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--train", action="store_true", help="add the training-step leg (autograd step, DNN input off / on HIP)")
    args = ap.parse_args()
    device = torch.device("cuda:0")
    rng = np.random.RandomState(0)
    V, F, E, D = 100000, 26, 16, 13
    cols = [SparseFeat("C%d" % i, V, E) for i in range(F)] + [DenseFeat("I%d" % i, 1) for i in range(D)]
    model = FiBiNET(cols, cols, device=device)
    model.set_weights_by_name({k: (rng.standard_normal(v.shape) * (0.05 if k.endswith("embeddings") else 0.1)).astype(np.float32)
                               for k, v in model.get_weights_by_name().items()})
    width = model.dnn_in_dim
    units = [256, 128, 64]
    dnn_flops = 2 * (width * units[0] + units[0] * units[1] + units[1] * units[2] + units[2])
    bl_bytes = 4 * (F * E + D + width)          # reads the embeddings and the dense values, writes the DNN input
    res = {"model": "FiBiNET", "fields": F, "embedding_dim": E, "dense": D, "bilinear_type": "interaction", "dnn_in_dim": width,
           "bilinear_flop_per_sample": bilinear_flops(F, E, "interaction"), "bilinear_hbm_bytes_per_sample": bl_bytes,
           "dnn_flop_per_sample": dnn_flops, "rows": {}}
    for n in [int(r) for r in args.rows.split(",")]:
        feed = {"C%d" % i: rng.randint(0, V, n).astype(np.int32) for i in range(F)}
        feed.update({"I%d" % i: rng.rand(n).astype(np.float32) for i in range(D)})
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
        buf = model._dnn_input(n)

        def bil():
            ops.senet_bilinear(ws["dnn_in"], senet_w=model.senet.weights_w12, senet_bilinear_w=model.senet_bilinear.matrices,
                               bilinear_w=model.bilinear.matrices, bilinear_type="interaction", fields=F, dim=E, dense_cols=D, out=buf)

        def dnn():
            ops.mlp(buf, model.dnn.kernels, model.dnn.biases, "relu", head_w=model.dense.w("kernel"),
                    global_bias=model.prediction.w("global_bias"), sigmoid_out=True, in_dim=width, out=out)
        ms_bil = _time(bil, args.iters)
        ms_dnn = _time(dnn, args.iters)
        bound_ms = bl_bytes * n / (STORE_TBPS * 1e12) * 1e3
        dnn_tf = dnn_flops * n / (ms_dnn * 1e-3) / 1e12
        res["rows"][str(n)] = {"forward_ms": round(ms_hip, 4), "samples_per_s": round(n / (ms_hip * 1e-3)),
                               "torch_ops_ms": round(ms_torch, 4), "torch_ops_samples_per_s": round(n / (ms_torch * 1e-3)),
                               "speedup_vs_torch_ops": round(ms_torch / ms_hip, 2), "bilinear_call_ms": round(ms_bil, 4),
                               "bilinear_hbm_bound_ms": round(bound_ms, 4), "bilinear_share_of_hbm_bound": round(bound_ms / ms_bil, 3),
                               "dnn_call_ms": round(ms_dnn, 4), "dnn_tflops": round(dnn_tf, 2),
                               "dnn_share_of_f32_mfma_peak": round(dnn_tf / F32_MFMA_PEAK_TF, 3)}
        if args.train:
            res["rows"][str(n)]["train"] = train_leg(model, staged, n, args.iters, F, E, D)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
