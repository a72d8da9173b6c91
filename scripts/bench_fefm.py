"""DeepFEFM and FwFM at the reference defaults on Criteo-shaped input (26 sparse fields of vocabulary 1e5, embedding_dim 16, 13 dense;
DNN 256-128-64; DeepFEFM's DNN reads 26*16 + 13 + 325 = 754 columns): samples/s of the whole forward (staged ids -> probabilities:
gather, field-pair kernel, DNN kernel) beside the same model's torch-ops forward (training.model_logits under no_grad), device-event
timing after warm-up, then the field-pair kernel and the DNN kernel alone.  ``--train`` adds one step of fit()'s autograd path with the
field-pair layer in torch ops and on HIP (training.HIP_AUTOGRAD_OPS off / on, alternating in the same process) and dctr_fieldpair_bwd
alone beside its bound (profiles/fefm_fieldpair_bwd.txt).  Prints one JSON line.

    python scripts/bench_fefm.py [--rows 4096,65536] [--iters 20] [--train]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

F32_MFMA_TF = 155.0          # measured f32-MFMA rate the cost model uses
F32_MFMA_PEAK_TF = 157.3
STORE_TBPS = 6.0             # plain-store HBM rate the cost model uses


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


def fieldpair_bwd_flops(F, E):
    """FLOP per sample of the FEFM backward: per pair two S x products for dx (2 * 2 E^2) and one outer product for dW (2 E^2)."""
    return F * (F - 1) // 2 * 6 * E * E


def train_leg(which, model, staged, n, iters, rounds=5):
    """One step of fit()'s autograd path (model_logits(training=True), BCE, backward over every trainable weight; no optimizer) with
    training.HIP_AUTOGRAD_OPS off (the torch ops: the baseline) and on, the two alternating in ``rounds`` windows of ``iters`` steps
    each; and dctr_fieldpair_bwd alone (dx and the weight gradient) beside the f32-MFMA time of its FLOP (FEFM) or the HBM time of
    its bytes (FwFM: x read, dx written)."""
    from deepctr_amd import ops, training
    device = model.device
    F, E = 26, 16
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
    min_rows = training.FEFM_HIP_MIN_ROWS
    try:
        training.FEFM_HIP_MIN_ROWS = 0          # the HIP route is timed at every row count: the threshold is read off this table
        for t in params:
            t.requires_grad_(True)
        for _ in range(rounds):
            for switch in (False, True):
                training.HIP_AUTOGRAD_OPS = switch
                ms[switch].append(_time(step, iters))
                losses[switch] = float(step().detach())
    finally:
        training.HIP_AUTOGRAD_OPS = True
        training.FEFM_HIP_MIN_ROWS = min_rows
        for t in params:
            t.requires_grad_(False)
            t.grad = None
    off, off_spread = _median_spread(ms[False])
    on, on_spread = _median_spread(ms[True])
    ws = model.stage_plan.run(staged, 0, n)
    dx = torch.empty(n, F * E, device=device)
    dl = torch.randn(n, device=device)
    if which == "DeepFEFM":
        dp = torch.randn(n, P, device=device)
        gd = torch.zeros(P, E, E, device=device)

        def bwd():
            ops.fieldpair_bwd(ws["dnn_in"], model.fefm.matrices, "fefm", d_pairs=dp, d_logit=dl, fields=F, dim=E, dx=dx, d_weights=gd)
        bound_ms = fieldpair_bwd_flops(F, E) * n / (F32_MFMA_TF * 1e12) * 1e3
        bound = "f32_mfma"
    else:
        gd = torch.zeros(F, F, device=device)

        def bwd():
            ops.fieldpair_bwd(ws["dnn_in"], model.fwfm_layers[0].field_strengths, "fwfm", d_logit=dl, fields=F, dim=E, dx=dx, d_weights=gd)
        bound_ms = 4 * (2 * F * E + 1) * n / (STORE_TBPS * 1e12) * 1e3
        bound = "hbm_bytes"
    ms_bwd = _time(bwd, iters)
    return {"step_ms_switch_off": round(off, 4), "step_ms_switch_off_spread": round(off_spread, 4), "step_ms_switch_on": round(on, 4),
            "step_ms_switch_on_spread": round(on_spread, 4), "step_speedup": round(off / on, 3), "windows": rounds, "steps_per_window": iters,
            "loss_switch_off": losses[False], "loss_switch_on": losses[True], "fieldpair_bwd_call_ms": round(ms_bwd, 4),
            "fieldpair_bwd_bound": bound, "fieldpair_bwd_bound_ms": round(bound_ms, 4),
            "fieldpair_bwd_share_of_bound": round(bound_ms / ms_bwd, 3)}


def main():
    from deepctr_amd import engine, models, ops, training
    from deepctr_amd.feature_column import DenseFeat, SparseFeat
    from deepctr_amd.models.deepfefm import fieldpair_flops
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="4096,65536")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--train", action="store_true", help="add the training-step leg (autograd step, field-pair layer off / on HIP)")
    args = ap.parse_args()
    device = torch.device("cuda:0")
    V, F, E, D = 100000, 26, 16, 13
    P = F * (F - 1) // 2
    cols = [SparseFeat("C%d" % i, V, E) for i in range(F)] + [DenseFeat("I%d" % i, 1) for i in range(D)]
    units = [256, 128, 64]
    res = {"fields": F, "embedding_dim": E, "dense": D, "pairs": P, "fefm_flop_per_sample": fieldpair_flops(F, E),
           "fefm_hbm_bytes_per_sample": 4 * (F * E + P), "models": {}}
    for which in ("DeepFEFM", "FwFM"):
        rng = np.random.RandomState(0)
        model = getattr(models, which)(cols, cols, device=device)
        model.set_weights_by_name({k: (rng.standard_normal(v.shape) * (0.05 if k.endswith("embeddings") else 0.1)).astype(np.float32)
                                   for k, v in model.get_weights_by_name().items()})
        sp = model.stage_plan
        width = model.dnn_in_dim if which == "DeepFEFM" else sp.in_dim
        dnn_flops = 2 * (width * units[0] + units[0] * units[1] + units[1] * units[2] + units[2])
        out_m = res["models"][which] = {"dnn_in_dim": width, "dnn_flop_per_sample": dnn_flops, "rows": {}}
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
            ws = sp.run(staged, 0, n)
            logit = torch.empty(n, dtype=torch.float32, device=device)

            if which == "DeepFEFM":
                def pair():
                    ops.fieldpair(ws["dnn_in"], model.fefm.matrices, kind="fefm", fields=F, dim=E, x_offset=0, pairs=ws["dnn_in"],
                                  pairs_offset=sp.in_dim, logit=logit, add=ws["lin"])
                # the larger of the matrix-pipe time and the HBM time (reads F*E floats, writes P floats and the logit per sample)
                bound_ms = max(fieldpair_flops(F, E) * n / (F32_MFMA_TF * 1e12), 4 * (F * E + P + 2) * n / (STORE_TBPS * 1e12)) * 1e3
            else:
                def pair():
                    ops.fieldpair(ws["dnn_in"], model.fwfm_layers[0].field_strengths, kind="fwfm", fields=F, dim=E, x_offset=0,
                                  logit=logit, add=ws["lin"])
                bound_ms = 4 * (F * E + 2) * n / (STORE_TBPS * 1e12) * 1e3

            def dnn():
                ops.mlp(ws["dnn_in"], model.dnn.kernels, model.dnn.biases, "relu", head_w=model.dense.w("kernel"), add=[logit],
                        global_bias=model.prediction.w("global_bias"), sigmoid_out=True, in_dim=width, out=out)
            ms_pair = _time(pair, args.iters)
            ms_dnn = _time(dnn, args.iters)
            dnn_tf = dnn_flops * n / (ms_dnn * 1e-3) / 1e12
            out_m["rows"][str(n)] = {"forward_ms": round(ms_hip, 4), "samples_per_s": round(n / (ms_hip * 1e-3)),
                                     "torch_ops_ms": round(ms_torch, 4), "torch_ops_samples_per_s": round(n / (ms_torch * 1e-3)),
                                     "speedup_vs_torch_ops": round(ms_torch / ms_hip, 2), "fieldpair_call_ms": round(ms_pair, 4),
                                     "fieldpair_bound_ms": round(bound_ms, 4), "fieldpair_share_of_bound": round(bound_ms / ms_pair, 3),
                                     "dnn_call_ms": round(ms_dnn, 4), "dnn_tflops": round(dnn_tf, 2),
                                     "dnn_share_of_f32_mfma_peak": round(dnn_tf / F32_MFMA_PEAK_TF, 3)}
            if args.train:
                out_m["rows"][str(n)]["train"] = train_leg(which, model, staged, n, args.iters)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
