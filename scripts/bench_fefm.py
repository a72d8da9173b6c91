"""DeepFEFM and FwFM at the reference defaults on Criteo-shaped input (26 sparse fields of vocabulary 1e5, embedding_dim 16, 13 dense;
DNN 256-128-64; DeepFEFM's DNN reads 26*16 + 13 + 325 = 754 columns): samples/s of the whole forward (staged ids -> probabilities:
gather, field-pair kernel, DNN kernel) beside the same model's torch-ops forward (training.model_logits under no_grad), device-event
timing after warm-up, then the field-pair kernel and the DNN kernel alone.  Prints one JSON line.

    python scripts/bench_fefm.py [--rows 4096,65536] [--iters 20]"""
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


def main():
    from deepctr_amd import engine, models, ops, training
    from deepctr_amd.feature_column import DenseFeat, SparseFeat
    from deepctr_amd.models.deepfefm import fieldpair_flops
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="4096,65536")
    ap.add_argument("--iters", type=int, default=20)
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
    print(json.dumps(res))


if __name__ == "__main__":
    main()
