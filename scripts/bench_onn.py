"""ONN at the reference defaults on Criteo-shaped input (26 sparse fields of vocabulary 1e5, 13 dense; DNN 256-128-64 over 325*d + 13
columns) at embedding_dim 4 (the reference's SparseFeat default) and 16: samples/s of the whole forward (staged ids -> probabilities:
linear part, dctr_ffm_fwd, DNN kernel) beside the same model's torch-ops forward (training.model_logits under no_grad), device-event
timing after warm-up, then dctr_ffm_fwd alone on each route and the DNN call alone, each beside its bound.  Prints one JSON line.

    python scripts/bench_onn.py [--dims 4,16] [--rows 4096,65536] [--iters 20]"""
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
GATHER_TBPS = 5.5            # whole-row gathers from tables beyond the Infinity Cache (the cost model of DESIGN.md §4.11)
STORE_TBPS = 6.0             # plain stores


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
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="4,16")
    ap.add_argument("--rows", default="4096,65536")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch-ops forward")
    args = ap.parse_args()
    device = torch.device("cuda:0")
    V, F, D = 100000, 26, 13
    P = F * (F - 1) // 2
    units = [256, 128, 64]
    res = {"fields": F, "dense": D, "pairs": P, "vocabulary": V, "dims": {}}
    for d in [int(v) for v in args.dims.split(",")]:
        rng = np.random.RandomState(0)
        cols = [SparseFeat("C%d" % i, V, d) for i in range(F)] + [DenseFeat("I%d" % i, 1) for i in range(D)]
        model = models.ONN(cols, cols, device=device)
        g = torch.Generator(device=device).manual_seed(0)
        for m in model.masters:
            m.copy_(torch.randn(m.shape, generator=g, device=device) * 0.3)
        for k, t in model.named_weights():
            if not k.startswith("sparse_emb_") and "moving_variance" not in k:
                t.copy_(torch.randn(t.shape, generator=g, device=device) * 0.1)
        width = model.dnn_in_dim
        read_b, write_b = F * (F - 1) * d * 4, width * 4
        dnn_flops = 2 * (width * units[0] + units[0] * units[1] + units[1] * units[2] + units[2])
        out_d = res["dims"][str(d)] = {"table_bytes": F * (F - 1) * d * 4 * V, "read_bytes_per_sample": read_b,
                                       "written_bytes_per_sample": write_b, "dnn_in_dim": width, "dnn_flop_per_sample": dnn_flops,
                                       "rows": {}}
        for n in [int(r) for r in args.rows.split(",")]:
            feed = {"C%d" % i: rng.randint(0, V, n).astype(np.int32) for i in range(F)}
            feed.update({"I%d" % i: rng.rand(n).astype(np.float32) for i in range(D)})
            staged = engine.Staged(n)
            model._stage_inputs(feed, staged)
            out = torch.empty(n, dtype=torch.float32, device=device)
            r = out_d["rows"][str(n)] = {"ffm_route": ops.ffm_route(n, F, d)}

            def hip():
                model._begin()
                model._forward(staged, 0, n, out)
            ms_hip = _time(hip, args.iters)
            r.update(forward_ms=round(ms_hip, 4), samples_per_s=round(n / (ms_hip * 1e-3)))
            if not args.no_torch:
                def torch_ops():
                    with torch.no_grad():
                        training.model_logits(model, staged, 0, n)
                ms_torch = _time(torch_ops, max(2, args.iters // 5))
                r.update(torch_ops_ms=round(ms_torch, 4), torch_ops_samples_per_s=round(n / (ms_torch * 1e-3)),
                         speedup_vs_torch_ops=round(ms_torch / ms_hip, 2))
            bufs = model._buffers(n)
            desc = model._descriptors(staged, 0, n, bufs)
            bound_ms = (read_b * n / (GATHER_TBPS * 1e12) + write_b * n / (STORE_TBPS * 1e12)) * 1e3
            r["ffm_bound_ms"] = round(bound_ms, 4)
            for route in ("auto", "direct"):
                def ffm():
                    ops.ffm(None, model.masters, dim=d, scale=model._scale, shift=model._shift, dense=staged.dense, n_dense=D,
                            out=bufs["dnn_in"], desc=desc, batch=n, route=route)
                ms = _time(ffm, args.iters)
                key = "ffm_lds" if route == "auto" else "ffm_direct"
                r[key + "_ms"] = round(ms, 4)
                r[key + "_share_of_bound"] = round(bound_ms / ms, 3)
                r[key + "_tbps"] = round((read_b + write_b) * n / (ms * 1e-3) / 1e12, 3)
            logit = torch.zeros(n, dtype=torch.float32, device=device)

            def dnn():
                ops.mlp(bufs["dnn_in"], model.dnn.kernels, model.dnn.biases, "relu", head_w=model.dense.w("kernel"), add=[logit],
                        global_bias=model.prediction.w("global_bias"), sigmoid_out=True, in_dim=width, out=out)
            ms_dnn = _time(dnn, args.iters)
            dnn_tf = dnn_flops * n / (ms_dnn * 1e-3) / 1e12
            r.update(dnn_call_ms=round(ms_dnn, 4), dnn_tflops=round(dnn_tf, 2), dnn_share_of_f32_mfma_peak=round(dnn_tf / F32_MFMA_PEAK_TF, 3),
                     dnn_bound_ms=round(dnn_flops * n / (155.0 * 1e12) * 1e3, 4))
        del model
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
