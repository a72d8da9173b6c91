"""IFM and DIFM at the reference defaults on Criteo-shaped input (26 sparse fields of vocabulary 1e5 + 13 bucketised fields, 39 fields of
embedding_dim 4; DNN 256-128-64; DIFM: 8 heads of 8): samples/s of the whole forward (staged ids -> probabilities: fused gather,
(attention,) DNN kernel, dctr_ifm_fwd) beside the same model's torch-ops forward (training.model_logits under no_grad), device-event
timing after warm-up, then dctr_ifm_fwd alone on each route beside its HBM-byte bound — for DIFM with both factor sources projected in
the launch (the form the model uses), and beside the alternative (dctr_sgemm for the K = 2,496 product, handed over as m').  Prints one JSON line.

    python scripts/bench_ifm.py [--rows 4096,65536] [--iters 20]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_TBPS = 6.0               # achievable streaming rate the bound is quoted at


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
    from deepctr_amd.feature_column import SparseFeat
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="4096,65536")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch-ops forward")
    args = ap.parse_args()
    device = torch.device("cuda:0")
    V, F, d = 100000, 39, 4
    cols = [SparseFeat("C%d" % i, V, d) for i in range(26)] + [SparseFeat("I%d" % i, 64, d) for i in range(13)]
    res = {"fields": F, "dim": d, "vocabulary": V, "models": {}}
    for kind in ("IFM", "DIFM"):
        rng = np.random.RandomState(0)
        model = getattr(models, kind)(cols, cols, device=device)
        g = torch.Generator(device=device).manual_seed(0)
        for k, t in model.named_weights():
            t.copy_(torch.randn(t.shape, generator=g, device=device) * (0.3 if k.endswith("embeddings") else 0.1))
        Ks = [64] if kind == "IFM" else [model.att_out_dim, 64]
        # dctr_ifm_fwd per sample: the embeddings, the factor sources, F linear weights gathered (a 64-B sector each) and F ids, one float out
        hbm_b = F * d * 4 + sum(Ks) * 4 + F * (64 + 4) + 4
        flop = sum(2 * K * F for K in Ks) + 4 * F * d + 2 * F
        out_m = res["models"][kind] = {"factor_K": Ks, "ifm_hbm_bytes_per_sample": hbm_b, "ifm_flop_per_sample": flop,
                                       "kernel_bytes_from_l2_per_16_samples": sum(K * F * 4 for K in Ks), "rows": {}}
        for n in [int(r) for r in args.rows.split(",")]:
            feed = {fc.name: rng.randint(0, fc.vocabulary_size, n).astype(np.int32) for fc in cols}
            staged = engine.Staged(n)
            model._stage_inputs(feed, staged)
            out = torch.empty(n, dtype=torch.float32, device=device)
            r = out_m["rows"][str(n)] = {"ifm_route": ops.ifm_route(n, F, d, len(Ks))}

            def hip():
                model._begin()
                model._forward(staged, 0, n, out)
            ms_hip = _time(hip, args.iters)
            r.update(forward_ms=round(ms_hip, 4), samples_per_s=round(n / (ms_hip * 1e-3)))
            if kind == "DIFM":          # the same forward with the vector-wise product on dctr_sgemm in front, handed over as m'
                model.vector_part_in_kernel = False
                r["forward_gemm_in_front_ms"] = round(_time(hip, args.iters), 4)
                model.vector_part_in_kernel = True
            if not args.no_torch:
                def torch_ops():
                    with torch.no_grad():
                        training.model_logits(model, staged, 0, n)
                ms_torch = _time(torch_ops, max(2, args.iters // 5))
                r.update(torch_ops_ms=round(ms_torch, 4), torch_ops_samples_per_s=round(n / (ms_torch * 1e-3)),
                         speedup_vs_torch_ops=round(ms_torch / ms_hip, 2))
            ws, bufs, add, desc = model._stage_run(staged, 0, n)
            hidden = model._dnn_hidden(ws, bufs)
            if kind == "IFM":
                sources = [(hidden, model.dense.w("kernel"))]
            else:
                ops.interacting(ws["dnn_in"], [model.att.weights_qkvr], model.att_embedding_size, model.att_head_num, model.att_res, True,
                                fields=F, dim=d, out=bufs["att"])
                sources = [(bufs["att"], model.dense.w("kernel")), (hidden, model.dense_1.w("kernel"))]
            bound_ms = hbm_b * n / (HBM_TBPS * 1e12) * 1e3
            r["ifm_bound_ms"] = round(bound_ms, 4)
            for route in ("auto", "workspace"):
                def ifm():
                    ops.ifm(ws["dnn_in"], F, d, sources=sources, softmax=kind == "IFM", lin=model.lin_positions, lin_desc=desc, add=add,
                            global_bias=model.prediction.w("global_bias"), sigmoid_out=True, out=out, route=route)
                ms = _time(ifm, args.iters)
                key = "ifm_lds" if route == "auto" else "ifm_workspace"
                r[key + "_ms"] = round(ms, 4)
                r[key + "_share_of_bound"] = round(bound_ms / ms, 3)
                r[key + "_tflops"] = round(flop * n / (ms * 1e-3) / 1e12, 3)
            if kind == "DIFM":
                # the alternative: the large-K product on the training step's GEMM, handed over as m'
                mp = torch.zeros(n, F, dtype=torch.float32, device=device)

                def gemm_then_ifm():
                    ops.sgemm(bufs["att"], model.dense.w("kernel"), out=mp)
                    ops.ifm(ws["dnn_in"], F, d, sources=sources[1:], mprime=mp, lin=model.lin_positions, lin_desc=desc, add=add,
                            global_bias=model.prediction.w("global_bias"), sigmoid_out=True, out=out)
                r["gemm_then_ifm_ms"] = round(_time(gemm_then_ifm, args.iters), 4)
        del model
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
