"""EDCN at Criteo's sparse shape (26 SparseFeat of embedding_dim 16: D = 416, vocabulary 1e5), cross_num 2, for every bridge type and
both cross parameterizations: samples/s of the whole forward (staged ids -> probabilities: fused gather, ops.edcn) beside the same
model's torch-ops forward (training.model_logits under no_grad) and beside the layered route of ops.edcn; and dctr_edcn_fwd alone (the
model's logit form, on the model's own dnn_in) beside its f32-MFMA bound.  The bound is arithmetic, not a measurement: per row and round
2 D^2 FLOP for the DNN, + 2 D^2 for a matrix cross, + 4 D^2 for the concatenation bridge, at 157.3 TFLOP/s.  attention_pooling has no
fused route: its forward IS the layered one.  Device-event timing after warm-up.  Prints one JSON line.

    python scripts/bench_edcn.py [--rows 65536] [--iters 20]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MFMA_F32_TFLOPS = 157.3
BRIDGES = ("pointwise_addition", "hadamard_product", "concatenation", "attention_pooling")


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


def tower_flops(D, cross_num, bridge_type, parameterization):
    per = 2 * D * D + (2 * D * D if parameterization == "matrix" else 0) + (4 * D * D if bridge_type == "concatenation" else 0)
    return cross_num * per


def main():
    from deepctr_amd import engine, models, ops, training
    from deepctr_amd.feature_column import SparseFeat
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="65536")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--fields", type=int, default=26)
    ap.add_argument("--dim", type=int, default=16)
    ap.add_argument("--cross-num", type=int, default=2)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch-ops forward")
    args = ap.parse_args()
    device = torch.device("cuda:0")
    cols = [SparseFeat("C%d" % i, 100000, args.dim) for i in range(args.fields)]
    D = args.fields * args.dim
    res = {"mfma_f32_tflops": MFMA_F32_TFLOPS, "fields": args.fields, "dim": args.dim, "cross_num": args.cross_num, "configs": {}}
    rng = np.random.RandomState(0)
    for n in [int(r) for r in args.rows.split(",")]:
        feed = {fc.name: rng.randint(0, fc.vocabulary_size, n).astype(np.int32) for fc in cols}
        for bridge_type in BRIDGES:
            for par in ("vector", "matrix"):
                model = models.EDCN(cols, cols, cross_num=args.cross_num, cross_parameterization=par, bridge_type=bridge_type, device=device)
                g = torch.Generator(device=device).manual_seed(0)
                for k, t in model.named_weights():
                    if not k.endswith("embeddings"):
                        t.copy_(torch.randn(t.shape, generator=g, device=device) * (1.0 if k.endswith("_field_weight") else 0.05))
                staged = engine.Staged(n)
                model._stage_inputs(feed, staged)
                out = torch.empty(n, dtype=torch.float32, device=device)
                r = res["configs"]["%s/%s/%d" % (bridge_type, par, n)] = {"route": model.route()}

                def hip():
                    model._begin()
                    model._forward(staged, 0, n, out)
                ms_hip = _time(hip, args.iters)
                r.update(forward_ms=round(ms_hip, 4), samples_per_s=round(n / (ms_hip * 1e-3)))
                if not args.no_torch:
                    def torch_ops():
                        with torch.no_grad():
                            training.model_logits(model, staged, 0, n)
                    ms_torch = _time(torch_ops, max(2, args.iters // 4))
                    r.update(torch_ops_ms=round(ms_torch, 4), torch_ops_samples_per_s=round(n / (ms_torch * 1e-3)),
                             speedup_vs_torch_ops=round(ms_torch / ms_hip, 2))
                # ---- the tower alone, on the model's own dnn_in: both routes -----------------------------------------------------------
                model._begin()
                ws = model.stage_plan.run(staged, 0, n)
                targs, tkw = model._tower_args()
                logit = torch.empty(n, dtype=torch.float32, device=device)

                def tower(route=None):
                    ops.edcn(ws["dnn_in"], model.n_fields, model.emb_dim, *targs, head_w=model.dense.w("kernel"), logit=logit, route=route, **tkw)
                ms_layered = _time(lambda: tower("layered"), args.iters)
                r["tower_layered_ms"] = round(ms_layered, 4)
                if r["route"] == "fused":
                    ms_fused = _time(tower, args.iters)
                    bound = n * tower_flops(D, args.cross_num, bridge_type, par) / (MFMA_F32_TFLOPS * 1e12) * 1e3
                    r.update(tower_fused_ms=round(ms_fused, 4), tower_bound_ms=round(bound, 4), tower_share_of_bound=round(bound / ms_fused, 3),
                             tower_speedup_vs_layered=round(ms_layered / ms_fused, 2))
                del model
                torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
