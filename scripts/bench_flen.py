"""FLEN at two shapes — the reference example's (examples/run_flen.py: 21 SparseFeat in the groups user / context / item = 12 / 6 / 3,
embedding_dim 16, vocabulary 1e5) and Criteo's (26 SparseFeat of embedding_dim 16 split 9 / 9 / 8 over three groups + 13 DenseFeat) —
with the default 256-128-64 DNN: samples/s of the whole forward (staged ids -> probabilities: fused gather, dctr_fieldwise_fwd, DNN
kernel) beside the same model's torch-ops forward (training.model_logits under no_grad); dctr_fieldwise_fwd alone (the model's logit
form) beside its byte bound B*F*d*4, on the model's own dnn_in (rows the gather just wrote: cache-resident at small batches) and on a
ring of buffers larger than the 256-MiB Infinity Cache; dctr_fieldwise_bwd (dlogit form, dx added to) beside 2*B*F*d*4; and one HIP
training step beside one torch-autograd step of the same model and batch.  Device-event timing after warm-up.  Prints one JSON line.

    python scripts/bench_flen.py [--rows 4096,65536] [--iters 20]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_TBPS = 6.3               # achievable streaming rate the bound is quoted at
RING_BYTES = 600 << 20       # the "cold" ring: more than twice the Infinity Cache


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


def shapes():
    from deepctr_amd.feature_column import DenseFeat, SparseFeat
    V = 100000
    grp = ["user"] * 12 + ["context"] * 6 + ["item"] * 3
    example = [SparseFeat("C%d" % i, V, 16, group_name=grp[i]) for i in range(21)]
    grp = ["user"] * 9 + ["context"] * 9 + ["item"] * 8
    criteo = [SparseFeat("C%d" % i, V, 16, group_name=grp[i]) for i in range(26)] + [DenseFeat("I%d" % i, 1) for i in range(13)]
    return (("example", example), ("criteo", criteo))


def main():
    from deepctr_amd import engine, models, ops, training
    from deepctr_amd.feature_column import DenseFeat
    from deepctr_amd.training_hip import HipTrainer
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="4096,65536")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch-ops forward and the autograd step")
    args = ap.parse_args()
    device = torch.device("cuda:0")
    res = {"hbm_tbps": HBM_TBPS, "shapes": {}}
    for tag, cols in shapes():
        rng = np.random.RandomState(0)
        model = models.FLEN(cols, cols, device=device)
        g = torch.Generator(device=device).manual_seed(0)
        for k, t in model.named_weights():
            if "field_wise" not in k:
                t.copy_(torch.randn(t.shape, generator=g, device=device) * (0.1 if k.endswith("embeddings") else 0.05))
        sp, layer, d = model.stage_plan, model.fieldwise, model.emb_dim
        F = sum(n for _, n in model.groups)
        out_s = res["shapes"][tag] = {"fields": F, "groups": [n for _, n in model.groups], "dim": d, "in_dim": sp.in_dim, "rows": {}}
        tr = HipTrainer(model)
        for n in [int(r) for r in args.rows.split(",")]:
            feed = {fc.name: (rng.rand(n).astype(np.float32) if isinstance(fc, DenseFeat) else
                              rng.randint(0, fc.vocabulary_size, n).astype(np.int32)) for fc in cols}
            yt = torch.from_numpy((rng.rand(n) > 0.5).astype(np.float32)).to(device)
            staged = engine.Staged(n)
            model._stage_inputs(feed, staged)
            out = torch.empty(n, dtype=torch.float32, device=device)
            r = out_s["rows"][str(n)] = {"route": ops.fieldwise_route(model.groups, d)}

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
            # ---- the two ops alone ----------------------------------------------------------------------------------------------
            model._begin()
            ws = sp.run(staged, 0, n)
            x = ws["dnn_in"]
            stride = x.stride(0)
            ring = [torch.randn(n, stride, device=device) * 0.1 for _ in range(max(2, min(128, -(-RING_BYTES // (n * stride * 4)))))]
            logit, dl = torch.empty(n, device=device), torch.randn(n, device=device) / n
            dx = torch.zeros(n, stride, device=device)
            head = model._heads()[0]
            bias = layer.biases
            grads = [torch.zeros_like(layer.w(k)) for k in ("kernel_mf", "kernel_fm", "bias_mf", "bias_fm")] + [torch.zeros_like(head)]
            bound = n * F * d * 4 / (HBM_TBPS * 1e12) * 1e3
            r["fwd_bound_ms"], r["bwd_bound_ms"] = round(bound, 5), round(2 * bound, 5)
            turn = [0]

            def fwd(buf):
                ops.fieldwise(buf, model.groups, d, layer.w("kernel_mf"), layer.w("kernel_fm"), *bias, head_w=head, logit=logit)

            def bwd(buf):
                ops.fieldwise_bwd(buf, model.groups, d, layer.w("kernel_mf"), layer.w("kernel_fm"), *bias, dlogit=dl, head_w=head, dx=dx,
                                  accumulate=True, d_kernel_mf=grads[0], d_kernel_fm=grads[1], d_bias_mf=grads[2], d_bias_fm=grads[3],
                                  d_head_w=grads[4])

            def cold(fn):
                def run():
                    turn[0] = (turn[0] + 1) % len(ring)
                    fn(ring[turn[0]])
                return run
            for name, fn, b in (("fwd", fwd, bound), ("bwd", bwd, 2 * bound)):
                warm, cool = _time(lambda: fn(x), args.iters), _time(cold(fn), max(args.iters, len(ring)))
                r[name + "_ms"], r[name + "_cold_ms"] = round(warm, 5), round(cool, 5)
                r[name + "_share_of_bound"], r[name + "_cold_share_of_bound"] = round(b / warm, 3), round(b / cool, 3)
            del ring
            # ---- one training step ----------------------------------------------------------------------------------------------
            r["hip_step_ms"] = round(_time(lambda: tr.step(staged, 0, n, yt), args.iters), 4)
            if not args.no_torch:
                params = [t for k, t in model.named_weights() if "moving_" not in k]
                for t in params:
                    t.requires_grad_(True)
                opt = training._OPTS["adam"](params)

                def autograd_step():
                    model._begin()
                    lg = training.model_logits(model, staged, 0, n, training=True)
                    loss = torch.nn.functional.binary_cross_entropy_with_logits(lg, yt)
                    opt.zero_grad(set_to_none=True)
                    loss.backward()
                    opt.step()
                try:
                    r["autograd_step_ms"] = round(_time(autograd_step, max(2, args.iters // 4)), 4)
                finally:
                    for t in params:
                        t.requires_grad_(False)
                del opt
                r["hip_step_speedup"] = round(r["autograd_step_ms"] / r["hip_step_ms"], 2)
            torch.cuda.empty_cache()
        del model, tr
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
