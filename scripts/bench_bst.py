"""BST at a BST-like shape (T = 50 behaviours, two history features of embedding_dim 16: E = 32; att_head_num 8; vocabulary 1e5):
samples/s of the whole forward (staged ids -> probabilities: fused gather, key lookups, ops.transformer in place, attention pooling,
DNN) beside the same model's torch-ops forward (training.model_logits under no_grad), and dctr_transformer_fwd alone on the model's own
key buffer (the fused route and, forced, the general route) beside its f32-MFMA bound.  The bound is arithmetic, not a measurement:
6 T E^2 + 4 T^2 E + 16 T E^2 FLOP per sample and layer (ops.transformer_flops) at 157.3 TFLOP/s.  Device-event timing after warm-up.
With --train-rows: dctr_transformer_train_fwd and dctr_transformer_bwd alone on the key buffer beside the backward's bound
(ops.transformer_bwd_flops), and the autograd step at each of the given row counts with the HIP Transformer off (the torch ops of
training._transformer) and on, alternating window by window: the table of profiles/transformer_bwd.txt.  Prints one JSON line.

    python scripts/bench_bst.py [--rows 4096] [--iters 20] [--train-rows 256,1024,4096]"""
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
    from deepctr_amd.feature_column import DenseFeat, SparseFeat, VarLenSparseFeat
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="4096")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--seq-len", type=int, default=50)
    ap.add_argument("--dim", type=int, default=16)
    ap.add_argument("--heads", type=int, default=8)
    ap.add_argument("--layers", default="1,2")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch-ops forward")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--train-rows", default="", help="comma-separated row counts of the autograd step, HIP Transformer off / on")
    args = ap.parse_args()
    device = torch.device("cuda:0")
    T, V = args.seq_len, 100000
    names = ["item_id", "cate_id"]
    cols = [SparseFeat("user", V, args.dim), SparseFeat("gender", 2, args.dim)] + [SparseFeat(n, V, args.dim) for n in names]
    cols += [VarLenSparseFeat(SparseFeat("hist_" + n, V, args.dim, embedding_name=n), T, length_name="seq_length") for n in names]
    cols.append(DenseFeat("pay_score", 1))
    E = args.dim * len(names)
    res = {"mfma_f32_tflops": MFMA_F32_TFLOPS, "seq_len": T, "dim": E, "heads": args.heads, "configs": {}}
    rng = np.random.RandomState(0)
    for n in [int(r) for r in args.rows.split(",")]:
        lens = rng.randint(1, T + 1, n).astype(np.int32)
        feed = {"user": rng.randint(0, V, n).astype(np.int32), "gender": rng.randint(0, 2, n).astype(np.int32),
                "pay_score": rng.rand(n).astype(np.float32), "seq_length": lens}
        for nm in names:
            feed[nm] = rng.randint(1, V, n).astype(np.int32)
            ids = rng.randint(1, V, (n, T)).astype(np.int32)
            ids[np.arange(T)[None, :] >= lens[:, None]] = 0
            feed["hist_" + nm] = ids
        for L in [int(v) for v in args.layers.split(",")]:
            model = models.BST(cols, names, transformer_num=L, att_head_num=args.heads, device=device)
            g = torch.Generator(device=device).manual_seed(0)
            for k, t in model.named_weights():
                if k.endswith("embeddings"):
                    t.copy_(torch.randn(t.shape, generator=g, device=device) * 0.3)
                elif not k.endswith(("gamma", "lookup_table")):
                    t.copy_(torch.randn(t.shape, generator=g, device=device) * 0.05)
            staged = engine.Staged(n)
            model._stage_inputs(feed, staged)
            out = torch.empty(n, dtype=torch.float32, device=device)
            r = res["configs"]["L%d/%d" % (L, n)] = {"route": ops.transformer_route(T, E, args.heads, L, **_flags(model))}

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
            # ---- the block alone, out of place over a copy of the model's key buffer: both routes ------------------------------------
            model._begin()
            ws = model.stage_plan.run(staged, 0, n)
            keys = model._attention_inputs(staged, 0, n, ws)["k"].clone()
            y = torch.empty_like(keys)
            lt = staged.length["seq_length"][:n]
            layers = [t.operands() for t in model.transformers]

            def block(route=None):
                ops.transformer(keys, layers, args.heads, query_lengths=lt, key_lengths=lt, out=y, route=route, **model.transformers[0].flags())
            ms_fused = _time(block, args.iters)
            ms_general = _time(lambda: block("general"), args.iters)
            bound = n * ops.transformer_flops(T, E, L) / (MFMA_F32_TFLOPS * 1e12) * 1e3
            r.update(block_ms=round(ms_fused, 4), block_general_ms=round(ms_general, 4), block_bound_ms=round(bound, 4),
                     block_share_of_bound=round(bound / ms_fused, 3), block_gflops=round(n * ops.transformer_flops(T, E, L) / ms_fused * 1e-6, 1))
            if args.train_rows:
                import transformer_bwd_timing as tbt
                tbt.kernels(r, model.transformers, args.heads, keys, dict(query_lengths=lt, key_lengths=lt), None, args.iters, args.windows)
                tbt.steps(r, model, staged, n, [int(v) for v in args.train_rows.split(",")],
                          [("transformer_torch", {"TRANSFORMER_HIP_MIN_ROWS": 1 << 62}), ("transformer_hip", {"TRANSFORMER_HIP_MIN_ROWS": 0})],
                          args.iters, args.windows)
            del model
            torch.cuda.empty_cache()
    print(json.dumps(res))


def _flags(model):
    f = dict(model.transformers[0].flags())
    f.pop("ln_eps")
    return f


if __name__ == "__main__":
    main()
