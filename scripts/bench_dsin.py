"""DSIN at a DSIN-like shape (S = 5 sessions of T = 10 behaviours, two session features: E = 32 and E = 64; vocabulary 1e5): the whole
forward (staged ids -> probabilities: fused gather, session lookups, dctr_transformer_fwd over all sessions, the attention kernels,
dctr_bilstm_fwd, DNN) beside the same model's torch-ops forward (training.model_logits under no_grad, the same device), and
dctr_bilstm_fwd alone on the model's own session interests beside training._bilstm in torch ops: the default route and the streamed
route forced.  The bound beside the kernel's time is arithmetic, not a measurement: S x 2 x 4u (D + u) multiply-adds per sample and
layer (ops.bilstm_macs) at the f32 MFMA rate.  Medians of device-event timings over repeated windows, after warm-up of every shape;
the two sides of a comparison alternate window by window.  Prints one JSON line and exits 1 when a speed condition fails (a HIP path
slower than its torch-ops counterpart).

    python scripts/bench_dsin.py [--rows 4096] [--iters 20] [--windows 7]"""
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


def _window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def _time_pair(fa, fb, iters_a, iters_b, windows):
    """Medians (ms per call) of ``windows`` windows of each side, alternating a, b, a, b ..."""
    for _ in range(3):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(windows):
        ta.append(_window(fa, iters_a))
        tb.append(_window(fb, iters_b))
    return float(np.median(ta)), float(np.median(tb))


def main():
    from deepctr_amd import engine, models, ops, training
    from deepctr_amd.feature_column import DenseFeat, SparseFeat, VarLenSparseFeat
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--sessions", type=int, default=5)
    ap.add_argument("--seq-len", type=int, default=10)
    ap.add_argument("--dims", type=int, nargs="+", default=[16, 32], help="embedding_dim of each of the two session features")
    args = ap.parse_args()
    device = torch.device("cuda:0")
    S, T, V, n = args.sessions, args.seq_len, 100000, args.rows
    names = ["item", "cate"]
    res = {"mfma_f32_tflops": MFMA_F32_TFLOPS, "sessions": S, "seq_len": T, "rows": n, "configs": {}}
    rng = np.random.RandomState(0)
    ok = True
    for dim in args.dims:
        E = dim * len(names)
        cols = [SparseFeat("user", V, dim), SparseFeat("gender", 2, dim)] + [SparseFeat(nm, V, dim) for nm in names]
        sess_len = rng.randint(0, S + 1, n).astype(np.int32)
        feed = {"user": rng.randint(0, V, n).astype(np.int32), "gender": rng.randint(0, 2, n).astype(np.int32),
                "pay_score": rng.rand(n).astype(np.float32), "sess_length": sess_len}
        for nm in names:
            feed[nm] = rng.randint(1, V, n).astype(np.int32)
        for i in range(S):
            fill = rng.randint(0, T + 1, n) * (i < sess_len)
            for nm in names:
                cols.append(VarLenSparseFeat(SparseFeat("sess_%d_%s" % (i, nm), V, dim, embedding_name=nm), T))
                ids = rng.randint(1, V, (n, T)).astype(np.int32)
                ids[np.arange(T)[None, :] >= fill[:, None]] = 0
                feed["sess_%d_%s" % (i, nm)] = ids
        cols.append(DenseFeat("pay_score", 1))
        model = models.DSIN(cols, names, sess_max_count=S, att_embedding_size=E // 8, att_head_num=8, device=device)
        g = torch.Generator(device=device).manual_seed(0)
        for k, t in model.named_weights():
            if k.endswith("embeddings"):
                t.copy_(torch.randn(t.shape, generator=g, device=device) * 0.3)
            elif "kernel" in k.rsplit("/", 1)[1]:
                t.copy_(torch.randn(t.shape, generator=g, device=device) * 0.1)
        staged = engine.Staged(n)
        model._stage_inputs(feed, staged)
        out = torch.empty(n, dtype=torch.float32, device=device)
        r = res["configs"]["E%d" % E] = {"route": ops.bilstm_route(S, E, E, 2)}

        def hip():
            model._begin()
            model._forward(staged, 0, n, out)

        def torch_ops():
            with torch.no_grad():
                training.model_logits(model, staged, 0, n)
        ms_hip, ms_torch = _time_pair(hip, torch_ops, args.iters, max(2, args.iters // 10), args.windows)
        r.update(forward_ms=round(ms_hip, 4), samples_per_s=round(n / (ms_hip * 1e-3)), torch_ops_ms=round(ms_torch, 4),
                 speedup_vs_torch_ops=round(ms_torch / ms_hip, 2))
        ok = ok and ms_hip <= ms_torch
        # ---- the BiLSTM alone, over a copy of the model's session interests --------------------------------------------------------
        hip()
        x = model._per_batch(n, dict)["sess_fea"].clone()
        y = torch.empty_like(x)
        layers = model.bilstm.operands()

        def kernel(route=None):
            ops.bilstm(x, layers, out=y, route=route)

        def restated():
            with torch.no_grad():
                training._bilstm(x, layers)
        ms_k, ms_t = _time_pair(kernel, restated, args.iters, max(2, args.iters // 10), args.windows)
        ms_s, _ = _time_pair(lambda: kernel("streamed"), kernel, args.iters, args.iters, args.windows)
        with torch.no_grad():
            err = float((y - training._bilstm(x, layers)).abs().max())
        macs = float(n) * ops.bilstm_macs(S, E, E, 2)
        bound = 2 * macs / (MFMA_F32_TFLOPS * 1e12) * 1e3
        r.update(bilstm_ms=round(ms_k, 4), bilstm_streamed_ms=round(ms_s, 4), bilstm_torch_ops_ms=round(ms_t, 4),
                 bilstm_speedup_vs_torch_ops=round(ms_t / ms_k, 2), bilstm_bound_ms=round(bound, 5), bilstm_share_of_bound=round(bound / ms_k, 4),
                 bilstm_us_per_step_and_layer=round(ms_k * 1e3 / (S * 2), 3), bilstm_macs_per_sample=ops.bilstm_macs(S, E, E, 2),
                 bilstm_max_abs_diff_vs_torch_ops=err)
        ok = ok and ms_k <= ms_t
        del model
        torch.cuda.empty_cache()
    res["conditions_hold"] = bool(ok)
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
