"""DSIN at a DSIN-like shape (S = 5 sessions of T = 10 behaviours, two session features: E = 32 and E = 64; vocabulary 1e5): the whole
forward (staged ids -> probabilities: fused gather, session lookups, dctr_transformer_fwd over all sessions, the attention kernels,
dctr_bilstm_fwd, DNN) beside the same model's torch-ops forward (training.model_logits under no_grad, the same device), and
dctr_bilstm_fwd alone on the model's own session interests beside training._bilstm in torch ops: the default route and the streamed
route forced.  The bound beside the kernel's time is arithmetic, not a measurement: S x 2 x 4u (D + u) multiply-adds per sample and
layer (ops.bilstm_macs) at the f32 MFMA rate.
With --train-rows: the backward as well.  dctr_bilstm_train_fwd and dctr_bilstm_bwd alone (all six weight gradients and dx, dropout
masks on; default route and streamed) beside the backward's bound, three times the forward's multiply-adds (ops.bilstm_bwd_macs), and
the autograd step (model_logits in training mode, the loss, torch.autograd.grad over every trainable weight) at each of the given row
counts with training.HIP_AUTOGRAD_OPS off and on, alternating window by window: the table of profiles/dsin_bilstm_bwd.txt; then
dctr_transformer_train_fwd and dctr_transformer_bwd alone over [rows x sessions, T, E] beside the backward's bound, and the step
with every HIP op off, with the BiLSTM alone on HIP (the Transformer on the torch ops of training._transformer) and with both on HIP:
the table of profiles/transformer_bwd.txt.  Medians of device-event timings over repeated windows, after warm-up of every shape;
the two sides of a comparison alternate window by window.  Prints one JSON line and exits 1 when a speed condition fails (a HIP path
slower than its torch-ops counterpart).

    python scripts/bench_dsin.py [--rows 4096] [--iters 20] [--windows 7] [--train-rows 256,1024,4096]"""
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


def _train(r, model, staged, x, S, E, args):
    """dctr_bilstm_train_fwd / dctr_bilstm_bwd alone on the session interests, and the autograd step with the switch off and on per
    row count."""
    from deepctr_amd import ops, training
    n = x.shape[0]
    layers = model.bilstm.operands()
    masks = [(torch.rand(n, E, device=x.device) >= 0.2).float() / 0.8 for _ in range(4)]
    out, tape = ops.bilstm_train(x, layers, masks)
    d_out, dx = torch.randn_like(out), torch.empty_like(x)
    gw = [torch.zeros_like(w) for layer in layers for w in layer]

    def fwd():
        ops.bilstm_train(x, layers, masks, out=out, tape=tape)

    def bwd(route=None):
        ops.bilstm_bwd(x, layers, tape, d_out, masks, dx=dx, d_weights=gw, route=route)
    ms_f, ms_b = _time_pair(fwd, bwd, args.iters, args.iters, args.windows)
    ms_bs, _ = _time_pair(lambda: bwd("streamed"), bwd, args.iters, args.iters, args.windows)
    bound = 2 * float(n) * ops.bilstm_bwd_macs(S, E, E, 2) / (MFMA_F32_TFLOPS * 1e12) * 1e3
    r.update(bilstm_train_fwd_ms=round(ms_f, 4), bilstm_bwd_ms=round(ms_b, 4), bilstm_bwd_streamed_ms=round(ms_bs, 4),
             bilstm_bwd_bound_ms=round(bound, 5), bilstm_bwd_share_of_bound=round(bound / ms_b, 4),
             bilstm_bwd_macs_per_sample=ops.bilstm_bwd_macs(S, E, E, 2),
             bilstm_bwd_route="resident" if ops.bilstm_bwd_supported(S, E, E, 2, route="resident") else "streamed")
    frozen = training.frozen_weights(model)
    params = [t for k, t in model.named_weights() if "moving_" not in k and t.data_ptr() not in frozen]
    y = torch.randint(0, 2, (n,), device=x.device).float()
    steps = r["autograd_step_ms"] = {}
    try:
        for t in params:
            t.requires_grad_(True)
        for rows in [int(v) for v in args.train_rows.split(",")]:
            rows = min(rows, n)

            def step():
                model._begin()
                logit = training.model_logits(model, staged, 0, rows, training=True)
                loss = torch.nn.functional.binary_cross_entropy_with_logits(logit, y[:rows])
                torch.autograd.grad(loss, params, allow_unused=True)

            def switched(on):
                def run():
                    training.HIP_AUTOGRAD_OPS = on
                    step()
                return run
            iters = max(2, args.iters // 5)
            ms_off, ms_on = _time_pair(switched(False), switched(True), iters, iters, args.windows)
            steps[str(rows)] = {"torch_ms": round(ms_off, 3), "hip_ms": round(ms_on, 3), "speedup": round(ms_off / ms_on, 2)}
    finally:
        training.HIP_AUTOGRAD_OPS = True
        for t in params:
            t.requires_grad_(False)
    # ---- the Transformer over all sessions: the two launches alone, and the step with it off (BiLSTM on HIP) and on ----------------
    import transformer_bwd_timing as tbt
    T = args.seq_len
    xs = torch.randn(n * S, T, E, device=x.device)
    m = torch.rand(n * S, T, device=x.device) < 0.7
    tbt.kernels(r, [model.transformer], model.transformer.head_num, xs, dict(query_mask=m, key_mask=m), "mean", args.iters, args.windows)
    keep = dict(steps)
    tbt.steps(r, model, staged, n, [int(v) for v in args.train_rows.split(",")],
              [("torch", {"HIP_AUTOGRAD_OPS": False}), ("bilstm_hip", {"TRANSFORMER_HIP_MIN_ROWS": 1 << 62}),
               ("bilstm_and_transformer_hip", {"TRANSFORMER_HIP_MIN_ROWS": 0})], args.iters, args.windows)
    r["transformer_autograd_step_ms"] = r.pop("autograd_step_ms")
    r["autograd_step_ms"] = keep


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
    ap.add_argument("--train-rows", default="", help="comma-separated row counts of the autograd step, switch off / on (empty: forward only)")
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
        if args.train_rows:
            _train(r, model, staged, x, S, E, args)
        del model
        torch.cuda.empty_cache()
    res["conditions_hold"] = bool(ok)
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
