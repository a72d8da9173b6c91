"""DIEN at a DIEN-like shape (T = 50 behaviours, two history features of embedding_dim 16: E = 32; vocabulary 1e5), per gru_type: the
whole forward (staged ids -> probabilities: fused gather, key lookups, dctr_gru_fwd, the attention kernels, DNN) beside the same model's
torch-ops forward (training.model_logits under no_grad, the same device), and dctr_gru_fwd alone on the model's own key buffer: the
default route, the streamed route forced, and for the plain stack the two-layer launch beside two one-layer launches.  The bound beside
the kernel's time is arithmetic, not a measurement: T x 6 E^2 multiply-adds per sample and layer (ops.gru_macs) at the f32 MFMA rate.
With --train-rows: the backward as well.  dctr_gru_bwd alone for the evolution layer's cell (default route and streamed) beside its
bound, the forward's 6 E^2 multiply-adds recomputed + 12 E^2 for the four gradient products per step and sample (ops.gru_bwd_macs),
and the autograd step (model_logits in training mode, the loss, torch.autograd.grad over every trainable weight) at each of the
given row counts with training.HIP_AUTOGRAD_OPS on and off: the table of profiles/dien_gru_bwd.txt.
Medians of device-event timings over repeated windows, after warm-up of every shape.  Prints one JSON line and exits 1 when a speed
condition fails (the default route slower than the torch-ops forward; the two-layer launch slower than two one-layer launches).

    python scripts/bench_dien.py [--rows 4096] [--iters 20] [--windows 7] [--train-rows 256,1024,4096]"""
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
GRU_TYPES = ("GRU", "AIGRU", "AGRU", "AUGRU")


def _time(fn, iters, windows):
    """Median over ``windows`` timed windows of ``iters`` calls each, ms per call."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters)
    return float(np.median(out))


def _train(r, model, staged, feed, keys, lt, att, gru_type, lens, E, T, args):
    """dctr_gru_bwd alone on the evolution layer, and the autograd step with the switch on and off per row count."""
    from deepctr_amd import ops, training
    n = keys.shape[0]
    plain = gru_type == "GRU"
    kw = dict(cell=model.gru2.cell, att_scores=None if plain else att, scale_input=gru_type == "AIGRU", return_sequence=plain)
    l2 = model.gru2.operands()
    h = ops.dynamic_gru(keys, lt, [l2], cell=kw["cell"], att_scores=kw["att_scores"], scale_input=kw["scale_input"])
    d_out = torch.randn((n, T, E) if plain else (n, E), device=keys.device)
    dx, d_att = torch.empty_like(keys), torch.empty_like(att)
    gw = [torch.zeros_like(w) for w in l2]

    def bwd(route=None):
        ops.gru_bwd(keys, lt, l2, h, d_out, dx=dx, d_att=None if plain else d_att, d_weights=gw, route=route, **kw)
    ms_b = _time(bwd, args.iters, args.windows)
    ms_bs = _time(lambda: bwd("streamed"), args.iters, args.windows)
    bound = 2 * float(np.minimum(lens, T).sum()) * 18 * E * E / (MFMA_F32_TFLOPS * 1e12) * 1e3
    r.update(gru_bwd_ms=round(ms_b, 4), gru_bwd_streamed_ms=round(ms_bs, 4), gru_bwd_bound_ms=round(bound, 5),
             gru_bwd_share_of_bound=round(bound / ms_b, 4), gru_bwd_macs_per_sample_full_length=ops.gru_bwd_macs(T, E))
    frozen = training.frozen_weights(model)
    params = [t for k, t in model.named_weights() if "moving_" not in k and t.data_ptr() not in frozen]
    y = torch.randint(0, 2, (n,), device=keys.device).float()
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
            cell = steps[str(rows)] = {}
            for switch in (True, False, True, False):            # alternately: drift shows as a difference between the two passes
                training.HIP_AUTOGRAD_OPS = switch
                ms = _time(step, max(2, args.iters // 5), max(3, args.windows // 2))
                cell.setdefault("hip_ms" if switch else "torch_ms", []).append(round(ms, 3))
            training.HIP_AUTOGRAD_OPS = True
            cell["speedup"] = round(min(cell["torch_ms"]) / max(cell["hip_ms"]), 2)
    finally:
        training.HIP_AUTOGRAD_OPS = True
        for t in params:
            t.requires_grad_(False)


def main():
    from deepctr_amd import engine, models, ops, training
    from deepctr_amd.feature_column import DenseFeat, SparseFeat, VarLenSparseFeat
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--seq-len", type=int, default=50)
    ap.add_argument("--dim", type=int, default=16)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch-ops forward")
    ap.add_argument("--train-rows", default="", help="comma-separated row counts of the autograd step, switch on / off (empty: forward only)")
    args = ap.parse_args()
    device = torch.device("cuda:0")
    T, V, n = args.seq_len, 100000, args.rows
    names = ["item_id", "cate_id"]
    cols = [SparseFeat("user", V, args.dim), SparseFeat("gender", 2, args.dim)] + [SparseFeat(nm, V, args.dim) for nm in names]
    cols += [VarLenSparseFeat(SparseFeat("hist_" + nm, V, args.dim, embedding_name=nm), T, length_name="seq_length") for nm in names]
    cols.append(DenseFeat("pay_score", 1))
    E = args.dim * len(names)
    res = {"mfma_f32_tflops": MFMA_F32_TFLOPS, "seq_len": T, "dim": E, "rows": n, "configs": {}}
    rng = np.random.RandomState(0)
    lens = rng.randint(1, T + 1, n).astype(np.int32)
    feed = {"user": rng.randint(0, V, n).astype(np.int32), "gender": rng.randint(0, 2, n).astype(np.int32),
            "pay_score": rng.rand(n).astype(np.float32), "seq_length": lens}
    for nm in names:
        feed[nm] = rng.randint(1, V, n).astype(np.int32)
        ids = rng.randint(1, V, (n, T)).astype(np.int32)
        ids[np.arange(T)[None, :] >= lens[:, None]] = 0
        feed["hist_" + nm] = ids
    ok = True
    for gru_type in GRU_TYPES:
        model = models.DIEN(cols, names, gru_type=gru_type, device=device)
        g = torch.Generator(device=device).manual_seed(0)
        for k, t in model.named_weights():
            if k.endswith("embeddings"):
                t.copy_(torch.randn(t.shape, generator=g, device=device) * 0.3)
            elif k.endswith("kernel") or "kernel" in k.rsplit("/", 1)[1]:
                t.copy_(torch.randn(t.shape, generator=g, device=device) * 0.1)
        staged = engine.Staged(n)
        model._stage_inputs(feed, staged)
        out = torch.empty(n, dtype=torch.float32, device=device)
        L = 2 if gru_type == "GRU" else 1
        r = res["configs"][gru_type] = {"route": ops.gru_route(T, E, L)}

        def hip():
            model._begin()
            model._forward(staged, 0, n, out)
        ms_hip = _time(hip, args.iters, args.windows)
        r.update(forward_ms=round(ms_hip, 4), samples_per_s=round(n / (ms_hip * 1e-3)))
        if not args.no_torch:
            def torch_ops():
                with torch.no_grad():
                    training.model_logits(model, staged, 0, n)
            ms_torch = _time(torch_ops, max(2, args.iters // 10), max(3, args.windows // 2))
            r.update(torch_ops_ms=round(ms_torch, 4), speedup_vs_torch_ops=round(ms_torch / ms_hip, 2))
            ok = ok and ms_hip <= ms_torch
        # ---- the recurrence alone, over a copy of the model's key buffer -----------------------------------------------------------
        model._begin()
        ws = model.stage_plan.run(staged, 0, n)
        keys = model._attention_inputs(staged, 0, n, ws)["k"].clone()
        lt = staged.length["seq_length"][:n]
        att = torch.rand(n, T, device=device)
        seq, mid, fin = torch.empty_like(keys), torch.empty_like(keys), torch.empty(n, E, device=device)
        l1, l2 = model.gru1.operands(), model.gru2.operands()
        if gru_type == "GRU":
            def kernel(route=None):
                ops.dynamic_gru(keys, lt, [l1, l2], out=seq, route=route)

            def two_launches():
                ops.dynamic_gru(keys, lt, [l1], out=mid)
                ops.dynamic_gru(mid, lt, [l2], out=seq)
            ms_two = _time(two_launches, args.iters, args.windows)
        else:
            def kernel(route=None):
                ops.dynamic_gru(keys, lt, [l2], cell=model.gru2.cell, att_scores=att, scale_input=gru_type == "AIGRU", return_sequence=False,
                                out=fin, route=route)
            ms_two = None
        ms_k = _time(kernel, args.iters, args.windows)
        ms_s = _time(lambda: kernel("streamed"), args.iters, args.windows)
        # every sample runs its own length: the multiply-adds of the steps that exist
        macs = float(np.minimum(lens, T).sum()) * 6 * E * E * L
        bound = 2 * macs / (MFMA_F32_TFLOPS * 1e12) * 1e3
        r.update(gru_ms=round(ms_k, 4), gru_streamed_ms=round(ms_s, 4), gru_bound_ms=round(bound, 5), gru_share_of_bound=round(bound / ms_k, 4),
                 gru_us_per_step_and_layer=round(ms_k * 1e3 / (T * L), 3), gru_macs_per_sample_full_length=ops.gru_macs(T, E, L))
        if ms_two is not None:
            r.update(two_one_layer_launches_ms=round(ms_two, 4), two_layer_launch_speedup=round(ms_two / ms_k, 2))
            ok = ok and ms_k <= ms_two
        if args.train_rows:
            _train(r, model, staged, feed, keys, lt, att, gru_type, lens, E, T, args)
        del model
        torch.cuda.empty_cache()
    res["conditions_hold"] = bool(ok)
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
