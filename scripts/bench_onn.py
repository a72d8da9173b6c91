"""ONN at the reference defaults on Criteo-shaped input (26 sparse fields of vocabulary 1e5, 13 dense; DNN 256-128-64 over 325*d + 13
columns) at embedding_dim 4 (the reference's SparseFeat default) and 16: samples/s of the whole forward (staged ids -> probabilities:
linear part, dctr_ffm_fwd, DNN kernel) beside the same model's torch-ops forward (training.model_logits under no_grad), device-event
timing after warm-up, then dctr_ffm_fwd alone on each route and the DNN call alone, each beside its bound.  ``--train-rows`` runs the
training leg instead: dctr_ffm_bwd per route beside its atomic-byte bound on uniform and skewed ids, and one step of fit()'s autograd
path with the pair products in torch ops and on HIP (profiles/onn_ffm_bwd.txt).  Prints one JSON line.

    python scripts/bench_onn.py [--dims 4,16] [--rows 4096,65536] [--iters 20] [--train-rows 4096,65536]"""
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
ATOMIC_TBPS = 1.3            # chip-wide rate of global float atomic adds, in added bytes (256-B wave-instructions spread over many rows)


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


def train_leg(model, d, n, iters, rounds=3):
    """The training leg at ``n`` rows: dctr_ffm_bwd alone per route and id distribution beside its atomic-byte bound — every gradient
    element is one float atomic, B*F*(F-1)*d*4 added bytes over the chip-wide float-atomic rate — and one step of fit()'s autograd path
    (model_logits(training=True), BCE, backward over every trainable weight; no optimizer) with training.HIP_AUTOGRAD_OPS off (the
    torch ops: the baseline) and on, alternating in ``rounds`` windows of ``iters`` steps.  Ids: uniform over the vocabulary, and skewed
    — half of each column holds one id."""
    from deepctr_amd import engine, ops, training
    device = model.device
    V, F, D = 100000, 26, 13
    P = F * (F - 1) // 2
    rng = np.random.RandomState(1)
    bound_ms = n * F * (F - 1) * d * 4 / (ATOMIC_TBPS * 1e12) * 1e3
    res = {"ffm_bwd_atomic_bytes": n * F * (F - 1) * d * 4, "ffm_bwd_bound_ms": round(bound_ms, 4), "ids": {}}
    g = torch.randn(n, P * d, device=device)
    grads = [torch.zeros_like(m) for m in model.masters]
    for dist in ("uniform", "skewed"):
        ids = rng.randint(0, V, (n, F))
        if dist == "skewed":
            ids[rng.rand(n, F) < 0.5] = 7
        feed = {"C%d" % i: ids[:, i].astype(np.int32) for i in range(F)}
        feed.update({"I%d" % i: rng.rand(n).astype(np.float32) for i in range(D)})
        staged = engine.Staged(n)
        model._stage_inputs(feed, staged)
        desc = model._descriptors(staged, 0, n, model._buffers(n))
        r = res["ids"][dist] = {}
        for route in ("auto", "direct"):
            def bwd():
                ops.ffm_bwd(None, model.masters, g, grads, dim=d, desc=desc, batch=n, route=route)
            ms = _time(bwd, iters)
            key = "ffm_bwd_lds" if route == "auto" else "ffm_bwd_direct"
            r[key + "_ms"] = round(ms, 4)
            r[key + "_share_of_bound"] = round(bound_ms / ms, 3)
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
        min_rows = training.ONN_HIP_MIN_ROWS
        try:
            training.ONN_HIP_MIN_ROWS = 0           # the HIP route is timed at every row count: a threshold is read off this table
            for t in params:
                t.requires_grad_(True)
            for _ in range(rounds):
                for switch in (False, True):
                    training.HIP_AUTOGRAD_OPS = switch
                    ms[switch].append(_time(step, iters))
                    losses[switch] = float(step().detach())
        finally:
            training.HIP_AUTOGRAD_OPS = True
            training.ONN_HIP_MIN_ROWS = min_rows
            for t in params:
                t.requires_grad_(False)
                t.grad = None
        off, off_spread = _median_spread(ms[False])
        on, on_spread = _median_spread(ms[True])
        r.update(step_ms_switch_off=round(off, 4), step_ms_switch_off_spread=round(off_spread, 4), step_ms_switch_on=round(on, 4),
                 step_ms_switch_on_spread=round(on_spread, 4), step_speedup=round(off / on, 3), windows=rounds, steps_per_window=iters,
                 loss_switch_off=losses[False], loss_switch_on=losses[True])
    return res


def main():
    from deepctr_amd import engine, models, ops, training
    from deepctr_amd.feature_column import DenseFeat, SparseFeat
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="4,16")
    ap.add_argument("--rows", default="4096,65536")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch-ops forward")
    ap.add_argument("--train-rows", default="", help="row counts of the training leg (dctr_ffm_bwd and the autograd step); with it the "
                                                     "forward legs are skipped")
    args = ap.parse_args()
    device = torch.device("cuda:0")
    V, F, D = 100000, 26, 13
    P = F * (F - 1) // 2
    units = [256, 128, 64]
    res = {"fields": F, "dense": D, "pairs": P, "vocabulary": V, "dims": {}}
    for d in [int(v) for v in args.dims.split(",")]:
        if args.train_rows:
            cols = [SparseFeat("C%d" % i, V, d) for i in range(F)] + [DenseFeat("I%d" % i, 1) for i in range(D)]
            model = models.ONN(cols, cols, device=device)
            res["dims"][str(d)] = {"train_rows": {str(n): train_leg(model, d, n, args.iters) for n in
                                                  [int(r) for r in args.train_rows.split(",")]}}
            print("d=%d: %s" % (d, json.dumps(res["dims"][str(d)])), file=sys.stderr, flush=True)
            del model
            torch.cuda.empty_cache()
            continue
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
