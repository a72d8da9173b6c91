"""CCPM and FGCNN at their default configurations (B = 4096, vocabulary 1e5): the conv / pool stack alone (dctr_fieldconv_fwd on its
default route and with the resident and the streamed route forced, beside training._field_conv in torch ops) at CCPM's defaults (26 fields, E 8) and at
FGCNN's (26 and 39 fields, E 8 and 16), and both models' whole forward (staged ids -> probabilities) beside the same model's torch-ops
forward (training.model_logits under no_grad, the same device).  The bound beside a kernel's time is arithmetic, not a measurement:
E x sum over the stages of rows w C_in C_out multiply-adds per sample (ops.field_conv_macs) at the f32 MFMA rate.  Medians of
device-event timings over repeated windows, after warm-up of every shape; the two sides of a comparison alternate window by window.
Prints one JSON line and exits 1 when a speed condition fails (a HIP path slower than its torch-ops counterpart, or the route the library
chooses slower than the other one).

    python scripts/bench_ccpm_fgcnn.py [--rows 4096] [--iters 20] [--windows 7]"""
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
CCPM_STACK = ((6, 5), (4, 4))
FGCNN_STACK = ((7, 7, 7, 7), (14, 16, 18, 20))


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


def bench_stack(ops, training, device, n, F, E, widths, filters, pools, args):
    g = torch.Generator(device=device).manual_seed(F * 100 + E)
    x = torch.randn((n, F, E), generator=g, device=device) * 0.3
    ks, bs, cin = [], [], 1
    for w, c in zip(widths, filters):
        ks.append(torch.randn((w, 1, cin, c), generator=g, device=device) / float(np.sqrt(cin)))
        bs.append(torch.randn((c,), generator=g, device=device) * 0.2)
        cin = c
    y = ops.field_conv(x, ks, bs, pools)

    def kernel(route=None):
        ops.field_conv(x, ks, bs, pools, out=y.view(n, -1), route=route)

    def restated():
        with torch.no_grad():
            training._field_conv(x, ks, bs, pools)
    ms_k, ms_t = _time_pair(kernel, restated, args.iters, max(2, args.iters // 10), args.windows)
    auto = ops.field_conv_route(F, E, ks, pools)
    fits = _fits(ops, F, E, ks, pools)
    ms_r = ms_s = None
    if fits:
        ms_r, ms_s = _time_pair(lambda: kernel("resident"), lambda: kernel("streamed"), args.iters, args.iters, args.windows)
    with torch.no_grad():
        err = float((y - training._field_conv(x, ks, bs, pools)[0]).abs().max())
    macs = ops.field_conv_macs(F, E, ks, pools)
    bound = 2.0 * n * macs / (MFMA_F32_TFLOPS * 1e12) * 1e3
    r = dict(route=auto, ms=round(ms_k, 4), torch_ops_ms=round(ms_t, 4), speedup_vs_torch_ops=round(ms_t / ms_k, 2), bound_ms=round(bound, 5),
             share_of_bound=round(bound / ms_k, 4), macs_per_sample=macs, max_abs_diff_vs_torch_ops=err)
    good = ms_k <= ms_t
    if fits:        # the router's choice is not the slower of the two (the 2 % allowance for timing noise is a guess, not a measured spread)
        r.update(resident_ms=round(ms_r, 4), streamed_ms=round(ms_s, 4))
        good = good and (ms_r if auto == "resident" else ms_s) <= 1.02 * (ms_s if auto == "resident" else ms_r)
    return r, good


def _fits(ops, F, E, ks, pools):
    """Can the resident route be forced at this shape?  (The library answers DCTR_E_UNSUPPORTED past the LDS.)"""
    from deepctr_amd import _C
    try:
        return ops.field_conv_route(F, E, ks, pools, route="resident") == "resident"
    except _C.DctrError:
        return False


def bench_model(engine, models, training, device, n, which, F, E, args):
    from deepctr_amd.feature_column import SparseFeat
    V = 100000
    rng = np.random.RandomState(F * 100 + E)
    cols = [SparseFeat("C%d" % i, V, E) for i in range(F)]
    feed = {"C%d" % i: rng.randint(0, V, n).astype(np.int32) for i in range(F)}
    model = getattr(models, which)(cols, cols, device=device)
    g = torch.Generator(device=device).manual_seed(0)
    for k, t in model.named_weights():
        if k.endswith("embeddings"):
            t.copy_(torch.randn(t.shape, generator=g, device=device) * 0.3)
        elif k.startswith("conv2d") and k.endswith("kernel"):
            t.copy_(torch.randn(t.shape, generator=g, device=device) / float(np.sqrt(t.shape[2])))
    staged = engine.Staged(n)
    model._stage_inputs(feed, staged)
    out = torch.empty(n, dtype=torch.float32, device=device)

    def hip():
        model._begin()
        model._forward(staged, 0, n, out)

    def torch_ops():
        with torch.no_grad():
            training.model_logits(model, staged, 0, n)
    ms_hip, ms_torch = _time_pair(hip, torch_ops, args.iters, max(2, args.iters // 10), args.windows)
    del model
    torch.cuda.empty_cache()
    return dict(forward_ms=round(ms_hip, 4), samples_per_s=round(n / (ms_hip * 1e-3)), torch_ops_ms=round(ms_torch, 4),
                speedup_vs_torch_ops=round(ms_torch / ms_hip, 2)), ms_hip <= ms_torch


def main():
    from deepctr_amd import engine, models, ops, training
    from deepctr_amd.models.ccpm import kmax_schedule
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    args = ap.parse_args()
    device = torch.device("cuda:0")
    n = args.rows
    res = {"mfma_f32_tflops": MFMA_F32_TFLOPS, "rows": n, "stacks": {}, "models": {}}
    ok = True
    shapes = [("ccpm", 26, 8)] + [("fgcnn", F, E) for F in (26, 39) for E in (8, 16)]
    for which, F, E in shapes:
        widths, filters = CCPM_STACK if which == "ccpm" else FGCNN_STACK
        pools = [("kmax", k) for k in kmax_schedule(F, len(widths))] if which == "ccpm" else [("max", 2)] * len(widths)
        r, good = bench_stack(ops, training, device, n, F, E, widths, filters, pools, args)
        res["stacks"]["%s_F%d_E%d" % (which, F, E)] = r
        ok = ok and good
    for which, F, E in (("CCPM", 26, 8), ("FGCNN", 26, 8), ("FGCNN", 39, 16)):
        r, good = bench_model(engine, models, training, device, n, which, F, E, args)
        res["models"]["%s_F%d_E%d" % (which, F, E)] = r
        ok = ok and good
    res["conditions_hold"] = bool(ok)
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
