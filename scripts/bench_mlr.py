"""MLR at the reference defaults (region_num 4) on Criteo-shaped input (26 sparse fields of vocabulary 1e5, 13 dense), without and
with a bias part (over the same columns), on uniform and skewed ids (half of each column on one id), device-event timing after
warm-up, medians of alternating windows:

  * dctr_mlr_fwd alone beside its byte bound — per sample the ids, one row-sized 32-B sector per field and row, the dense values, out;
  * the model forward (staged ids -> prediction) beside the same model's torch-ops forward (training._mlr_output under no_grad);
  * dctr_mlr_bwd alone, the rate of its float atomics in added bytes (rows of 32 - 48 B: the 1.3 TB/s of 256-B shapes is NOT a bound
    known to apply, so the rate is reported, not a share);
  * one step of fit()'s autograd path (forward, clipped BCE on the prediction, backward over every weight; no optimizer) with
    training.HIP_AUTOGRAD_OPS off (the torch ops: the baseline) and on.

Prints one JSON line (profiles/mlr.txt keeps it).

``--vocab`` sizes every table (default 1e5: 26 tables of 32 / 48-B rows are 83 / 125 MB and stay resident in the 256-MB Infinity Cache
across back-to-back calls; 1e6 puts them at 0.83 / 1.25 GB, beyond it); ``--forward-only`` skips the backward and the autograd step.

    python scripts/bench_mlr.py [--rows 4096,65536] [--iters 20] [--windows 3] [--vocab 100000] [--forward-only]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GATHER_TBPS = 5.5            # row gathers from tables beyond the Infinity Cache (the cost model of DESIGN.md §4.11)
SECTOR = 32                  # bytes a gathered row costs at least


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


def _alternate(fns, iters, windows):
    """{name: (median ms, spread ms)} of ``windows`` alternating windows of ``iters`` calls each."""
    ms = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            ms[k].append(_time(fn, iters))
    return {k: (sorted(v)[len(v) // 2], max(v) - min(v)) for k, v in ms.items()}


def leg(model, n, dist, iters, windows, V=100000, forward_only=False):
    from deepctr_amd import engine, ops, training
    device = model.device
    F, D = 26, 13
    K = model.n_columns
    rng = np.random.RandomState(1)
    ids = rng.randint(0, V, (n, F))
    if dist == "skewed":
        ids[rng.rand(n, F) < 0.5] = 7
    feed = {"C%d" % i: ids[:, i].astype(np.int32) for i in range(F)}
    feed.update({"I%d" % i: rng.rand(n).astype(np.float32) for i in range(D)})
    staged = engine.Staged(n)
    model._stage_inputs(feed, staged)
    model._begin()
    bufs = model._buffers(n)
    desc = model._descriptors(staged, 0, n, bufs)
    nf = len(model.entries)
    out = torch.empty(n, dtype=torch.float32, device=device)
    z = torch.empty(n, K, dtype=torch.float32, device=device)
    row_bytes = sum(max(SECTOR, -(-e["width"] * 4 // SECTOR) * SECTOR) for e in model.entries)
    fwd_bytes = F * 4 + row_bytes + D * 4 + 4
    bound_ms = fwd_bytes * n / (GATHER_TBPS * 1e12) * 1e3
    r = {"fwd_bytes_per_sample": fwd_bytes, "fwd_bound_ms": round(bound_ms, 5), "field_entries": nf}

    def fwd(zz=None):
        ops.mlr(None, model.region_num, model.has_bias, model.learner_task, dense=staged.dense, dense_w=model._dense_w, out=out, z=zz,
                desc=desc, batch=n, n_fields=nf, device=device)

    def forward():
        model._begin()
        model._forward(staged, 0, n, out)

    def torch_ops():
        with torch.no_grad():
            training._mlr_output(model, staged, 0, n)

    t = _alternate({"fwd": fwd, "fwd_z": lambda: fwd(z), "forward": forward, "torch_ops": torch_ops}, iters, windows)
    r.update(mlr_fwd_ms=round(t["fwd"][0], 5), mlr_fwd_spread_ms=round(t["fwd"][1], 5), mlr_fwd_share_of_bound=round(bound_ms / t["fwd"][0], 3),
             mlr_fwd_with_z_ms=round(t["fwd_z"][0], 5), forward_ms=round(t["forward"][0], 5), forward_spread_ms=round(t["forward"][1], 5),
             samples_per_s=round(n / (t["forward"][0] * 1e-3)), torch_ops_ms=round(t["torch_ops"][0], 5),
             torch_ops_spread_ms=round(t["torch_ops"][1], 5), speedup_vs_torch_ops=round(t["torch_ops"][0] / t["forward"][0], 2))
    if forward_only:
        return r
    # ---- backward alone ------------------------------------------------------------------------------------------------------------
    fwd(z)
    d_out = torch.randn(n, device=device)
    dz = torch.empty(n, K, dtype=torch.float32, device=device)
    gm = {}
    grads = []
    for e in model.entries:
        g = gm.get(e["master"].data_ptr())
        if g is None:
            g = gm[e["master"].data_ptr()] = torch.zeros_like(e["master"])
        grads.append(g[:, e["first"]:])
    atomic_bytes = sum(e["width"] for e in model.entries) * 4 * n

    def bwd():
        ops.mlr_bwd(None, model.region_num, z, d_out, bias=model.has_bias, task=model.learner_task, grads=grads, dz=dz, desc=desc, batch=n,
                    n_fields=nf)

    t = _alternate({"bwd": bwd}, iters, windows)
    r.update(mlr_bwd_ms=round(t["bwd"][0], 5), mlr_bwd_spread_ms=round(t["bwd"][1], 5), mlr_bwd_atomic_bytes=atomic_bytes,
             mlr_bwd_atomic_tbps=round(atomic_bytes / (t["bwd"][0] * 1e-3) / 1e12, 4))
    del gm, grads
    # ---- the autograd step ---------------------------------------------------------------------------------------------------------
    y = (torch.rand(n, device=device) > 0.5).float()
    params = [t_ for _, t_ in model.named_weights()]
    losses = {}

    def step():
        model._begin()
        p = training.model_logits(model, staged, 0, n, training=True).clamp(1e-7, 1.0 - 1e-7)
        loss = -(y * torch.log(p) + (1.0 - y) * torch.log(1.0 - p)).mean()
        for t_ in params:
            t_.grad = None
        loss.backward()
        return loss

    def switched(on):
        def run():
            training.HIP_AUTOGRAD_OPS = on
            return step()
        return run

    min_rows = training.MLR_HIP_MIN_ROWS
    try:
        training.MLR_HIP_MIN_ROWS = 0               # the HIP route is timed at every row count: a threshold is read off this table
        for t_ in params:
            t_.requires_grad_(True)
        t = _alternate({"off": switched(False), "on": switched(True)}, max(2, iters // 4), windows)
        for on in (False, True):
            losses[on] = float(switched(on)().detach())
    finally:
        training.HIP_AUTOGRAD_OPS = True
        training.MLR_HIP_MIN_ROWS = min_rows
        for t_ in params:
            t_.requires_grad_(False)
            t_.grad = None
    r.update(step_ms_switch_off=round(t["off"][0], 4), step_ms_switch_off_spread=round(t["off"][1], 4), step_ms_switch_on=round(t["on"][0], 4),
             step_ms_switch_on_spread=round(t["on"][1], 4), step_speedup=round(t["off"][0] / t["on"][0], 3), loss_switch_off=losses[False],
             loss_switch_on=losses[True])
    return r


def main():
    from deepctr_amd.feature_column import DenseFeat, SparseFeat
    from deepctr_amd.models.mlr import MLR
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="4096,65536")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--vocab", type=int, default=100000)
    ap.add_argument("--forward-only", action="store_true")
    args = ap.parse_args()
    device = torch.device("cuda:0")
    V, F, D = args.vocab, 26, 13
    res = {"fields": F, "dense": D, "vocabulary": V, "region_num": 4, "iters": args.iters, "windows": args.windows, "models": {}}
    cols = [SparseFeat("C%d" % i, V, 4) for i in range(F)] + [DenseFeat("I%d" % i, 1) for i in range(D)]
    for tag, bias in (("no_bias", None), ("bias", cols)):
        model = MLR(cols, bias_feature_columns=bias, device=device)
        g = torch.Generator(device=device).manual_seed(0)
        for _, t in model.named_weights():
            t.copy_(torch.randn(t.shape, generator=g, device=device) * 0.1)
        m = res["models"][tag] = {"columns": model.n_columns,
                                  "row_pitch_bytes": [int(mm.shape[1]) * 4 for _, _, mm in next(iter(model.masters.values()))],
                                  "table_bytes": sum(int(mm.numel()) * 4 for runs in model.masters.values() for _, _, mm in runs), "rows": {}}
        for n in [int(v) for v in args.rows.split(",")]:
            m["rows"][str(n)] = {dist: leg(model, n, dist, args.iters, args.windows, V, args.forward_only) for dist in ("uniform", "skewed")}
            print("%s n=%d: %s" % (tag, n, json.dumps(m["rows"][str(n)])), file=sys.stderr, flush=True)
        del model
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
