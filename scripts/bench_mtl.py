"""The multi-task forward at three shapes: MMOE at the example's shape (29 SparseFeat of embedding_dim 4 + 11 dense values: Din 127,
3 experts of (256, 128), no tower DNN), MMOE at Criteo's shape (26 SparseFeat of embedding_dim 16 + 13 dense values: Din 429, the same
experts, tower (64,)) and PLE (1 shared / 1 specific expert of (256,), 2 levels, tower (64,)) at Criteo's shape.  Per shape: samples/s of
the whole forward (staged ids -> [T, rows] probabilities: fused gather, ops.mtl_level per level, ops.mtl_towers) beside the same model's
torch-ops forward (autograd_logits + autograd_outputs under no_grad) and beside the forced-layered route; and dctr_mtl_level_fwd alone
(the first level, on the model's own dnn_in) beside its f32-MFMA bound and at each tile height.  The bound is arithmetic, not a
measurement: 2 K N FLOP per row and layer of every expert and gate DNN plus the gate logits, at 157.3 TFLOP/s.  Device-event timing
after warm-up.  Training (DESIGN.md §4.15 "Training"): one HIP training step (training_hip.HipTrainer, Adam) beside one torch-autograd step
(the loop body of models/multitask/_fit.py:fit_torch, Adam) of the same model on ``--train-rows`` rows, and dctr_mtl_mix_bwd alone on
``--rows`` rows of the first level beside its byte bound — h and d_out read, dh written, at 6.3 TB/s.  Prints one JSON line.

    python scripts/bench_mtl.py [--rows 65536] [--train-rows 4096] [--iters 20]"""
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
HBM_TBPS = 6.3               # achievable streaming rate the bound is quoted at


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


def level_flops(in_dim, lv):
    dims = [in_dim] + list(lv.experts[0].hidden_units)
    per_expert = sum(2 * dims[i] * dims[i + 1] for i in range(len(dims) - 1))
    gd = [in_dim] + list(lv.gate_dnns[0].hidden_units)
    per_gate = sum(2 * gd[i] * gd[i + 1] for i in range(len(gd) - 1))
    return len(lv.experts) * per_expert + sum(per_gate + 2 * gd[-1] * len(ms) for ms in lv.members)


def train_times(model, cols, rows, iters, with_torch, rng):
    """One HIP step and one autograd step (both Adam, both with the l2 penalties) of ``model`` on ``rows`` rows, in ms."""
    from deepctr_amd import engine, training, training_hip
    from deepctr_amd.feature_column import SparseFeat
    from deepctr_amd.models.multitask import _fit
    feed = {fc.name: (rng.randint(0, fc.vocabulary_size, rows).astype(np.int32) if isinstance(fc, SparseFeat) else
                      rng.rand(rows).astype(np.float32)) for fc in cols}
    staged = engine.Staged(rows)
    model._stage_inputs(feed, staged)
    yt = torch.from_numpy((rng.rand(model.num_tasks, rows) > 0.5).astype(np.float32)).to(model.device)
    model.compile("adam")
    r = {"rows": rows, "hip_supported": bool(training_hip.supported(model))}
    if with_torch:          # first: the HIP step moves the weights through raw pointers
        params = [t for k, t in model.named_weights() if "moving_" not in k]
        for t in params:
            t.requires_grad_(True)
        opt = training._OPTS["adam"](params)
        regs = training.regularized_weights(model)
        w = model._compiled["loss_weights"]

        def autograd_step():
            model._begin()
            pairs = _fit.task_losses(model, model.autograd_logits(staged, 0, rows, training=True), yt)
            loss = sum(wt * l for wt, (l, _) in zip(w, pairs))
            for t, l2 in regs:
                loss = loss + l2 * (t * t).sum()
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
        try:
            r["autograd_step_ms"] = round(_time(autograd_step, max(2, iters // 4)), 4)
        finally:
            for t in params:
                t.requires_grad_(False)
        del opt
    if r["hip_supported"]:
        tr = training_hip.HipTrainer(model, "adam")
        acc = torch.zeros(model.num_tasks, dtype=torch.float32, device=model.device)
        r["hip_step_ms"] = round(_time(lambda: tr.step(staged, 0, rows, yt, loss_acc=acc), iters), 4)
        if with_torch:
            r["hip_step_speedup"] = round(r["autograd_step_ms"] / r["hip_step_ms"], 2)
    return r


def mix_bwd_time(model, x, n, iters):
    """dctr_mtl_mix_bwd on the first level (expert outputs and gate inputs of random values) beside its byte bound."""
    from deepctr_amd import ops
    lv, dev = model.levels[0], model.device
    E, G, H, n_all = len(lv.experts), len(lv.gate_dense), lv.experts[0].hidden_units[-1], sum(len(ms) for ms in lv.members)
    dz = lv.gate_dnns[0].hidden_units[-1] if lv.gate_dnns[0].hidden_units else model.stage_plan.in_dim
    new = lambda cols: torch.randn(n, cols, dtype=torch.float32, device=dev)      # noqa: E731
    h, d_out, dh, ds = new(E * H), new(G * H), new(E * H), new(n_all)
    zs = [x[:, :dz] if not lv.gate_dnns[0].hidden_units else new(dz) for _ in range(G)]
    gk = [g.w("kernel") for g in lv.gate_dense]
    ms = _time(lambda: ops.mtl_mix_bwd(h, E, H, zs, gk, lv.members, d_out, dh, ds), iters)
    bound = n * (2 * E * H + G * H) * 4 / (HBM_TBPS * 1e12) * 1e3
    return {"mix_bwd_ms": round(ms, 4), "mix_bwd_bound_ms": round(bound, 4), "mix_bwd_share_of_bound": round(bound / ms, 3)}


def main():
    from deepctr_amd import engine, models
    from deepctr_amd.feature_column import DenseFeat, SparseFeat
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--train-rows", type=int, default=4096, help="rows of the training steps (0: skip them)")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch-ops forward and the autograd step")
    args = ap.parse_args()
    device = torch.device("cuda:0")
    n = args.rows
    census = [SparseFeat("C%d" % i, 50, 4) for i in range(29)] + [DenseFeat("I%d" % i, 1) for i in range(11)]
    criteo = [SparseFeat("C%d" % i, 100000, 16) for i in range(26)] + [DenseFeat("I%d" % i, 1) for i in range(13)]
    shapes = (("mmoe_example", "MMOE", census, dict(tower_dnn_hidden_units=())),
              ("mmoe_criteo", "MMOE", criteo, dict(tower_dnn_hidden_units=(64,))),
              ("ple_criteo", "PLE", criteo, dict(shared_expert_num=1, specific_expert_num=1, num_levels=2, expert_dnn_hidden_units=(256,),
                                                 tower_dnn_hidden_units=(64,))))
    res = {"mfma_f32_tflops": MFMA_F32_TFLOPS, "rows": n, "configs": {}}
    rng = np.random.RandomState(0)
    for tag, kind, cols, kw in shapes:
        feed = {fc.name: (rng.randint(0, fc.vocabulary_size, n).astype(np.int32) if isinstance(fc, SparseFeat) else
                          rng.rand(n).astype(np.float32)) for fc in cols}
        model = getattr(models, kind)(cols, device=device, **kw)
        g = torch.Generator(device=device).manual_seed(0)
        for k, t in model.named_weights():
            if not k.endswith("embeddings"):
                t.copy_(torch.randn(t.shape, generator=g, device=device) * (1.0 if "gate_softmax" in k else 0.05))
        staged = engine.Staged(n)
        model._stage_inputs(feed, staged)
        out = torch.empty(model.num_tasks, n, dtype=torch.float32, device=device)
        r = res["configs"][tag] = {"route": model.route(), "in_dim": model.stage_plan.in_dim}

        def hip():
            model._begin()
            model._forward(staged, 0, n, out)
        ms_hip = _time(hip, args.iters)
        r.update(forward_ms=round(ms_hip, 4), samples_per_s=round(n / (ms_hip * 1e-3)))
        model._route = "layered"
        ms_lay = _time(hip, args.iters)
        model._route = None
        r.update(layered_ms=round(ms_lay, 4), layered_samples_per_s=round(n / (ms_lay * 1e-3)))
        if not args.no_torch:
            def torch_ops():
                with torch.no_grad():
                    model.autograd_outputs(model.autograd_logits(staged, 0, n))
            ms_torch = _time(torch_ops, max(2, args.iters // 4))
            r.update(torch_ops_ms=round(ms_torch, 4), torch_ops_samples_per_s=round(n / (ms_torch * 1e-3)),
                     speedup_vs_torch_ops=round(ms_torch / ms_hip, 2))
        # ---- the first level alone, on the model's own dnn_in --------------------------------------------------------------------------
        model._begin()
        ws = model.stage_plan.run(staged, 0, n)
        lv, in_dim = model.levels[0], model.stage_plan.in_dim
        lout = torch.empty(n, len(lv.gate_dense) * lv.experts[0].hidden_units[-1], dtype=torch.float32, device=device)
        bound = n * level_flops(in_dim, lv) / (MFMA_F32_TFLOPS * 1e12) * 1e3
        r["level_bound_ms"] = round(bound, 4)
        r["level_layered_ms"] = round(_time(lambda: model._level_call(lv, ws["dnn_in"], in_dim, [0], out=lout, route="layered"), args.iters), 4)
        if r["route"] == "fused":
            from deepctr_amd import ops
            for rows in (0, 16, 32, 64):
                kwl = model._dnn_kw(lv.experts, "expert_")
                ms = _time(lambda: ops.mtl_level(ws["dnn_in"], in_dim, [0], [d.kernels for d in lv.experts], [d.biases for d in lv.experts],
                                                 [gd.w('kernel') for gd in lv.gate_dense], lv.members, expert_src=lv.expert_src,
                                                 gate_src=lv.gate_src, out=lout, tile_rows=rows, **kwl), args.iters)
                r["level_fused_ms_rows%d" % rows] = round(ms, 4)
            r["level_share_of_bound"] = round(bound / r["level_fused_ms_rows0"], 3)
        r.update(mix_bwd_time(model, ws["dnn_in"], n, args.iters))
        if args.train_rows:
            r["train"] = train_times(model, cols, args.train_rows, args.iters, not args.no_torch, rng)
        del model
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
