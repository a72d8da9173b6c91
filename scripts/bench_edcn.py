"""EDCN at Criteo's sparse shape (26 SparseFeat of embedding_dim 16: D = 416, vocabulary 1e5), cross_num 2, for every bridge type and
both cross parameterizations: samples/s of the whole forward (staged ids -> probabilities: fused gather, ops.edcn) beside the same
model's torch-ops forward (training.model_logits under no_grad) and beside the layered route of ops.edcn; and dctr_edcn_fwd alone (the
model's logit form, on the model's own dnn_in) beside its f32-MFMA bound.  The bound is arithmetic, not a measurement: per row and round
2 D^2 FLOP for the DNN, + 2 D^2 for a matrix cross, + 4 D^2 for the concatenation bridge, at 157.3 TFLOP/s.  attention_pooling has no
fused route: its forward IS the layered one.  Device-event timing after warm-up.  Prints one JSON line.

With ``--train-rows`` it measures the training side instead (profiles/edcn_bwd.txt keeps the output), per supported bridge x
parameterization and row count, ``--runs`` times over in one call:
  * dctr_edcn_train_fwd and dctr_edcn_bwd alone (every gradient the autograd step asks for) beside the backward's f32-MFMA bound: twice the
    forward's products plus the recomputed u, i.e. per row and round 4 D^2 FLOP for the DNN, 4 D^2 (+ 2 D^2) for a matrix cross and
    8 D^2 for the concatenation bridge, at 157.3 TFLOP/s;
  * the weight-gradient pass's share: dctr_edcn_bwd with and without the [D, D] / [2D, D] gradients;
  * one step of fit()'s autograd path (forward, BCE on the logit, backward over every weight; no optimizer) with the op off (behind an
    unreachable training.EDCN_HIP_MIN_ROWS) and on at every row count.

    python scripts/bench_edcn.py [--rows 65536] [--iters 20]
    python scripts/bench_edcn.py --train-rows 4096,65536 [--iters 20] [--runs 2]"""
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


def bwd_flops(D, cross_num, bridge_type, parameterization):
    per = 4 * D * D + (6 * D * D if parameterization == "matrix" else 0) + (8 * D * D if bridge_type == "concatenation" else 0)
    return cross_num * per


def train_leg(model, feed, n, iters, bridge_type, par):
    from deepctr_amd import engine, ops, training
    device = model.device
    F, d, D, L = model.n_fields, model.emb_dim, model.cross_dim, model.cross_num
    staged = engine.Staged(n)
    model._stage_inputs(feed, staged)
    (gates, cw, cb, dw, db), tkw = model._tower_args()
    kw = dict(bridge_type=bridge_type, parameterization=par, tau=model.tau, activation=tkw["activation"], bridge_weights=tkw["bridge_weights"],
              bridge_activation=tkw["bridge_activation"], head_w=model.dense.w("kernel"))
    x = torch.randn(n, D, device=device) * 0.05
    d_logit = torch.randn(n, device=device)
    logit = torch.empty(n, device=device)
    tape = torch.empty(L, n, 3 * D, device=device)
    concat = bridge_type == "concatenation"
    ms_fwd = _time(lambda: ops.edcn_train(x, F, d, gates, cw, cb, dw, db, logit=logit, tape=tape, **kw), iters)
    dx = torch.empty(n, D, device=device)
    like = lambda ws: [torch.empty_like(w) for w in ws]       # noqa: E731
    small = dict(dx=dx, d_gates=like(gates), d_cross_b=like(cb), d_dnn_b=like(db), d_head_w=True)
    big = dict(d_dnn_w=like(dw))
    if par == "matrix":
        big["d_cross_w"] = like(cw)
    else:
        small["d_cross_w"] = like(cw)
    if concat:
        small["d_bridge_b"] = like([b[1] for b in tkw["bridge_weights"]])
        big["d_bridge_w"] = like([b[0] for b in tkw["bridge_weights"]])
    ms_full = _time(lambda: ops.edcn_bwd(x, F, d, gates, cw, cb, dw, db, tape, d_logit=d_logit, **dict(kw, **dict(small, **big))), iters)
    ms_rest = _time(lambda: ops.edcn_bwd(x, F, d, gates, cw, cb, dw, db, tape, d_logit=d_logit, **dict(kw, **small)), iters)
    bound = n * bwd_flops(D, L, bridge_type, par) / (MFMA_F32_TFLOPS * 1e12) * 1e3
    r = {"edcn_train_fwd_ms": round(ms_fwd, 4), "edcn_bwd_ms": round(ms_full, 4), "edcn_bwd_bound_ms": round(bound, 4),
         "edcn_bwd_share_of_bound": round(bound / ms_full, 3), "edcn_bwd_without_weight_grads_ms": round(ms_rest, 4),
         "weight_grad_pass_share": round((ms_full - ms_rest) / ms_full, 3),
         "workspace_bytes": ops.edcn_bwd_workspace_bytes(n, F, d, L, bridge_type, par, tkw["activation"], tkw["bridge_activation"])}
    y = (torch.rand(n, device=device) > 0.5).float()
    params = [t_ for k_, t_ in model.named_weights() if "moving_" not in k_]

    def step():
        model._begin()
        loss = torch.nn.functional.binary_cross_entropy_with_logits(training.model_logits(model, staged, 0, n, training=True), y)
        for t_ in params:
            t_.grad = None
        loss.backward()
        return loss

    def switched(op):
        def run():
            # the op is timed at every row count (the thresholds are read off this table), or kept off behind an unreachable threshold
            training.EDCN_HIP_MIN_ROWS, training.EDCN_HIP_MAX_ROWS = (0, 1 << 62) if op else (1 << 62, 1 << 62)
            return step()
        return run

    legs = {"op_off": switched(False), "op_on": switched(True)}
    min_rows = training.EDCN_HIP_MIN_ROWS, training.EDCN_HIP_MAX_ROWS
    try:
        for t_ in params:
            t_.requires_grad_(True)
        ms = {k: _time(fn, iters) for k, fn in legs.items()}
        losses = {k: float(fn().detach()) for k, fn in legs.items()}
    finally:
        training.EDCN_HIP_MIN_ROWS, training.EDCN_HIP_MAX_ROWS = min_rows
        for t_ in params:
            t_.requires_grad_(False)
            t_.grad = None
    for k in legs:
        r["step_ms_" + k] = round(ms[k], 4)
        r["loss_" + k] = losses[k]
    r["step_speedup_op_on_vs_op_off"] = round(ms["op_off"] / ms["op_on"], 3)
    return r


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
    ap.add_argument("--train-rows", default=None, help="measure dctr_edcn_train_fwd / dctr_edcn_bwd and the autograd step at these row counts instead")
    ap.add_argument("--runs", type=int, default=2, help="--train-rows: repeat the whole measurement this many times")
    args = ap.parse_args()
    device = torch.device("cuda:0")
    cols = [SparseFeat("C%d" % i, 100000, args.dim) for i in range(args.fields)]
    D = args.fields * args.dim
    if args.train_rows:
        res = {"mfma_f32_tflops": MFMA_F32_TFLOPS, "fields": args.fields, "dim": args.dim, "cross_num": args.cross_num, "runs": []}
        rng = np.random.RandomState(0)
        for _ in range(args.runs):
            run = {}
            for n in [int(r) for r in args.train_rows.split(",")]:
                feed = {fc.name: rng.randint(0, fc.vocabulary_size, n).astype(np.int32) for fc in cols}
                for bridge_type in BRIDGES[:3]:
                    for par in ("vector", "matrix"):
                        model = models.EDCN(cols, cols, cross_num=args.cross_num, cross_parameterization=par, bridge_type=bridge_type,
                                            device=device)
                        run["%s/%s/%d" % (bridge_type, par, n)] = train_leg(model, feed, n, args.iters, bridge_type, par)
                        print("%s/%s/%d %s" % (bridge_type, par, n, json.dumps(run["%s/%s/%d" % (bridge_type, par, n)])), flush=True)
                        del model
                        torch.cuda.empty_cache()
            res["runs"].append(run)
        print(json.dumps(res))
        return
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
