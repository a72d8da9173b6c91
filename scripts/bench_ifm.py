"""IFM and DIFM at the reference defaults on Criteo-shaped input (26 sparse fields of vocabulary 1e5 + 13 bucketised fields, 39 fields of
embedding_dim 4; DNN 256-128-64; DIFM: 8 heads of 8): samples/s of the whole forward (staged ids -> probabilities: fused gather,
(attention,) DNN kernel, dctr_ifm_fwd) beside the same model's torch-ops forward (training.model_logits under no_grad), device-event
timing after warm-up, then dctr_ifm_fwd alone on each route beside its HBM-byte bound — for DIFM with both factor sources projected in
the launch (the form the model uses), and beside the alternative (dctr_sgemm for the K = 2,496 product, handed over as m').  Prints one JSON line.

    python scripts/bench_ifm.py [--rows 4096,65536] [--iters 20]

With ``--train-rows`` it measures the training side instead (profiles/ifm_bwd.txt keeps the line), per model and row count, ``--runs``
times over:
  * dctr_ifm_bwd alone with the outputs the autograd step asks for (dx, dterms, both sources' dact and dkernel; dm' in the workspace)
    beside its byte bound — per sample the x, m, terms and act reads and the dx, dterms, dm' and dact writes at 6.0 TB/s;
  * the dkernel pass's share: the same call without the dkernel outputs, and the difference;
  * one step of fit()'s autograd path (forward, BCE on the logit, backward over every weight; no optimizer) with
    training.HIP_AUTOGRAD_OPS off (torch ops throughout), with the switch on and this op kept off behind its row threshold (the
    baseline the threshold is read against: DIFM's attention stack is already a HIP op there), and with the op on.

    python scripts/bench_ifm.py --train-rows 4096,65536 [--iters 20] [--runs 2]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_TBPS = 6.0               # achievable streaming rate the bound is quoted at


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


def train_leg(model, kind, cols, n, iters, F, d):
    from deepctr_amd import engine, ops, training
    device = model.device
    rng = np.random.RandomState(1)
    feed = {fc.name: rng.randint(0, fc.vocabulary_size, n).astype(np.int32) for fc in cols}
    staged = engine.Staged(n)
    model._stage_inputs(feed, staged)
    model._begin()
    ws, bufs, add, desc = model._stage_run(staged, 0, n)
    hidden = model._dnn_hidden(ws, bufs)
    if kind == "IFM":
        sources = [(hidden, model.dense.w("kernel"))]
    else:
        ops.interacting(ws["dnn_in"], [model.att.weights_qkvr], model.att_embedding_size, model.att_head_num, model.att_res, True,
                        fields=F, dim=d, out=bufs["att"])
        sources = [(bufs["att"], model.dense.w("kernel")), (hidden, model.dense_1.w("kernel"))]
    Ks = [int(a.shape[1]) for a, _ in sources]
    x = ws["dnn_in"]
    with torch.no_grad():
        terms = model.linear_terms(staged, 0, n).contiguous()
    factor = torch.empty(n, F, dtype=torch.float32, device=device)
    ops.ifm(x, F, d, sources=sources, softmax=kind == "IFM", lin=(None,) * F, lin_desc=ops._ifm_term_columns(terms, F), factor_out=factor)
    d_out = torch.randn(n, device=device) / n
    dx = torch.empty(n, F * d, dtype=torch.float32, device=device)
    dterms = torch.empty(n, F, dtype=torch.float32, device=device)
    dact = [torch.empty(n, K, dtype=torch.float32, device=device) for K in Ks]
    dkernel = [torch.empty(K, F, dtype=torch.float32, device=device) for K in Ks]
    # per sample: x, m, terms and act read; dx, dterms, dm' and dact written
    bwd_bytes = (F * d + F + F + sum(Ks)) * 4 + (F * d + F + F + sum(Ks)) * 4
    bound_ms = bwd_bytes * n / (HBM_TBPS * 1e12) * 1e3

    def bwd(with_dkernel=True):
        ops.ifm_bwd(x, F, d, factor, d_out, sources=sources, terms=terms, softmax=kind == "IFM", dx=dx, dterms=dterms, dact=dact,
                    dkernel=dkernel if with_dkernel else None)

    ms_full, ms_rest = _time(bwd, iters), _time(lambda: bwd(False), iters)
    r = {"factor_K": Ks, "ifm_bwd_bytes_per_sample": bwd_bytes, "ifm_bwd_bound_ms": round(bound_ms, 5), "ifm_bwd_ms": round(ms_full, 5),
         "ifm_bwd_share_of_bound": round(bound_ms / ms_full, 3), "ifm_bwd_without_dkernel_ms": round(ms_rest, 5),
         "dkernel_pass_ms": round(ms_full - ms_rest, 5), "dkernel_pass_share": round((ms_full - ms_rest) / ms_full, 3),
         "workspace_bytes": ops.ifm_bwd_workspace_bytes(n, F, d, Ks)}
    # ---- the autograd step ---------------------------------------------------------------------------------------------------------
    y = (torch.rand(n, device=device) > 0.5).float()
    params = [t_ for k_, t_ in model.named_weights() if "moving_" not in k_]

    def step():
        model._begin()
        loss = torch.nn.functional.binary_cross_entropy_with_logits(training.model_logits(model, staged, 0, n, training=True), y)
        for t_ in params:
            t_.grad = None
        loss.backward()
        return loss

    def switched(switch, op):
        def run():
            training.HIP_AUTOGRAD_OPS = switch
            # the op is timed at every row count (the threshold is read off this table), or kept off behind an unreachable threshold
            training.IFM_HIP_MIN_ROWS = training.DIFM_HIP_MIN_ROWS = 0 if op else 1 << 62
            return step()
        return run

    # "switch_off": every differentiable HIP op off; "op_off": the switch on (DIFM's attention stack is ops.InteractingFunction) with
    # this op kept off — the baseline of the threshold; "op_on": the switch on and the op taken
    legs = {"switch_off": switched(False, False), "op_off": switched(True, False), "op_on": switched(True, True)}
    min_rows = training.IFM_HIP_MIN_ROWS, training.DIFM_HIP_MIN_ROWS
    try:
        for t_ in params:
            t_.requires_grad_(True)
        ms = {k: _time(fn, iters) for k, fn in legs.items()}
        losses = {k: float(fn().detach()) for k, fn in legs.items()}
    finally:
        training.HIP_AUTOGRAD_OPS = True
        training.IFM_HIP_MIN_ROWS, training.DIFM_HIP_MIN_ROWS = min_rows
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
    ap.add_argument("--rows", default="4096,65536")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch-ops forward")
    ap.add_argument("--train-rows", default=None, help="measure dctr_ifm_bwd and the autograd step at these row counts instead")
    ap.add_argument("--runs", type=int, default=2, help="--train-rows: repeat the whole measurement this many times")
    args = ap.parse_args()
    device = torch.device("cuda:0")
    V, F, d = 100000, 39, 4
    cols = [SparseFeat("C%d" % i, V, d) for i in range(26)] + [SparseFeat("I%d" % i, 64, d) for i in range(13)]
    res = {"fields": F, "dim": d, "vocabulary": V, "models": {}}
    if args.train_rows:
        res.update(iters=args.iters, warmup=3, hbm_tbps=HBM_TBPS, runs=[])
        del res["models"]
        for _ in range(args.runs):
            run = {}
            for kind in ("IFM", "DIFM"):
                model = getattr(models, kind)(cols, cols, device=device)
                g = torch.Generator(device=device).manual_seed(0)
                for k, t in model.named_weights():
                    t.copy_(torch.randn(t.shape, generator=g, device=device) * (0.3 if k.endswith("embeddings") else 0.1))
                run[kind] = {}
                for n in [int(r) for r in args.train_rows.split(",")]:
                    run[kind][str(n)] = train_leg(model, kind, cols, n, args.iters, F, d)
                    print("%s n=%d: %s" % (kind, n, json.dumps(run[kind][str(n)])), file=sys.stderr, flush=True)
                del model
                torch.cuda.empty_cache()
            res["runs"].append(run)
        print(json.dumps(res))
        return
    for kind in ("IFM", "DIFM"):
        rng = np.random.RandomState(0)
        model = getattr(models, kind)(cols, cols, device=device)
        g = torch.Generator(device=device).manual_seed(0)
        for k, t in model.named_weights():
            t.copy_(torch.randn(t.shape, generator=g, device=device) * (0.3 if k.endswith("embeddings") else 0.1))
        Ks = [64] if kind == "IFM" else [model.att_out_dim, 64]
        # dctr_ifm_fwd per sample: the embeddings, the factor sources, F linear weights gathered (a 64-B sector each) and F ids, one float out
        hbm_b = F * d * 4 + sum(Ks) * 4 + F * (64 + 4) + 4
        flop = sum(2 * K * F for K in Ks) + 4 * F * d + 2 * F
        out_m = res["models"][kind] = {"factor_K": Ks, "ifm_hbm_bytes_per_sample": hbm_b, "ifm_flop_per_sample": flop,
                                       "kernel_bytes_from_l2_per_16_samples": sum(K * F * 4 for K in Ks), "rows": {}}
        for n in [int(r) for r in args.rows.split(",")]:
            feed = {fc.name: rng.randint(0, fc.vocabulary_size, n).astype(np.int32) for fc in cols}
            staged = engine.Staged(n)
            model._stage_inputs(feed, staged)
            out = torch.empty(n, dtype=torch.float32, device=device)
            r = out_m["rows"][str(n)] = {"ifm_route": ops.ifm_route(n, F, d, len(Ks))}

            def hip():
                model._begin()
                model._forward(staged, 0, n, out)
            ms_hip = _time(hip, args.iters)
            r.update(forward_ms=round(ms_hip, 4), samples_per_s=round(n / (ms_hip * 1e-3)))
            if kind == "DIFM":          # the same forward with the vector-wise product on dctr_sgemm in front, handed over as m'
                model.vector_part_in_kernel = False
                r["forward_gemm_in_front_ms"] = round(_time(hip, args.iters), 4)
                model.vector_part_in_kernel = True
            if not args.no_torch:
                def torch_ops():
                    with torch.no_grad():
                        training.model_logits(model, staged, 0, n)
                ms_torch = _time(torch_ops, max(2, args.iters // 5))
                r.update(torch_ops_ms=round(ms_torch, 4), torch_ops_samples_per_s=round(n / (ms_torch * 1e-3)),
                         speedup_vs_torch_ops=round(ms_torch / ms_hip, 2))
            ws, bufs, add, desc = model._stage_run(staged, 0, n)
            hidden = model._dnn_hidden(ws, bufs)
            if kind == "IFM":
                sources = [(hidden, model.dense.w("kernel"))]
            else:
                ops.interacting(ws["dnn_in"], [model.att.weights_qkvr], model.att_embedding_size, model.att_head_num, model.att_res, True,
                                fields=F, dim=d, out=bufs["att"])
                sources = [(bufs["att"], model.dense.w("kernel")), (hidden, model.dense_1.w("kernel"))]
            bound_ms = hbm_b * n / (HBM_TBPS * 1e12) * 1e3
            r["ifm_bound_ms"] = round(bound_ms, 4)
            for route in ("auto", "workspace"):
                def ifm():
                    ops.ifm(ws["dnn_in"], F, d, sources=sources, softmax=kind == "IFM", lin=model.lin_positions, lin_desc=desc, add=add,
                            global_bias=model.prediction.w("global_bias"), sigmoid_out=True, out=out, route=route)
                ms = _time(ifm, args.iters)
                key = "ifm_lds" if route == "auto" else "ifm_workspace"
                r[key + "_ms"] = round(ms, 4)
                r[key + "_share_of_bound"] = round(bound_ms / ms, 3)
                r[key + "_tflops"] = round(flop * n / (ms * 1e-3) / 1e12, 3)
            if kind == "DIFM":
                # the alternative: the large-K product on the training step's GEMM, handed over as m'
                mp = torch.zeros(n, F, dtype=torch.float32, device=device)

                def gemm_then_ifm():
                    ops.sgemm(bufs["att"], model.dense.w("kernel"), out=mp)
                    ops.ifm(ws["dnn_in"], F, d, sources=sources[1:], mprime=mp, lin=model.lin_positions, lin_desc=desc, add=add,
                            global_bias=model.prediction.w("global_bias"), sigmoid_out=True, out=out)
                r["gemm_then_ifm_ms"] = round(_time(gemm_then_ifm, args.iters), 4)
        del model
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
