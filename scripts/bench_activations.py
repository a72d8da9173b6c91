"""What the tf.keras activation names of the DNN (elu, selu, softplus, softsign, exponential, hard_sigmoid, swish, gelu) cost beside
relu, on the DeepFM of BASELINE configs[1] (26 sparse features of 16 + 13 dense, DNN 256-128-64) at 4096 rows.  A measurement, no
gate; every figure is taken beside relu's in the same process.
  forward   the DNN launch (dctr_mlp_fwd with the head) over a materialised [4096, 429] input on the tile route (tile_rows 32)
  step      HipTrainer.step (forward, loss gradient, backward, Adam over every parameter) of the model built with that name
  mlp_bwd   dctr_mlp_bwd alone: the chained form (act' from the outputs) and, for swish / gelu, the layer-by-layer form with the forward's
            saved pre-activations and with the recompute GEMM
Each figure: the median of --repeats event-timed runs of --iters launches (microseconds per launch / step)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deepctr_amd import models, ops  # noqa: E402
from deepctr_amd.feature_column import DenseFeat, SparseFeat  # noqa: E402
from deepctr_amd.training_hip import HipTrainer  # noqa: E402

NAMES = ("relu", "elu", "selu", "softplus", "softsign", "exponential", "hard_sigmoid", "swish", "gelu")


def timed(fn, iters, repeats):
    for _ in range(max(4, iters // 8)):
        fn()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / iters)
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-step", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(0)
    B, dims = args.batch, [429, 256, 128, 64]
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)      # noqa: E731
    x = f32(rng.standard_normal((B, 432)))
    ks = [f32(rng.standard_normal((k, n)) / np.sqrt(k)) for k, n in zip(dims[:-1], dims[1:])]
    bs = [f32(rng.standard_normal(n) * 0.1) for n in dims[1:]]
    hw, dl = f32(rng.standard_normal(dims[-1]) * 0.1), f32(rng.standard_normal(B))
    y = torch.empty(B, device=dev)
    acts = [torch.empty(B, n, device=dev) for n in dims[1:]]
    pre = [torch.empty(B, n, device=dev) for n in dims[1:]]
    dk, db, dhw = [torch.zeros_like(k) for k in ks], [torch.zeros_like(b) for b in bs], torch.zeros_like(hw)
    dx = torch.empty(B, 432, device=dev)
    rows = {}
    for name in NAMES:
        r = rows[name] = {}
        r["forward"] = timed(lambda: ops.mlp(x, ks, bs, name, head_w=hw, in_dim=dims[0], out=y, tile_rows=32), args.iters, args.repeats)
        ops.mlp(x, ks, bs, name, head_w=hw, in_dim=dims[0], out=y, save_acts=acts)
        ws = {}
        kw = dict(biases=bs) if name in ("swish", "gelu") else {}
        r["mlp_bwd"] = timed(lambda: ops.mlp_bwd(x, dims[0], ks, acts, name, hw, dl, dk, db, dhw, dx=dx, workspace=ws, **kw), args.iters, args.repeats)
        if name in ("swish", "gelu"):
            xin, kin = x, dims[0]
            for l in range(len(ks)):                      # the forward's pre-activations, as HipTrainer keeps them
                ops.mlp(xin, [ks[l]], [bs[l]], "linear", in_dim=kin, out=pre[l])
                ops.dnn_train_layer(pre[l], name, h=acts[l])
                xin, kin = acts[l], dims[l + 1]
            r["mlp_bwd saved_z"] = timed(lambda: ops.mlp_bwd(x, dims[0], ks, acts, name, hw, dl, dk, db, dhw, dx=dx, workspace=ws, biases=bs,
                                                             saved_z=pre), args.iters, args.repeats)
    if not args.skip_step:
        cols = [SparseFeat("C%d" % i, 100000, 16) for i in range(1, 27)] + [DenseFeat("I%d" % i, 1) for i in range(1, 14)]
        ring = 8
        n = ring * B
        feed = {"C%d" % i: rng.randint(0, 100000, n).astype(np.int32) for i in range(1, 27)}
        feed.update({"I%d" % i: rng.rand(n).astype(np.float32) for i in range(1, 14)})
        yt = torch.from_numpy((rng.rand(n) > 0.5).astype(np.float32)).to(dev)
        for name in NAMES:
            model = models.DeepFM(cols, cols, dnn_activation=name, device=dev)
            tr = HipTrainer(model)
            staged = model.stage(feed)
            state = {"i": 0}

            def step():
                lo = (state["i"] % ring) * B
                state["i"] += 1
                tr.step(staged, lo, lo + B, yt[lo:lo + B])
            rows[name]["step"] = timed(step, max(8, args.iters // 2), args.repeats)
            del tr, model, staged
    print("%s, %d rows, DNN %s; microseconds, (x relu)" % (torch.cuda.get_device_name(0), B, "-".join(str(d) for d in dims)))
    cols_ = ["forward", "mlp_bwd", "mlp_bwd saved_z"] + ([] if args.skip_step else ["step"])
    print("| activation | " + " | ".join(cols_) + " |")
    print("|---|" + "---|" * len(cols_))
    for name in NAMES:
        cells = []
        for c in cols_:
            v = rows[name].get(c)
            base = rows["relu"].get(c if c != "mlp_bwd saved_z" else "mlp_bwd")
            cells.append("—" if v is None else "%.1f (%.2f)" % (v, v / base))
        print("| %s | %s |" % (name, " | ".join(cells)))


if __name__ == "__main__":
    main()
