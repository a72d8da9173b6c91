"""Optimizer-launch lab: every rule of deepctr_amd.optimizers on dctr_opt_apply, beside the dctr_opt_multi ADAM launch it is measured
against, over DeepFM's Criteo segment list (26 tables of 1e5 x 16 + the linear tables + the DNN; batch 4096).

The gradient buffers and touched maps are what one real backward pass leaves (HipTrainer.step(apply=False)); the timed launches run
with zero_grad off so that every one of them meets that same state (a real step also clears the touched groups, about a tenth of
all groups at this batch).  Per rule: device-event time of a window of launches, the median over rounds that alternate with the baseline, and
the bytes the launch has to move — w and every state slot read and written, the touched bytes read, g read where touched — as a rate.
Then Adam / Adagrad / RMSprop / SGD on both entry points, pair by pair, without and with the l2 penalty sum.
Not read by bench.py.      python scripts/bench_optimizers.py [--rounds 7] [--reps 200] [--own-slots]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deepctr_amd import models, ops, optimizers  # noqa: E402
from deepctr_amd.feature_column import DenseFeat, SparseFeat  # noqa: E402
from deepctr_amd.training_hip import HipTrainer  # noqa: E402

RULES = [
    ("SGD", dict()), ("SGD", dict(momentum=0.9, nesterov=True)), ("Adagrad", dict()), ("RMSprop", dict()),
    ("RMSprop", dict(centered=True)), ("RMSprop", dict(momentum=0.5, centered=True)), ("Adam", dict()), ("Adam", dict(amsgrad=True)),
    ("Adam", dict(clipvalue=0.01)), ("Adam", dict(global_clipnorm=1.0)), ("Adamax", dict()), ("Adadelta", dict()),
    ("Ftrl", dict(l1_regularization_strength=1e-4)), ("Ftrl", dict(learning_rate_power=-0.3)),
]


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--own-slots", action="store_true", help="pair table: dctr_opt_apply on state slots of its own, not on dctr_opt_multi's m / v")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(0)
    cols = [SparseFeat("C%d" % i, 100000, 16) for i in range(1, 27)] + [DenseFeat("I%d" % i, 1) for i in range(1, 14)]
    model = models.DeepFM(cols, cols, device=dev)
    tr = HipTrainer(model)                      # the name path: dctr_adam_seg_t segments, m and v
    B = args.batch
    feed = {"C%d" % i: rng.randint(0, 100000, B).astype(np.int32) for i in range(1, 27)}
    feed.update({"I%d" % i: rng.rand(B).astype(np.float32) for i in range(1, 14)})
    y = torch.from_numpy((rng.rand(B) > 0.5).astype(np.float32)).to(dev)
    tr.step(model.stage(feed), 0, B, y, apply=False)
    torch.cuda.synchronize()
    n = sum(p.w.numel() for p in tr.params)
    groups = sum(p.w.numel() // 4 if p.touched is None else int(p.touched.sum()) for p in tr.params)       # 16-byte groups of g read
    marks = sum(0 if p.touched is None else p.touched.numel() for p in tr.params)
    print("%d segments, %.1f M parameters, %.1f %% of the gradient groups touched by a batch of %d"
          % (len(tr.params), n / 1e6, 100.0 * groups / (n / 4), B), flush=True)

    def bytes_of(slots, clip_pass=False):
        b = n * 8 * (1 + slots) + groups * 16 + marks
        return b + (groups * 16 + marks + sum(p.w.numel() * 4 for p in tr.params if p.l2)) if clip_pass else b

    def base():
        ops.opt_multi("adam", tr.segs, tr.n_segs, tr.max_n, 1e-6, zero_grad=False)
    launches = [("dctr_opt_multi ADAM (the figure to beat)", base, bytes_of(2))]
    keep = []
    for name, kw in RULES:
        opt = getattr(optimizers, name)(1e-6, **kw)
        rule = dict(opt._rule(), clipvalue=opt.clipvalue)
        slots = [[torch.full_like(p.w, v) for v in rule["slots"]] for p in tr.params]
        segs = ops.make_opt_segments([(p.w, p.g, s, p.l2, p.touched) for p, s in zip(tr.params, slots)], dev)
        clip = ops.grad_clip_workspace(segs[1], segs[2], dev) if (opt.clipnorm or opt.global_clipnorm) else None
        keep.append((slots, segs, clip))

        def run(opt=opt, rule=rule, segs=segs, clip=clip):
            if clip is not None:
                ops.grad_clip_scales(segs[0], segs[1], segs[2], opt.global_clipnorm or opt.clipnorm, clip[0], clip[1],
                                     global_norm=opt.global_clipnorm is not None)
            ops.opt_apply(rule, segs[0], segs[1], segs[2], opt._step_lr(1), zero_grad=False, clip_scale=None if clip is None else clip[1])
        label = "%s(%s)" % (name, ", ".join("%s=%r" % kv for kv in kw.items()))
        launches.append(("dctr_opt_apply %s: %d slot(s)%s" % (label, len(rule["slots"]), " + clip pre-pass" if clip else ""), run,
                         bytes_of(len(rule["slots"]), clip is not None)))
    for _, fn, _ in launches:                   # warm-up: code objects, every buffer touched once
        window(fn, 3)
    times = [[] for _ in launches]
    for _ in range(args.rounds):                # alternate: every launch once per round, the baseline among them
        for i, (_, fn, _) in enumerate(launches):
            times[i].append(window(fn, args.reps))
    ref = statistics.median(times[0])
    for (label, _, nbytes), ts in zip(launches, times):
        med = statistics.median(ts)
        print("%-78s %7.1f us (min %7.1f, max %7.1f)  %6.1f MB  %5.2f TB/s  x%.3f of the baseline"
              % (label, med, min(ts), max(ts), nbytes / 1e6, nbytes / med / 1e6, med / ref), flush=True)

    # The four kinds both entry points have, pair by pair, without and with the l2 penalty sum fit() asks of every launch.  The old
    # launch and the new one alternate within a round, by default on the SAME buffers (the name path's m / v): where a buffer lies
    # moves a launch by more than the two entry points differ — the last row, the old launch against itself on a second set of m / v,
    # says by how much.  "spread" is (max - min) / median of the old launch's own rounds; a pair holds when the new launch is slower
    # by no more than that, and never by more than 3 % (what two machines differ by).
    pen = torch.zeros(1, dtype=torch.float64, device=dev)
    pairs = []
    for kind, cls, b1, b2 in (("adam", "Adam", 0.9, 0.999), ("adagrad", "Adagrad", 0.0, 0.0), ("rmsprop", "RMSprop", 0.0, 0.9),
                              ("sgd", "SGD", 0.0, 0.0)):
        rule = dict(getattr(optimizers, cls)(1e-6)._rule(), clipvalue=None)
        if args.own_slots:
            slots = [[torch.full_like(p.w, v) for v in rule["slots"]] for p in tr.params]
        else:
            slots = [{2: [p.m, p.v], 1: [p.v], 0: []}[len(rule["slots"])] for p in tr.params]
        segs = ops.make_opt_segments([(p.w, p.g, s, p.l2, p.touched) for p, s in zip(tr.params, slots)], dev)
        keep.append((slots, segs))
        for with_pen in (False, True):
            pk = dict(penalty=pen, penalty_scale=float(B)) if with_pen else {}

            def old(kind=kind, b1=b1, b2=b2, pk=pk):
                ops.opt_multi(kind, tr.segs, tr.n_segs, tr.max_n, 1e-6, b1, b2, 1e-7, zero_grad=False, **pk)

            def new(rule=rule, segs=segs, pk=pk):
                ops.opt_apply(rule, segs[0], segs[1], segs[2], 1e-6, zero_grad=False, **pk)
            pairs.append(("%s%s" % (kind, " + penalty" if with_pen else ""), len(rule["slots"]), old, new))
    mv2 = [(torch.zeros_like(p.w), torch.zeros_like(p.w)) for p in tr.params]
    segs2 = ops.make_adam_segments([(p.w, m, v, p.g, p.l2, p.touched) for p, (m, v) in zip(tr.params, mv2)], dev)
    pairs.append(("adam: old vs old", 2, pairs[0][2],
                  lambda: ops.opt_multi("adam", segs2[0], segs2[1], segs2[2], 1e-6, 0.9, 0.999, 1e-7, zero_grad=False)))
    for _, _, old, new in pairs:
        window(old, 3), window(new, 3)
    pt = [([], []) for _ in pairs]
    for _ in range(args.rounds):
        for (_, _, old, new), (to, tn) in zip(pairs, pt):
            to.append(window(old, args.reps))
            tn.append(window(new, args.reps))
    print("\nthe new launch on %s" % ("state slots of its own" if args.own_slots else "the old launch's own m / v"))
    print("pair                  slots   dctr_opt_multi us (min, max, spread)   dctr_opt_apply us (min, max)   new / old   margin   verdict")
    for (label, ns, _, _), (to, tn) in zip(pairs, pt):
        mo, mn = statistics.median(to), statistics.median(tn)
        spread = (max(to) - min(to)) / mo
        margin = min(spread, 0.03)
        print("%-21s %5d   %7.1f (%7.1f, %7.1f, %5.2f %%)          %7.1f (%7.1f, %7.1f)       %6.3f   %5.2f %%   %s"
              % (label, ns, mo, min(to), max(to), 100 * spread, mn, min(tn), max(tn), mn / mo, 100 * margin,
                 "ok" if mn <= mo * (1 + margin) else "MISS"), flush=True)

if __name__ == "__main__":
    main()
