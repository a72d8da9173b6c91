"""What the four multi-task models share: a list of outputs on the tf.keras surface (MultiTaskModel) and the expert / gate / tower
stack on ``ops.mtl_level`` / ``ops.mtl_towers``."""
import numpy as np
import torch

from ... import ops
from ... import training as tops
from ...engine import EmbeddingStage, Staged, on_model_device
from ...layers.activation import require_base_activation
from ...layers.core import DNN, Dense, PredictionLayer
from .._common import FeatureModel

_BCE = ("binary_crossentropy", "logloss", "bce")
_MSE = ("mse", "mean_squared_error")


def check_tasks(task_types, task_names, need_many=True):
    """The argument checks the reference's SharedBottom / MMOE / PLE open with (mmoe.py:42-53)."""
    num_tasks = len(task_names)
    if need_many and num_tasks <= 1:
        raise ValueError("num_tasks must be greater than 1")
    if len(task_types) != num_tasks:
        raise ValueError("num_tasks must be equal to the length of task_types")
    for task_type in task_types:
        if task_type not in ['binary', 'regression']:
            raise ValueError("task must be binary or regression, {} is illegal".format(task_type))


class Level(object):
    """One expert / gate level: DNN layers of the experts and the gates, the gates' softmax Dense, and the wiring of ops.mtl_level."""

    def __init__(self, experts, expert_src, gate_dnns, gate_dense, gate_src, members, n_slots):
        self.experts, self.expert_src, self.gate_dnns, self.gate_dense = experts, expert_src, gate_dnns, gate_dense
        self.gate_src, self.members, self.n_slots = gate_src, members, n_slots


class MultiTaskModel(FeatureModel):
    """A model with one output per task, as tf.keras gives it for ``Model(outputs=[...])``: predict() returns a list of T arrays
    [N, 1] in ``task_names`` order; compile() / fit() / evaluate() take one loss, loss weight and label array per task (a list, or a
    dict keyed by task name).  The single-output paths of engine.Model are not used."""

    def __init__(self, name, dnn_feature_columns, device, task_types, task_names):
        super(MultiTaskModel, self).__init__(name, list(dnn_feature_columns), device, "binary")
        self.task_types, self.task_names = list(task_types), list(task_names)
        self.num_tasks = len(self.task_names)
        self.levels, self.bottom, self.esmm = [], None, False
        self._want_logits = False

    # ---- construction helpers ------------------------------------------------------------------------------------------------------
    def _build_inputs(self, dnn_feature_columns, seed):
        self.linear_tables, self.linear = {}, None
        self.build_embeddings(dnn_feature_columns, seed)
        self.stage_plan = EmbeddingStage(self.tables, {}, [], dnn_feature_columns, device=self.device)
        self.dnn = None
        self.dnn_layers = []            # every DNN of the model: training.regularized_weights applies l2_reg_dnn to their kernels
        return self.stage_plan.in_dim

    def _dnn(self, units, in_dim, name=None):
        kw = {} if name is None else {"name": name}
        # the expert / gate level and tower kernels (dctr_mtl_*) read the activation code themselves
        require_base_activation(type(self).__name__, self._dnn_cfg["activation"])
        d = self._add(DNN(tuple(units), self._dnn_cfg["activation"], self._dnn_cfg["l2"], self._dnn_cfg["dropout"], self._dnn_cfg["bn"],
                          seed=self._dnn_cfg["seed"], device=self.device, **kw).build_for(in_dim))
        self.dnn_layers.append(d)
        return d

    def _build_towers(self, tower_units, in_dim, names=None, prediction_names=None):
        """Per task: DNN(tower_units), Dense(1, use_bias=False), PredictionLayer — the reference's creation order (mmoe.py:86-94)."""
        self.towers, self.heads, self.predictions = [], [], []
        last = tower_units[-1] if len(tower_units) else in_dim
        for t in range(self.num_tasks):
            self.towers.append(self._dnn(tower_units, in_dim, None if names is None else names[t]))
            self.heads.append(self._add(Dense(1, use_bias=False, device=self.device).build_for(last)))
            pname = self.task_names[t] if prediction_names is None else prediction_names[t]
            self.predictions.append(self._add(PredictionLayer(self.task_types[t], device=self.device,
                                                              **({} if pname is None else {"name": pname})).build_for()))

    # ---- forward ------------------------------------------------------------------------------------------------------------------
    def _begin(self):
        super(MultiTaskModel, self)._begin()
        self._bn = {id(d): d.bn_params() for d in self.dnn_layers if d.bn_layers}       # scale / shift follow the current weights
        self._dice = {id(d): d.dice_params() for d in self.dnn_layers if d.dice_layers}

    def _dnn_kw(self, dnns, prefix):
        kw = {}
        if any(id(d) in self._bn for d in dnns):
            kw[prefix + "bn"] = [self._bn.get(id(d)) for d in dnns]
        if any(id(d) in self._dice for d in dnns):
            kw[prefix + "dice"] = [self._dice.get(id(d)) for d in dnns]
        return kw

    def _level_call(self, lv, x, in_dim, offsets, out=None, route=None):
        kw = self._dnn_kw(lv.experts, "expert_")
        if lv.gate_dnns[0].hidden_units:
            kw.update(gate_dnn_kernels=[d.kernels for d in lv.gate_dnns], gate_dnn_biases=[d.biases for d in lv.gate_dnns])
            kw.update(self._dnn_kw(lv.gate_dnns, "gate_"))
        return ops.mtl_level(x, in_dim, offsets, [d.kernels for d in lv.experts], [d.biases for d in lv.experts],
                             [g.w('kernel') for g in lv.gate_dense], lv.members, expert_src=lv.expert_src, gate_src=lv.gate_src,
                             activation=lv.experts[0].activation, out=out, route=route, **kw)

    def _towers_call(self, x, in_dim, offsets, out, route=None):
        logits = self._want_logits
        return ops.mtl_towers(x, in_dim, offsets, [d.kernels for d in self.towers], [d.biases for d in self.towers],
                              [h.w('kernel') for h in self.heads], [p.w('global_bias') for p in self.predictions],
                              binary=[t == "binary" and not logits for t in self.task_types], activation=self.towers[0].activation,
                              esmm=self.esmm and not logits, out=out, route=route, **self._dnn_kw(self.towers, ""))

    def _stack(self, x, in_dim):
        """From the DNN input to what the towers read: (buffer, slot width, slot offset per tower)."""
        B = x.shape[0]
        offsets = [0]
        for i, lv in enumerate(self.levels):
            G, H = len(lv.gate_dense), lv.experts[0].hidden_units[-1]
            out = self._per_batch((B, i), lambda: torch.empty(B, G * H, dtype=torch.float32, device=self.device))
            self._level_call(lv, x, in_dim, offsets, out=out, route=self._route)
            x, in_dim, offsets = out, H, [g * H for g in range(G)]
        if self.bottom is not None and self.bottom.hidden_units:
            d = self.bottom
            x = ops.mlp(x, d.kernels, d.biases, d.activation, dice=self._dice.get(id(d)), bn=self._bn.get(id(d)), in_dim=in_dim)
            in_dim = d.hidden_units[-1]
        if len(offsets) == 1:
            offsets = offsets * self.num_tasks
        return x, in_dim, offsets[:self.num_tasks]

    _route = None           # "layered": force the layered route of every level and of the towers (tests, scripts/bench_mtl.py)

    def _forward(self, staged, lo, hi, out):
        ws = self.stage_plan.run(staged, lo, hi)
        x, in_dim, offsets = self._stack(ws["dnn_in"], self.stage_plan.in_dim)
        self._towers_call(x, in_dim, offsets, out, route=self._route)

    def _per_batch(self, key, alloc):
        bufs = self._buf.get(key)
        if bufs is None:
            if len(self._buf) >= 16:
                self._buf.clear()
            bufs = self._buf[key] = alloc()
        return bufs

    def route(self):
        """'fused' when every level and the towers take their one-launch route, else 'layered' (the library's answers)."""
        in_dim, act = self.stage_plan.in_dim, self.towers[0].activation
        answers = []
        for lv in self.levels:
            answers.append(ops.mtl_route(in_dim, lv.experts[0].hidden_units, len(lv.experts), lv.members, lv.gate_dnns[0].hidden_units,
                                         n_slots=lv.n_slots, expert_src=lv.expert_src, gate_src=lv.gate_src, activation=act))
            in_dim = lv.experts[0].hidden_units[-1]
        if self.bottom is not None and self.bottom.hidden_units:
            in_dim = self.bottom.hidden_units[-1]
        answers.append(ops.mtl_route(in_dim, self.towers[0].hidden_units, self.num_tasks, towers=True, n_slots=self.num_tasks,
                                     expert_src=list(range(self.num_tasks)), activation=act, esmm=self.esmm))
        return "fused" if all(a == "fused" for a in answers) and self._route is None else "layered"

    # ---- the forward in differentiable torch ops ------------------------------------------------------------------------------------
    def autograd_logits(self, staged, lo, hi, training=False):
        """The T pre-sigmoid tower outputs [B] each (ESMM: the ctr and the cvr logit)."""
        parts, _extra, _lin, _fms = tops.stage_forward(self.stage_plan, staged, lo, hi)
        xs = [torch.cat(parts, dim=-1)]
        for lv in self.levels:
            hs = [tops.dnn_forward(d, xs[s if len(xs) > 1 else 0], training) for d, s in zip(lv.experts, lv.expert_src)]
            outs = []
            for gd, dense, s, ms in zip(lv.gate_dnns, lv.gate_dense, lv.gate_src, lv.members):
                p = torch.softmax(tops.dnn_forward(gd, xs[s if len(xs) > 1 else 0], training) @ dense.w("kernel"), dim=-1)
                outs.append((torch.stack([hs[m] for m in ms], dim=1) * p.unsqueeze(-1)).sum(1))
            xs = outs
        if self.bottom is not None:
            xs = [tops.dnn_forward(self.bottom, xs[0], training)]
        if len(xs) == 1:
            xs = xs * self.num_tasks
        return [(tops.dnn_forward(tw, x, training) @ h.w("kernel")).reshape(-1) + p.w("global_bias")
                for tw, h, p, x in zip(self.towers, self.heads, self.predictions, xs)]

    def autograd_outputs(self, logits):
        """The model's outputs from autograd_logits' values; has_logit[t]: output t is sigmoid(logits[t]) or logits[t] itself."""
        if self.esmm:
            ctr = torch.sigmoid(logits[0])
            return [ctr, ctr * torch.sigmoid(logits[1])], [True, False]
        return [torch.sigmoid(l) if t == "binary" else l for l, t in zip(logits, self.task_types)], [True] * self.num_tasks

    # ---- the HIP training step (training_hip.HipTrainer; DESIGN.md §4.15 "Training") --------------------------------------------------
    def _hip_supported(self):
        """Every DNN is a plain relu / linear / sigmoid / tanh stack (no BatchNormalization, no dropout, no Dice / PReLU) and every task
        pairs binary with binary_crossentropy or regression with mse (the compiled losses; the defaults before compile())."""
        for d in self.dnn_layers:
            if (d.activation not in ("relu", "linear", "sigmoid", "tanh") or d.bn_layers or getattr(d, "dice_layers", None)
                    or float(getattr(d, "dropout_rate", 0) or 0) > 0 or getattr(d, "output_activation", None) not in (None, d.activation)
                    or len(d.kernels) > 8):
                return False
        losses = (self._compiled or {}).get("loss") or ["binary_crossentropy" if t == "binary" else "mse" for t in self.task_types]
        return all((t == "binary") == (l in _BCE) and (l in _BCE or l in _MSE) for t, l in zip(self.task_types, losses))

    def _hip_params(self, tr):
        l2d = float((getattr(self, "regularizers", None) or {}).get("dnn", 0.0))
        tr.own["dnn"] = {id(d): ([tr.param(k, l2d) for k in d.kernels], [tr.param(b) for b in d.biases]) for d in self.dnn_layers}
        tr.own["gates"] = [[tr.param(g.w("kernel")) for g in lv.gate_dense] for lv in self.levels]
        tr.own["heads"] = [tr.param(h.w("kernel")) for h in self.heads]
        tr.own["gbias"] = [tr.param(p.w("global_bias")) if p.use_bias else None for p in self.predictions]

    def _hip_buffers(self, buf, B):
        """The step's own per-batch buffers, kept in the trainer's ``buf`` of this batch size."""
        m = buf.get("mtl")
        if m is not None:
            return m
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=self.device)      # noqa: E731
        m = buf["mtl"] = {"acts": {id(d): [new(B, k.shape[1]) for k in d.kernels] for d in self.dnn_layers}, "levels": [], "scratch": {},
                          "ws": {}}
        in_dim = self.stage_plan.in_dim
        for lv in self.levels:
            E, G, H, n_all = len(lv.experts), len(lv.gate_dense), lv.experts[0].hidden_units[-1], sum(len(ms) for ms in lv.members)
            dz = lv.gate_dnns[0].hidden_units[-1] if lv.gate_dnns[0].hidden_units else in_dim
            m["levels"].append({"h": new(B, E * H), "out": new(B, G * H), "d_out": new(B, G * H), "dh": new(B, E * H), "ds": new(B, n_all),
                                "logits": new(B, n_all), "z": [new(B, dz) for _ in range(G)] if lv.gate_dnns[0].hidden_units else None,
                                "dz": [new(B, dz) for _ in range(G)] if lv.gate_dnns[0].hidden_units else None})
            in_dim = H
        if self.bottom is not None and self.bottom.hidden_units:
            m["bottom"], m["d_bottom"] = new(B, self.bottom.hidden_units[-1]), new(B, self.bottom.hidden_units[-1])
        return m

    def _hip_scratch(self, m, i, B, n):
        """The i-th [B, n] scratch gradient of the step (reused by every stage: a stage's sums are launched before the next writes)."""
        t = m["scratch"].get((i, n))
        if t is None:
            t = m["scratch"][(i, n)] = torch.empty(B, n, dtype=torch.float32, device=self.device)
        return t

    def _hip_reader_grads(self, m, B, n, dst, offsets, backward):
        """The gradient of slots that several DNNs may read.  ``offsets[r]``: the first column in ``dst`` of the slot reader r reads;
        ``backward(r, dx)`` runs reader r's backward, writing dx [B, n].  A slot with one reader gets its columns written in place; with
        several, each writes to scratch and ops.mtl_sum_slots forms the sum in reader order."""
        by_slot = {}
        for r, off in enumerate(offsets):
            by_slot.setdefault(off, []).append(r)
        used = 0
        for off, readers in by_slot.items():
            if len(readers) == 1:
                backward(readers[0], dst[:, off:off + n])
                continue
            parts = []
            for r in readers:
                parts.append(self._hip_scratch(m, used, B, n))
                used += 1
                backward(r, parts[-1])
            for k in range(0, len(parts), 16):
                ops.mtl_sum_slots(parts[k:k + 16], n, dst, dst_offset=off, accumulate=k > 0)
        return set(by_slot)

    def _hip_dnn_bwd(self, tr, m, d, x, in_dim, d_out, dx):
        pk, pb = tr.own["dnn"][id(d)]
        ops.mlp_bwd(x, in_dim, d.kernels, m["acts"][id(d)], d.activation, None, None, [p.g for p in pk], [p.g for p in pb], None, dx=dx,
                    d_out=d_out, workspace=m["ws"])

    def _hip_forward_backward(self, tr, staged, lo, hi, ws, buf, y, binary):
        """Forward by the layered route with the activations saved, ops.mtl_loss_grad, then backwards: the towers, the bottom, and per
        level ops.mtl_mix_bwd, the gates' softmax Dense, the gate DNNs and the experts; ``y``: float32 [T, B]."""
        B, T = hi - lo, self.num_tasks
        m = self._hip_buffers(buf, B)
        acts, c = m["acts"], self._compiled or {}
        x, in_dim, offsets = ws["dnn_in"], self.stage_plan.in_dim, [0]
        stages = []                                                     # (input buffer, its width per slot, slot offsets) of every level
        for lv, lb in zip(self.levels, m["levels"]):
            H = lv.experts[0].hidden_units[-1]
            slot = lambda s: x[:, offsets[s if len(offsets) > 1 else 0]:][:, :in_dim]      # noqa: E731
            for e, (d, s) in enumerate(zip(lv.experts, lv.expert_src)):
                ops.mlp(slot(s), d.kernels, d.biases, d.activation, in_dim=in_dim, out=lb["h"][:, e * H:(e + 1) * H], save_acts=acts[id(d)])
            zs = []
            for d, s in zip(lv.gate_dnns, lv.gate_src):
                if d.hidden_units:
                    zs.append(ops.mlp(slot(s), d.kernels, d.biases, d.activation, in_dim=in_dim, out=lb["z"][len(zs)], save_acts=acts[id(d)]))
                else:
                    zs.append(slot(s))
            ops.mtl_mix(lb["h"], len(lv.experts), H, zs, [g.w("kernel") for g in lv.gate_dense], lv.members, out=lb["out"])
            stages.append((x, in_dim, offsets, zs))
            x, in_dim, offsets = lb["out"], H, [g * H for g in range(len(lv.gate_dense))]
        bottom = self.bottom if self.bottom is not None and self.bottom.hidden_units else None
        if bottom is not None:
            bx, b_in = x, in_dim
            x = ops.mlp(bx, bottom.kernels, bottom.biases, bottom.activation, in_dim=b_in, out=m["bottom"], save_acts=acts[id(bottom)])
            in_dim, offsets = bottom.hidden_units[-1], [0]
        if len(offsets) == 1:
            offsets = offsets * T
        offsets = offsets[:T]
        pred, gb = buf["pred"], tr.own["gbias"]
        for t, (d, hd, off) in enumerate(zip(self.towers, self.heads, offsets)):
            ops.mlp(x[:, off:off + in_dim], d.kernels, d.biases, d.activation if d.kernels else "linear", head_w=hd.w("kernel"),
                    global_bias=None if gb[t] is None else gb[t].w, sigmoid_out=self.task_types[t] == "binary", in_dim=in_dim, out=pred[t],
                    save_acts=acts[id(d)] if d.kernels else None)
        acc = tr._loss_acc
        if acc is None:
            acc = buf["loss"].zero_()
        losses = c.get("loss") or ["binary_crossentropy" if t == "binary" else "mse" for t in self.task_types]
        ops.mtl_loss_grad(pred, y, buf["dlogit"], acc, losses, [t == "binary" for t in self.task_types], c.get("loss_weights"),
                          esmm=self.esmm, dbias=[None if p is None else p.g for p in gb])
        # backwards: the towers write the gradient of what they read
        if self.levels and bottom is None:
            d_x = m["levels"][-1]["d_out"]
        else:
            d_x = m["d_bottom"] if bottom is not None else buf["dx"]

        def tower_bwd(t, dx):
            d, hd, xt = self.towers[t], tr.own["heads"][t], x[:, offsets[t]:offsets[t] + in_dim]
            if d.kernels:
                pk, pb = tr.own["dnn"][id(d)]
                ops.mlp_bwd(xt, in_dim, d.kernels, acts[id(d)], d.activation, hd.w, buf["dlogit"][t], [p.g for p in pk], [p.g for p in pb],
                            hd.g, dx=dx, workspace=m["ws"])
            else:
                ops.dense1_bwd(xt, in_dim, hd.w, buf["dlogit"][t], dx, hd.g)
        written = self._hip_reader_grads(m, B, in_dim, d_x, offsets, tower_bwd)
        if bottom is not None:
            d_prev = m["levels"][-1]["d_out"] if self.levels else buf["dx"]
            self._hip_dnn_bwd(tr, m, bottom, bx, b_in, d_x, d_prev)
            written = {0}
        for i in range(len(self.levels) - 1, -1, -1):
            lv, lb = self.levels[i], m["levels"][i]
            xin, k_in, offs, zs = stages[i]
            E, G, H = len(lv.experts), len(lv.gate_dense), lv.experts[0].hidden_units[-1]
            for off in [g * H for g in range(G) if g * H not in written]:
                lb["d_out"][:, off:off + H].zero_()                     # (a gate output nothing downstream reads)
            gk = [g.w("kernel") for g in lv.gate_dense]
            ops.mtl_mix_bwd(lb["h"], E, H, zs, gk, lv.members, lb["d_out"], lb["dh"], lb["ds"], logits=lb["logits"])
            d_prev = m["levels"][i - 1]["d_out"] if i else buf["dx"]
            slot_of = lambda s: offs[s if len(offs) > 1 else 0]        # noqa: E731
            firsts = [sum(len(ms) for ms in lv.members[:g]) for g in range(G)]

            def reader_bwd(r, dx):
                if r < E:
                    xs = xin[:, slot_of(lv.expert_src[r]):][:, :k_in]
                    self._hip_dnn_bwd(tr, m, lv.experts[r], xs, k_in, lb["dh"][:, r * H:(r + 1) * H], dx)
                    return
                g = r - E
                n, d = len(lv.members[g]), lv.gate_dnns[g]
                dz = zs[g].shape[1] if d.hidden_units else k_in
                cols = slice(firsts[g], firsts[g] + n)
                # the gate's softmax Dense: a bias-free linear layer over z_g with d_out = d loss / d gate logits
                ops.mlp_bwd(zs[g], dz, [gk[g]], [lb["logits"][:, cols]], "linear", None, None, [tr.own["gates"][i][g].g], [None], None,
                            dx=lb["dz"][g] if d.hidden_units else dx, d_out=lb["ds"][:, cols], workspace=m["ws"])
                if d.hidden_units:
                    self._hip_dnn_bwd(tr, m, d, xin[:, slot_of(lv.gate_src[g]):][:, :k_in], k_in, lb["dz"][g], dx)
            written = self._hip_reader_grads(m, B, k_in, d_prev, [slot_of(s) for s in list(lv.expert_src) + list(lv.gate_src)], reader_bwd)

    # ---- the multi-output surface -------------------------------------------------------------------------------------------------
    def _pipeline(self, x, batch_size):
        return None

    @on_model_device
    def predict_tensor(self, x, batch_size=256, _span_done=None):
        """predict() that leaves the result on the device: float32 [T, N], row t = task t.  ``x``: the feed, or a Staged object."""
        staged = x if isinstance(x, Staged) else self.stage(x)
        out = torch.empty(self.num_tasks, staged.n, dtype=torch.float32, device=self.device)
        if staged.n == 0:
            return out
        self._begin()
        bs = self._rows_per_launch(staged, int(batch_size) if batch_size else staged.n)
        for lo in range(0, staged.n, bs):
            hi = min(staged.n, lo + bs)
            self._forward(staged, lo, hi, out[:, lo:hi])
        self._check_status()
        return out

    def predict(self, x, batch_size=256, verbose=0, **kwargs):
        y = self.predict_tensor(x, batch_size).cpu().numpy()
        return [np.ascontiguousarray(y[t]).reshape(-1, 1) for t in range(self.num_tasks)]

    def predict_on_batch(self, x):
        return self.predict(x, batch_size=None)

    def predict_logits(self, x, batch_size=256):
        """The values the PredictionLayers receive plus their bias, one [N, 1] array per task.  ESMM's second entry is the cvr
        logit: its ctcvr output is a product of two probabilities and has no logit of its own."""
        try:
            self._want_logits = True
            return self.predict(x, batch_size)
        finally:
            self._want_logits = False

    def __call__(self, x, training=False):
        return [torch.from_numpy(y) for y in self.predict(x, batch_size=None)]

    def sharded_predict(self, *args, **kwargs):
        raise NotImplementedError("sharded_predict is not implemented for multi-output models")

    def _per_task(self, what, value, default=None):
        """A per-task option given as one value, a list of T, or a dict keyed by task name -> list of T."""
        T = self.num_tasks
        if value is None:
            return list(default) if default is not None else [None] * T
        if isinstance(value, dict):
            unknown = [k for k in value if k not in self.task_names]
            if unknown:
                raise ValueError("%s: unknown task names %s (tasks: %s)" % (what, unknown, self.task_names))
            base = list(default) if default is not None else [None] * T
            return [value.get(n, b) for n, b in zip(self.task_names, base)]
        if isinstance(value, (list, tuple)):
            if len(value) != T:
                raise ValueError("%s: %d entries for %d tasks" % (what, len(value), T))
            return list(value)
        return [value] * T

    def compile(self, optimizer="adam", loss=None, loss_weights=None, metrics=None, **kwargs):
        default = ["binary_crossentropy" if t == "binary" else "mse" for t in self.task_types]
        losses = [d if l is None else l for l, d in zip(self._per_task("compile(loss=...)", loss, default), default)]
        for l in losses:
            if not isinstance(l, str) or l.lower() not in _BCE + _MSE:
                raise NotImplementedError("loss %r is not supported (binary_crossentropy, mse)" % (l,))
        weights = [1.0 if w is None else float(w) for w in self._per_task("compile(loss_weights=...)", loss_weights, [1.0] * self.num_tasks)]
        self._compiled = {"optimizer": optimizer, "loss": [l.lower() for l in losses], "loss_weights": weights, "metrics": list(metrics or [])}

    def _labels(self, y, n=None):
        """y: a list of T arrays or a dict keyed by task name -> float32 [T, n]."""
        if isinstance(y, dict):
            missing = [k for k in self.task_names if k not in y]
            if missing:
                raise ValueError("labels missing for the tasks %s" % missing)
            y = [y[k] for k in self.task_names]
        if not isinstance(y, (list, tuple)) or len(y) != self.num_tasks:
            raise ValueError("model %s takes one label array per task (%s)" % (self.name, self.task_names))
        out = np.stack([np.asarray(v, dtype=np.float32).reshape(-1) for v in y])
        if n is not None and out.shape[1] != n:
            raise ValueError("%d labels for %d samples" % (out.shape[1], n))
        return out

    @staticmethod
    def _loss_value(name, p, y):
        return MultiTaskModel._metric("binary_crossentropy" if name in _BCE else "mse", p, y)

    @on_model_device
    def evaluate(self, x, y, batch_size=256, verbose=0, return_dict=False, **kwargs):
        """[total, loss_1 .. loss_T, then every compiled metric per task], or the name -> value dict with ``return_dict=True``; the
        total is sum_t w_t loss_t plus the l2 penalties, as tf.keras reports it."""
        if self._compiled is None:
            self.compile()
        c = self._compiled
        ps = [p.reshape(-1).astype(np.float64) for p in self.predict(x, batch_size)]
        ys = self._labels(y, ps[0].shape[0]).astype(np.float64)
        per = [self._loss_value(l, p, yy) for l, p, yy in zip(c["loss"], ps, ys)]
        total = float(sum(w * v for w, v in zip(c["loss_weights"], per))) + tops.l2_penalty(self)
        vals = [("loss", total)] + [("%s_loss" % n, v) for n, v in zip(self.task_names, per)]
        for n, p, yy in zip(self.task_names, ps, ys):
            vals += [("%s_%s" % (n, self._metric_name(m)), self._metric(m, p, yy)) for m in c["metrics"]]
        return dict(vals) if return_dict else [v for _, v in vals]

    def test_on_batch(self, x, y, **kwargs):
        return self.evaluate(x, y, batch_size=None, **kwargs)

    @on_model_device
    def fit(self, x=None, y=None, batch_size=256, epochs=1, verbose=1, validation_split=0.0, shuffle=True, **kwargs):
        from ._fit import fit_multitask
        return fit_multitask(self, x, y, batch_size=batch_size, epochs=epochs, verbose=verbose, validation_split=validation_split,
                             shuffle=shuffle, **kwargs)

    @on_model_device
    def train_on_batch(self, x, y, **kwargs):
        from ._fit import fit_multitask
        return fit_multitask(self, x, y, batch_size=None, epochs=1, verbose=0, shuffle=False, **kwargs).history["loss"][-1]
