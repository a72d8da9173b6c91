"""HIP training step — SURVEY.md §8(f) rank 1: backward + optimizer of the hot path on HIP kernels.

``HipTrainer`` owns what every model shares: the optimiser state, the parameters of the fields / the linear part / ``model.dnn`` /
``model.dense`` / the global bias, the DNN's forward and backward (``_dnn_forward`` / ``_dnn_backward``, their layer-by-layer forms for
``dnn_dropout``, ``dnn_use_bn`` and a Dice DNN), the loss gradient and the frame of ``step()``: ``dctr_embed_pool`` per sequence feature +
``dctr_embed_gather_fm`` forward, then the model's part, then ``dctr_embed_gather_fm_bwd`` → ``dctr_embed_pool_bwd`` → ``dctr_opt_multi``
(one launch over every parameter; ``dctr_opt_apply`` when compile() holds an ``optimizers`` object: DESIGN.md §7.1).  No torch autograd,
no torch optimizer: PyTorch only owns the buffers.

What lies between the stage and the loss is the model class's, beside its forward and its ``_autograd_logit`` (the ``_hip_*`` hooks
of ``models/_common.py:FeatureModel``): ``_hip_supported`` says whether an instance trains here, ``_hip_params`` registers its
private parameters through ``HipTrainer.param``, ``_hip_forward_backward`` is its part of the step.  DeepFM / WDL / FNN
(models/deepfm.py), NFM and PNN (interaction kernel in front of the DNN), AFM (AFMLayer instead of the DNN), DCN and DCNMix
(``dctr_crossnet_bwd`` / ``dctr_crossnet_mix_bwd``), xDeepFM (``dctr_cin_bwd``), FLEN (``dctr_fieldwise_bwd``), DIN (attention input / weighted sum / lookup scatter
kernels, Dice as tf.keras runs it under fit()) and the multi-task models (models/multitask/_base.py: ``dctr_mtl_mix_bwd``, ``dctr_mtl_loss_grad``,
``dctr_mtl_sum_slots``; T outputs, ``y`` [T, B]) bring one; a model without, ``afm_dropout`` and a PReLU DNN keep ``training.py``'s step.

Semantics follow tf.keras as the reference uses it (``model.compile("adam", "binary_crossentropy")``,
examples/run_classification_criteo.py:44-50; also "adagrad", "rmsprop", "sgd" by name with tf.keras' defaults): Adam lr
1e-3, beta 0.9 / 0.999, epsilon 1e-7, NON-lazy on embeddings
(every row of a table decays every step, as ``_resource_apply_sparse`` does), L2 regularisers of the constructor
(``l2_reg_embedding``, ``l2_reg_linear``, ``l2_reg_dnn``) added to the gradients.
"""
import math

import torch

from . import ops
from .training import BN_MOMENTUM  # (keras BatchNormalization default momentum, as the torch step uses)


def supported(model):
    """Can this model train on the HIP step?  The model class answers (FeatureModel._hip_supported: no, unless the class brings
    its own ``_hip_forward_backward``), so a subclass trains as its base does."""
    return getattr(model, "stage_plan", None) is not None and bool(model._hip_supported())


class _Param(object):
    __slots__ = ("w", "m", "v", "g", "l2", "touched", "slots")

    def __init__(self, w, l2=0.0, slots=None):
        self.w = w
        if slots is None:               # an optimizer given by name: the two moments of dctr_adam_seg_t
            self.m = torch.zeros_like(w)
            self.v = torch.zeros_like(w)
            self.slots = None
        else:                           # an optimizers object: only the state its rule needs, at its initial values (dctr_opt_seg_t)
            self.slots = [torch.full_like(w, v) if v else torch.zeros_like(w) for v in slots]
            self.m = self.slots[0] if len(self.slots) > 0 else None
            self.v = self.slots[1] if len(self.slots) > 1 else None
        self.g = torch.zeros_like(w)
        self.l2 = float(l2)
        self.touched = None     # embedding tables: one byte per 16-B group of g (include/dctr.h, dctr_field_grad_t)

    def track_rows(self):
        """Embedding table [vocab, dim % 4 == 0]: the scatter kernels mark the 16-B groups of ``g`` they add to, and the optimizer
        step reads / clears only those (a 4096-row batch touches a few percent of a 1e5-row table)."""
        if self.touched is None and self.w.dim() == 2 and self.w.shape[1] % 4 == 0 and self.w.is_contiguous():
            self.touched = torch.zeros(self.w.numel() // 4, dtype=torch.uint8, device=self.w.device)
        return self


class _Frozen(object):
    """A weight that takes no part in training (Embedding.trainable == False): ``g`` is None = a NULL gradient table."""
    __slots__ = ("w", "g", "l2", "touched")

    def __init__(self, w):
        self.w, self.g, self.l2, self.touched = w, None, 0.0, None

    def track_rows(self):
        return self


class _ParamRows(object):
    """Rows [lo, hi) of a registered parameter as a handle of their own: ``w`` and ``g`` are views into the parameter's, which
    keeps its one optimizer segment (FLEN: the DNN's head is the rows of dense/kernel behind the field-wise vector's)."""
    __slots__ = ("w", "g", "l2", "touched")

    def __init__(self, p, lo, hi):
        self.w, self.g, self.l2, self.touched = p.w[lo:hi], None if p.g is None else p.g[lo:hi], p.l2, None


# tf.keras defaults of the optimizers model.compile() takes by name (optimizer_v2/*.py)
OPT_DEFAULTS = {"adam": dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-7), "adagrad": dict(lr=1e-3, eps=1e-7, init_acc=0.1),
                "rmsprop": dict(lr=1e-3, beta2=0.9, eps=1e-7), "sgd": dict(lr=1e-2)}


def trainer_for(model):
    """The trainer of ``model`` under what compile() holds now (training.compiled_optimizer): the one on ``model._hip_trainer`` while
    that is the same name or the same optimizers object — a second fit() continues its moments — and a new one otherwise."""
    from .training import compiled_optimizer
    opt = compiled_optimizer(model)
    tr = getattr(model, "_hip_trainer", None)
    if tr is None or not (tr.optimizer is opt or (isinstance(opt, str) and tr.optimizer == opt)):
        tr = model._hip_trainer = HipTrainer(model, opt)
    return tr


def takes_optimizer(model):
    """Does compile()'s optimizer run on the HIP step: one of OPT_DEFAULTS' names, or an optimizers object (training.compiled_optimizer)."""
    from . import optimizers
    from .training import compiled_optimizer
    opt = compiled_optimizer(model)
    return isinstance(opt, optimizers.Optimizer) or (isinstance(opt, str) and opt in OPT_DEFAULTS)


class HipTrainer(object):
    def __init__(self, model, optimizer="adam", lr=None, beta1=None, beta2=None, eps=None):
        if not supported(model):
            raise ValueError("model is outside the HIP training step's family (see training_hip.supported)")
        # a name keeps dctr_opt_multi with tf.keras' defaults, bit for bit; an optimizers object (or what optimizers.get makes one of)
        # runs dctr_opt_apply over dctr_opt_seg_t segments that carry only the state slots its rule needs
        self.model = model
        self.opt, self.rule = None, None
        if isinstance(optimizer, str):
            optimizer = optimizer.lower()
            if optimizer not in OPT_DEFAULTS:
                raise ValueError("optimizer %r not supported (adam, adagrad, rmsprop, sgd)" % optimizer)
            d = OPT_DEFAULTS[optimizer]
            self.optimizer = self.kind = optimizer
            self.lr = float(d["lr"] if lr is None else lr)
            self.b1 = float(d.get("beta1", 0.0) if beta1 is None else beta1)
            self.b2 = float(d.get("beta2", 0.0) if beta2 is None else beta2)
            self.eps = float(d.get("eps", 0.0) if eps is None else eps)
            self.init_acc = float(d.get("init_acc", 0.0))
        else:
            from . import optimizers
            self.optimizer = self.opt = optimizers.get(optimizer)
            self.rule = dict(self.opt._rule(), clipvalue=self.opt.clipvalue)
            self.kind = type(self.opt).__name__.lower()
        self.t = 0 if self.opt is None else int(self.opt.iterations)
        sp = model.stage_plan
        reg = getattr(model, "regularizers", {})
        l2e, l2l, l2d = reg.get("embedding", 0.0), reg.get("linear", 0.0), reg.get("dnn", 0.0)
        self.params = []
        self._by_ptr = {}
        # SparseFeat(trainable=False) (reference inputs.py:25: emb.trainable = feat.trainable; FAQ "pretrained embeddings"):
        # a frozen table gets NO gradient buffer (the backward kernels skip NULL gradient tables), no optimizer segment and
        # no l2 decay — fit() leaves it bit-identical
        self._frozen = set()
        for embs in (getattr(model, "tables", None) or {}, getattr(model, "linear_tables", None) or {}):
            for emb in embs.values():
                if not getattr(emb, "trainable", True):
                    self._frozen.add(emb.embeddings.data_ptr())
        param = self.param
        # per field: (gradient table, gradient of the linear table).  Sequence features are pooled by dctr_embed_pool into
        # per-batch buffers the gather reads as identity fields: their gradients land in per-batch buffers too
        # (_buffers) and dctr_embed_pool_bwd scatters them on to the tables.
        self.field_params = []
        for f in sp.fields:
            pt = param(f.table, l2e).track_rows()
            pl = param(f.lin_table, l2l) if f.lin_table is not None else None
            self.field_params.append((f, pt, pl))
        # features of the linear part alone (feature_column.py:171-210 builds the linear logit from linear_feature_columns only): their
        # 1-wide tables are parameters too; the second gather of the forward (EmbeddingStage.run_lin_only) has its own backward in step()
        from .feature_column import VarLenSparseFeat as _VarLen
        self.lin_only_params = [(fc, param(model.linear_tables[fc.embedding_name].embeddings, l2l)) for fc in sp.lin_only]
        self.lin_only_varlen = [(fc, p) for fc, p in self.lin_only_params if isinstance(fc, _VarLen)]
        # Linear.kernel (dense features of the linear part): the forward reads a copy permuted into dense-matrix column
        # order (EmbeddingStage.refresh); the backward kernel scatters straight into the real kernel's gradient
        self.p_dense_lin, self.dense_rows = None, None
        if model.linear is not None and sp.n_dense and sp.n_lin_dense and sp.has_linear:
            self.p_dense_lin = param(model.linear.w("linear_kernel"), l2l)
            self.dense_rows = torch.as_tensor(sp.dense_lin_rows, dtype=torch.int32, device=model.device)
        self.p_kernels = [param(k, l2d) for k in model.dnn.kernels] if model.dnn is not None else []
        self.p_biases = [param(b) for b in model.dnn.biases] if model.dnn is not None else []
        self.p_head = param(model.dense.w("kernel")) if getattr(model, "dense", None) is not None else None
        # DNN(dropout_rate > 0 / use_bn=True): training-mode BatchNormalization (gamma / beta trained, stored statistics moved by the
        # forward) and Dropout (reference layers/core.py:196-208) — the layer-by-layer form of _dnn_forward / _dnn_backward
        dnn = model.dnn
        self.drop_rate = float(getattr(dnn, "dropout_rate", 0) or 0) if dnn is not None else 0.0
        self.bn_layers = list(getattr(dnn, "bn_layers", None) or []) if dnn is not None else []
        self.slow_dnn = bool(self.drop_rate > 0 or self.bn_layers)
        self.dice_dnn = dnn is not None and dnn.activation in ("dice", "Dice")
        # swish / gelu: act' needs the pre-activations, so the forward keeps them (buf["pre"]) as Dice's does
        self.zact_dnn = dnn is not None and dnn.activation in ("swish", "silu", "gelu")
        self.p_dice_alpha = [param(d[0]) for d in dnn.dice_params()] if self.dice_dnn else []
        self.p_bn = [(param(b.w("gamma")) if b.scale else None, param(b.w("beta")) if b.center else None) for b in self.bn_layers]
        self.drop_base = int(getattr(dnn, "seed", 1024) or 0) * 0x9E3779B1 + 12345 if dnn is not None else 0
        self.n_steps = 0            # forward passes so far: the dropout masks of a step are a function of (drop_base, n_steps, layer)
        self.penalty_acc, self.penalty_rows = None, 0   # (fit(): device float64 accumulator of rows * l2 penalties; rows of the next update)
        self.own = {}               # the model's private parameter handles and per-trainer state (FeatureModel._hip_params)
        model._hip_params(self)
        # (a multi-output model has ``predictions``, one per task, and registers their biases itself: FeatureModel._hip_params)
        pred = getattr(model, "prediction", None)
        self.p_gbias = param(pred.w("global_bias")) if pred is not None and pred.use_bias else None
        self._buf = {}
        if self.opt is not None:
            self.segs, self.n_segs, self.max_n = ops.make_opt_segments([(p.w, p.g, p.slots, p.l2, p.touched) for p in self.params],
                                                                       model.device)
            self.clip_ws = self.clip_scale = None
            if self.opt.clipnorm is not None or self.opt.global_clipnorm is not None:
                self.clip_ws, self.clip_scale = ops.grad_clip_workspace(self.n_segs, self.max_n, model.device)
            return
        if self.init_acc:
            for p in self.params:
                p.v.fill_(self.init_acc)            # Adagrad's initial_accumulator_value
        self.segs, self.n_segs, self.max_n = ops.make_adam_segments([(p.w, p.m, p.v, p.g, p.l2, p.touched) for p in self.params],
                                                                    model.device)

    def param(self, t, l2=0.0):
        """The parameter handle of weight tensor ``t`` (one per storage: DIN's history tables are its query tables; a frozen table
        gets a _Frozen)."""
        key = t.data_ptr()
        if key not in self._by_ptr:
            if key in self._frozen:
                self._by_ptr[key] = _Frozen(t)
            else:
                self._by_ptr[key] = _Param(t, l2, None if self.rule is None else self.rule["slots"])
                self.params.append(self._by_ptr[key])
        return self._by_ptr[key]

    def param_rows(self, p, lo, hi):
        """A handle on rows [lo, hi) of the registered parameter ``p`` (HipTrainer.param): what ``p_head`` may be set to by a model
        whose Dense(1) kernel meets more than its DNN (FeatureModel._hip_params)."""
        return _ParamRows(p, lo, hi)

    def _buffers(self, B):
        b = self._buf.get(B)
        if b is None:
            dev = self.model.device
            sp = self.model.stage_plan
            units = [k.shape[1] for k in self.model.dnn.kernels] if self.model.dnn is not None else []
            # one output per sample, or per task and sample (models/multitask: pred / dlogit [T, B], one summed loss per task)
            outs = (len(self.model.predictions),) if getattr(self.model, "prediction", None) is None else ()
            if len(self._buf) >= 4:            # ragged remainder sizes (N % span) must not pile up per-B buffers
                self._buf.clear()
            b = self._buf[B] = {
                "acts": [torch.empty(B, n, dtype=torch.float32, device=dev) for n in units],
                "pre": [torch.empty(B, n, dtype=torch.float32, device=dev) for n in units] if (self.slow_dnn or self.dice_dnn or self.zact_dnn) else None,
                "dpre": [torch.empty(B, n, dtype=torch.float32, device=dev) for n in units] if self.slow_dnn else None,
                "bn_stat": [(torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev))
                            for n in units] if self.bn_layers else None,
                "pred": torch.empty(outs + (B,), dtype=torch.float32, device=dev),
                "dlogit": torch.empty(outs + (B,), dtype=torch.float32, device=dev),
                "dx": torch.empty(B, sp.out_stride, dtype=torch.float32, device=dev),
                "loss": torch.zeros(outs or (1,), dtype=torch.float32, device=dev),
                "pooled_g": {}, "pooled_lin_g": {},
            }
            entries = []
            for f, pt, pl in self.field_params:
                if f.kind == "pooled":
                    b["pooled_g"][f.fc.name] = torch.zeros(B, f.dim, dtype=torch.float32, device=dev)
                    if pl is not None:
                        b["pooled_lin_g"][f.fc.name] = torch.zeros(B, dtype=torch.float32, device=dev)
                    entries.append((b["pooled_g"][f.fc.name], b["pooled_lin_g"].get(f.fc.name)))
                else:
                    entries.append((pt.g, None if pl is None else pl.g, pt.touched))
            b["field_grads"] = ops.make_field_grads(entries, dev)
            if self.lin_only_params:
                # the second gather's fields (EmbeddingStage: desc2): a SparseFeat scatters d logit into its linear table's gradient, a
                # pooled sequence into a per-batch vector that dctr_embed_pool_bwd carries on to the table
                b["lin2_pool_g"] = {fc.name: torch.zeros(B, 1, dtype=torch.float32, device=dev) for fc, _ in self.lin_only_varlen}
                entries2 = [(None, b["lin2_pool_g"][fc.name].reshape(-1) if fc.name in b["lin2_pool_g"] else p.g) for fc, p in self.lin_only_params]
                b["field_grads2"] = ops.make_field_grads(entries2, dev)
        return b

    def bind_cross_views(self):
        """(Re-)point a cross net's Keras-named per-layer weights at views of its packed parameter tensors (models/dcn.py); nothing
        to do for a model without them."""
        self.own.get("bind_views", lambda: None)()

    # ---- the model's DNN (+ Dense(1) head) ------------------------------------------------------------------------------
    def dropout_seed(self, layer):
        """Seed of DNN layer ``layer``'s dropout mask in the CURRENT step (dctr_dnn_train_layer_t.dropout_seed)."""
        return (self.drop_base + self.n_steps * 1000003 + layer * 7919) & 0xFFFFFFFFFFFFFFFF

    def _bn_dict(self, l, buf):
        if not self.bn_layers:
            return None
        b = self.bn_layers[l]
        return dict(gamma=b.w("gamma") if b.scale else None, beta=b.w("beta") if b.center else None,
                    moving_mean=b.w("moving_mean"), moving_var=b.w("moving_variance"), eps=b.epsilon, momentum=b.momentum,
                    batch_mean=buf["bn_stat"][l][0], batch_var=buf["bn_stat"][l][1])

    def _dice_forward(self, x, in_dim, dnn, pre, acts):
        """A Dice DNN under training=True (the model's, DIN's attention unit) needs the statistics of ALL rows of a layer before its
        activation: layer by layer, pre-activations by the MLP kernel as a one-layer linear net -> ``pre``, dctr_dice_train_fwd ->
        ``acts``.  Returns (batch statistics per layer, last activations, their width)."""
        dice = dnn.dice_params()
        stats, xin, kin = [], x, in_dim
        for l, (W, b) in enumerate(zip(dnn.kernels, dnn.biases)):
            ops.mlp(xin, [W], [b], "linear", in_dim=kin, out=pre[l])
            alpha, mmean, mvar = dice[l]
            stats.append(ops.dice_train_fwd(pre[l], alpha, mmean, mvar, acts[l], eps=1e-9, momentum=BN_MOMENTUM))
            xin, kin = acts[l], W.shape[1]
        return stats, xin, kin

    def _dnn_forward(self, x, in_dim, buf, out, head=True, add=(), binary=False):
        """model.dnn over x[:, :in_dim] with the activations saved in buf["acts"]; ``head``: + Dense(1) + add + global bias (+ sigmoid)
        -> out [B]; headless: the last layer's activations -> out (a 2-D view)."""
        dnn = self.model.dnn
        hk = dict(head_w=self.p_head.w, add=list(add), global_bias=None if self.p_gbias is None else self.p_gbias.w,
                  sigmoid_out=binary) if head else {}
        if not (self.dice_dnn or self.slow_dnn or self.zact_dnn):
            ops.mlp(x, dnn.kernels, dnn.biases, dnn.activation, in_dim=in_dim, out=out, save_acts=buf["acts"], **hk)
            return
        if self.dice_dnn:
            buf["dice_batch"], xin, kin = self._dice_forward(x, in_dim, dnn, buf["pre"], buf["acts"])
            if not head:
                out[:, :kin].copy_(xin)             # (the stack's tail may carry alignment padding)
        else:   # training-mode BatchNormalization / Dropout: dense part (one-layer linear launch) -> dctr_dnn_train_layer_fwd, layer by layer
            # (swish / gelu without either: the same two launches per layer leave the pre-activations in buf["pre"] for the backward)
            L = len(dnn.kernels)
            xin, kin = x, in_dim
            for l, (W, b) in enumerate(zip(dnn.kernels, dnn.biases)):
                ops.mlp(xin, [W], [b], "linear", in_dim=kin, out=buf["pre"][l])
                h = out if (not head and l == L - 1) else buf["acts"][l]
                ops.dnn_train_layer(buf["pre"][l], dnn.activation, h=h, bn=self._bn_dict(l, buf), dropout_rate=self.drop_rate,
                                    dropout_seed=self.dropout_seed(l))
                xin, kin = h, W.shape[1]
        if head:
            ops.mlp(xin, [], [], "linear", in_dim=kin, out=out, **hk)

    def _dnn_backward(self, x, in_dim, buf, dx, dlogit=None, d_out=None):
        """Backward of _dnn_forward: weight gradients accumulated, dx [B, >= in_dim] written.  With a head ``dlogit`` [B] comes in,
        headless ``d_out`` (2-D view) = gradient w.r.t. the last layer's activations."""
        dnn = self.model.dnn
        dk, db = [p.g for p in self.p_kernels], [p.g for p in self.p_biases]
        hw, hg = (self.p_head.w, self.p_head.g) if dlogit is not None else (None, None)
        if self.dice_dnn:
            ops.mlp_bwd(x, in_dim, dnn.kernels, buf["acts"], "dice", hw, dlogit, dk, db, hg, dx=dx, d_out=d_out, biases=dnn.biases,
                        dice=dnn.dice_params(), d_dice_alpha=[p.g for p in self.p_dice_alpha], dice_batch=buf["dice_batch"],
                        saved_z=buf["pre"], workspace=buf.setdefault("mlp_bwd_ws_dice", {}))
            return
        if self.zact_dnn and not self.slow_dnn:
            ops.mlp_bwd(x, in_dim, dnn.kernels, buf["acts"], dnn.activation, hw, dlogit, dk, db, hg, dx=dx, d_out=d_out, biases=dnn.biases,
                        saved_z=buf["pre"], workspace=buf.setdefault("mlp_bwd_ws_z", {}))
            return
        if not self.slow_dnn:
            # the weight-gradient launches go to a second stream (dctr_mlp_bwd_args_t.dw_stream): they run beside the embedding
            # scatter / CIN / CrossNet backward that follow on the main stream; step() joins before the optimizer
            side = self._side_stream()
            ops.mlp_bwd(x, in_dim, dnn.kernels, buf["acts"], dnn.activation, hw, dlogit, dk, db, hg, dx=dx, d_out=d_out,
                        dw_stream=side, workspace=buf.setdefault("mlp_bwd_ws", {}))
            self._side_used = side is not None
            return
        L = len(dnn.kernels)
        units = [k.shape[1] for k in dnn.kernels]
        if dlogit is not None:              # Dense(1): dH_last = dlogit (x) head_w, d_head_w += h_last^T dlogit
            dh = buf["dpre"][L - 1]
            ops.dense1_bwd(buf["acts"][L - 1], units[-1], hw, dlogit, dh, hg)
        else:
            dh = d_out
        for l in range(L - 1, -1, -1):
            dz = buf["dpre"][l]
            pg = self.p_bn[l] if self.p_bn else (None, None)
            ops.dnn_train_layer(buf["pre"][l], dnn.activation, bn=self._bn_dict(l, buf), dropout_rate=self.drop_rate,
                                dropout_seed=self.dropout_seed(l), dh=dh, dz=dz,
                                d_gamma=None if pg[0] is None else pg[0].g, d_beta=None if pg[1] is None else pg[1].g)
            xin, kin = (x, in_dim) if l == 0 else (buf["acts"][l - 1], units[l - 1])
            dst = dx if l == 0 else buf["dpre"][l - 1]
            # dense part of the layer: d_bias += colsum(dz), dW += x^T dz, dH_{l-1} = dz W^T  (one-layer headless linear dctr_mlp_bwd)
            # (one cached workspace per layer: the call would otherwise allocate one per layer and step)
            ops.mlp_bwd(xin, kin, [dnn.kernels[l]], [buf["acts"][l]], "linear", None, None, [dk[l]], [db[l]], None, dx=dst, d_out=dz,
                        workspace=buf.setdefault("mlp_bwd_ws_l%d" % l, {}))
            dh = dst

    side_stream = True          # False: everything on the caller's stream (A/B in scripts/bench_train.py --no-side-stream)

    def _side_stream(self):
        if not self.side_stream or self.model.device.type != "cuda":
            return None
        if getattr(self, "_side", None) is None:
            self._side = torch.cuda.Stream(device=self.model.device)
        return self._side

    def _join_side(self):
        if getattr(self, "_side_used", False):
            torch.cuda.current_stream(self.model.device).wait_stream(self._side)
            self._side_used = False

    def _loss_grad(self, buf, y, binary):
        acc = getattr(self, "_loss_acc", None)        # fit(): the epoch's running sum of per-sample losses (no per-step launches for it)
        if acc is None:
            buf["loss"].zero_()
        ops.bce_grad(buf["pred"], y, buf["dlogit"], loss_sum=buf["loss"] if acc is None else acc,
                     dlogit_sum=None if self.p_gbias is None else self.p_gbias.g, task="binary" if binary else "regression",
                     weight=getattr(self, "_sample_weight", None))

    def _dnn_step(self, x, in_dim, buf, y, binary, add=(), dx=None):
        """DNN + head over x[:, :in_dim] (+ the logits ``add``) -> buf["pred"], the loss gradient, the DNN's backward -> ``dx``
        (default buf["dx"]): the middle of every model whose head sits on its DNN."""
        self._dnn_forward(x, in_dim, buf, buf["pred"], head=True, add=add, binary=binary)
        self._loss_grad(buf, y, binary)
        self._dnn_backward(x, in_dim, buf, buf["dx"] if dx is None else dx, dlogit=buf["dlogit"])

    def step(self, staged, lo, hi, y, apply=True, loss_acc=None, weight=None):
        """One optimizer step on rows [lo, hi) of the staged inputs; y: device float tensor [hi-lo].  Returns the mean
        loss of the batch BEFORE the update (a device tensor; no host synchronisation here).  ``apply=False`` stops
        after the backward pass and leaves the gradients in the ``g`` buffers (tests).  ``loss_acc`` (a device float32 tensor of
        one element): the batch's SUMMED loss is added to it instead — no per-step zero / divide launches, nothing returned
        (fit() keeps one accumulator per epoch).  ``weight``: device float32 [hi-lo], tf.keras' per-sample weights of the batch
        (loss = sum w_b l_b / B: dctr_bce_grad_w)."""
        self._loss_acc = loss_acc
        self._sample_weight = weight
        model, sp = self.model, self.model.stage_plan
        model._trainer_owns_cross = True    # (_DCN._begin: no re-packing of the cross weights for this call)
        model._trainer_step = True          # (_begin: only what the step reads — no inference-form BatchNormalization scale / shift, no
        try:                                #  zero-padded DNN copies, no packed cross operands; predict() refreshes them itself)
            model._begin()                  # weight-derived forward buffers follow the last update
        finally:
            model._trainer_owns_cross = False
            model._trainer_step = False
        self.n_steps += 1
        B = hi - lo
        buf = self._buffers(B)
        binary = model.task == "binary"
        # forward (pool launches + two launches, activations saved)
        sp.pool_trace = []
        try:
            ws = sp.run(staged, lo, hi)
            pool_calls = sp.pool_trace
        finally:
            sp.pool_trace = None
        if self.lin_only_params:            # the linear-only features' logit joins the linear logit every model adds to its head
            ws["lin"].add_(ws["lin2"])
        model._hip_forward_backward(self, staged, lo, hi, ws, buf, y, binary)
        # embedding / linear / FM backward
        for t in list(buf["pooled_g"].values()) + list(buf["pooled_lin_g"].values()):
            t.zero_()
        for gname in sp.fm_group_names[1:]:      # FM groups beyond the gather's own: d e_f += dlogit (S_g - e_f) on their slice of dnn_in
            first, nf_g, dim_g = sp.group_slices[gname]
            ops.fm_bwd(ws["dnn_in"][:, first:], nf_g, dim_g, buf["dlogit"], buf["dx"][:, first:], accumulate=True)
        g = sp.gather_args(staged, lo, hi, ws)
        ops.embed_gather_fm_bwd(g, buf["field_grads"], d_dnn_in=buf["dx"], d_fm=buf["dlogit"] if sp.fm_group_names else None,
                                d_lin=buf["dlogit"] if sp.has_linear else None,
                                g_dense_lin_w=None if self.p_dense_lin is None else self.p_dense_lin.g,
                                dense_lin_rows=self.dense_rows)
        # sequence features: pooled-vector gradients -> rows of their tables
        pooled = [(f, pt, pl) for f, pt, pl in self.field_params if f.kind == "pooled"]
        assert len(pool_calls) == len(pooled) + len(self.lin_only_varlen)
        for (args, _keep), (f, pt, pl) in zip(pool_calls, pooled):
            ops.embed_pool_bwd(args, d_out=buf["pooled_g"][f.fc.name], d_lin_out=buf["pooled_lin_g"].get(f.fc.name),
                               g_table=pt.g, g_lin_table=None if pl is None else pl.g, touched=pt.touched)
        if self.lin_only_params:
            # features of the linear part alone: d logit -> rows of their linear tables (the backward of run_lin_only's gather; pooled
            # sequences through their per-batch vectors)
            for t in buf["lin2_pool_g"].values():
                t.zero_()
            nf = len(sp.fields)
            g2 = ops.make_gather_args(ws["desc2"], ws["n_fields2"], staged.ids[nf:, lo:hi], staged.ids.stride(0), 1, B, 1, False,
                                      ws["any_hash2"], lin_logit=ws["lin2"], status=ws["status"])
            ops.embed_gather_fm_bwd(g2, buf["field_grads2"], d_lin=buf["dlogit"])
            for (args, _keep), (fc, p) in zip(pool_calls[len(pooled):], self.lin_only_varlen):
                if p.g is not None:
                    ops.embed_pool_bwd(args, d_out=buf["lin2_pool_g"][fc.name], g_table=p.g)
        self._join_side()
        if apply:
            self.apply_update()
        return None if loss_acc is not None else buf["loss"] / B

    def apply_update(self):
        """The optimizer step over every parameter in one launch (the gradients are zeroed behind it).  Separate from ``step`` so
        that a data-parallel fit can exchange the gradients of a step between its backward and its update (training._DataParallel)."""
        if self.opt is not None:
            self.t = int(self.opt.iterations) + 1   # (the object counts: it may serve more than one model)
            return self._apply_object()
        self.t += 1
        lr = self.lr
        if self.kind == "adam":
            lr = self.lr * math.sqrt(1.0 - self.b2 ** self.t) / (1.0 - self.b1 ** self.t)
        # fit(): the l2 penalties of THIS step's weights, weighted by the batch's rows, ride the launch (tf.keras' reported loss is the
        # batch-size-weighted mean of data loss + regularisation losses: training._fit_hip sets penalty_acc / penalty_rows)
        pen = self.penalty_acc if self.penalty_rows else None
        ops.opt_multi(self.kind, self.segs, self.n_segs, self.max_n, lr, self.b1, self.b2, self.eps, penalty=pen,
                      penalty_scale=float(self.penalty_rows) if pen is not None else 0.0)
        # the weights moved through raw pointers (torch's version counters did not): derived inference copies are stale
        self.model._raw_weight_writes = getattr(self.model, "_raw_weight_writes", 0) + 1

    def _apply_object(self):
        """apply_update for an optimizers object: the scheduled rate of this update (evaluated on the host at ``iterations`` before
        the increment: a launch scalar, no device sync), the clipnorm / global_clipnorm pre-pass when the object asks for one (one
        more read of w and g; the scales stay on the device), dctr_opt_apply, and ``iterations`` written back."""
        opt = self.opt
        lr = opt._step_lr(self.t)
        scale = None
        if self.clip_scale is not None:
            g_clip = opt.global_clipnorm is not None
            ops.grad_clip_scales(self.segs, self.n_segs, self.max_n, opt.global_clipnorm if g_clip else opt.clipnorm, self.clip_ws,
                                 self.clip_scale, global_norm=g_clip)
            scale = self.clip_scale
        pen = self.penalty_acc if self.penalty_rows else None
        ops.opt_apply(self.rule, self.segs, self.n_segs, self.max_n, lr, clip_scale=scale, penalty=pen,
                      penalty_scale=float(self.penalty_rows) if pen is not None else 0.0)
        opt.iterations = self.t
        self.model._raw_weight_writes = getattr(self.model, "_raw_weight_writes", 0) + 1

    def batch_statistics(self):
        """True when the step takes statistics over the BATCH (training-mode BatchNormalization / Dice): under data-parallel fit a rank
        normalises with its own sub-batch's statistics (training._DataParallel: per-replica statistics, stored ones averaged)."""
        return bool(self.bn_layers or self.dice_dnn or self.model._hip_batch_statistics())
