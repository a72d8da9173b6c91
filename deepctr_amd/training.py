"""``fit`` / ``train_on_batch`` — SURVEY.md §8(f) rank 1.

``fit_model`` picks one of two training steps.  The models ``training_hip.supported`` names train on the HIP step (``_fit_hip``:
hand-written backward and optimizer kernels, no autograd).  Every other model or option trains on PyTorch autograd (``_fit_torch``)
over a differentiable restatement of the SAME forward, built from torch ops on the SAME device and the SAME weight tensors, so
``predict`` after ``fit`` runs the HIP kernels on the trained weights.  That restatement is ``model_logits``: the shared pieces
(``stage_forward``, ``dnn_forward``, the layer restatements ``_interacting`` / ``_bilinear`` / ``_fefm``) live here, each model's
own part in its model file (``FeatureModel.autograd_logits``).  It is also the oracle every HIP gradient test differentiates and the
"torch ops" baseline of the scripts/bench_*.py; it is not a performance path and nothing in ``predict`` routes through it.  Parity of
the torch forward with the HIP forward is a GPU test (tests/test_gpu_fit.py); the CPU suite pins it to the reference's outputs.

Sequence features, hashing, DIN attention, dropout, BatchNormalization / Dice in training mode and the l2 regularisers of the
reference constructors are covered.
"""
from itertools import combinations

import numpy as np
import torch

from . import ops
from .engine import prehashed_on_host
from .feature_column import SparseFeat


class History(object):
    def __init__(self):
        self.history = {}
        self.epoch = []


def _rows_for(fc, ids, mask_zero_hash):
    if fc.use_hash and not prehashed_on_host(fc):
        return ops.hash_bucket(ids.contiguous(), fc.vocabulary_size, mask_zero_hash)
    return ids.to(torch.int64)


def _pool(seq, fc, mask, length, weight):
    """reference layers/sequence.py:76-106,155-183 in torch (differentiable)."""
    B, T, E = seq.shape
    if length is not None:
        m = (torch.arange(T, device=seq.device)[None, :] < length.reshape(-1, 1))
        cnt = length.reshape(-1, 1).to(seq.dtype)
    else:
        m = mask
        cnt = m.sum(dim=1, keepdim=True).to(seq.dtype)
    if weight is not None:
        w = weight.reshape(B, T)
        if fc.weight_norm:
            w = torch.softmax(torch.where(m, w, torch.full_like(w, float(-2 ** 32 + 1))), dim=1)
        else:
            w = torch.where(m, w, torch.zeros_like(w))
        seq = seq * w.unsqueeze(-1)
    mf = m.to(seq.dtype).unsqueeze(-1)
    if fc.combiner == "max":
        return (seq - (1 - mf) * 1e9).max(dim=1).values
    s = (seq * mf).sum(dim=1)
    if fc.combiner == "mean":
        s = s / (cnt + 1e-8)
    return s


def stage_forward(sp, staged, lo, hi):
    """Differentiable EmbeddingStage: returns (dnn_in [B,in_dim], linear logit [B] or None, [FM logits])."""
    B = hi - lo
    dev = sp.device
    embs, lin = [], torch.zeros(B, device=dev)
    has_lin = False
    for i, f in enumerate(sp.fields):
        fc = f.fc
        if f.kind == "sparse":
            rows = _rows_for(fc, staged.ids[i, lo:hi], fc.name in sp.mask_feat_list)
            e = f.table[rows]
            if f.lin_table is not None:
                lin = lin + f.lin_table.reshape(-1)[rows]
                has_lin = True
        else:
            rows = _rows_for(fc, staged.seq[fc.name][lo:hi], True)
            length = staged.length[fc.length_name][lo:hi] if fc.length_name is not None else None
            weight = staged.weight[fc.weight_name][lo:hi] if fc.weight_name is not None else None
            mask = rows != 0
            e = _pool(f.table[rows], fc, mask, length, weight)
            if f.lin_table is not None:
                lin = lin + _pool(f.lin_table.reshape(-1)[rows].unsqueeze(-1), fc, mask, length, weight).reshape(-1)
                has_lin = True
        embs.append(e)
    fms = []
    for g in sp.fm_group_names:
        x = torch.stack(_group_embeddings(sp, embs, g), dim=1)
        fms.append(0.5 * (x.sum(1).pow(2) - (x * x).sum(1)).sum(-1))
    parts = list(embs)
    extra = {}
    for name, off in sp.extra_offsets.items():
        extra[name] = len(parts)
        parts.append(None)                       # filled by the caller (DIN attention output)
    dense = staged.dense[lo:hi] if staged.dense is not None else None
    if dense is not None:
        if sp.n_dense_dnn:
            parts.append(dense[:, :sp.n_dense_dnn])
        if sp.dense_lin_w is not None:
            lin = lin + dense @ sp.dense_lin_w
            has_lin = True
    nf = len(sp.fields)
    for k, fc in enumerate(sp.lin_only):
        lt = sp.linear_tables[fc.embedding_name].embeddings.reshape(-1)
        if isinstance(fc, SparseFeat):
            rows = _rows_for(fc, staged.ids[nf + k, lo:hi], fc.name in sp.mask_feat_list)
            lin = lin + lt[rows]
        else:
            rows = _rows_for(fc, staged.seq[fc.name][lo:hi], True)
            length = staged.length[fc.length_name][lo:hi] if fc.length_name is not None else None
            weight = staged.weight[fc.weight_name][lo:hi] if fc.weight_name is not None else None
            lin = lin + _pool(lt[rows].unsqueeze(-1), fc, rows != 0, length, weight).reshape(-1)
        has_lin = True
    return parts, extra, (lin if has_lin else None), fms


BN_MOMENTUM = 0.99      # tf.keras BatchNormalization default; Dice builds its BN with it (layers/activation.py:51-53)


def _act(name, x, dice=None, training=False):
    if name in ("dice", "Dice"):
        alpha, mean, var = dice
        if training:
            # Dice's BatchNormalization(center=False, scale=False, epsilon=1e-9) as tf.keras runs it under fit(): normalise
            # with the statistics of THIS batch over every axis but the last (biased variance, gradients flow through
            # them) and move the stored statistics towards them (layers/activation.py:59-64)
            dims = tuple(range(x.dim() - 1))
            bm = x.mean(dim=dims)
            bv = x.var(dim=dims, unbiased=False)
            with torch.no_grad():
                mean.mul_(BN_MOMENTUM).add_(bm.detach(), alpha=1.0 - BN_MOMENTUM)
                var.mul_(BN_MOMENTUM).add_(bv.detach(), alpha=1.0 - BN_MOMENTUM)
            mean, var = bm, bv
        xp = torch.sigmoid((x - mean) / torch.sqrt(var + 1e-9))
        return alpha * (1 - xp) * x + xp * x
    return _ACTS[name](x)


# the tf.keras 2.x definitions (keras/activations.py) in torch ops: what csrc/act_device.h computes
_F = torch.nn.functional
_ACTS = {"relu": torch.relu, "sigmoid": torch.sigmoid, "tanh": torch.tanh, "linear": lambda v: v, None: lambda v: v,
         "elu": _F.elu, "selu": _F.selu, "softsign": _F.softsign, "exponential": torch.exp, "swish": _F.silu, "silu": _F.silu,
         "gelu": _F.gelu,                                                                # (the erf form: approximate=False)
         "softplus": lambda v: torch.clamp(v, min=0) + torch.log1p(torch.exp(-v.abs())),   # (no threshold: keras has none)
         "hard_sigmoid": lambda v: torch.clamp(0.2 * v + 0.5, 0.0, 1.0)}                 # (Keras 2; torch's hardsigmoid is relu6(z + 3) / 6)


def _dropout(x, rate, training):
    """keras Dropout (inverted scaling) in training mode; the mask comes from torch's generator, not TF's."""
    return torch.nn.functional.dropout(x, float(rate), True) if training and rate and rate > 0 else x


def _batch_norm(bn, x, training):
    """tf.keras BatchNormalization(axis=-1) as DNN(use_bn=True) calls it (layers/core.py:200-201): training mode normalises
    with the batch statistics (biased variance, gradients through them) and moves the stored statistics with the layer's
    momentum; inference mode uses the stored statistics."""
    mean, var = bn.w("moving_mean"), bn.w("moving_variance")
    if training:
        dims = tuple(range(x.dim() - 1))
        bm = x.mean(dim=dims)
        bv = x.var(dim=dims, unbiased=False)
        with torch.no_grad():
            mean.mul_(bn.momentum).add_(bm.detach(), alpha=1.0 - bn.momentum)
            var.mul_(bn.momentum).add_(bv.detach(), alpha=1.0 - bn.momentum)
        mean, var = bm, bv
    inv = torch.rsqrt(var + bn.epsilon)
    if bn.scale:
        inv = inv * bn.w("gamma")
    off = -mean * inv
    if bn.center:
        off = bn.w("beta") + off
    return x * inv + off


def dnn_forward(dnn, x, training=False):
    dice_layers = getattr(dnn, "dice_layers", None) or []
    bn_layers = getattr(dnn, "bn_layers", None) or []
    for i, (w, b) in enumerate(zip(dnn.kernels, dnn.biases)):
        x = x @ w + b
        if bn_layers:
            x = _batch_norm(bn_layers[i], x, training)
        act = dnn.layer_activation(i) if hasattr(dnn, "layer_activation") else dnn.activation
        d = dice_layers[i].params() if (dice_layers and dice_layers[i] is not None) else None
        x = _act(act, x, d, training)
        x = _dropout(x, getattr(dnn, "dropout_rate", 0), training)             # layers/core.py:204-205
    return x


def frozen_weights(model):
    """data_ptr()s of the tables built from SparseFeat(trainable=False) (reference inputs.py:25: ``emb.trainable =
    feat.trainable``; docs FAQ "pretrained embeddings"): neither training path may touch them."""
    out = set()
    for embs in (getattr(model, "tables", None) or {}, getattr(model, "linear_tables", None) or {}, getattr(model, "fg_tables", None) or {},
                 getattr(model, "mlr_tables", None) or {}):
        for emb in embs.values():
            if not getattr(emb, "trainable", True):
                out.add(emb.embeddings.data_ptr())
    return out


def l2_penalty(model, regs=None):
    """sum over the regularised weights of l2 * sum(w^2), in float64 — the value tf.keras adds to the data loss wherever it reports a
    loss: fit's `loss`, evaluate() / test_on_batch, `val_loss` (regularisers: reference inputs.py:22, layers/core.py:170,
    interaction.py:100,258,387; docs/source/Model_Methods.md:24-43).  No float64 copy of a table is made (C5's tables are 1.3 GB each)."""
    if regs is None:
        frozen = frozen_weights(model)
        regs = [(t, l2) for t, l2 in regularized_weights(model) if t.data_ptr() not in frozen]
    tot = 0.0
    for t, l2 in regs:
        tot += l2 * float(torch.linalg.vector_norm(t.detach().reshape(-1), dtype=torch.float64).item()) ** 2
    return tot


def regularized_weights(model):
    """[(tensor, l2)] for every weight the reference attaches ``l2(l2_reg_*)`` to: embedding tables (inputs.py:22-41), the
    linear part (feature_column.py:171-210, layers/utils.py:142-158), DNN kernels (core.py:160-166), CrossNet / CrossNetMix
    kernels (interaction.py:387, :481-500), CIN filters (:258), AFMLayer.attention_W (:100), FwFMLayer.field_pair_strengths (:1385-1389)
    and FEFMLayer's pair matrices (:1459-1463).  keras l2(l) adds
    l * sum(w^2) to the loss — over the WHOLE table every step, as the HIP step's 2*l2*w term does."""
    reg = getattr(model, "regularizers", None) or {}
    out, seen = [], set()

    def add(t, l2):
        if t is not None and l2 and t.data_ptr() not in seen:
            seen.add(t.data_ptr())
            out.append((t, float(l2)))

    for emb in (getattr(model, "tables", None) or {}).values():
        add(emb.embeddings, reg.get("embedding", 0.0))
    for emb in (getattr(model, "fg_tables", None) or {}).values():         # FGCNN's second embedding set (fgcnn.py:64-65)
        add(emb.embeddings, reg.get("embedding", 0.0))
    for emb in (getattr(model, "linear_tables", None) or {}).values():
        add(emb.embeddings, reg.get("linear", 0.0))
    if getattr(model, "linear", None) is not None:
        add(model.linear.w("linear_kernel"), reg.get("linear", 0.0))
    for emb in (getattr(model, "mlr_tables", None) or {}).values():        # MLR: every one-wide table and every Linear of its 2R (+1)
        add(emb.embeddings, reg.get("linear", 0.0))                        # logits carries l2(l2_reg_linear) (mlr.py:60-72)
    for lin in getattr(model, "mlr_linears", None) or []:
        add(lin._weights.get("linear_kernel"), reg.get("linear", 0.0))
    dnn = getattr(model, "dnn", None)
    if dnn is not None:
        for k in dnn.kernels:
            add(k, reg.get("dnn", 0.0))
    for dnn in getattr(model, "dnn_layers", None) or []:          # EDCN: one DNN and one CrossNet per round (edcn.py:75-78)
        for k in dnn.kernels:
            add(k, reg.get("dnn", 0.0))
    crosses = list(getattr(model, "cross_layers", None) or [])
    if getattr(model, "cross", None) is not None:
        crosses.append(model.cross)
    for cross in crosses:
        for name, t in cross._weights.items():
            if name.startswith(("kernel", "U_list", "V_list", "C_list")):
                add(t, reg.get("cross", 0.0))
    cin = getattr(model, "cin", None)
    if cin is not None:
        for f in cin.filters:
            add(f, reg.get("cin", 0.0))
    for layer in getattr(model, "afm_layers", None) or []:
        add(layer.w("attention_W"), getattr(layer, "l2_reg_w", 0.0))
    for layer in getattr(model, "fwfm_layers", None) or []:     # the whole [F,F] variable, not the triangle the forward reads
        add(layer.field_strengths, layer.regularizer)
    fefm = getattr(model, "fefm", None)
    if fefm is not None:
        for m in fefm.matrices:
            add(m, fefm.regularizer)
    return out


def _pair_indices(n):
    """(ii, jj): the pairs i < j of n fields in itertools.combinations order, as two index lists."""
    pairs = list(combinations(range(n), 2))
    return [i for i, _ in pairs], [j for _, j in pairs]


def _group_embeddings(sp, embs, g):
    """The [B, dim] embeddings of embedding group ``g`` of an EmbeddingStage, in field order (``embs``: one entry per field)."""
    first, n, dim = sp.group_slices[g]
    return [embs[k] for k, f in enumerate(sp.fields) if first <= f.out_offset < first + n * dim]


def _interacting(layer, x):
    """InteractingLayer.call (reference interaction.py:749-779) in torch ops: x [B,F,E] -> [B,F,d*H]."""
    d, H = layer.att_embedding_size, layer.head_num
    B, F = x.shape[0], x.shape[1]

    def heads(w):
        return (x @ w).reshape(B, F, H, d).permute(2, 0, 1, 3)                 # [H,B,F,d]
    q, k, v = heads(layer.w("query")), heads(layer.w("key")), heads(layer.w("value"))
    s = q @ k.transpose(-1, -2)
    if layer.scaling:
        s = s / d ** 0.5
    o = (torch.softmax(s, dim=-1) @ v).permute(1, 2, 0, 3).reshape(B, F, H * d)
    if layer.use_res:
        o = o + x @ layer.w("res")
    return torch.relu(o)


HIP_AUTOGRAD_OPS = True     # the autograd step may run an operator as one differentiable HIP op (interacting_stack); off: torch ops only


def interacting_stack(layers, x):
    """A stack of InteractingLayers over x [B,F,E] -> [B,F,d*H] inside the autograd step.  On the GPU, with gradients enabled, the
    whole stack is ops.InteractingFunction: dctr_interacting_fwd forward and dctr_interacting_bwd backward, one launch each, nothing
    between the layers in HBM (profiles/autoint_interacting_bwd.txt: faster at 4,096 and at 65,536 rows, so no row threshold).
    Everything else — the CPU, torch.no_grad() (model_logits as the reference of the HIP forward), HIP_AUTOGRAD_OPS off, layers that
    differ in their options, a shape the backward refuses — takes the torch ops of _interacting, layer by layer."""
    layers = list(layers)
    if layers and x.is_cuda and torch.is_grad_enabled() and HIP_AUTOGRAD_OPS and x.dtype == torch.float32:
        first = layers[0]
        d, H, res, scaling = first.att_embedding_size, first.head_num, bool(first.use_res), bool(first.scaling)
        same = all((l.att_embedding_size, l.head_num, bool(l.use_res), bool(l.scaling)) == (d, H, res, scaling) for l in layers)
        if same and ops.interacting_bwd_supported(x.shape[1], x.shape[2], len(layers), d, H, res):
            flat = [w for l in layers for w in l.weights_qkvr]
            return ops.InteractingFunction.apply(x, d, H, res, scaling, *flat).reshape(x.shape[0], x.shape[1], d * H)
    for layer in layers:
        x = _interacting(layer, x)
    return x


# Below this many rows FEFMLayer's autograd step stays on the torch ops: the HIP route validates the 325 weight tensors on the host in
# both launches and hands autograd 325 gradient views, which at 4,096 rows of the Criteo shape costs more than the kernels save (6.82
# against 6.27 ms a step; the two routes cross near 5,400 rows and at 8,192 HIP wins: profiles/fefm_fieldpair_bwd.txt).  FwFM has one
# weight tensor and no threshold.
FEFM_HIP_MIN_ROWS = 8192


# Below this many rows FiBiNET's autograd step stays on the torch ops.  At 4,096 rows of the Criteo shape the HIP route lost (11.03
# against 10.17 ms a step, 0.92x): dctr_bilinear_bwd walks its tiles five times for the 650 weight sums and then has 256 tiles for 256
# workgroups, 1.08 ms a call, beside the host's handling of 650 weight tensors in both launches.  At 8,192 rows it won (7.51 against
# 11.41 ms, 1.52x) and at 65,536 by 2.27x (profiles/fibinet_bilinear_bwd.txt); no size between 4,096 and 8,192 was measured, so the
# threshold is the smallest size measured to win.
FIBINET_HIP_MIN_ROWS = 8192


def _fieldpair_on_hip(x, weights, kind, min_rows=0):
    """The gate of fefm_pairs / fwfm_logit: interacting_stack's, something must actually require grad, and FEFM's row threshold."""
    return (x.is_cuda and torch.is_grad_enabled() and HIP_AUTOGRAD_OPS and x.dtype == torch.float32 and x.shape[0] >= min_rows
            and (x.requires_grad or any(w.requires_grad for w in weights))
            and ops.fieldpair_bwd_supported(x.shape[1], x.shape[2], kind))


def fefm_pairs(layer, x, want_pairs=True, want_logit=False):
    """FEFMLayer over x [B,F,E] inside the autograd step: (pairs [B,P] or None, their row sum [B] or None).  On the GPU, with gradients
    enabled and something requiring grad, it is ops.FieldPairFunction: dctr_fieldpair_fwd forward and dctr_fieldpair_bwd backward, one
    launch each, no [B,P,E] intermediate in HBM (profiles/fefm_fieldpair_bwd.txt).  Everything else — the CPU, torch.no_grad(),
    HIP_AUTOGRAD_OPS off, fewer than FEFM_HIP_MIN_ROWS rows, a shape the backward refuses — takes the torch ops of _fefm."""
    if not (want_pairs or want_logit):
        return None, None
    ws = layer.matrices
    if _fieldpair_on_hip(x, ws, "fefm", FEFM_HIP_MIN_ROWS):
        return ops.FieldPairFunction.apply(x, "fefm", bool(want_pairs), bool(want_logit), *ws)
    pairs = _fefm(layer, x)
    return (pairs if want_pairs else None), (pairs.sum(-1) if want_logit else None)


def fwfm_logit(layer, x):
    """FwFMLayer over x [B,F,E] inside the autograd step: the logit [B].  The gate of fefm_pairs; otherwise the einsum over the Gram
    matrix and the strict upper triangle of field_pair_strengths."""
    r = layer.field_strengths
    if _fieldpair_on_hip(x, [r], "fwfm"):
        return ops.FieldPairFunction.apply(x, "fwfm", False, True, r)[1]
    gram = torch.einsum("bie,bje->bij", x, x)
    return (gram * torch.triu(r, diagonal=1)).sum((1, 2))


# ONN's pair products have no row threshold: at the Criteo shape the autograd step with ops.FieldAwareFunction took 0.25x (d = 4) and
# 0.27x (d = 16) of the torch ops' time at 4,096 rows and 0.20x / 0.32x at 65,536, and with half of every column on one id 0.03x down to
# 0.004x (profiles/onn_ffm_bwd.txt).  The name stays so that a measurement at another shape has somewhere to put its answer.
ONN_HIP_MIN_ROWS = 0


def _ffm_on_hip(masters, views, rows, min_rows=0):
    """The gate of ONN's pair products inside the autograd step (models/onn.py).  ``masters`` per field the fused table [V_j, F-1, d] or
    None for a sequence field, ``views`` per field its F-1 per-name weights (or a callable giving a sequence field's pooled rows).  On
    the GPU, with gradients enabled, HIP_AUTOGRAD_OPS on, float32 tables, at least ``min_rows`` rows and every view the slot of its
    table, returns the inputs of ops.FieldAwareFunction — dctr_ffm_fwd forward and dctr_ffm_bwd backward, one launch each in place of
    F(F-1) gathers and index-put backwards (profiles/onn_ffm_bwd.txt) — else None: the torch ops."""
    tables = [m for m in masters if m is not None]
    if not (tables and torch.is_grad_enabled() and HIP_AUTOGRAD_OPS and rows >= min_rows
            and all(m.is_cuda and m.dtype == torch.float32 for m in tables)):
        return None
    return ops.FieldAwareFunction.inputs_of(masters, views)


# MLR has no row threshold: at the Criteo shape the autograd step with ops.MLRFunction took 0.20 .. 0.22x of the torch ops' time at 4,096
# rows and 0.16 .. 0.20x at 65,536, and with half of every column on one id 0.15 .. 0.16x down to 0.03x (profiles/mlr.txt; no smaller
# row count was measured).  The name stays so that a measurement at another shape has somewhere to put its answer.
MLR_HIP_MIN_ROWS = 0


# Below this many rows IFM's / DIFM's autograd step keeps the torch ops of InputAwareModel._autograd_logit.  From profiles/ifm_bwd.txt
# (Criteo shape, two runs in one call, ms a step with the switch on and the op off / on):
#   IFM   4,096 rows   6.88 / 6.45 and  6.43 / 5.10      65,536 rows  14.61 / 14.32 and 14.52 / 14.37
#   DIFM  4,096 rows   7.49 / 7.83 and  6.62 / 7.05      65,536 rows  50.45 / 51.04 and 50.38 / 50.91
# IFM's op is no slower at both row counts in both runs: no threshold.  DIFM's loses at both (0.94 - 0.96x and 0.99x): its K = 2,496
# product and both of its gradients are three rocBLAS GEMMs on the torch route, and dctr_ifm_fwd + dctr_ifm_bwd's MFMA passes (a wave
# per 16 samples reading kernel^T from L2, 0.97 ms for the backward alone at 65,536 rows) do not beat them.  The default keeps DIFM on
# the torch ops behind an unreachable threshold; its attention stack stays on ops.InteractingFunction.
IFM_HIP_MIN_ROWS = 0
DIFM_HIP_MIN_ROWS = 1 << 62


def _ifm_on_hip(x, min_rows=0):
    """The gate of input_aware_fm inside the autograd step (models/ifm.py), worded as _fieldpair_on_hip: on the GPU, with gradients
    enabled, HIP_AUTOGRAD_OPS on, float32, at least ``min_rows`` rows and a field count dctr_ifm_bwd takes.  x: [B,F,d]."""
    return bool(x.is_cuda and torch.is_grad_enabled() and HIP_AUTOGRAD_OPS and x.dtype == torch.float32 and x.dim() == 3
                and x.shape[0] >= min_rows and ops.ifm_bwd_supported(x.shape[1], x.shape[2]))


def input_aware_fm(x, sources, softmax, terms=None, mprime=None):
    """The input-aware FM over x [B,F,d] inside the autograd step as ONE differentiable op (ops.InputAwareFMFunction: dctr_ifm_fwd
    forward with the factor kept, dctr_ifm_bwd backward): ``sources`` = the (act [B,K], kernel [K,F]) pairs whose products sum to m',
    m = F * softmax(m') with ``softmax`` else m', ``terms`` [B,F] the first-order terms by position or None.  Returns the logit [B]
    without the unrefined tail.  The caller asks _ifm_on_hip first: there is no torch form of this entry."""
    flat = [t for act, kernel in sources for t in (act, kernel)]
    return ops.InputAwareFMFunction.apply(x, terms, mprime, bool(softmax), *flat)


# The row counts at which EDCN's autograd step takes ops.EDCNTowerFunction; outside them it keeps the torch ops of
# _EDCN._autograd_logit.  From profiles/edcn_bwd.txt (26 x 16, cross_num 2, two runs in one call, ms a step with the op off / on):
#                                  4,096 rows                      65,536 rows
#   addition       vector   5.14 / 4.62 and 4.13 / 3.53     11.72 / 14.14 and 11.78 / 14.36
#   addition       matrix   5.24 / 4.56 and 4.17 / 3.88     12.62 / 24.65 and 12.60 / 24.61
#   product        vector   5.14 / 4.57 and 4.20 / 3.50     12.02 / 14.30 and 11.96 / 14.28
#   product        matrix   5.21 / 4.59 and 4.17 / 3.87     12.70 / 24.61 and 12.73 / 24.68
#   concatenation  vector   5.46 / 4.62 and 4.38 / 4.16     15.02 / 28.00 and 15.10 / 28.20
#   concatenation  matrix   5.44 / 4.80 and 4.39 / 4.79     15.83 / 38.04 and 15.88 / 38.24
# The op is no slower at 4,096 rows in 11 of the 12 measurements (1.05 - 1.20x; concatenation x matrix 1.13x and 0.92x) and loses at
# 65,536 in all of them (0.83x down to 0.41x): its row pass holds 16 rows a workgroup, one workgroup per CU, and sits at 0.04 - 0.10 of
# its f32-MFMA bound, while rocBLAS runs the large batch near its own.  A lower threshold alone cannot say "wins at the smaller count,
# loses at the larger": EDCN_HIP_MIN_ROWS is 0 (it wins at the smallest count measured) and EDCN_HIP_MAX_ROWS, the largest count at which
# it was measured to win, closes the range from above.  Not measured: any other row count or shape.
EDCN_HIP_MIN_ROWS = 0
EDCN_HIP_MAX_ROWS = 4096


def _edcn_on_hip(model, x, training):
    """The gate of edcn_tower inside the autograd step (models/edcn.py), worded as _ifm_on_hip: on the GPU, with gradients enabled,
    HIP_AUTOGRAD_OPS on, float32, no BatchNormalization (its training statistics are not the kernel's affine), no active dropout,
    EDCN_HIP_MIN_ROWS .. EDCN_HIP_MAX_ROWS rows, and shapes and options dctr_edcn_bwd takes.  x: [B,F,d]."""
    if not (x.is_cuda and torch.is_grad_enabled() and HIP_AUTOGRAD_OPS and x.dtype == torch.float32 and x.dim() == 3
            and EDCN_HIP_MIN_ROWS <= x.shape[0] <= EDCN_HIP_MAX_ROWS):
        return False
    dnns = model.dnn_layers
    if any(dn.bn_layers for dn in dnns) or (training and any(getattr(dn, "dropout_rate", 0) for dn in dnns)):
        return False
    return ops.edcn_bwd_supported(x.shape[1], x.shape[2], model.cross_num, model.bridge_type, model.parameterization, dnns[0].activation,
                                  model.bridges[0].activation)


def edcn_tower(model, x):
    """EDCN's tower with its head over x [B,F,d] inside the autograd step as ONE differentiable op (ops.EDCNTowerFunction:
    dctr_edcn_train_fwd forward with the tape kept, dctr_edcn_bwd backward).  Returns the logit [B] of Dense(1) over [c, h, br].  The
    caller asks _edcn_on_hip first: there is no torch form of this entry."""
    (gates, cross_w, cross_b, dnn_w, dnn_b), kw = model._tower_args()
    flat = list(gates) + list(cross_w) + list(cross_b) + list(dnn_w) + list(dnn_b)
    if model.bridge_type == "concatenation":
        flat += [b[0] for b in kw["bridge_weights"]] + [b[1] for b in kw["bridge_weights"]]
    opts = (model.bridge_type, model.parameterization, model.tau, kw["activation"], kw["bridge_activation"])
    return ops.EDCNTowerFunction.apply(x, opts, model.dense.w("kernel"), *flat)


def _mlr_mix(z, region_num, bias, task):
    """z [B, K] (columns region 0..R-1, learner R..2R-1, bias 2R) -> MLR's prediction [B] (reference models/mlr.py:45-54)."""
    R = int(region_num)
    s = torch.softmax(z[:, :R], dim=-1)
    a = torch.sigmoid(z[:, R:2 * R]) if task == "binary" else z[:, R:2 * R]
    out = (s * a).sum(-1)
    return out * torch.sigmoid(z[:, 2 * R]) if bias else out


def _mlr_output(model, staged, lo, hi, dtype=None):
    """MLR's PREDICTION [B] of rows [lo, hi) in torch ops from the per-name weights (models/mlr.py: ``groups`` = its 2R (+1) linear
    logits): the CPU suite's restatement, the autograd step on the CPU / under no_grad / with HIP_AUTOGRAD_OPS off, and the baseline of
    scripts/bench_mlr.py.  ``dtype``: compute in that dtype (the tests' float64)."""
    B = hi - lo
    cast = (lambda t: t) if dtype is None else (lambda t: t.to(dtype))
    dense = cast(staged.dense[lo:hi]) if staged.dense is not None else None
    zs = []
    for g in model.groups:
        z = torch.zeros(B, dtype=dtype or torch.float32, device=model.device)
        for fc in g.features:
            w = cast(g.tables[fc.embedding_name].embeddings)
            if isinstance(fc, SparseFeat):
                z = z + w[model.sparse_rows(staged, fc, lo, hi)].reshape(-1)
            else:
                rows = _rows_for(fc, staged.seq[fc.name][lo:hi], True)
                length = staged.length[fc.length_name][lo:hi] if fc.length_name is not None else None
                weight = cast(staged.weight[fc.weight_name][lo:hi]) if fc.weight_name is not None else None
                z = z + _pool(w[rows], fc, rows != 0, length, weight).reshape(-1)
        if g.dense_pos is not None:
            z = z + (dense.index_select(1, g.dense_pos) @ cast(g.linear.w("linear_kernel"))).reshape(-1)
        zs.append(z)
    return _mlr_mix(torch.stack(zs, dim=1), model.region_num, model.has_bias, model.learner_task)


def _mlr_on_hip(plan, views, rows, region_num, bias, min_rows=0):
    """The gate of MLR inside the autograd step (models/mlr.py), _ffm_on_hip's: on the GPU, with gradients enabled, HIP_AUTOGRAD_OPS on,
    at least ``min_rows`` rows, K <= 64 and every view the column of its fused table, returns the inputs of ops.MLRFunction —
    dctr_mlr_fwd forward and dctr_mlr_bwd backward, one launch each in place of K gathers and index-put backwards per feature — else
    None: the torch ops of _mlr_output."""
    tables = [f["master"] for f in plan if f["master"] is not None]
    if not (torch.is_grad_enabled() and HIP_AUTOGRAD_OPS and rows >= min_rows
            and all(m.is_cuda and m.dtype == torch.float32 for m in tables) and ops.mlr_supported(region_num, bias)):
        return None
    return ops.MLRFunction.inputs_of(plan, views)


def senet_bilinear(model, xcat):
    """FiBiNET's DNN input inside the autograd step.  ``model`` carries ``senet``, ``senet_bilinear``, ``bilinear`` (the three layers),
    ``n_fields``, ``emb_dim`` and ``bilinear_type``; ``xcat`` [B, F*E + D] is the torch.cat of the F embedding parts and the dense
    parts.  Returns the whole DNN-input row [B, 2*P*E + D]: per pair the bilinear over the SENET output and the bilinear over x, then
    the dense values.  On the GPU, with gradients enabled and something requiring grad, it is ops.SenetBilinearFunction:
    dctr_bilinear_fwd forward and dctr_bilinear_bwd backward, one launch each, no [B,P,E] tensor and no large cat in HBM
    (profiles/fibinet_bilinear_bwd.txt).  Everything else — the CPU, torch.no_grad(), HIP_AUTOGRAD_OPS off, fewer than
    FIBINET_HIP_MIN_ROWS rows, a shape the backward refuses — takes the torch ops of _bilinear."""
    F, E = model.n_fields, model.emb_dim
    B, D = xcat.shape[0], xcat.shape[1] - F * E
    w12 = list(model.senet.weights_w12)
    ws = w12 + model.senet_bilinear.matrices + model.bilinear.matrices
    if (xcat.is_cuda and torch.is_grad_enabled() and HIP_AUTOGRAD_OPS and xcat.dtype == torch.float32 and B >= FIBINET_HIP_MIN_ROWS
            and (xcat.requires_grad or any(w.requires_grad for w in ws))
            and ops.senet_bilinear_bwd_supported(F, E, model.bilinear_type, "model", w12[0].shape[1])):
        return ops.SenetBilinearFunction.apply(xcat, F, E, D, model.bilinear_type, "model", *ws)
    x = xcat[:, :F * E].reshape(B, F, E)
    a2 = torch.relu(torch.relu(x.mean(-1) @ w12[0]) @ w12[1])
    # concat_func joins the two [B,P,E] outputs on the last axis (reference layers/utils.py:236), then Flatten
    h = torch.cat([_bilinear(model.senet_bilinear, x * a2.unsqueeze(-1)), _bilinear(model.bilinear, x)], dim=-1)
    return torch.cat([h.reshape(B, -1), xcat[:, F * E:]], dim=-1)


def _layer_norm(ln, x):
    """LayerNormalization.call (reference layers/normalization.py:34-43) in torch ops."""
    mean = x.mean(dim=-1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=-1, keepdim=True)
    y = (x - mean) / torch.sqrt(var + ln.eps)
    if ln.scale:
        y = y * ln.w("gamma")
    if ln.center:
        y = y + ln.w("beta")
    return y


def _transformer(layer, queries, keys, query_mask, key_mask, training=False):
    """Transformer.call (reference sequence.py:523-635) in torch ops: queries, keys [B,T,E], bool masks [B,T] -> [B,T,E], or [B,1,E]
    with output_type 'mean' / 'sum'.  Dropout on the attention weights and the feed-forward hidden layer (:609, :623)."""
    B, T, E = queries.shape
    H, d = layer.head_num, layer.att_embedding_size
    if layer.use_positional_encoding:
        scale = float(np.float32(E ** 0.5))
        queries = queries + layer.query_pe.w("lookup_table") * scale
        keys = keys + layer.key_pe.w("lookup_table") * scale

    def heads(x, w):
        return (x @ w).reshape(B, T, H, d).permute(0, 2, 1, 3)                 # [B,H,T,d]
    q, k, v = heads(queries, layer.w("query")), heads(keys, layer.w("key")), heads(keys, layer.w("value"))
    s = q @ k.transpose(-1, -2) / d ** 0.5
    neg = torch.full_like(s, float(-2 ** 32 + 1))
    s = torch.where(key_mask[:, None, None, :], s, neg)
    if layer.blinding:
        s = torch.where(torch.eye(T, dtype=torch.bool, device=s.device)[None, None], neg, s)
    p = torch.softmax(s - s.max(dim=-1, keepdim=True).values, dim=-1) * query_mask[:, None, :, None].to(s.dtype)
    p = _dropout(p, layer.dropout_rate, training)
    r = (p @ v).permute(0, 2, 1, 3).reshape(B, T, E)
    if layer.use_res:
        r = r + queries
    if layer.use_layer_norm:
        r = _layer_norm(layer.ln, r)
    if layer.use_feed_forward:
        f = _dropout(torch.relu(r @ layer.w("fw1")), layer.dropout_rate, training) @ layer.w("fw2")
        if layer.use_res:
            r = r + f
        if layer.use_layer_norm:
            r = _layer_norm(layer.ln, r)
    if layer.output_type == "mean":
        return r.mean(dim=1, keepdim=True)
    if layer.output_type == "sum":
        return r.sum(dim=1, keepdim=True)
    return r


# Below this many rows (samples of the [B, T, E] input) the Transformer's autograd step would stay on the torch ops of _transformer.
# 0: on one MI355X the HIP route won by more than the 3 % boxes differ by at every size measured — 256, 1,024 and 4,096 rows a step,
# BST with one and two layers (T 50, E 32) by 3.9 .. 15 %, DSIN (T 10, 5 sessions) at E 32 by 6.9 .. 8.7 % and at E 64 by 3.3 .. 5.8 %
# (profiles/transformer_bwd.txt).
TRANSFORMER_HIP_MIN_ROWS = 0


def transformer(layers, x, query_mask, key_mask, training=False, lengths=None, keys=None):
    """A stack of Transformer layers over x [B,T,E] inside the autograd step; bool masks [B,T] as _transformer takes them, or with
    ``lengths`` (int32 [B], both masks then being t < length) the lengths form.  On the GPU, with gradients enabled and something
    requiring grad, the whole stack is ONE ops.TransformerFunction: dctr_transformer_train_fwd forward (a tape of the layers' inputs)
    and dctr_transformer_bwd backward, where _transformer runs some twenty-five torch ops per layer and autograd replays them.
    Everything else — the CPU, torch.no_grad(), HIP_AUTOGRAD_OPS off, another dtype, an active dropout, separate ``keys``, layers that
    differ in their options or pool before the last one, fewer than TRANSFORMER_HIP_MIN_ROWS rows, a shape the backward refuses — takes _transformer, layer by
    layer (the keys of a layer past the first are its queries)."""
    layers = list(layers)
    own_keys = keys is not None and keys is not x
    if (layers and not own_keys and x.is_cuda and torch.is_grad_enabled() and HIP_AUTOGRAD_OPS and x.dtype == torch.float32
            and x.shape[0] >= TRANSFORMER_HIP_MIN_ROWS and not (training and any(l.dropout_rate for l in layers))):
        first = layers[0]
        flags, H, out_type = first.flags(), first.head_num, layers[-1].output_type
        same = all((l.flags(), l.head_num) == (flags, H) for l in layers) and all(l.output_type is None for l in layers[:-1])
        ws = [l.operands().get(name) for l in layers for name in ops.TRANSFORMER_WEIGHTS]
        if not (flags["use_feed_forward"] and flags["use_res"]):        # the reference computes the feed-forward and drops it
            ws = [None if i % 9 in (3, 4) else w for i, w in enumerate(ws)]
        opts = {k: v for k, v in flags.items() if k != "ln_eps"}
        if (same and (x.requires_grad or any(w is not None and w.requires_grad for w in ws))
                and ops.transformer_bwd_supported(x.shape[1], x.shape[2], H, len(layers), output_type=out_type, **opts)):
            if lengths is not None:
                lens = lengths.reshape(-1).to(torch.int32)
                masks = (lens, lens, None, None)
            else:
                masks = (None, None, query_mask.contiguous(), key_mask.contiguous())
            y = ops.TransformerFunction.apply(x, masks[0], masks[1], masks[2], masks[3], H, flags, out_type, *ws)
            return y if out_type is None else y.unsqueeze(1)
    for i, layer in enumerate(layers):
        x = _transformer(layer, x, keys if own_keys and i == 0 else x, query_mask, key_mask, training)
    return x


def _gru(x, lengths, layers, cell="GRU", att_scores=None, scale_input=False, return_sequence=True):
    """DynamicGRU.call (reference sequence.py:786-803) in torch ops: tf's GRUCell / the AGRU and AUGRU cells of contrib/utils.py
    (:208-261, :327-378) under dynamic_rnn's sequence_length rule (contrib/rnn_v2.py:1324-1401) — at t >= length the state is copied
    through and the emitted row is zero.  x [B,T,E], lengths [B], layers [(gate kernel [2E,2E], gate bias [2E], candidate kernel
    [2E,E], candidate bias [E])] stacked, att_scores [B,T] -> [B,T,E], or the final state [B,E]."""
    B, T, E = x.shape
    lengths = lengths.reshape(-1)
    a = None if att_scores is None else att_scores.reshape(B, T)
    if scale_input:
        x = x * a.unsqueeze(-1)
    live = torch.arange(T, device=x.device)[None, :] < lengths[:, None]            # [B,T]
    for wg, bg, wc, bc in layers:
        h = torch.zeros(B, E, dtype=x.dtype, device=x.device)
        rows = []
        for t in range(T):
            xt = x[:, t]
            ru = torch.sigmoid(torch.cat([xt, h], dim=-1) @ wg + bg)
            r, u = ru[:, :E], ru[:, E:]
            c = torch.tanh(torch.cat([xt, r * h], dim=-1) @ wc + bc)
            if cell == "AGRU":
                at = a[:, t:t + 1]
                hn = (1.0 - at) * h + at * c
            else:
                if cell == "AUGRU":
                    u = (1.0 - a[:, t:t + 1]) * u
                hn = u * h + (1.0 - u) * c
            m = live[:, t:t + 1]
            h = torch.where(m, hn, h)
            rows.append(torch.where(m, hn, torch.zeros_like(hn)))
        x = torch.stack(rows, dim=1)
    return x if return_sequence else h


def dynamic_gru(x, lengths, layers, cell="GRU", att_scores=None, scale_input=False, return_sequence=True):
    """DynamicGRU inside the autograd step, the arguments of _gru.  On the GPU, with gradients enabled and something requiring grad,
    every layer is ops.DynamicGRUFunction: dctr_gru_fwd forward and dctr_gru_bwd backward, one launch each where _gru runs T steps of
    some fifteen torch ops and autograd replays them (profiles/dien_gru_bwd.txt: faster at every size measured, so no row threshold).
    A stack of plain layers is one application per layer (a stack with scores is nothing DynamicGRU builds and goes to _gru whole).
    Everything else — the CPU, torch.no_grad(), HIP_AUTOGRAD_OPS off, another dtype, a shape the backward refuses — takes _gru, per
    layer."""
    layers = list(layers)
    if len(layers) != 1 and (cell != "GRU" or scale_input or not layers):       # nothing DynamicGRU builds: a stack is plain
        return _gru(x, lengths, layers, cell, att_scores, scale_input, return_sequence)
    on_hip = x.is_cuda and torch.is_grad_enabled() and HIP_AUTOGRAD_OPS and x.dtype == torch.float32
    need_att = cell != "GRU" or bool(scale_input)
    for i, layer in enumerate(layers):
        seq = bool(return_sequence) or i < len(layers) - 1
        if (on_hip and (x.requires_grad or any(w.requires_grad for w in layer) or (need_att and att_scores.requires_grad))
                and ops.gru_bwd_supported(x.shape[1], x.shape[2], cell, scale_input, seq)):
            x = ops.DynamicGRUFunction.apply(x, lengths, att_scores if need_att else None, cell, bool(scale_input), seq, *layer)
        else:
            x = _gru(x, lengths, [layer], cell, att_scores, scale_input, seq)
    return x


def _bilstm(x, layers, res_layers=0, merge_mode="ave", recurrent_activation="sigmoid", dropout_rate=0.0, training=False):
    """BiLSTM.call (reference sequence.py:375-409) over keras' LSTM in torch ops.  x [B,T,Din]; layers [(fw kernel [D,4u], fw recurrent
    kernel [u,4u], fw bias [4u], bw kernel, bw recurrent kernel, bw bias)], gate order i | f | c~ | o; every step runs (no mask).  The
    backward stack walks t = T-1 .. 0 and its output is put back into time order before the next layer.  ``training``: the input
    dropout of every LSTM, one mask [B,1,D] per LSTM and call shared over the steps (keras' implementation=2).  Returns [B,T,u]
    ([B,T,2u] for 'concat', the pair (fw, bw) for None)."""
    gate = torch.sigmoid if recurrent_activation == "sigmoid" else (lambda z: torch.clamp(0.2 * z + 0.5, 0.0, 1.0))

    def lstm(seq, w, u_, b, backwards):
        B, T, _ = seq.shape
        n = u_.shape[0]
        if training and dropout_rate:
            seq = seq * _dropout(torch.ones_like(seq[:, :1]), dropout_rate, True)
        zx = seq @ w + b
        h = torch.zeros(B, n, dtype=seq.dtype, device=seq.device)
        c = torch.zeros_like(h)
        rows = [None] * T
        for t in (range(T - 1, -1, -1) if backwards else range(T)):
            z = zx[:, t] + h @ u_
            i, f, o = gate(z[:, :n]), gate(z[:, n:2 * n]), gate(z[:, 3 * n:])
            c = f * c + i * torch.tanh(z[:, 2 * n:3 * n])
            h = o * torch.tanh(c)
            rows[t] = h
        return torch.stack(rows, dim=1)

    fw = bw = x
    L = len(layers)
    for li, (wf, uf, bf, wb, ub, bb) in enumerate(layers):
        of, ob = lstm(fw, wf, uf, bf, False), lstm(bw, wb, ub, bb, True)
        if li >= L - res_layers:
            of, ob = of + fw, ob + bw
        fw, bw = of, ob
    if merge_mode == "fw":
        return fw
    if merge_mode == "bw":
        return bw
    if merge_mode == "concat":
        return torch.cat([fw, bw], dim=-1)
    if merge_mode == "sum":
        return fw + bw
    if merge_mode == "ave":
        return (fw + bw) / 2
    if merge_mode == "mul":
        return fw * bw
    if merge_mode is None:
        return fw, bw
    raise ValueError('Invalid merge mode. Merge mode should be one of {"fw","bw","sum", "mul", "ave", "concat", None}')


# Below this many rows BiLSTM's autograd step would stay on the torch ops of _bilstm.  0: on one MI355X the HIP route won at every
# size measured (256, 1,024 and 4,096 rows, E 32 and 64: profiles/dsin_bilstm_bwd.txt).
BILSTM_HIP_MIN_ROWS = 0


def bilstm(x, layers, res_layers=0, merge_mode="ave", recurrent_activation="sigmoid", dropout_rate=0.0, training=False):
    """BiLSTM inside the autograd step, the arguments of _bilstm.  On the GPU, with gradients enabled and something requiring grad,
    both stacks, all layers and all steps are ONE ops.BiLSTMFunction: dctr_bilstm_train_fwd forward (input dropout and a tape of h_t,
    c_t) and dctr_bilstm_bwd backward, where _bilstm runs 2 x layers x T cells of a dozen torch ops and autograd replays them.  The
    dropout masks are drawn by the same calls in the same order as _bilstm draws them (fw then bw, layer by layer), so a seeded step
    sees the same masks on both routes.  Everything else — the CPU, torch.no_grad(), HIP_AUTOGRAD_OPS off, another dtype, fewer than
    BILSTM_HIP_MIN_ROWS rows, hard_sigmoid or a shape the backward refuses — takes _bilstm."""
    layers = [tuple(layer) for layer in layers]
    if not (layers and x.is_cuda and torch.is_grad_enabled() and HIP_AUTOGRAD_OPS and x.dtype == torch.float32
            and x.shape[0] >= BILSTM_HIP_MIN_ROWS and recurrent_activation in ("sigmoid", "hard_sigmoid")
            and (x.requires_grad or any(w.requires_grad for layer in layers for w in layer))
            and ops.bilstm_bwd_supported(x.shape[1], x.shape[2], layers[0][1].shape[0], len(layers), res_layers, merge_mode,
                                         recurrent_activation)):
        return _bilstm(x, layers, res_layers, merge_mode, recurrent_activation, dropout_rate, training)
    masks = None
    if training and dropout_rate:
        B, u = x.shape[0], layers[0][1].shape[0]
        masks = [_dropout(torch.ones(B, 1, x.shape[2] if li == 0 else u, dtype=x.dtype, device=x.device), dropout_rate, True)
                 for li in range(len(layers)) for _ in range(2)]
    return ops.BiLSTMFunction.apply(x, masks, int(res_layers), merge_mode, recurrent_activation, *[w for layer in layers for w in layer])


def _bilinear(layer, x):
    """BilinearInteraction.call (reference interaction.py:1190-1209) in torch ops: x [B,F,E] -> [B,P,E], pairs i < j in
    itertools.combinations order."""
    F = x.shape[1]
    ii, jj = _pair_indices(F)
    if layer.bilinear_type == "all":
        vid = x[:, :F - 1] @ layer.w("bilinear_weight")
    elif layer.bilinear_type == "each":
        vid = torch.einsum("bfe,fed->bfd", x[:, :F - 1], torch.stack(layer.matrices))
    else:
        return torch.einsum("bpe,ped->bpd", x[:, ii], torch.stack(layer.matrices)) * x[:, jj]
    return vid[:, ii] * x[:, jj]


def _fefm(layer, x):
    """FEFMLayer.call (reference interaction.py:1469-1488) in torch ops: x [B,F,E] -> [B,P], pairs i < j in itertools.combinations
    order, x_i^T (W + W^T) x_j."""
    ii, jj = _pair_indices(x.shape[1])
    w = torch.stack(layer.matrices)
    return (torch.einsum("bpe,ped->bpd", x[:, ii], w + w.transpose(1, 2)) * x[:, jj]).sum(-1)


def _field_conv(x, kernels, biases, pools):
    """The conv / pool stack of CCPM and FGCNNLayer in torch ops.  x [B,F,E] (or [B,F,E,C_0]); per stage keras' Conv2D kernel
    [w, 1, C_in, C_out] (or [w, C_in, C_out]) and bias [C_out]: a cross-correlation along the fields under 'same' padding, (w - 1) // 2
    zero rows in front and the rest behind, tanh; then ('kmax', k): the k largest rows in descending order of value, or ('max', p):
    windows of p rows at stride p, the trailing rows dropped.  Returns (last pooled map, every stage's), each channel-last [B,rows,E,C]."""
    h = (x.unsqueeze(-1) if x.dim() == 3 else x).permute(0, 3, 1, 2)          # [B,C,rows,E]
    maps = []
    for kern, bias, (kind, arg) in zip(kernels, biases, pools):
        if kern.dim() == 4:
            kern = kern[:, 0]
        w = kern.shape[0]
        before = (w - 1) // 2
        h = torch.nn.functional.pad(h, (0, 0, before, w - 1 - before))
        h = torch.tanh(torch.nn.functional.conv2d(h, kern.permute(2, 1, 0).unsqueeze(-1), bias))
        if kind == "kmax":
            h = torch.topk(h, int(arg), dim=2, sorted=True).values
        else:
            p, n = int(arg), h.shape[2] // int(arg)
            h = h[:, :, :n * p].reshape(h.shape[0], h.shape[1], n, p, h.shape[3]).amax(dim=3)
        maps.append(h.permute(0, 2, 3, 1))
    return maps[-1], maps


def field_conv_selected(x, kernels, biases, pools, sels=None):
    """The conv / pool stack of _field_conv with its pooling written as an explicit SELECTION, the arguments of _field_conv.  Per stage
    ``sel`` [B,rout,E,C] (int64) is the row of the stage's conv output every pooled element comes from, by the reference's own rules on
    ties: ('kmax', k) the k largest in descending order with equal values in row order (tf.nn.top_k: "if two elements are equal, the
    lower-index element appears first"), ('max', p) the FIRST maximum of every window (what MaxPool's gradient routes to).  The pooled
    map is ``gather(conv output, sel)``, so the gradient of a pooled element reaches exactly the row it was taken from: on an exact tie
    tf.keras and this function move one element, where _field_conv's ``amax`` spreads the gradient evenly over the tied rows and
    ``topk`` promises no order.  Away from exact ties the values and gradients are _field_conv's up to rounding (the convolution is
    summed tap by tap here).  ``sels``: None, or the selection of every stage to pool by instead of choosing (a tape: the pooling then
    makes no choice of its own, whatever the precision).  Returns (last pooled map, every stage's, every stage's sel), the maps
    channel-last [B,rows,E,C]."""
    h = x.unsqueeze(-1) if x.dim() == 3 else x              # [B,rows,E,C]
    maps, chosen = [], []
    for s, (kern, bias, (kind, arg)) in enumerate(zip(kernels, biases, pools)):
        if kern.dim() == 4:
            kern = kern[:, 0]
        w, rows, arg = kern.shape[0], h.shape[1], int(arg)
        before = (w - 1) // 2
        hp = torch.nn.functional.pad(h, (0, 0, 0, 0, before, w - 1 - before))
        z = bias + hp[:, 0:rows] @ kern[0]
        for d in range(1, w):
            z = z + hp[:, d:d + rows] @ kern[d]
        y = torch.tanh(z)
        if sels is not None:
            sel = sels[s].long()
        else:
            with torch.no_grad():
                if kind == "kmax":
                    sel = torch.sort(y, dim=1, descending=True, stable=True).indices[:, :arg]
                else:
                    n = rows // arg
                    win = y[:, :n * arg].reshape(y.shape[0], n, arg, y.shape[2], y.shape[3])
                    # the first maximum, spelled out: the smallest position in the window that holds the window's maximum
                    pos = torch.arange(arg, device=y.device).view(1, 1, arg, 1, 1)
                    first = torch.where(win == win.amax(dim=2, keepdim=True), pos, arg).amin(dim=2)
                    sel = first + (torch.arange(n, device=y.device) * arg).view(1, n, 1, 1)
        h = torch.gather(y, 1, sel)
        maps.append(h)
        chosen.append(sel)
    return maps[-1], maps, chosen


def _fgcnn_layer(layer, x):
    """FGCNNLayer.call (reference interaction.py:994-1020) in torch ops: x [B,F,E] -> the new features [B, new, E]."""
    B, E = x.shape[0], x.shape[2]
    _, maps = _field_conv(x, layer.conv_kernels, layer.conv_biases, layer.pools)
    out = []
    for m, dense in zip(maps, layer.dense_layers):
        out.append(torch.tanh(m.reshape(B, -1) @ dense.w("kernel") + dense.w("bias")).reshape(B, -1, E))
    return torch.cat(out, dim=1)


def model_logits(model, staged, lo, hi, training=False):
    """Pre-sigmoid logits [B] of rows [lo, hi) of any model, torch ops only: the model's own ``autograd_logits``
    (models/_common.py:FeatureModel; every model file overrides its part of it).  ``training`` switches Dice and BatchNormalization
    to batch statistics (and updates their moving statistics) and applies dropout, as tf.keras does inside fit(); the default is
    the inference form the HIP forward implements and the gradient tests differentiate."""
    return model.autograd_logits(staged, lo, hi, training)


class KerasAdam(torch.optim.Optimizer):
    """Adam as tf.keras applies it (optimizer_v2/adam.py, _resource_apply_dense; also what the HIP step's optimizer launch computes):
        lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t);   m = beta1 m + (1 - beta1) g;   v = beta2 v + (1 - beta2) g^2;
        w -= lr_t m / (sqrt(v) + epsilon)
    — epsilon sits beside sqrt(v), NOT beside sqrt(v / (1 - beta2^t)) as in torch.optim.Adam: for gradients around 1e-6 (an l2 penalty's
    2 l w on a row no sample touched) the two move a weight by 0.4 lr and 0.95 lr in the first step."""

    def __init__(self, params, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-7):
        super(KerasAdam, self).__init__(params, dict(lr=lr, beta1=beta1, beta2=beta2, eps=eps))

    @torch.no_grad()
    def step(self, closure=None):
        for group in self.param_groups:
            b1, b2 = group["beta1"], group["beta2"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if not st:
                    st["t"], st["m"], st["v"] = 0, torch.zeros_like(p), torch.zeros_like(p)
                st["t"] += 1
                g = p.grad
                st["m"].mul_(b1).add_(g, alpha=1.0 - b1)
                st["v"].mul_(b2).addcmul_(g, g, value=1.0 - b2)
                lr_t = group["lr"] * (1.0 - b2 ** st["t"]) ** 0.5 / (1.0 - b1 ** st["t"])
                p.addcdiv_(st["m"], st["v"].sqrt().add_(group["eps"]), value=-lr_t)


_OPTS = {"adam": lambda p: KerasAdam(p, lr=1e-3, eps=1e-7), "adagrad": lambda p: torch.optim.Adagrad(p, lr=1e-3, eps=1e-7,
                                                                                                         initial_accumulator_value=0.1),
         "sgd": lambda p: torch.optim.SGD(p, lr=1e-2), "rmsprop": lambda p: torch.optim.RMSprop(p, lr=1e-3, alpha=0.9, eps=1e-7)}


class KerasOptimizer(torch.optim.Optimizer):
    """The update rules of ``deepctr_amd.optimizers`` on torch tensors, for the autograd step — and the float32
    comparison of dctr_opt_apply's tests.  ``opt``: an optimizers object; its schedule is evaluated at ``iterations`` before the
    increment, clipnorm / global_clipnorm / clipvalue act on the gradient as it arrives (the l2 penalties are part of the loss here, so
    it already holds 2 l2 w), and ``iterations`` is written back.  Non-lazy: every element moves on every update."""

    def __init__(self, params, opt):
        super(KerasOptimizer, self).__init__(params, {})
        self.opt = opt
        self.rule = opt._rule()

    def _clipped(self, params):
        opt = self.opt
        grads = [p.grad for p in params]
        if opt.clipnorm is not None:
            grads = [g * (opt.clipnorm / torch.clamp(torch.linalg.vector_norm(g.double()), min=opt.clipnorm)).to(g.dtype) for g in grads]
        elif opt.global_clipnorm is not None:
            total = torch.sqrt(sum(torch.linalg.vector_norm(g.double()) ** 2 for g in grads))
            scale = opt.global_clipnorm / torch.clamp(total, min=opt.global_clipnorm)
            grads = [g * scale.to(g.dtype) for g in grads]
        if opt.clipvalue is not None:
            grads = [g.clamp(-opt.clipvalue, opt.clipvalue) for g in grads]
        return grads

    @torch.no_grad()
    def step(self, closure=None):
        from .optimizers import KIND_ADAGRAD, KIND_ADADELTA, KIND_ADAM, KIND_ADAMAX, KIND_FTRL, KIND_RMSPROP, KIND_SGD
        params = [p for group in self.param_groups for p in group["params"] if p.grad is not None]
        t = int(self.opt.iterations) + 1           # (the object counts: it may serve more than one model)
        r, kind = self.rule, self.rule["kind"]
        lr = self.opt._step_lr(t)             # (Adam / Adamax: with the bias correction, as the HIP launch takes it)
        for p, g in zip(params, self._clipped(params)):
            st = self.state[p]
            if not st:
                st["s"] = [torch.full_like(p, v) for v in r["slots"]]
            s = st["s"]
            if kind == KIND_SGD:
                if not s:
                    p.add_(g, alpha=-lr)
                else:
                    s[0].mul_(r["momentum"]).add_(g, alpha=-lr)
                    if r["nesterov"]:
                        p.add_(s[0], alpha=r["momentum"]).add_(g, alpha=-lr)
                    else:
                        p.add_(s[0])
            elif kind == KIND_ADAGRAD:
                s[0].addcmul_(g, g)
                p.addcdiv_(g, s[0].sqrt().add_(r["eps"]), value=-lr)
            elif kind == KIND_RMSPROP:
                rho = r["beta2"]
                s[0].mul_(rho).addcmul_(g, g, value=1.0 - rho)
                den = s[0]
                if r["centered"]:
                    s[1].mul_(rho).add_(g, alpha=1.0 - rho)
                    den = s[0] - s[1] * s[1]
                if r["momentum"] > 0:
                    s[-1].mul_(r["momentum"]).addcdiv_(g, (den + r["eps"]).sqrt_(), value=lr)
                    p.sub_(s[-1])
                else:
                    p.addcdiv_(g, den.sqrt().add_(r["eps"]), value=-lr)
            elif kind == KIND_ADAM:
                s[0].mul_(r["beta1"]).add_(g, alpha=1.0 - r["beta1"])
                s[1].mul_(r["beta2"]).addcmul_(g, g, value=1.0 - r["beta2"])
                v = s[1]
                if r["amsgrad"]:
                    torch.maximum(s[2], s[1], out=s[2])
                    v = s[2]
                p.addcdiv_(s[0], v.sqrt().add_(r["eps"]), value=-lr)
            elif kind == KIND_ADAMAX:
                s[0].mul_(r["beta1"]).add_(g, alpha=1.0 - r["beta1"])
                torch.maximum(s[1] * r["beta2"], g.abs(), out=s[1])
                p.addcdiv_(s[0], s[1] + r["eps"], value=-lr)
            elif kind == KIND_ADADELTA:
                rho = r["beta2"]
                s[0].mul_(rho).addcmul_(g, g, value=1.0 - rho)
                d = (s[1] + r["eps"]).sqrt_() / (s[0] + r["eps"]).sqrt_() * g
                s[1].mul_(rho).addcmul_(d, d, value=1.0 - rho)
                p.add_(d, alpha=-lr)
            elif kind == KIND_FTRL:
                pw, l1 = -r["lr_power"], r["l1"]
                l2 = r["l2_ftrl"] + r["beta"] / (2.0 * lr)
                gs = g + (2.0 * r["l2_shrinkage"]) * p
                n1 = s[0] + g * g
                pn1, pn0 = (n1.sqrt(), s[0].sqrt()) if pw == 0.5 else (n1.pow(pw), s[0].pow(pw))
                s[1].add_(gs - (pn1 - pn0) / lr * p)
                q = pn1 / lr + 2.0 * l2
                p.copy_(torch.where(s[1].abs() > l1, (torch.sign(s[1]) * l1 - s[1]) / q, torch.zeros_like(p)))
                s[0].copy_(n1)
            else:
                raise ValueError("optimizer kind %r" % (kind,))
        self.opt.iterations = t


def compiled_optimizer(model):
    """What compile() holds, as the two training steps take it: one of _OPTS' names in lower case; an ``optimizers`` object — for one
    of those objects itself, a Keras config dict, a foreign object with ``get_config()`` (a tf.keras optimizer) or a name only
    ``optimizers.get`` knows, converted once and kept while compile() holds the same value; or the value unchanged (a torch.optim
    factory, an unknown name: _fit_torch's business)."""
    from . import optimizers
    opt = model._compiled["optimizer"]
    if isinstance(opt, str):
        if opt.lower() in _OPTS:
            return opt.lower()
        if opt.lower() not in ("adamax", "adadelta", "ftrl"):
            return opt
    elif isinstance(opt, type) and issubclass(opt, optimizers.Optimizer):
        raise ValueError("compile() got the class %s, not an instance: compile(%s(...))" % (opt.__name__, opt.__name__))
    elif isinstance(opt, (optimizers.Optimizer, torch.optim.Optimizer)) or callable(opt):
        return opt
    kept = getattr(model, "_optimizer_object", None)
    if kept is None or kept[0] is not opt:
        kept = model._optimizer_object = (opt, optimizers.get(opt))
    return kept[1]


def torch_optimizer(model, params):
    """The torch.optim.Optimizer of the autograd step for what compile() holds (compiled_optimizer)."""
    from . import optimizers
    opt = compiled_optimizer(model)
    if isinstance(opt, optimizers.Optimizer):
        # kept on the model while compile() holds the same object and the weights are the same tensors, as the HIP step keeps its
        # trainer: a second fit() continues the moments on either path
        kept = getattr(model, "_keras_optimizer", None)
        ptrs = [p.data_ptr() for p in params]
        if kept is None or kept[0].opt is not opt or kept[1] != ptrs or any(a is not b for a, b in zip(kept[0].param_groups[0]["params"], params)):
            kept = model._keras_optimizer = (KerasOptimizer(params, opt), ptrs)
        return kept[0]
    if isinstance(opt, str):
        if opt not in _OPTS:
            raise ValueError("optimizer %r not supported (adam, adagrad, sgd, rmsprop or a torch.optim factory)" % opt)
        return _OPTS[opt](params)
    if callable(opt):
        return opt(params)
    return opt


def permute_staged_(staged, yt, perm, wt=None):
    """Row permutation, IN PLACE, of everything staged per sample (id matrix [F,N], dense [N,ND], sequences, lengths, weights)
    and of the labels (and per-sample loss weights ``wt``): tf.keras' fit(shuffle=True) permutes samples each epoch.  In place so
    that device pointers cached by the launch-argument structs stay valid; ``perm``: int64 tensor on the staged tensors' device."""
    if staged.ids is not None:
        staged.ids.copy_(staged.ids.index_select(1, perm))
    if staged.dense is not None:
        staged.dense.copy_(staged.dense.index_select(0, perm))
    if getattr(staged, "hashed", None) is not None:
        staged.hashed.copy_(staged.hashed.index_select(1, perm))
    for group in (staged.seq, staged.length, staged.weight, getattr(staged, "extra", None) or {}):
        for k in group:
            group[k].copy_(group[k].index_select(0, perm))
    yt.copy_(yt.index_select(0, perm))
    if wt is not None:
        wt.copy_(wt.index_select(0, perm))


class _BatchCursor(object):
    """The batch order of tf.keras.Model.fit over ARRAYS.  Keras feeds them through ONE iterator for the whole fit()
    (TensorLikeDataAdapter: ``should_recreate_iterator()`` is False; the index dataset is ``range(n).repeat(epochs)``, shuffled per
    PASS): with ``steps_per_epoch`` below the batches of a pass, epoch e + 1 continues with the NEXT batches of the same pass — rows
    past ``steps * batch_size`` are trained on, in later epochs — and a new permutation is drawn each time a pass over the arrays
    completes, not at every epoch.  Without ``steps_per_epoch`` an epoch is one pass: permute, then every batch in order."""

    def __init__(self, n_tr, bs, steps, permute):
        self.n_tr, self.bs, self.permute = int(n_tr), int(bs), permute
        self.per_pass = (self.n_tr + self.bs - 1) // self.bs
        self.steps = self.per_pass if steps is None else int(steps)
        self.pos = 0                                     # next batch of the current pass

    def epoch(self):
        """(lo, hi) of this epoch's batches; the cursor stays where the epoch ended."""
        for _ in range(self.steps):
            if self.pos == 0 and self.permute is not None:
                self.permute()                           # a pass begins
            lo = self.pos * self.bs
            yield lo, min(self.n_tr, lo + self.bs)
            self.pos = (self.pos + 1) % self.per_pass


class _DataParallel(object):
    """Data-parallel fit over the ranks of a torch.distributed process group (one process per GPU; "nccl" = RCCL over xGMI, or gloo):
    the reference's only multi-GPU example TRAINS (examples/run_classification_criteo_multi_gpu.py:47-52, keras multi_gpu_model: a
    batch is split over the replicas, their gradients are summed on the host).  Here every rank holds the full (replicated) weights
    and the whole staged training set in the same order; of every global batch [lo, hi) rank r takes the contiguous sub-shard
    ``parallel.shard_bounds(hi - lo, r, world)``, runs forward + backward on it, and the ranks then exchange gradients in THREE
    collectives per step, sized by the rows a step touches rather than by the tables:
      1. all-gather of the per-table counts of touched rows,
      2. all-gather of the touched row numbers (one concatenated list; every rank forms the per-table union),
      3. ONE all-reduce(sum) of [the union rows of every embedding table's gradient (+ its linear table's entries) | every dense
         gradient], each rank's share scaled by B_local / B_global (the loss is a mean over the GLOBAL batch),
    after which every rank applies the same optimizer step to the same gradients: the replicas stay bit-identical with each other.
    At C2 and 8 x 4096 rows that is ~50 MB per step instead of the 177 MB of the tables (C5: 218 MB instead of 34 GB).  The epoch's
    loss is one more all-reduce per epoch.

    Models that take statistics over the batch while training (BatchNormalization: DNN(use_bn=True), layers/core.py:200-201; Dice:
    layers/activation.py:37-64, DIN's default att_activation, models/sequence/din.py:25-27) train with PER-REPLICA statistics — every
    rank normalises its own sub-batch with that sub-batch's mean / variance, exactly what the replicas of keras multi_gpu_model (the
    reference's only multi-GPU form) do.  The STORED statistics (moving_mean / moving_variance, which multi_gpu_model's replicas race to
    assign) ride the step's one all-reduce: every rank moves its copy with its sub-batch's statistics, the copies are then replaced by
    their B_local / B_global-weighted mean = momentum * old + (1 - momentum) * (weighted mean of the replicas' batch statistics), so
    the replicas stay bit-identical with each other here too.  Not the whole-batch statistics: that would take a second exchange in
    the middle of every forward and backward pass, and is not what the reference's replicas compute."""

    def __init__(self, group=None, seed=None, device=None):
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            raise RuntimeError("fit_distributed needs an initialised torch.distributed process group")
        self.dist, self.group = dist, group
        self.world, self.rank = dist.get_world_size(group), dist.get_rank(group)
        self.host = dist.get_backend(group) == "gloo"          # gloo exchanges host tensors (several ranks may share one GPU)
        # device tensors of the collectives live on the MODEL's device (RCCL: one GPU per rank — not on whatever device is current)
        self.device = torch.device(device) if device is not None else (torch.device("cuda", torch.cuda.current_device()) if not self.host else None)
        s = torch.tensor([int(np.random.randint(0, 2 ** 31 - 1)) if seed is None else int(seed)], dtype=torch.int64)
        self._bcast(s)
        self.rng = np.random.RandomState(int(s.item()))         # the SAME shuffle on every rank
        self._tables = None
        self._moving = None

    def _bcast(self, t):
        if self.host:
            self.dist.broadcast(t, src=0, group=self.group)
            return t
        d = t.to(self.device)
        self.dist.broadcast(d, src=0, group=self.group)
        t.copy_(d.cpu())
        return t

    def moving_statistics(self, model):
        """The stored BatchNormalization / Dice statistics of a model (class docstring): they ride the gradient all-reduce."""
        if self._moving is None:
            self._moving = [t for name, t in model.named_weights() if name.rsplit("/", 1)[-1] in ("moving_mean", "moving_variance")]
        return self._moving

    def _all_reduce(self, t):
        if self.host and t.is_cuda:
            h = t.cpu()
            self.dist.all_reduce(h, op=self.dist.ReduceOp.SUM, group=self.group)
            t.copy_(h)
        else:
            self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM, group=self.group)
        return t

    def _all_gather(self, t):
        """[n] -> [world, n]"""
        src = t.cpu() if (self.host and t.is_cuda) else t
        out = torch.empty(self.world * src.numel(), dtype=src.dtype, device=src.device)
        self.dist.all_gather(list(out.chunk(self.world)), src.contiguous(), group=self.group)
        return out.view(self.world, -1).to(t.device)

    def permutation(self, n):
        return self.rng.permutation(n)

    def shard(self, lo, hi):
        from .parallel import shard_bounds
        a, b = shard_bounds(hi - lo, self.rank, self.world)
        return lo + a, lo + b

    # ---- gradient exchange of the HIP step ---------------------------------------------------------------------------------
    def _plan(self, tr):
        """(row-tracked tables with their linear companions, dense parameters) of a trainer."""
        if self._tables is None:
            lin_of = {}
            for f, pt, pl in tr.field_params:
                if pl is not None and getattr(pt, "touched", None) is not None and getattr(pl, "g", None) is not None \
                        and pl.w.shape[0] == pt.w.shape[0] and id(pl) not in lin_of:
                    lin_of[id(pl)] = pt
            tables = [p for p in tr.params if p.touched is not None]
            comp = {id(pt): [p for p in tr.params if lin_of.get(id(p)) is pt] for pt in tables}
            taken = {id(p) for ps in comp.values() for p in ps}
            dense = [p for p in tr.params if p.touched is None and id(p) not in taken]
            self._tables = (tables, comp, dense)
        return self._tables

    def exchange(self, tr, b_local, b_global):
        tables, comp, dense = self._plan(tr)
        dev = tr.model.device
        scale = float(b_local) / float(max(b_global, 1))
        rows = [p.touched.view(p.w.shape[0], -1).amax(dim=1).nonzero().view(-1) for p in tables]
        counts = torch.tensor([r.numel() for r in rows], dtype=torch.int64, device=dev)
        all_counts = self._all_gather(counts)                                    # [world, n_tables]
        totals = all_counts.sum(dim=1)
        width = int(totals.max().item())
        mine = torch.zeros(max(width, 1), dtype=torch.int64, device=dev)
        if rows and int(totals[self.rank].item()):
            mine[:int(totals[self.rank].item())] = torch.cat(rows)
        all_rows = self._all_gather(mine)                                        # [world, width]
        offs = torch.cumsum(all_counts, dim=1) - all_counts                      # start of table t in rank r's list
        oc, ac = offs.cpu().tolist(), all_counts.cpu().tolist()
        unions, parts = [], []
        for t, p in enumerate(tables):
            u = torch.unique(torch.cat([all_rows[r, oc[r][t]:oc[r][t] + ac[r][t]] for r in range(self.world)]))
            unions.append(u)
            parts.append(p.g.index_select(0, u).reshape(-1))
            parts.extend(q.g.view(q.w.shape[0], -1).index_select(0, u).reshape(-1) for q in comp[id(p)])
        parts.extend(p.g.reshape(-1) for p in dense)
        moving = self.moving_statistics(tr.model)                  # (scaled like the gradients: their sum is the weighted mean)
        parts.extend(t.reshape(-1) for t in moving)
        flat = torch.cat(parts) if parts else torch.zeros(0, dtype=torch.float32, device=dev)
        if scale != 1.0:
            flat.mul_(scale)
        self._all_reduce(flat)
        o = 0
        for p, u in zip(tables, unions):
            n = u.numel() * p.w.shape[1]
            p.g.index_copy_(0, u, flat[o:o + n].view(u.numel(), -1))
            o += n
            p.touched.view(p.w.shape[0], -1).index_fill_(0, u, 1)                # (rows another rank touched: the update must see them)
            for q in comp[id(p)]:
                k = q.g.numel() // q.w.shape[0]
                q.g.view(q.w.shape[0], -1).index_copy_(0, u, flat[o:o + u.numel() * k].view(u.numel(), -1))
                o += u.numel() * k
        for p in dense:
            n = p.g.numel()
            p.g.copy_(flat[o:o + n].view_as(p.g))
            o += n
        for t in moving:
            n = t.numel()
            t.copy_(flat[o:o + n].view_as(t))
            o += n

    def exchange_torch(self, params, b_local, b_global, moving=()):
        """The torch-autograd step: one flat all-reduce over every .grad (dense tables included — the fallback step is not the fast one)
        and the stored BatchNormalization / Dice statistics ``moving`` (class docstring)."""
        scale = float(b_local) / float(max(b_global, 1))
        flat = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in params] +
                         [t.detach().reshape(-1) for t in moving]) * scale
        self._all_reduce(flat)
        o = 0
        for p in params:
            n = p.numel()
            p.grad = flat[o:o + n].view_as(p).clone()
            o += n
        with torch.no_grad():
            for t in moving:
                n = t.numel()
                t.copy_(flat[o:o + n].view_as(t))
                o += n

    def loss_mean(self, total, count):
        t = torch.tensor([float(total), float(count)], dtype=torch.float64)
        if not self.host:
            t = t.to(self.device)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM, group=self.group)
        return float(t[0].item()) / max(float(t[1].item()), 1.0)


def _fit_hip(model, staged, yt, n_tr, bs, epochs, shuffle, epoch_end, wt=None, steps=None, initial_epoch=0, dp=None):
    """fit() on the HIP training step (training_hip.HipTrainer): no autograd, no torch optimizer.  The trainer (Adam
    moments, step count) lives on the model, so successive fit / train_on_batch calls continue the same optimisation.
    The reported loss is what tf.keras reports: the batch-size-weighted mean over the epoch's steps of [data loss + the l2 penalties
    l * sum(w^2) of the constructor's regularisers at THAT step's weights].  The penalties (they also enter the gradients, as 2 l w inside
    the optimizer launch) are summed by the optimizer launch itself, on the weights it is about to update (dctr_opt_multi_l2 /
    dctr_opt_apply: no further pass over the tables).  Only a model whose optimizer segments do not carry exactly its regularisers
    (checked below, by value) keeps the penalties of the epoch's two ends, averaged; tests/test_gpu_l2.py holds that none does."""
    from .training_hip import trainer_for
    tr = trainer_for(model)
    perm_of = np.random.permutation if dp is None else dp.permutation
    cursor = _BatchCursor(n_tr, bs, steps, (lambda: permute_staged_(
        staged, yt, torch.from_numpy(perm_of(n_tr)).to(yt.device), wt)) if shuffle else None)
    frozen = frozen_weights(model)
    regs = [(t, l2) for t, l2 in regularized_weights(model) if t.data_ptr() not in frozen]

    # every regularised, trainable weight should be a segment of the optimizer launch with its l2 (the trainer packs some of them —
    # CrossNet kernels — into tensors of its own): checked by value, once; a model whose segments do not carry exactly the regularisers
    # keeps the penalties of the epoch's two ends, averaged
    pen_model = l2_penalty(model, regs)
    pen_segs = sum(float(p.l2) * float(torch.linalg.vector_norm(p.w.detach().reshape(-1), dtype=torch.float64).item()) ** 2
                   for p in tr.params if getattr(p, "l2", 0.0))
    exact = abs(pen_model - pen_segs) <= 1e-9 * max(abs(pen_model), abs(pen_segs)) + 1e-30
    pen_acc = torch.zeros(1, dtype=torch.float64, device=model.device) if exact else None
    tr.penalty_acc = pen_acc
    try:
        return _fit_hip_epochs(model, tr, staged, yt, wt, cursor, dp, epochs, initial_epoch, epoch_end, pen_acc,
                               None if exact else (lambda: l2_penalty(model, regs)), pen_model)
    finally:
        tr.penalty_acc, tr.penalty_rows = None, 0


def _fit_hip_epochs(model, tr, staged, yt, wt, cursor, dp, epochs, initial_epoch, epoch_end, pen_acc, penalty, pen0):
    for ep in range(initial_epoch, epochs):
        # the epoch's loss: dctr_bce_grad adds every batch's summed loss into that batch's element of ONE device vector (summed in
        # float64 at the end of the epoch; step() refreshes the weight-derived buffers itself) — no per-step zero / divide / add launches
        # and no host round trip for it
        tot = torch.zeros(max(cursor.steps, 1), dtype=torch.float32, device=model.device)
        if pen_acc is not None:
            pen_acc.zero_()
        seen = rows = 0
        for i, (lo, hi) in enumerate(cursor.epoch()):
            tr.penalty_rows = int(hi - lo)                   # (the GLOBAL batch: replicas hold the same weights, every rank sums the same penalties)
            rows += int(hi - lo)
            if dp is None:
                tr.step(staged, int(lo), int(hi), yt[lo:hi], loss_acc=tot[i:i + 1], weight=None if wt is None else wt[lo:hi])
                seen += hi - lo
                continue
            a, b = dp.shard(int(lo), int(hi))                # this rank's rows of the global batch
            if b > a:
                tr.step(staged, a, b, yt[a:b], apply=False, loss_acc=tot[i:i + 1], weight=None if wt is None else wt[a:b])
            dp.exchange(tr, b - a, hi - lo)
            tr.apply_update()
            seen += b - a
        model._check_status()
        total = float(tot.double().sum().item())
        mean = total / max(seen, 1) if dp is None else dp.loss_mean(total, seen)
        if pen_acc is not None:
            mean += float(pen_acc.item()) / max(rows, 1)
        else:
            pen1 = penalty()
            mean += 0.5 * (pen0 + pen1)
            pen0 = pen1
        if epoch_end(ep, mean):
            break
    return epoch_end.finish()


_FIT_UNSUPPORTED = ()
_FIT_OPTIONS = ("sample_weight", "class_weight", "steps_per_epoch", "initial_epoch", "validation_steps", "validation_batch_size",
                "validation_freq")
_FIT_IGNORED = ("workers", "use_multiprocessing", "max_queue_size")


class _EpochEnd(object):
    """What runs after every epoch of either training path: validation loss (validation_split rows, or ``validation_data``
    as tf.keras.Model.fit takes it), the History record, the verbose line and the ``callbacks`` protocol the reference's
    examples rely on (docs FAQ: EarlyStopping / ModelCheckpoint): ``on_epoch_end(epoch, logs)`` is called when present and
    ``model.stop_training`` ends the loop.  Callback classes themselves are tf.keras' and out of scope: any object with
    that method works."""

    def __init__(self, model, feed, y, n_tr, n_val, bs, epochs, verbose, validation_data, callbacks, validation_steps=None,
                 validation_batch_size=None, validation_freq=1):
        self.model, self.bs, self.epochs, self.verbose = model, bs, epochs, verbose
        # tf.keras.Model.fit: validation runs at the end of epoch e (1-based) when e % validation_freq == 0 (an int) or e is in
        # validation_freq (a collection); over the first `validation_steps` batches of `validation_batch_size` (default: batch_size)
        # rows when validation_steps is given, else over all validation rows
        self.val_bs = int(validation_batch_size) if validation_batch_size else bs
        self.val_steps = None if validation_steps is None else int(validation_steps)
        self.val_freq = validation_freq if validation_freq is not None else 1
        if isinstance(self.val_freq, (int, np.integer)):
            if int(self.val_freq) < 1:
                raise ValueError("fit(validation_freq=%r): an int >= 1 or a collection of epochs" % (validation_freq,))
        else:
            self.val_freq = set(int(e) for e in self.val_freq)
        self.val = None
        if validation_data is not None:
            if len(validation_data) != 2:
                raise NotImplementedError("fit(validation_data=...) takes (x_val, y_val); sample weights are not supported")
            self.val = (validation_data[0], np.asarray(validation_data[1], dtype=np.float32).reshape(-1))
        elif n_val:
            self.val = ({k: np.asarray(v)[n_tr:] for k, v in feed.items()}, y[n_tr:])
        if self.val is not None and self.val_steps is not None:
            n_rows = int(np.asarray(self.val[1]).shape[0])
            have = (n_rows + self.val_bs - 1) // max(self.val_bs, 1)
            if self.val_steps < 1 or self.val_steps > have:       # (tf.keras: "Your input ran out of data" and a truncated evaluation)
                raise ValueError("fit(validation_steps=%d): the validation arrays hold %d batches of %d" % (self.val_steps, have, self.val_bs))
        self.callbacks = list(callbacks or [])
        self.hist = History()
        self.hist.history["loss"] = []
        self.hist.model = model
        model.stop_training = False
        for cb in self.callbacks:
            if hasattr(cb, "set_model"):
                cb.set_model(model)
            if hasattr(cb, "on_train_begin"):
                cb.on_train_begin({})

    def __call__(self, ep, loss):
        h = self.hist
        h.history["loss"].append(loss)
        h.epoch.append(ep)
        logs = {"loss": loss}
        due = (ep + 1) % int(self.val_freq) == 0 if isinstance(self.val_freq, (int, np.integer)) else (ep + 1) in self.val_freq
        if self.val is not None and due:
            for k, v in self.model.evaluate(self.val[0], self.val[1], batch_size=self.val_bs, steps=self.val_steps, return_dict=True).items():
                logs["val_" + k] = v                      # val_loss and val_<metric> of the compiled metrics
                h.history.setdefault("val_" + k, []).append(v)
        if self.verbose:
            print("Epoch %d/%d - loss: %.4f%s" % (ep + 1, self.epochs, loss,
                                                  (" - val_loss: %.4f" % logs["val_loss"]) if "val_loss" in logs else ""))
        for cb in self.callbacks:
            if hasattr(cb, "on_epoch_end"):
                cb.on_epoch_end(ep, logs)
        return bool(getattr(self.model, "stop_training", False))

    def finish(self):
        for cb in self.callbacks:
            if hasattr(cb, "on_train_end"):
                cb.on_train_end({})
        return self.hist


def fit_model(model, x, y, batch_size=256, epochs=1, verbose=1, validation_split=0.0, shuffle=True, validation_data=None,
              callbacks=None, _dp=None, **kwargs):
    from . import _C
    _C.require_device()
    if model._compiled is None:
        raise RuntimeError("You must compile your model before training/testing. Use `model.compile(optimizer, loss)`.")
    for k, v in kwargs.items():
        if k in _FIT_IGNORED or k in _FIT_OPTIONS:
            continue
        if k in _FIT_UNSUPPORTED:
            if v is None:
                continue
            raise NotImplementedError("fit(%s=...) is not implemented by this build (it would silently train on a different "
                                      "objective if ignored)" % k)
        raise TypeError("fit() got an unexpected keyword argument %r" % k)
    feed = model._as_feed(x)
    n = model._num_rows(feed)
    y = np.asarray(y, dtype=np.float32).reshape(-1)
    n_val = 0 if validation_data is not None else int(n * validation_split)
    n_tr = n - n_val
    tr = {k: np.asarray(v)[:n_tr] for k, v in feed.items()}
    staged = model.stage(tr)
    yt = torch.from_numpy(y[:n_tr]).to(model.device)
    w = loss_weights(y[:n_tr], kwargs.get("sample_weight"), kwargs.get("class_weight"), n, n_tr)
    wt = None if w is None else torch.from_numpy(w).to(model.device)
    loss_name0 = model._compiled["loss"] or ("binary_crossentropy" if model.task == "binary" else "mse")
    from . import training_hip
    if (getattr(model, "hip_training", True) and training_hip.takes_optimizer(model) and training_hip.supported(model)
            and ((loss_name0 in ("binary_crossentropy", "logloss") and model.task == "binary")
                 or (loss_name0 in ("mse", "mean_squared_error") and model.task != "binary"))):
        fit = _fit_hip
    else:
        fit = _fit_torch
    bs = int(batch_size) if batch_size else n_tr
    steps, initial_epoch = kwargs.get("steps_per_epoch"), int(kwargs.get("initial_epoch") or 0)
    if steps is not None:
        steps = int(steps)
        if steps < 1 or steps > (n_tr + bs - 1) // max(bs, 1):
            # tf.keras builds ONE iterator of `epochs` passes over the arrays (_BatchCursor) and stops training with "Your input ran out
            # of data" when the epochs together ask for more batches than that holds: an error here instead of a silently shorter run
            raise ValueError("fit(steps_per_epoch=%d): the arrays hold %d batches of %d" % (steps, (n_tr + bs - 1) // max(bs, 1), bs))
    if initial_epoch < 0:
        raise ValueError("fit(initial_epoch=%d)" % initial_epoch)
    return fit(model, staged, yt, n_tr, bs, epochs, shuffle,
               _EpochEnd(model, feed, y, n_tr, n_val, bs, epochs, verbose, validation_data, callbacks,
                         validation_steps=kwargs.get("validation_steps"), validation_batch_size=kwargs.get("validation_batch_size"),
                         validation_freq=kwargs.get("validation_freq", 1)),
               wt=wt, steps=steps, initial_epoch=initial_epoch, **({} if _dp is None else {"dp": _dp}))


def loss_weights(y, sample_weight, class_weight, n, n_tr):
    """The per-sample loss weights of tf.keras.Model.fit (the reference's models are Keras Models; fit is inherited): ``sample_weight``
    [n] (sliced like the inputs by validation_split) times ``class_weight[label]`` (a dict label -> weight; every label present must
    have an entry, as Keras requires).  None when neither is given.  float32 [n_tr]."""
    if sample_weight is None and not class_weight:
        return None
    w = np.ones(n_tr, dtype=np.float32)
    if sample_weight is not None:
        sw = np.asarray(sample_weight, dtype=np.float32).reshape(-1)
        if sw.shape[0] != n:
            raise ValueError("fit(sample_weight=...): %d weights for %d samples" % (sw.shape[0], n))
        w *= sw[:n_tr]
    if class_weight:
        cw = {float(k): float(v) for k, v in dict(class_weight).items()}
        labels = np.unique(y)
        missing = [float(v) for v in labels if float(v) not in cw]
        if missing:
            raise ValueError("fit(class_weight=...): no weight for the labels %s" % missing)
        for lab in labels:
            w[y == lab] *= np.float32(cw[float(lab)])
    return w


def _fit_torch(model, staged, yt, n_tr, bs, epochs, shuffle, epoch_end, wt=None, steps=None, initial_epoch=0, dp=None):
    """fit() on torch autograd over ``model_logits`` (models / options outside the HIP step).  Device-agnostic torch code: the
    CPU suite drives it directly on CPU-built models; evaluate() of a validation split needs the GPU forward."""
    frozen = frozen_weights(model)
    params = [t for name, t in model.named_weights() if "moving_" not in name and t.data_ptr() not in frozen]
    for t in params:
        t.requires_grad_(True)
    opt = torch_optimizer(model, params)
    loss_name = model._compiled["loss"] or ("binary_crossentropy" if model.task == "binary" else "mse")
    regs = [(t, l2) for t, l2 in regularized_weights(model) if t.data_ptr() not in frozen]
    perm_of = np.random.permutation if dp is None else dp.permutation
    cursor = _BatchCursor(n_tr, bs, steps, (lambda: permute_staged_(
        staged, yt, torch.from_numpy(perm_of(n_tr)).to(yt.device), wt)) if shuffle else None)
    try:
        for ep in range(initial_epoch, epochs):
            tot, cnt = 0.0, 0
            for g_lo, g_hi in cursor.epoch():
                lo, hi = (g_lo, g_hi) if dp is None else dp.shard(int(g_lo), int(g_hi))
                if hi <= lo:                                       # (more ranks than rows in the last batch: zero gradients from here)
                    opt.zero_grad(set_to_none=True)
                    dp.exchange_torch(params, 0, g_hi - g_lo, dp.moving_statistics(model))
                    opt.step()
                    continue
                model._begin()
                logit = model_logits(model, staged, int(lo), int(hi), training=True)
                if getattr(model, "output_kind", "logit") == "prediction":
                    # the model's output is not the sigmoid of a logit (MLR): Keras then clips the probability and takes the logs, so a
                    # clamped row has zero gradient — the formula `shown` has below, differentiated as written (Keras' + 1e-7 inside
                    # the logs is left out there too)
                    if loss_name in ("binary_crossentropy", "logloss") and model.task == "binary":
                        pc = logit.clamp(1e-7, 1.0 - 1e-7)
                        loss = -(yt[lo:hi] * torch.log(pc) + (1.0 - yt[lo:hi]) * torch.log(1.0 - pc))
                    else:
                        loss = torch.nn.functional.mse_loss(logit, yt[lo:hi], reduction="none")
                    shown = loss.detach()
                elif loss_name in ("binary_crossentropy", "logloss") and model.task == "binary":
                    # gradient (p - y) / B from the logit; the VALUE as keras' backend.binary_crossentropy reports it on probabilities
                    # (clipped to [1e-7, 1 - 1e-7]: a saturated row costs 16.1, not |logit|) — the pair the HIP step's dctr_bce_grad forms
                    loss = torch.nn.functional.binary_cross_entropy_with_logits(logit, yt[lo:hi], reduction="none")
                    with torch.no_grad():
                        pc = torch.sigmoid(logit).clamp(1e-7, 1.0 - 1e-7)
                        shown = -(yt[lo:hi] * torch.log(pc) + (1.0 - yt[lo:hi]) * torch.log(1.0 - pc))
                else:
                    pred = torch.sigmoid(logit) if model.task == "binary" else logit
                    loss = torch.nn.functional.mse_loss(pred, yt[lo:hi], reduction="none")
                    shown = loss.detach()
                loss = (loss if wt is None else loss * wt[lo:hi]).mean()      # Keras: sum_b w_b l_b / B
                shown = (shown if wt is None else shown * wt[lo:hi]).mean()
                added = model._autograd_added_loss() if hasattr(model, "_autograd_added_loss") else None
                if added is not None:                               # keras Model.add_loss (DIEN's alpha * auxiliary loss, dien.py:212-213)
                    loss = loss + added
                    shown = shown + added.detach()
                for t, l2 in regs:                                  # keras adds the regularisation losses to the loss
                    pen = l2 * (t * t).sum()
                    loss = loss + pen
                    shown = shown + pen.detach()
                opt.zero_grad(set_to_none=True)
                loss.backward()
                if dp is not None:
                    dp.exchange_torch(params, hi - lo, g_hi - g_lo, dp.moving_statistics(model))
                opt.step()
                tot += float(shown.item()) * (hi - lo)
                cnt += hi - lo
            for t in params:
                t.requires_grad_(False)
            stop = epoch_end(ep, tot / max(cnt, 1) if dp is None else dp.loss_mean(tot, cnt))
            for t in params:
                t.requires_grad_(True)
            if stop:
                break
    finally:
        for t in params:
            t.requires_grad_(False)
    return epoch_end.finish()
