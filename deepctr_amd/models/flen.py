"""FLEN — same signature as ``deepctr.models.flen.FLEN`` (reference deepctr/models/flen.py:22-81): linear logit +
Dense(1, use_bias=False) over [FieldWiseBiInteraction(embeddings by group), DNN(whole DNN input)].

The embedding groups (``group_name``) are contiguous column slices of dnn_in (EmbeddingStage.group_slices, the reference's order:
groups by first appearance, SparseFeat before VarLenSparseFeat inside a group).  Forward: fused gather (+ linear logit) -> dnn_in ->
ONE ``dctr_fieldwise_fwd`` launch that reads the slices in place and leaves a [B] logit with head dense/kernel[:d] (the [B, d] vector
never reaches memory) -> the DNN kernel with head dense/kernel[d:], adding that logit, the linear logits, the bias and the sigmoid.
Training: the HIP step (training_hip.HipTrainer) with ``dctr_fieldwise_bwd`` behind the DNN's backward."""
import itertools

import torch

from .. import ops
from .. import training as tops
from ..engine import EmbeddingStage
from ..layers.base import name_scope
from ..layers.core import DNN, Dense, PredictionLayer
from ..layers.interaction import FieldWiseBiInteraction
from ._common import FeatureModel


class _FLEN(FeatureModel):
    def __init__(self, linear_feature_columns, dnn_feature_columns, dnn_hidden_units, seed, dnn_dropout, dnn_activation, dnn_use_bn,
                 task, device):
        super(_FLEN, self).__init__("FLEN", list(linear_feature_columns) + list(dnn_feature_columns), device, task)
        with name_scope():
            self.build_linear(linear_feature_columns, seed)
            self.build_embeddings(dnn_feature_columns, seed)
            self.stage_plan = EmbeddingStage(self.tables, self.linear_tables, linear_feature_columns, dnn_feature_columns,
                                             device=self.device)
            sp = self.stage_plan
            if len(sp.group_slices) < 2:
                raise ValueError('A `Field-Wise Bi-Interaction` layer should be called on a list of at least 2 inputs: FLEN needs '
                                 'sparse / sequence features in at least 2 groups (group_name), got %s' % (list(sp.group_slices),))
            dims = sorted(set(f.dim for f in sp.fields))
            if len(dims) != 1:
                raise ValueError("FLEN concatenates the field-wise vector of every group: the embeddings need one embedding_dim, "
                                 "got %s" % (dims,))
            self.emb_dim = dims[0]
            self.groups = [(first, n) for first, n, _ in sp.group_slices.values()]      # (first column of dnn_in, fields)
            self.fieldwise = self._add(FieldWiseBiInteraction(seed=seed, device=self.device).build_for(len(self.groups), self.emb_dim))
            self.dnn = self._add(DNN(dnn_hidden_units, dnn_activation, 0, dnn_dropout, dnn_use_bn, seed=seed,
                                     device=self.device).build_for(sp.in_dim))
            last = dnn_hidden_units[-1] if len(dnn_hidden_units) else sp.in_dim
            self.dense = self._add(Dense(1, use_bias=False, seed=seed, device=self.device).build_for(self.emb_dim + last))
            self.prediction = self._add(PredictionLayer(task, device=self.device).build_for())

    def _heads(self):
        """dense/kernel's rows for the field-wise vector and for the DNN's output (views of the live weight)."""
        k = self.dense.w('kernel')
        return k[:self.emb_dim], k[self.emb_dim:]

    def _fieldwise_logit(self, dnn_in, logit):
        layer = self.fieldwise
        bias_mf, bias_fm = layer.biases
        ops.fieldwise(dnn_in, self.groups, self.emb_dim, layer.w('kernel_mf'), layer.w('kernel_fm'), bias_mf, bias_fm,
                      head_w=self._heads()[0], logit=logit)

    def _forward(self, staged, lo, hi, out):
        sp = self.stage_plan
        ws = sp.run(staged, lo, hi)
        B = hi - lo
        logit = self._per_batch(B, lambda: torch.zeros(B, dtype=torch.float32, device=self.device))
        self._fieldwise_logit(ws["dnn_in"], logit)
        # (without hidden units the DNN is the identity: the headed zero-layer launch over dnn_in)
        ops.mlp(ws["dnn_in"], self.dnn.kernels, self.dnn.biases, self.dnn.activation, dice=self.dnn.dice_params(), bn=self.dnn.bn_params(),
                head_w=self._heads()[1], add=[logit] + self._logits_to_add(ws), global_bias=self.prediction.w('global_bias'),
                sigmoid_out=self.task == "binary", in_dim=sp.in_dim, out=out)

    def _autograd_logit(self, staged, lo, hi, parts, extra, training):       # flen.py:67-75
        layer, sp = self.fieldwise, self.stage_plan
        xs = [torch.stack(tops._group_embeddings(sp, parts, g), dim=1) for g in sp.group_slices]
        s = [x.sum(1) for x in xs]
        h_mf = sum(layer.w('kernel_mf')[p] * s[i] * s[j] for p, (i, j) in enumerate(itertools.combinations(range(len(s)), 2)))
        h_fm = sum(layer.w('kernel_fm')[g] * (s[g].pow(2) - (x * x).sum(1)) for g, x in enumerate(xs))
        if layer.use_bias:
            h_mf, h_fm = h_mf + layer.w('bias_mf'), h_fm + layer.w('bias_fm')
        h = tops.dnn_forward(self.dnn, torch.cat(parts, dim=-1), training)
        return (torch.cat([h_mf + h_fm, h], dim=-1) @ self.dense.w("kernel")).reshape(-1)

    # ---- the HIP training step (training_hip.HipTrainer): the field-wise launch in front of the DNN step, its backward behind -------
    def _hip_supported(self):
        return self._hip_family_ok() and ops.fieldwise_bwd_supported(self.groups, self.emb_dim)

    def _hip_params(self, tr):
        layer = self.fieldwise
        tr.own["fieldwise"] = dict((k, tr.param(layer.w(k))) for k in ("kernel_mf", "kernel_fm", "bias_mf", "bias_fm"))
        # dense/kernel stays ONE parameter (one optimizer segment); the DNN's head is its rows behind the field-wise vector's
        tr.own["head_fw"] = tr.param_rows(tr.p_head, 0, self.emb_dim)
        tr.p_head = tr.param_rows(tr.p_head, self.emb_dim, None)

    def _hip_forward_backward(self, tr, staged, lo, hi, ws, buf, y, binary):
        sp, layer = self.stage_plan, self.fieldwise
        if "fw_logit" not in buf:
            buf["fw_logit"] = torch.zeros(hi - lo, dtype=torch.float32, device=self.device)
        own, head = tr.own["fieldwise"], tr.own["head_fw"]
        self._fieldwise_logit(ws["dnn_in"], buf["fw_logit"])
        tr._dnn_step(ws["dnn_in"], sp.in_dim, buf, y, binary, add=[buf["fw_logit"]] + self._hip_add(ws))
        bias_mf, bias_fm = layer.biases
        ops.fieldwise_bwd(ws["dnn_in"], self.groups, self.emb_dim, layer.w('kernel_mf'), layer.w('kernel_fm'), bias_mf, bias_fm,
                          dlogit=buf["dlogit"], head_w=head.w, dx=buf["dx"], accumulate=True, d_kernel_mf=own["kernel_mf"].g,
                          d_kernel_fm=own["kernel_fm"].g, d_bias_mf=own["bias_mf"].g, d_bias_fm=own["bias_fm"].g, d_head_w=head.g)


def FLEN(linear_feature_columns, dnn_feature_columns, dnn_hidden_units=(256, 128, 64), l2_reg_linear=0.00001, l2_reg_embedding=0.00001,
         l2_reg_dnn=0, seed=1024, dnn_dropout=0.0, dnn_activation='relu', dnn_use_bn=False, task='binary', device=None):
    """Instantiates the FLEN architecture on the MI355X forward path."""
    m = _FLEN(linear_feature_columns, dnn_feature_columns, dnn_hidden_units, seed, dnn_dropout, dnn_activation, dnn_use_bn, task, device)
    m.regularizers = {"embedding": float(l2_reg_embedding), "linear": float(l2_reg_linear), "dnn": float(l2_reg_dnn)}
    return m
