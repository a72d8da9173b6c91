"""FwFM — same signature as ``deepctr.models.fwfm.FwFM`` (reference deepctr/models/fwfm.py:21-71): linear logit + one FwFMLayer per
embedding group named in ``fm_group`` + (optionally) a DNN over the whole DNN input, logits added.

Forward: fused gather (+ linear logit) -> dnn_in -> one ``dctr_fieldpair_fwd`` launch per group (the group's slice of dnn_in read in
place; the first launch folds the linear logit into its own) -> the DNN kernel with dense/kernel as its head, adding the FwFM logits,
the bias and the sigmoid."""
import torch

from .. import ops
from .. import training as tops
from ..engine import EmbeddingStage
from ..feature_column import DEFAULT_GROUP_NAME
from ..layers.base import name_scope
from ..layers.core import DNN, Dense, PredictionLayer
from ..layers.interaction import FwFMLayer
from ._common import FeatureModel


def group_fields(sp, group, what):
    """(first column, n fields, embedding_dim) of one embedding group of an EmbeddingStage, checked as the pair layers need it: the
    reference's concat_func(axis=1) fails on mixed dims, and a group of one field has no pair."""
    first, n, dim = sp.group_slices[group]
    if n < 2:
        raise ValueError("%s: group %r holds %d field(s); a field pair needs at least 2 sparse / sequence fields" % (what, group, n))
    if dim is None:
        dims = sorted(set(f.dim for f in sp.fields[[f.out_offset for f in sp.fields].index(first):][:n]))
        raise ValueError("%s concatenates the embeddings of group %r on axis 1: they need one embedding_dim, got %s" % (what, group, dims))
    return first, n, dim


class _FwFM(FeatureModel):
    def __init__(self, linear_feature_columns, dnn_feature_columns, fm_group, dnn_hidden_units, l2_reg_field_strength, seed, dnn_dropout,
                 dnn_activation, dnn_use_bn, task, device):
        super(_FwFM, self).__init__("FwFM", list(linear_feature_columns) + list(dnn_feature_columns), device, task)
        with name_scope():
            self.build_linear(linear_feature_columns, seed)
            self.build_embeddings(dnn_feature_columns, seed)
            self.stage_plan = EmbeddingStage(self.tables, self.linear_tables, linear_feature_columns, dnn_feature_columns,
                                             device=self.device)
            sp = self.stage_plan
            # `k in fm_group` exactly as the reference evaluates it
            self.groups = [g for g in sp.group_slices if g in fm_group]
            if not self.groups:
                raise ValueError("FwFM: no embedding group of the feature columns is named in fm_group %r" % (fm_group,))
            self.fwfm_layers = []
            for g in self.groups:
                _, n, _ = group_fields(sp, g, "FwFM")
                layer = FwFMLayer(num_fields=n, regularizer=l2_reg_field_strength, device=self.device).build_for()
                self.fwfm_layers.append(self._add(layer))
            self.dnn = self.dense = None
            if dnn_hidden_units:
                self.dnn = self._add(DNN(dnn_hidden_units, dnn_activation, 0, dnn_dropout, dnn_use_bn, seed=seed,
                                         device=self.device).build_for(sp.in_dim))
                self.dense = self._add(Dense(1, use_bias=False, seed=seed, device=self.device).build_for(dnn_hidden_units[-1]))
            self.prediction = self._add(PredictionLayer(task, device=self.device).build_for())

    def _forward(self, staged, lo, hi, out):
        sp = self.stage_plan
        ws = sp.run(staged, lo, hi)
        B = hi - lo
        add = self._logits_to_add(ws)
        bufs = self._per_batch(B, lambda: [torch.zeros(B, dtype=torch.float32, device=self.device) for _ in self.groups])
        for k, (g, layer, y) in enumerate(zip(self.groups, self.fwfm_layers, bufs)):
            first, n, dim = sp.group_slices[g]
            ops.fieldpair(ws["dnn_in"], layer.field_strengths, kind="fwfm", fields=n, dim=dim, x_offset=first, logit=y,
                          add=add[0] if (k == 0 and add) else None)
        rest = list(bufs) + add[1:]
        kw = dict(global_bias=self.prediction.w('global_bias'), sigmoid_out=self.task == "binary", out=out)
        if self.dnn is not None:
            ops.mlp(ws["dnn_in"], self.dnn.kernels, self.dnn.biases, self.dnn.activation, dice=self.dnn.dice_params(),
                    bn=self.dnn.bn_params(), head_w=self.dense.w('kernel'), add=rest, in_dim=sp.in_dim, **kw)
        else:
            ops.mlp(rest[0].reshape(-1, 1), [], [], "linear", head_w=self._one(), add=rest[1:], in_dim=1, **kw)

    def _autograd_logit(self, staged, lo, hi, parts, extra, training):       # fwfm.py:51-66
        logit = torch.zeros(hi - lo, device=self.device)
        for g, layer in zip(self.groups, self.fwfm_layers):
            logit = logit + tops.fwfm_logit(layer, torch.stack(tops._group_embeddings(self.stage_plan, parts, g), dim=1))
        if self.dnn is not None:
            h = tops.dnn_forward(self.dnn, torch.cat(parts, dim=-1), training)
            logit = logit + (h @ self.dense.w("kernel")).reshape(-1)
        return logit


def FwFM(linear_feature_columns, dnn_feature_columns, fm_group=(DEFAULT_GROUP_NAME,), dnn_hidden_units=(256, 128, 64),
         l2_reg_linear=0.00001, l2_reg_embedding=0.00001, l2_reg_field_strength=0.00001, l2_reg_dnn=0, seed=1024, dnn_dropout=0,
         dnn_activation='relu', dnn_use_bn=False, task='binary', device=None):
    """Instantiates the Field-weighted Factorization Machine architecture on the MI355X forward path."""
    m = _FwFM(linear_feature_columns, dnn_feature_columns, fm_group, dnn_hidden_units, l2_reg_field_strength, seed, dnn_dropout,
              dnn_activation, dnn_use_bn, task, device)
    m.regularizers = {"embedding": float(l2_reg_embedding), "linear": float(l2_reg_linear), "dnn": float(l2_reg_dnn)}
    return m
