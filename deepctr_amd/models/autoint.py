"""AutoInt — same signature as ``deepctr.models.autoint.AutoInt`` (reference deepctr/models/autoint.py:21-84): linear logit + a stack of
InteractingLayers (multi-head self-attention across the fields) over the sparse embeddings, and / or a DNN over the whole DNN input,
joined by one Dense(1) over [Flatten(attention output), DNN output].

Forward: fused gather (+ linear logit) -> dnn_in -> ``dctr_interacting_fwd`` (every layer in one launch, the fields' leading F*E
columns of dnn_in read in place, the attention rows of dense/kernel taken on chip: one logit per row leaves) -> the DNN kernel with
the remaining rows of dense/kernel as its head, adding the linear and attention logits, the bias and the sigmoid."""
import torch

from .. import ops
from .. import training as tops
from ..engine import EmbeddingStage
from ..layers.base import name_scope
from ..layers.core import DNN, Dense, PredictionLayer
from ..layers.interaction import InteractingLayer
from ._common import FeatureModel


def interacting_flops(F, E, d, H, n_layers, use_res=True):
    """FLOP per sample of an InteractingLayer stack: the projections 2 F E_l d H per weight, Q K^T and P V 2 F F d H each."""
    dh, tot, e = d * H, 0, E
    for _ in range(n_layers):
        tot += (4 if use_res else 3) * 2 * F * e * dh + 2 * (2 * F * F * dh)
        e = dh
    return tot


class _AutoInt(FeatureModel):
    def __init__(self, linear_feature_columns, dnn_feature_columns, att_layer_num, att_embedding_size, att_head_num, att_res,
                 dnn_hidden_units, dnn_activation, dnn_use_bn, dnn_dropout, seed, task, device):
        if len(dnn_hidden_units) <= 0 and att_layer_num <= 0:
            raise ValueError("Either hidden_layer or att_layer_num must > 0")
        super(_AutoInt, self).__init__("AutoInt", list(linear_feature_columns) + list(dnn_feature_columns), device, task)
        with name_scope():
            self.build_linear(linear_feature_columns, seed)
            self.build_embeddings(dnn_feature_columns, seed)
            self.stage_plan = EmbeddingStage(self.tables, self.linear_tables, linear_feature_columns, dnn_feature_columns,
                                             device=self.device)
            sp = self.stage_plan
            # concat_func(sparse_embedding_list, axis=1) runs whatever the branches (autoint.py:58)
            dims = set(f.dim for f in sp.fields)
            if len(dims) > 1:
                raise ValueError("AutoInt concatenates the sparse / sequence embeddings on axis 1: they need one embedding_dim, got %s"
                                 % sorted(dims))
            self.n_fields = len(sp.fields)
            self.emb_dim = dims.pop() if dims else 0
            self.att_embedding_size, self.att_head_num, self.att_res = int(att_embedding_size), int(att_head_num), bool(att_res)
            self.att_layers = []
            width = self.emb_dim
            for _ in range(max(int(att_layer_num), 0)):
                layer = InteractingLayer(att_embedding_size, att_head_num, att_res, device=self.device).build_for(width)
                self.att_layers.append(self._add(layer))
                width = self.att_embedding_size * self.att_head_num
            self.att_out_dim = self.n_fields * width if self.att_layers else 0
            self.dnn = None
            last = 0
            if len(dnn_hidden_units) > 0:
                self.dnn = self._add(DNN(dnn_hidden_units, dnn_activation, 0, dnn_dropout, dnn_use_bn, seed=seed,
                                         device=self.device).build_for(sp.in_dim))
                last = dnn_hidden_units[-1]
            self.dense = self._add(Dense(1, use_bias=False, seed=seed, device=self.device).build_for(self.att_out_dim + last))
            self.prediction = self._add(PredictionLayer(task, device=self.device).build_for())

    def _att_weights(self):
        return [layer.weights_qkvr for layer in self.att_layers]

    def _forward(self, staged, lo, hi, out):
        sp = self.stage_plan
        ws = sp.run(staged, lo, hi)
        B = hi - lo
        add = self._logits_to_add(ws)
        kernel = self.dense.w('kernel')
        att = None
        if self.att_layers:
            att = self._per_batch(B, lambda: torch.zeros(B, dtype=torch.float32, device=self.device))
            ops.interacting(ws["dnn_in"], self._att_weights(), self.att_embedding_size, self.att_head_num, self.att_res, False,
                            fields=self.n_fields, dim=self.emb_dim, head_w=kernel[:self.att_out_dim], logit=att)
        if self.dnn is not None:
            ops.mlp(ws["dnn_in"], self.dnn.kernels, self.dnn.biases, self.dnn.activation, dice=self.dnn.dice_params(),
                    bn=self.dnn.bn_params(), head_w=kernel[self.att_out_dim:], add=add + ([att] if att is not None else []),
                    global_bias=self.prediction.w('global_bias'), sigmoid_out=self.task == "binary", in_dim=sp.in_dim, out=out)
        else:
            ops.mlp(att.reshape(-1, 1), [], [], "linear", head_w=self._one(), add=add, global_bias=self.prediction.w('global_bias'),
                    sigmoid_out=self.task == "binary", in_dim=1, out=out)

    def _autograd_logit(self, staged, lo, hi, parts, extra, training):       # autoint.py:55-79
        outs = []
        if self.att_layers:
            h = tops.interacting_stack(self.att_layers, torch.stack(parts[:self.n_fields], dim=1))          # [B,F,E] -> [B,F,d*H]
            outs.append(h.reshape(h.shape[0], -1))
        if self.dnn is not None:
            outs.append(tops.dnn_forward(self.dnn, torch.cat(parts, dim=-1), training))
        return (torch.cat(outs, dim=-1) @ self.dense.w("kernel")).reshape(-1)


def AutoInt(linear_feature_columns, dnn_feature_columns, att_layer_num=3, att_embedding_size=8, att_head_num=2, att_res=True,
            dnn_hidden_units=(256, 128, 64), dnn_activation='relu', l2_reg_linear=1e-5, l2_reg_embedding=1e-5, l2_reg_dnn=0,
            dnn_use_bn=False, dnn_dropout=0, seed=1024, task='binary', device=None):
    """Instantiates the AutoInt Network architecture on the MI355X forward path."""
    m = _AutoInt(linear_feature_columns, dnn_feature_columns, att_layer_num, att_embedding_size, att_head_num, att_res,
                 dnn_hidden_units, dnn_activation, dnn_use_bn, dnn_dropout, seed, task, device)
    m.regularizers = {"embedding": float(l2_reg_embedding), "linear": float(l2_reg_linear), "dnn": float(l2_reg_dnn)}
    return m
