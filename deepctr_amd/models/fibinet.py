"""FiBiNET — same signature as ``deepctr.models.fibinet.FiBiNET`` (reference deepctr/models/fibinet.py:19-66): linear logit + a DNN over
[Flatten(concat([BilinearInteraction(SENETLayer(embeddings)), BilinearInteraction(embeddings)])), dense values], then Dense(1).

Forward: fused gather (+ linear logit) -> dnn_in -> ``dctr_bilinear_fwd`` (SENET scalars, both bilinear layers and the dense tail in
one launch, the fields' leading F*E columns of dnn_in read in place) into a DNN-input buffer -> the DNN kernel with dense/kernel as its
head, adding the linear logit, the bias and the sigmoid.

fit() runs the autograd step; from training.FIBINET_HIP_MIN_ROWS rows on its DNN input is one differentiable HIP op
(training.senet_bilinear: ``dctr_bilinear_fwd`` forward, ``dctr_bilinear_bwd`` backward)."""
import torch

from .. import ops
from .. import training as tops
from ..engine import EmbeddingStage
from ..layers.base import name_scope
from ..layers.core import DNN, Dense, PredictionLayer
from ..layers.interaction import BilinearInteraction, SENETLayer
from ._common import FeatureModel


def bilinear_flops(F, E, bilinear_type):
    """MFMA FLOP per sample of the two bilinear layers: x_i W per pair ('interaction') or per field ('all' / 'each')."""
    n = F * (F - 1) // 2 if bilinear_type == "interaction" else F - 1
    return 2 * n * 2 * E * E


class _FiBiNET(FeatureModel):
    def __init__(self, linear_feature_columns, dnn_feature_columns, bilinear_type, reduction_ratio, dnn_hidden_units, seed,
                 dnn_dropout, dnn_activation, task, device):
        super(_FiBiNET, self).__init__("FiBiNET", list(linear_feature_columns) + list(dnn_feature_columns), device, task)
        with name_scope():
            self.build_linear(linear_feature_columns, seed)
            self.build_embeddings(dnn_feature_columns, seed)
            self.stage_plan = EmbeddingStage(self.tables, self.linear_tables, linear_feature_columns, dnn_feature_columns,
                                             device=self.device)
            sp = self.stage_plan
            # SENETLayer / BilinearInteraction take the sparse_embedding_list: >= 2 inputs (interaction.py:1094, :1169), and
            # concat_func(axis=1) / the shared [E, E] weights need one embedding_dim
            if len(sp.fields) < 2:
                raise ValueError("FiBiNET's SENETLayer and BilinearInteraction need at least 2 sparse / sequence fields, got %d"
                                 % len(sp.fields))
            dims = set(f.dim for f in sp.fields)
            if len(dims) > 1:
                raise ValueError("FiBiNET concatenates the sparse / sequence embeddings on axis 1: they need one embedding_dim, got %s"
                                 % sorted(dims))
            self.n_fields, self.emb_dim = len(sp.fields), dims.pop()
            self.bilinear_type = bilinear_type
            F, E = self.n_fields, self.emb_dim
            self.senet = self._add(SENETLayer(reduction_ratio, seed, device=self.device).build_for(F, E))
            self.senet_bilinear = self._add(BilinearInteraction(bilinear_type, seed, device=self.device).build_for(F, E))
            self.bilinear = self._add(BilinearInteraction(bilinear_type, seed, device=self.device).build_for(F, E))
            self.dnn_in_dim = F * (F - 1) * E + sp.n_dense_dnn
            self.dnn = None
            last = self.dnn_in_dim
            if len(dnn_hidden_units) > 0:
                self.dnn = self._add(DNN(dnn_hidden_units, dnn_activation, 0, dnn_dropout, False, seed=seed,
                                         device=self.device).build_for(self.dnn_in_dim))
                last = dnn_hidden_units[-1]
            self.dense = self._add(Dense(1, use_bias=False, seed=seed, device=self.device).build_for(last))
            self.prediction = self._add(PredictionLayer(task, device=self.device).build_for())

    def _dnn_input(self, B):
        # (zeros: the row padding to a multiple of 4 floats is never written, and the DNN kernels may read it)
        return self._per_batch(B, lambda: torch.zeros(B, (self.dnn_in_dim + 3) // 4 * 4, dtype=torch.float32, device=self.device))

    def _forward(self, staged, lo, hi, out):
        sp = self.stage_plan
        ws = sp.run(staged, lo, hi)
        buf = self._dnn_input(hi - lo)
        ops.senet_bilinear(ws["dnn_in"], senet_w=self.senet.weights_w12, senet_bilinear_w=self.senet_bilinear.matrices,
                           bilinear_w=self.bilinear.matrices, bilinear_type=self.bilinear_type, fields=self.n_fields,
                           dim=self.emb_dim, dense_cols=sp.n_dense_dnn, out=buf)
        kw = dict(head_w=self.dense.w('kernel'), add=self._logits_to_add(ws), global_bias=self.prediction.w('global_bias'),
                  sigmoid_out=self.task == "binary", in_dim=self.dnn_in_dim, out=out)
        if self.dnn is not None:
            ops.mlp(buf, self.dnn.kernels, self.dnn.biases, self.dnn.activation, dice=self.dnn.dice_params(), **kw)
        else:
            ops.mlp(buf, [], [], "linear", **kw)

    def _autograd_logit(self, staged, lo, hi, parts, extra, training):       # fibinet.py:50-63
        # the small cat [B, F*E + D]; training.senet_bilinear returns the whole DNN-input row from it
        h = tops.senet_bilinear(self, torch.cat(parts, dim=-1))
        if self.dnn is not None:
            h = tops.dnn_forward(self.dnn, h, training)
        return (h @ self.dense.w("kernel")).reshape(-1)


def FiBiNET(linear_feature_columns, dnn_feature_columns, bilinear_type='interaction', reduction_ratio=3,
            dnn_hidden_units=(256, 128, 64), l2_reg_linear=1e-5, l2_reg_embedding=1e-5, l2_reg_dnn=0, seed=1024, dnn_dropout=0,
            dnn_activation='relu', task='binary', device=None):
    """Instantiates the Feature Importance and Bilinear feature Interaction NETwork architecture on the MI355X forward path."""
    m = _FiBiNET(linear_feature_columns, dnn_feature_columns, bilinear_type, reduction_ratio, dnn_hidden_units, seed, dnn_dropout,
                 dnn_activation, task, device)
    m.regularizers = {"embedding": float(l2_reg_embedding), "linear": float(l2_reg_linear), "dnn": float(l2_reg_dnn)}
    return m
