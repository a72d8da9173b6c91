"""FGCNN — same signature as ``deepctr.models.fgcnn.FGCNN`` (reference deepctr/models/fgcnn.py:27-89): linear logit + a DNN over
[Flatten(combined), InnerProductLayer(combined)] with combined = [origin embeddings, FGCNNLayer('fg' embeddings)], then Dense(1).  Two
embedding sets over the same columns: the origin one and one under the table prefix 'fg' that feeds the feature generation.  The
dense values of the dnn columns take no part (fgcnn.py:63-68 drops them).

Forward: two fused gathers (the origin set with the linear logit, the 'fg' set) -> ``dctr_fieldconv_fwd`` over the 'fg' block (the whole
conv / max-pooling stack in one launch) -> each stage's recombination Dense through the DNN kernel straight into the combined
[B, (F + new) E] buffer -> ``dctr_inner_product_fwd`` over its F + new fields into the columns behind them -> the DNN kernel with
the Dense(1) kernel as its head, adding the linear logit, the bias and the sigmoid."""
import torch

from .. import ops
from .. import training as tops
from ..engine import EmbeddingStage
from ..feature_column import DenseFeat
from ..inputs import create_embedding_matrix
from ..layers.base import name_scope
from ..layers.core import DNN, Dense, PredictionLayer
from ..layers.interaction import FGCNNLayer
from ._common import FeatureModel


class _FGCNN(FeatureModel):
    def __init__(self, linear_feature_columns, dnn_feature_columns, conv_kernel_width, conv_filters, new_maps, pooling_width,
                 dnn_hidden_units, dnn_dropout, seed, task, device):
        if not (len(conv_kernel_width) == len(conv_filters) == len(new_maps) == len(pooling_width)):
            raise ValueError("conv_kernel_width,conv_filters,new_maps  and pooling_width must have same length")
        known = set(fc.name for fc in dnn_feature_columns)
        missing = [fc.name for fc in linear_feature_columns if fc.name not in known]
        if missing:
            # (the reference builds its inputs from dnn_feature_columns only, fgcnn.py:56, and fails here with KeyError)
            raise ValueError("FGCNN builds its inputs from dnn_feature_columns: the linear columns %s are not among them" % (missing,))
        super(_FGCNN, self).__init__("FGCNN", list(dnn_feature_columns), device, task)
        emb_cols = [fc for fc in dnn_feature_columns if not isinstance(fc, DenseFeat)]
        with name_scope():
            self.build_linear(linear_feature_columns, seed)
            self.build_embeddings(emb_cols, seed)
            self.fg_tables = create_embedding_matrix(emb_cols, 0, seed, prefix="fg", device=self.device)
            for t in self.fg_tables.values():
                self._add(t)
            self.stage_plan = EmbeddingStage(self.tables, self.linear_tables, linear_feature_columns, emb_cols, device=self.device)
            # the 'fg' set: the same ids through its own tables, no linear part
            self.fg_stage = EmbeddingStage(self.fg_tables, {}, [], emb_cols, device=self.device)
            sp = self.stage_plan
            if len(sp.fields) < 1:
                raise ValueError("FGCNN needs at least one sparse / sequence field in dnn_feature_columns")
            dims = sorted(set(f.dim for f in sp.fields))
            if len(dims) != 1:
                raise ValueError("FGCNN concatenates the sparse / sequence embeddings on axis 1: they need one embedding_dim, got %s" % (dims,))
            F, E = len(sp.fields), dims[0]
            self.n_fields, self.emb_dim = F, E
            self.fgcnn = None
            if len(conv_filters) > 0:
                self.fgcnn = self._add(FGCNNLayer(conv_filters, conv_kernel_width, new_maps, pooling_width, device=self.device)
                                       .build_for(F, E))
            self.n_combined = F + (self.fgcnn.new_features if self.fgcnn is not None else 0)
            Fc = self.n_combined
            self.dnn_in_dim = Fc * E + Fc * (Fc - 1) // 2
            self.dnn = None
            last = self.dnn_in_dim
            if len(dnn_hidden_units) > 0:
                self.dnn = self._add(DNN(dnn_hidden_units, 'relu', 0, dnn_dropout, False, seed=seed, device=self.device).build_for(last))
                last = dnn_hidden_units[-1]
            self.dense = self._add(Dense(1, use_bias=False, seed=seed, device=self.device).build_for(last))
            self.prediction = self._add(PredictionLayer(task, device=self.device).build_for())

    def _dnn_input(self, B):
        # (zeros: the row padding to a multiple of 4 floats is never written, and the DNN kernels may read it)
        return self._per_batch(B, lambda: torch.zeros(B, (self.dnn_in_dim + 3) // 4 * 4, dtype=torch.float32, device=self.device))

    def _begin(self):
        super(_FGCNN, self)._begin()
        self.fg_stage.refresh(None)

    def _forward(self, staged, lo, hi, out):
        sp, F, E, Fc = self.stage_plan, self.n_fields, self.emb_dim, self.n_combined
        ws = sp.run(staged, lo, hi)
        buf = self._dnn_input(hi - lo)
        buf[:, :F * E].copy_(ws["dnn_in"][:, :F * E])
        if self.fgcnn is not None:
            fg = self.fg_stage.run(staged, lo, hi)
            self.fgcnn.run(fg["dnn_in"], buf, out_offset=F * E, fields=F, dim=E)
        if Fc > 1:
            ops.inner_product(buf, True, fields=Fc, dim=E, out=buf[:, Fc * E:])
        kw = dict(head_w=self.dense.w('kernel'), add=self._logits_to_add(ws), global_bias=self.prediction.w('global_bias'),
                  sigmoid_out=self.task == "binary", in_dim=self.dnn_in_dim, out=out)
        if self.dnn is not None:
            ops.mlp(buf, self.dnn.kernels, self.dnn.biases, self.dnn.activation, dice=self.dnn.dice_params(), **kw)
        else:
            ops.mlp(buf, [], [], "linear", **kw)

    def _autograd_logit(self, staged, lo, hi, parts, extra, training):       # fgcnn.py:63-83
        F = self.n_fields
        combined = torch.stack(parts[:F], dim=1)                             # [B,F,E]
        if self.fgcnn is not None:
            fg = torch.stack(tops.stage_forward(self.fg_stage, staged, lo, hi)[0][:F], dim=1)
            combined = torch.cat([combined, tops._fgcnn_layer(self.fgcnn, fg)], dim=1)
        B, Fc = combined.shape[0], combined.shape[1]
        h = combined.reshape(B, -1)
        if Fc > 1:
            ii, jj = tops._pair_indices(Fc)
            h = torch.cat([h, (combined[:, ii] * combined[:, jj]).sum(-1)], dim=-1)
        if self.dnn is not None:
            h = tops.dnn_forward(self.dnn, h, training)
        return (h @ self.dense.w("kernel")).reshape(-1)


def FGCNN(linear_feature_columns, dnn_feature_columns, conv_kernel_width=(7, 7, 7, 7), conv_filters=(14, 16, 18, 20),
          new_maps=(3, 3, 3, 3), pooling_width=(2, 2, 2, 2), dnn_hidden_units=(256, 128, 64), l2_reg_linear=1e-5, l2_reg_embedding=1e-5,
          l2_reg_dnn=0, dnn_dropout=0, seed=1024, task='binary', device=None):
    """Instantiates the Feature Generation by Convolutional Neural Network architecture on the MI355X forward path."""
    m = _FGCNN(linear_feature_columns, dnn_feature_columns, conv_kernel_width, conv_filters, new_maps, pooling_width, dnn_hidden_units,
               dnn_dropout, seed, task, device)
    m.regularizers = {"embedding": float(l2_reg_embedding), "linear": float(l2_reg_linear), "dnn": float(l2_reg_dnn)}
    return m
