"""CCPM — same signature as ``deepctr.models.ccpm.CCPM`` (reference deepctr/models/ccpm.py:22-81): linear logit + a DNN over
Flatten of the field-axis conv / k-max pooling stack over the [B, F, E, 1] embedding block, then Dense(1).

Forward: fused gather (+ linear logit) -> dnn_in -> ``dctr_fieldconv_fwd`` (every Conv2D((w, 1), 'same', tanh) and KMaxPooling of the
stack in one launch, the F*E leading columns of dnn_in read in place) into the DNN-input buffer -> the DNN kernel with dense/kernel as
its head, adding the linear logit, the bias and the sigmoid."""
import torch

from .. import ops
from .. import training as tops
from ..engine import EmbeddingStage
from ..feature_column import DenseFeat
from ..layers.base import name_scope
from ..layers.core import DNN, Dense, PredictionLayer
from ..layers.interaction import _Conv2DWeights
from ._common import FeatureModel


def kmax_schedule(n, l):        # noqa: E741
    """The k of every KMaxPooling of a CCPM with l conv layers over n fields: the reference's own expression (ccpm.py:65), evaluated
    as it stands, then min(k, rows) over the rows that reach the layer (ccpm.py:69-70)."""
    ks, rows = [], int(n)
    for i in range(1, l + 1):
        k = max(1, int((1 - pow(i / l, l - i)) * n)) if i < l else 3
        rows = min(k, rows)
        ks.append(rows)
    return ks


class _CCPM(FeatureModel):
    def __init__(self, linear_feature_columns, dnn_feature_columns, conv_kernel_width, conv_filters, dnn_hidden_units, dnn_dropout, seed,
                 task, device):
        if len(conv_kernel_width) != len(conv_filters):
            raise ValueError("conv_kernel_width must have same element with conv_filters")
        if any(isinstance(fc, DenseFeat) for fc in dnn_feature_columns):
            raise ValueError("DenseFeat is not supported in dnn_feature_columns")      # inputs.py:224-225 (support_dense=False)
        super(_CCPM, self).__init__("CCPM", list(linear_feature_columns) + list(dnn_feature_columns), device, task)
        with name_scope():
            self.build_linear(linear_feature_columns, seed)
            self.build_embeddings(dnn_feature_columns, seed)
            self.stage_plan = EmbeddingStage(self.tables, self.linear_tables, linear_feature_columns, dnn_feature_columns,
                                             device=self.device)
            sp = self.stage_plan
            if len(sp.fields) < 1:
                raise ValueError("CCPM convolves over the sparse / sequence fields: dnn_feature_columns has none")
            dims = sorted(set(f.dim for f in sp.fields))
            if len(dims) != 1:
                raise ValueError("CCPM concatenates the sparse / sequence embeddings on axis 1: they need one embedding_dim, got %s" % (dims,))
            F, E = len(sp.fields), dims[0]
            self.n_fields, self.emb_dim = F, E
            self.conv_layers, cin = [], 1
            for width, filters in zip(conv_kernel_width, conv_filters):
                self.conv_layers.append(self._add(_Conv2DWeights(width, cin, filters, device=self.device)))
                cin = int(filters)
            self.pools = [("kmax", k) for k in kmax_schedule(F, len(conv_filters))]
            rows = self.pools[-1][1] if self.pools else F
            self.dnn_in_dim = rows * E * cin
            self.dnn = None
            last = self.dnn_in_dim
            if len(dnn_hidden_units) > 0:
                self.dnn = self._add(DNN(dnn_hidden_units, 'relu', 0, dnn_dropout, False, seed=seed, device=self.device).build_for(last))
                last = dnn_hidden_units[-1]
            self.dense = self._add(Dense(1, use_bias=False, seed=seed, device=self.device).build_for(last))
            self.prediction = self._add(PredictionLayer(task, device=self.device).build_for())

    @property
    def conv_kernels(self):
        return [c.w("kernel") for c in self.conv_layers]

    @property
    def conv_biases(self):
        return [c.w("bias") for c in self.conv_layers]

    def _dnn_input(self, B):
        # (zeros: the row padding to a multiple of 4 floats is never written, and the DNN kernels may read it)
        return self._per_batch(B, lambda: torch.zeros(B, (self.dnn_in_dim + 3) // 4 * 4, dtype=torch.float32, device=self.device))

    def _forward(self, staged, lo, hi, out):
        sp = self.stage_plan
        ws = sp.run(staged, lo, hi)
        buf = ws["dnn_in"]
        if self.conv_layers:
            buf = self._dnn_input(hi - lo)
            ops.field_conv(ws["dnn_in"], self.conv_kernels, self.conv_biases, self.pools, fields=self.n_fields, dim=self.emb_dim, out=buf)
        kw = dict(head_w=self.dense.w('kernel'), add=self._logits_to_add(ws), global_bias=self.prediction.w('global_bias'),
                  sigmoid_out=self.task == "binary", in_dim=self.dnn_in_dim, out=out)
        if self.dnn is not None:
            ops.mlp(buf, self.dnn.kernels, self.dnn.biases, self.dnn.activation, dice=self.dnn.dice_params(), **kw)
        else:
            ops.mlp(buf, [], [], "linear", **kw)

    def _autograd_logit(self, staged, lo, hi, parts, extra, training):       # ccpm.py:58-75
        x = torch.stack(parts[:self.n_fields], dim=1)                        # [B,F,E]
        h = x.unsqueeze(-1)
        if self.conv_layers:
            h = tops._field_conv(x, self.conv_kernels, self.conv_biases, self.pools)[0]
        h = h.reshape(x.shape[0], -1)
        if self.dnn is not None:
            h = tops.dnn_forward(self.dnn, h, training)
        return (h @ self.dense.w("kernel")).reshape(-1)


def CCPM(linear_feature_columns, dnn_feature_columns, conv_kernel_width=(6, 5), conv_filters=(4, 4),
         dnn_hidden_units=(128, 64), l2_reg_linear=1e-5, l2_reg_embedding=1e-5, l2_reg_dnn=0, dnn_dropout=0,
         seed=1024, task='binary', device=None):
    """Instantiates the Convolutional Click Prediction Model architecture on the MI355X forward path."""
    m = _CCPM(linear_feature_columns, dnn_feature_columns, conv_kernel_width, conv_filters, dnn_hidden_units, dnn_dropout, seed, task,
              device)
    m.regularizers = {"embedding": float(l2_reg_embedding), "linear": float(l2_reg_linear), "dnn": float(l2_reg_dnn)}
    return m
