"""NFM — same signature as ``deepctr.models.nfm.NFM`` (reference deepctr/models/nfm.py:19-62): linear logit + DNN over
[BiInteractionPooling(embeddings), dense values].  SURVEY §8(f) rank 4 sibling: the gather kernel produces the embeddings
(+ linear logit), ``dctr_bi_interaction_fwd`` pools them into columns reserved in front of the dense values, and the DNN
kernel reads that [E + n_dense] slice in place."""
import torch

from .. import ops
from .. import training as tops
from ..engine import EmbeddingStage
from ..layers.base import name_scope
from ..layers.core import DNN, Dense, PredictionLayer
from ._common import FeatureModel


class _NFM(FeatureModel):
    def __init__(self, linear_feature_columns, dnn_feature_columns, dnn_hidden_units, seed, bi_dropout, dnn_dropout,
                 dnn_activation, task, device):
        super(_NFM, self).__init__("NFM", list(linear_feature_columns) + list(dnn_feature_columns), device, task)
        self.bi_dropout = bi_dropout            # training-time only (nfm.py:52-53); the forward path ignores it
        with name_scope():
            self.build_linear(linear_feature_columns, seed)
            self.build_embeddings(dnn_feature_columns, seed)
            probe = EmbeddingStage(self.tables, self.linear_tables, linear_feature_columns, dnn_feature_columns,
                                   device=self.device)
            dims = set(f.dim for f in probe.fields)
            if len(dims) != 1:
                raise ValueError("NFM needs one embedding_dim for every sparse / sequence feature, got %s" % sorted(dims))
            self.n_emb, self.emb_dim = len(probe.fields), dims.pop()
            self.stage_plan = EmbeddingStage(self.tables, self.linear_tables, linear_feature_columns, dnn_feature_columns,
                                             extra_dims=(("bi_interaction", self.emb_dim),), device=self.device)
            sp = self.stage_plan
            self.dnn_in_dim = self.emb_dim + sp.n_dense_dnn
            self.dnn = self._add(DNN(dnn_hidden_units, dnn_activation, 0, dnn_dropout, False, seed=seed,
                                     device=self.device).build_for(self.dnn_in_dim))
            last = dnn_hidden_units[-1] if len(dnn_hidden_units) else self.dnn_in_dim
            self.dense = self._add(Dense(1, use_bias=False, seed=seed, device=self.device).build_for(last))
            self.prediction = self._add(PredictionLayer(task, device=self.device).build_for())

    def _forward(self, staged, lo, hi, out):
        sp = self.stage_plan
        ws = sp.run(staged, lo, hi)
        off = sp.extra_offsets["bi_interaction"]                # [.. embeddings .. | bi (E) | dense ..]
        ops.bi_interaction(ws["dnn_in"], fields=self.n_emb, dim=self.emb_dim, out=ws["dnn_in"][:, off:])
        ops.mlp(ws["dnn_in"][:, off:], self.dnn.kernels, self.dnn.biases, self.dnn.activation, dice=self.dnn.dice_params(), bn=self.dnn.bn_params(),
                head_w=self.dense.w('kernel'), add=self._logits_to_add(ws), global_bias=self.prediction.w('global_bias'),
                sigmoid_out=self.task == "binary", in_dim=self.dnn_in_dim, out=out)

    def _autograd_logit(self, staged, lo, hi, parts, extra, training):       # nfm.py:49-58: DNN over [BiInteractionPooling, dense]
        x0 = torch.stack(parts[:self.n_emb], dim=1)
        parts[extra["bi_interaction"]] = tops._dropout(0.5 * (x0.sum(1).pow(2) - (x0 * x0).sum(1)), self.bi_dropout, training)     # nfm.py:52-53
        return super(_NFM, self)._autograd_logit(staged, lo, hi, parts[extra["bi_interaction"]:], extra, training)

    # ---- the HIP training step (training_hip.HipTrainer): BiInteractionPooling (+ Dropout(bi_dropout)) around the DNN step ------------
    def _hip_supported(self):
        return self._hip_family_ok(extra_cols=True)

    def _hip_forward_backward(self, tr, staged, lo, hi, ws, buf, y, binary):
        off, E = self.stage_plan.extra_offsets["bi_interaction"], self.emb_dim
        x, dx = ws["dnn_in"][:, off:], buf["dx"]
        bi_rate = float(self.bi_dropout or 0)
        ops.bi_interaction(ws["dnn_in"], fields=self.n_emb, dim=E, out=x)
        if bi_rate > 0:                 # nfm.py:52-53: Dropout on the pooled vector, in place (layer slot 100 of the step's mask seeds)
            xe = x[:, :E]
            ops.dnn_train_layer(xe, "linear", h=xe, dropout_rate=bi_rate, dropout_seed=tr.dropout_seed(100))
        tr._dnn_step(x, self.dnn_in_dim, buf, y, binary, add=self._hip_add(ws), dx=dx[:, off:])
        dy = dx[:, off:]
        if bi_rate > 0:
            if "bi_dz" not in buf:
                buf["bi_dz"] = torch.empty(x.shape[0], E, dtype=torch.float32, device=self.device)
            dy = ops.dnn_train_layer(x[:, :E], "linear", dropout_rate=bi_rate, dropout_seed=tr.dropout_seed(100), dh=dx[:, off:off + E],
                                     dz=buf["bi_dz"])
        ops.bi_interaction_bwd(ws["dnn_in"], self.n_emb, E, dy, dx)


def NFM(linear_feature_columns, dnn_feature_columns, dnn_hidden_units=(256, 128, 64), l2_reg_embedding=1e-5,
        l2_reg_linear=1e-5, l2_reg_dnn=0, seed=1024, bi_dropout=0, dnn_dropout=0, dnn_activation='relu', task='binary',
        device=None):
    """Instantiates the Neural Factorization Machine architecture on the MI355X forward path."""
    m = _NFM(linear_feature_columns, dnn_feature_columns, dnn_hidden_units, seed, bi_dropout, dnn_dropout,
             dnn_activation, task, device)
    m.regularizers = {"embedding": float(l2_reg_embedding), "linear": float(l2_reg_linear), "dnn": float(l2_reg_dnn)}
    return m
