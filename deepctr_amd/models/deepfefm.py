"""DeepFEFM — same signature as ``deepctr.models.deepfefm.DeepFEFM`` (reference deepctr/models/deepfefm.py:23-108): linear logit + the
FEFM logit (the row sum of the FEFMLayer's pair scalars over the default embedding group) + a DNN over [embeddings, dense values, the
pair scalars], with the reference's ablation switches.

Forward: fused gather (+ linear logit) -> dnn_in -> ONE ``dctr_fieldpair_fwd`` launch (the default group's slice of dnn_in read in
place, the P = F(F-1)/2 scalars written into the same row behind the dense columns — the stage lays dnn_in out with a row stride that
leaves room for them — and their sum, plus the linear logit, into one logit vector) -> the DNN kernel with dense/kernel as its head,
adding that logit, the bias and the sigmoid."""
import torch

from .. import ops
from .. import training as tops
from ..engine import EmbeddingStage
from ..feature_column import DEFAULT_GROUP_NAME
from ..layers.base import name_scope
from ..layers.core import DNN, Dense, PredictionLayer
from ..layers.interaction import FEFMLayer
from ._common import FeatureModel
from .fwfm import group_fields


def fieldpair_flops(F, E):
    """FLOP per sample of the FEFM pair scalars: per pair x_i S (2 E^2) and the dot with x_j (2 E)."""
    return F * (F - 1) // 2 * 2 * (E * E + E)


class _DeepFEFM(FeatureModel):
    def __init__(self, linear_feature_columns, dnn_feature_columns, use_fefm, dnn_hidden_units, l2_reg_embedding_field, seed,
                 dnn_dropout, exclude_feature_embed_in_dnn, use_linear, use_fefm_embed_in_dnn, dnn_activation, dnn_use_bn, task, device):
        has_dnn = len(dnn_hidden_units) > 0
        if not has_dnn and not use_fefm and not use_linear:
            raise NotImplementedError      # (deepfefm.py:84-99: no DNN, no FEFM logit, no linear part: the eighth combination)
        super(_DeepFEFM, self).__init__("DeepFEFM", list(linear_feature_columns) + list(dnn_feature_columns), device, task)
        with name_scope():
            self.build_linear(linear_feature_columns, seed)
            self.build_embeddings(dnn_feature_columns, seed)
            self.stage_plan = EmbeddingStage(self.tables, self.linear_tables, linear_feature_columns, dnn_feature_columns,
                                             device=self.device)
            sp = self.stage_plan
            if DEFAULT_GROUP_NAME not in sp.group_slices:
                raise ValueError("DeepFEFM: the FEFMLayer runs over the group %r and no sparse / sequence feature is in it; "
                                 "a field pair needs at least 2" % DEFAULT_GROUP_NAME)
            self.group_first, self.n_fields, self.emb_dim = group_fields(sp, DEFAULT_GROUP_NAME, "DeepFEFM")
            self.n_pairs = self.n_fields * (self.n_fields - 1) // 2
            self.use_fefm, self.use_linear = bool(use_fefm), bool(use_linear)
            self.pairs_in_dnn, self.exclude_embed = bool(use_fefm_embed_in_dnn), bool(exclude_feature_embed_in_dnn)
            self.fefm = self._add(FEFMLayer(l2_reg_embedding_field, device=self.device).build_for(self.n_fields, self.emb_dim))
            if not self.pairs_in_dnn:
                self.dnn_in_dim = sp.in_dim
            elif self.exclude_embed:
                self.dnn_in_dim = self.n_pairs
            else:
                self.dnn_in_dim = sp.in_dim + self.n_pairs
                # the pair scalars land in dnn_in's own rows, behind the dense columns: a wider row stride, nothing copied
                sp.out_stride = (self.dnn_in_dim + 3) // 4 * 4
            self.dnn = None
            last = self.dnn_in_dim
            if has_dnn:
                self.dnn = self._add(DNN(dnn_hidden_units, dnn_activation, 0, dnn_dropout, dnn_use_bn, seed=seed,
                                         device=self.device).build_for(self.dnn_in_dim))
                last = dnn_hidden_units[-1]
            # (the reference builds Dense(1) over the DNN's output — its input when there are no hidden units — whether or not the
            # logit is used: the weight exists under dense/kernel)
            self.dense = self._add(Dense(1, use_bias=False, seed=seed, device=self.device).build_for(last))
            self.prediction = self._add(PredictionLayer(task, device=self.device).build_for())

    def _buffers(self, B):
        def alloc():
            bufs = {"logit": torch.zeros(B, dtype=torch.float32, device=self.device)}
            if self.pairs_in_dnn and self.exclude_embed:
                # (zeros: the row padding to a multiple of 4 floats is never written, and the DNN kernels may read it)
                bufs["pairs"] = torch.zeros(B, (self.n_pairs + 3) // 4 * 4, dtype=torch.float32, device=self.device)
            return bufs
        return self._per_batch(B, alloc)

    def _forward(self, staged, lo, hi, out):
        sp = self.stage_plan
        ws = sp.run(staged, lo, hi)
        bufs = self._buffers(hi - lo)
        add = self._logits_to_add(ws) if self.use_linear else []
        want_pairs = self.pairs_in_dnn and self.dnn is not None
        dnn_x, pairs, off = ws["dnn_in"], None, 0
        if want_pairs:
            if self.exclude_embed:
                dnn_x = pairs = bufs["pairs"]
            else:
                pairs, off = ws["dnn_in"], sp.in_dim
        logit = None
        if want_pairs or self.use_fefm:
            logit = bufs["logit"] if self.use_fefm else None
            fold = add[0] if (logit is not None and add) else None
            ops.fieldpair(ws["dnn_in"], self.fefm.matrices, kind="fefm", fields=self.n_fields, dim=self.emb_dim,
                          x_offset=self.group_first, pairs=pairs, pairs_offset=off, logit=logit, add=fold)
            if fold is not None:
                add = add[1:]
        rest = ([logit] if logit is not None else []) + add
        kw = dict(global_bias=self.prediction.w('global_bias'), sigmoid_out=self.task == "binary", out=out)
        if self.dnn is not None:
            ops.mlp(dnn_x, self.dnn.kernels, self.dnn.biases, self.dnn.activation, dice=self.dnn.dice_params(), bn=self.dnn.bn_params(),
                    head_w=self.dense.w('kernel'), add=rest, in_dim=self.dnn_in_dim, **kw)
        else:
            if not rest:                            # the linear part alone, and no linear feature column
                bufs["logit"].zero_()
                rest = [bufs["logit"]]
            ops.mlp(rest[0].reshape(-1, 1), [], [], "linear", head_w=self._one(), add=rest[1:], in_dim=1, **kw)

    def _autograd_logit(self, staged, lo, hi, parts, extra, training):       # deepfefm.py:62-99: the ablation switches
        # the pairs only when they enter the DNN, their sum only when use_fefm; neither: nothing is computed
        pairs, fefm_logit = tops.fefm_pairs(self.fefm, torch.stack(tops._group_embeddings(self.stage_plan, parts, DEFAULT_GROUP_NAME), dim=1),
                                            want_pairs=self.dnn is not None and self.pairs_in_dnn, want_logit=self.use_fefm)
        logit = torch.zeros(hi - lo, device=self.device)
        if self.dnn is not None:
            if not self.pairs_in_dnn:
                h = torch.cat(parts, dim=-1)
            elif self.exclude_embed:
                h = pairs
            else:
                h = torch.cat(parts + [pairs], dim=-1)
            logit = logit + (tops.dnn_forward(self.dnn, h, training) @ self.dense.w("kernel")).reshape(-1)
        if self.use_fefm:
            logit = logit + fefm_logit
        return logit

    def _autograd_tail(self, logit, lin, fms):
        return super(_DeepFEFM, self)._autograd_tail(logit, lin if self.use_linear else None, fms)


def DeepFEFM(linear_feature_columns, dnn_feature_columns, use_fefm=True, dnn_hidden_units=(256, 128, 64), l2_reg_linear=0.00001,
             l2_reg_embedding_feat=0.00001, l2_reg_embedding_field=0.00001, l2_reg_dnn=0, seed=1024, dnn_dropout=0.0,
             exclude_feature_embed_in_dnn=False, use_linear=True, use_fefm_embed_in_dnn=True, dnn_activation='relu', dnn_use_bn=False,
             task='binary', device=None):
    """Instantiates the DeepFEFM architecture (or, without hidden units, the shallow FEFM) on the MI355X forward path."""
    m = _DeepFEFM(linear_feature_columns, dnn_feature_columns, use_fefm, dnn_hidden_units, l2_reg_embedding_field, seed, dnn_dropout,
                  exclude_feature_embed_in_dnn, use_linear, use_fefm_embed_in_dnn, dnn_activation, dnn_use_bn, task, device)
    m.regularizers = {"embedding": float(l2_reg_embedding_feat), "linear": float(l2_reg_linear), "dnn": float(l2_reg_dnn)}
    return m
