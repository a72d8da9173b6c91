"""AFM — same signature as ``deepctr.models.afm.AFM`` (reference deepctr/models/afm.py:19-61): linear logit + one
AFMLayer (or FM) per embedding group named in ``fm_group``.  SURVEY §8(f) rank 4 sibling; the model-level consumer of
§8 row a11 (``dctr_afm_fwd``), which reads the group's embeddings in place from the gathered DNN-input buffer."""
import torch

from .. import ops
from .. import training as tops
from ..engine import EmbeddingStage
from ..feature_column import DEFAULT_GROUP_NAME, DenseFeat
from ..layers.base import name_scope
from ..layers.core import PredictionLayer
from ..layers.interaction import AFMLayer
from ._common import FeatureModel


class _AFM(FeatureModel):
    def __init__(self, linear_feature_columns, dnn_feature_columns, fm_group, use_attention, attention_factor, l2_reg_att,
                 afm_dropout, seed, task, device):
        super(_AFM, self).__init__("AFM", list(linear_feature_columns) + list(dnn_feature_columns), device, task)
        if any(isinstance(fc, DenseFeat) for fc in dnn_feature_columns):
            raise ValueError("DenseFeat is not supported in dnn_feature_columns")      # inputs.py:201-202 (support_dense=False)
        with name_scope():
            self.build_linear(linear_feature_columns, seed)
            self.build_embeddings(dnn_feature_columns, seed)
            probe = EmbeddingStage(self.tables, self.linear_tables, linear_feature_columns, dnn_feature_columns,
                                   device=self.device)
            # `k in fm_group` exactly as the reference evaluates it (a substring test for the default str argument)
            self.groups = [g for g in probe.group_slices if g in fm_group]
            self.use_attention = bool(use_attention)
            # without attention the reference applies FM per group: those are the gather kernel's FM groups
            self.stage_plan = EmbeddingStage(self.tables, self.linear_tables, linear_feature_columns, dnn_feature_columns,
                                             fm_groups=() if self.use_attention else tuple(self.groups), device=self.device)
            self.afm_layers = []
            if self.use_attention:
                for g in self.groups:
                    first, n, dim = self.stage_plan.group_slices[g]
                    if dim is None:
                        raise ValueError('A `AttentionalFM` layer requires inputs with same shapes')
                    layer = AFMLayer(attention_factor, l2_reg_att, afm_dropout, seed, device=self.device)
                    layer.build([(None, 1, dim)] * n)
                    self.afm_layers.append(self._add(layer))
            self.prediction = self._add(PredictionLayer(task, device=self.device).build_for())
        self.dnn = self.dense = None            # AFM has neither (afm.py:45-58); the HIP training step asks

    def _forward(self, staged, lo, hi, out):
        sp = self.stage_plan
        ws = sp.run(staged, lo, hi)
        B = hi - lo
        add = self._logits_to_add(ws)
        if self.use_attention:
            bufs = self._per_batch(B, lambda: [torch.zeros(B, 1, dtype=torch.float32, device=self.device) for _ in self.groups])
            for g, layer, y in zip(self.groups, self.afm_layers, bufs):
                first, n, dim = sp.group_slices[g]
                ops.afm(ws["dnn_in"][:, first:], layer.w("attention_W"), layer.w("attention_b"), layer.w("projection_h"),
                        layer.w("projection_p"), fields=n, dim=dim, out=y)
            head_in, rest = bufs[0], [b.reshape(-1) for b in bufs[1:]]
        else:
            fms = ([ws["fm"]] + list(ws["fm_extra"])) if sp.fm_group_names else []
            head_in, rest = fms[0].reshape(-1, 1), [f.reshape(-1) for f in fms[1:]]
        one = self._one()
        ops.mlp(head_in, [], [], "linear", head_w=one, add=add + rest, global_bias=self.prediction.w('global_bias'),
                sigmoid_out=self.task == "binary", in_dim=1, out=out)

    def _autograd_logit(self, staged, lo, hi, parts, extra, training):       # afm.py:45-58: one AFMLayer per group (FM: the stage's)
        logit = torch.zeros(hi - lo, device=self.device)
        for g, layer in zip(self.groups, self.afm_layers):
            embs = tops._group_embeddings(self.stage_plan, parts, g)
            ii, jj = tops._pair_indices(len(embs))
            bi = torch.stack([embs[i] for i in ii], dim=1) * torch.stack([embs[j] for j in jj], dim=1)     # [B,P,E]
            att = torch.relu(bi @ layer.w("attention_W") + layer.w("attention_b"))
            score = torch.softmax(att @ layer.w("projection_h"), dim=1)
            att_out = tops._dropout((score * bi).sum(1), getattr(layer, "dropout_rate", 0), training)     # interaction.py:142-143
            logit = logit + (att_out @ layer.w("projection_p")).reshape(-1)
        return logit

    # ---- the HIP training step (training_hip.HipTrainer): no DNN — linear logit + AFMLayer per group (or the gather's FM groups) ------
    def _hip_supported(self):
        # dctr_afm_fwd streams any shape, dctr_afm_bwd holds four samples' tiles in LDS: a group past that trains on the autograd step
        sp = self.stage_plan
        return (self._hip_family_ok(extra_fm=True, need_dnn=False) and not any(getattr(l, "dropout_rate", 0) for l in self.afm_layers)
                and all(ops.afm_bwd_supported(sp.group_slices[g][1], sp.group_slices[g][2], l.attention_factor)
                        for g, l in zip(self.groups, self.afm_layers)))

    def _hip_params(self, tr):          # l2_reg_att applies to attention_W only (interaction.py:100)
        tr.own["afm"] = [(tr.param(l.w("attention_W"), getattr(l, "l2_reg_w", 0.0)), tr.param(l.w("attention_b")),
                          tr.param(l.w("projection_h")), tr.param(l.w("projection_p"))) for l in self.afm_layers]

    def _hip_forward_backward(self, tr, staged, lo, hi, ws, buf, y, binary):
        sp = self.stage_plan
        add = self._hip_add(ws)
        if "afm_out" not in buf:
            buf["afm_out"] = [torch.zeros(hi - lo, 1, dtype=torch.float32, device=self.device) for _ in self.afm_layers]
        outs = buf["afm_out"]
        for g, layer, o in zip(self.groups, self.afm_layers, outs):
            first, n, dim = sp.group_slices[g]
            ops.afm(ws["dnn_in"][:, first:], layer.w("attention_W"), layer.w("attention_b"), layer.w("projection_h"),
                    layer.w("projection_p"), fields=n, dim=dim, out=o)
        head_in = outs[0] if outs else add[0].reshape(-1, 1)
        rest = [o.reshape(-1) for o in outs[1:]] if outs else add[1:]
        ops.mlp(head_in, [], [], "linear", head_w=self._one(), add=(add + rest) if outs else rest,
                global_bias=None if tr.p_gbias is None else tr.p_gbias.w, sigmoid_out=binary, in_dim=1, out=buf["pred"])
        tr._loss_grad(buf, y, binary)
        dx = buf["dx"]
        dx.zero_()                                   # groups outside fm_group contribute nothing to the logit
        for g, layer, ps in zip(self.groups, self.afm_layers, tr.own["afm"]):
            first, n, dim = sp.group_slices[g]
            ops.afm_bwd(ws["dnn_in"][:, first:], n, dim, layer.w("attention_W"), layer.w("attention_b"), layer.w("projection_h"),
                        layer.w("projection_p"), buf["dlogit"], dx[:, first:], ps[0].g, ps[1].g, ps[2].g, ps[3].g)


def AFM(linear_feature_columns, dnn_feature_columns, fm_group=DEFAULT_GROUP_NAME, use_attention=True, attention_factor=8,
        l2_reg_linear=1e-5, l2_reg_embedding=1e-5, l2_reg_att=1e-5, afm_dropout=0, seed=1024, task='binary', device=None):
    """Instantiates the Attentional Factorization Machine architecture on the MI355X forward path."""
    m = _AFM(linear_feature_columns, dnn_feature_columns, fm_group, use_attention, attention_factor, l2_reg_att,
             afm_dropout, seed, task, device)
    m.regularizers = {"embedding": float(l2_reg_embedding), "linear": float(l2_reg_linear), "dnn": 0.0}
    return m
