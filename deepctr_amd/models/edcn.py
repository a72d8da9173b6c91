"""EDCN — same signature as ``deepctr.models.edcn.EDCN`` (reference deepctr/models/edcn.py:18-94): the parallel Deep & Cross tower with
information sharing at every layer.  Per round a one-layer CrossNet and a one-layer DNN of the input's width D = fields * embedding_dim
run side by side, a BridgeModule joins their outputs, and two RegulationModules (field-wise softmax gates) split the joined vector into
the next round's inputs; Dense(1, use_bias=False) over [cross_out, deep_out, bridge_out] of the last round + the linear logit.

Forward: fused gather (+ linear logit) -> dnn_in -> ``ops.edcn``: ONE ``dctr_edcn_fwd`` launch for the whole tower, head, linear logit,
bias and sigmoid where the library takes the shape on chip, else the layered route.  Training: the autograd step, with
the tower as one differentiable HIP op (``ops.EDCNTowerFunction``) where ``training._edcn_on_hip`` says so, else in torch ops."""
import torch

from .. import ops
from .. import training as tops
from ..engine import EmbeddingStage
from ..feature_column import DenseFeat
from ..layers.activation import require_base_activation
from ..layers.base import name_scope
from ..layers.core import DNN, Dense, PredictionLayer, RegulationModule
from ..layers.interaction import BridgeModule, CrossNet
from ._common import FeatureModel


class _EDCN(FeatureModel):
    def __init__(self, linear_feature_columns, dnn_feature_columns, cross_num, cross_parameterization, bridge_type, tau, seed, dnn_dropout,
                 dnn_use_bn, dnn_activation, task, device):
        if cross_num == 0:
            raise ValueError("Cross layer num must > 0")
        if bridge_type not in BridgeModule.TYPES:
            raise ValueError("bridge_type must be one of %s, got %r" % (", ".join(BridgeModule.TYPES), bridge_type))
        require_base_activation("EDCN", dnn_activation)          # (the fused tower, dctr_edcn_fwd, reads the activation code itself)
        if any(isinstance(fc, DenseFeat) for fc in dnn_feature_columns):
            raise ValueError("DenseFeat is not supported in dnn_feature_columns")      # inputs.py:224-225 (support_dense=False)
        known = set(fc.name for fc in dnn_feature_columns)
        missing = [fc.name for fc in linear_feature_columns if fc.name not in known]
        if missing:
            # (the reference builds its inputs from dnn_feature_columns only and fails here with KeyError)
            raise ValueError("EDCN builds its inputs from dnn_feature_columns: the linear columns %s are not among them" % (missing,))
        super(_EDCN, self).__init__("EDCN", list(dnn_feature_columns), device, task)
        with name_scope():
            self.build_linear(linear_feature_columns, seed)
            self.build_embeddings(dnn_feature_columns, seed)
            self.stage_plan = EmbeddingStage(self.tables, self.linear_tables, linear_feature_columns, dnn_feature_columns,
                                             device=self.device)
            sp = self.stage_plan
            dims = sorted(set(f.dim for f in sp.fields))
            if len(dims) != 1:
                raise ValueError("EDCN concatenates the sparse / sequence embeddings on axis 1: they need one embedding_dim, got %s" % (dims,))
            F, d = len(sp.fields), dims[0]
            self.n_fields, self.emb_dim, self.cross_dim = F, d, F * d
            self.cross_num, self.parameterization, self.bridge_type, self.tau = int(cross_num), cross_parameterization, bridge_type, tau
            reg = lambda: self._add(RegulationModule(tau, device=self.device).build_for(F, d))         # noqa: E731
            # the reference's creation order (edcn.py:67-84): the auto names follow it
            self.regulations = [reg(), reg()]                       # [deep gate, cross gate] of round 0, 1, ...
            self.cross_layers, self.dnn_layers, self.bridges = [], [], []
            for i in range(self.cross_num):
                self.cross_layers.append(self._add(CrossNet(1, parameterization=cross_parameterization, seed=seed,
                                                            device=self.device).build_for(self.cross_dim)))
                self.dnn_layers.append(self._add(DNN([self.cross_dim], dnn_activation, 0, dnn_dropout, dnn_use_bn, seed=seed,
                                                     device=self.device).build_for(self.cross_dim)))
                self.bridges.append(self._add(BridgeModule(bridge_type, device=self.device).build_for(self.cross_dim)))
                if i + 1 < self.cross_num:
                    self.regulations += [reg(), reg()]
            self.dense = self._add(Dense(1, use_bias=False, device=self.device).build_for(3 * self.cross_dim))
            self.prediction = self._add(PredictionLayer(task, device=self.device).build_for())
        self.dnn = None                 # (FeatureModel's single-DNN hooks do not apply: dnn_layers / cross_layers hold one per round)

    def _tower_args(self):
        dnns = self.dnn_layers
        act = dnns[0].activation
        kw = dict(bridge_type=self.bridge_type, parameterization=self.parameterization, tau=self.tau, activation=act,
                  bn=[dn.bn_params()[0] for dn in dnns] if dnns[0].bn_layers else None,
                  dice=[dn.dice_params()[0] for dn in dnns] if dnns[0].dice_layers else None,
                  bridge_weights=[b.weights_for_op() for b in self.bridges] if self.bridges[0].weights_for_op() is not None else None,
                  bridge_activation=self.bridges[0].activation)
        return ([r.g for r in self.regulations], [c.w('kernel0') for c in self.cross_layers], [c.w('bias0') for c in self.cross_layers],
                [dn.w('kernel0') for dn in dnns], [dn.w('bias0') for dn in dnns]), kw

    def route(self):
        """'fused' or 'layered': what ops.edcn does for this model (the library's answer)."""
        return ops.edcn_route(self.n_fields, self.emb_dim, self.cross_num, self.bridge_type, self.parameterization,
                              self.dnn_layers[0].activation, self.bridges[0].activation)

    def _forward(self, staged, lo, hi, out):
        ws = self.stage_plan.run(staged, lo, hi)
        args, kw = self._tower_args()
        ops.edcn(ws["dnn_in"], self.n_fields, self.emb_dim, *args, head_w=self.dense.w('kernel'), add=self._logits_to_add(ws),
                 global_bias=self.prediction.w('global_bias'), sigmoid_out=self.task == "binary", logit=out.reshape(-1), **kw)

    def _autograd_gate(self, layer):
        return torch.softmax(layer.g * layer.tau, dim=1)            # [1, F, 1]

    def _autograd_logit(self, staged, lo, hi, parts, extra, training):       # edcn.py:66-87
        F, d = self.n_fields, self.emb_dim
        x = torch.stack(parts[:F], dim=1)                            # [B, F, d]
        B = x.shape[0]
        if tops._edcn_on_hip(self, x, training):
            return tops.edcn_tower(self, x)                          # one differentiable HIP op
        deep = (x * self._autograd_gate(self.regulations[0])).reshape(B, F * d)
        cross = (x * self._autograd_gate(self.regulations[1])).reshape(B, F * d)
        for i in range(self.cross_num):
            cl, bridge = self.cross_layers[i], self.bridges[i]
            w, b = cl.w("kernel0"), cl.w("bias0").reshape(-1)
            if self.parameterization == "vector":
                c = cross * (cross @ w) + b + cross
            else:
                c = cross * (cross @ w.t() + b) + cross
            h = tops.dnn_forward(self.dnn_layers[i], deep, training)
            if self.bridge_type == "pointwise_addition":
                br = c + h
            elif self.bridge_type == "hadamard_product":
                br = c * h
            elif self.bridge_type == "concatenation":
                br = tops._act(bridge.activation, torch.cat([c, h], dim=-1) @ bridge.dense.w("kernel") + bridge.dense.w("bias"), None, training)
            else:
                att = []
                for dn, t in ((bridge.dense_x, c), (bridge.dense_h, h)):
                    hid = tops._act(dn.activation, t @ dn.w("kernel0") + dn.w("bias0"),
                                    dn.dice_layers[0].params() if dn.dice_layers else None, training)
                    att.append(torch.softmax(hid @ dn.w("kernel1") + dn.w("bias1"), dim=-1))
                br = att[0] * c + att[1] * h
            if i + 1 < self.cross_num:
                b3 = br.reshape(B, F, d)
                deep = (b3 * self._autograd_gate(self.regulations[2 * i + 2])).reshape(B, F * d)
                cross = (b3 * self._autograd_gate(self.regulations[2 * i + 3])).reshape(B, F * d)
        return (torch.cat([c, h, br], dim=-1) @ self.dense.w("kernel")).reshape(-1)


def EDCN(linear_feature_columns, dnn_feature_columns, cross_num=2, cross_parameterization='vector', bridge_type='concatenation', tau=1.0,
         l2_reg_linear=1e-5, l2_reg_embedding=1e-5, l2_reg_cross=1e-5, l2_reg_dnn=0, seed=1024, dnn_dropout=0, dnn_use_bn=False,
         dnn_activation='relu', task='binary', device=None):
    """Instantiates the Enhanced Deep&Cross Network architecture on the MI355X forward path."""
    m = _EDCN(linear_feature_columns, dnn_feature_columns, cross_num, cross_parameterization, bridge_type, tau, seed, dnn_dropout, dnn_use_bn,
              dnn_activation, task, device)
    m.regularizers = {"embedding": float(l2_reg_embedding), "linear": float(l2_reg_linear), "dnn": float(l2_reg_dnn),
                      "cross": float(l2_reg_cross)}
    return m
