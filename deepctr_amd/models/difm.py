"""DIFM (Dual Input-aware Factorization Machine) — same signature as ``deepctr.models.difm.DIFM`` (reference deepctr/models/difm.py:20-82):
the input-aware factor is the sum of a vector-wise part, Dense(F) over the flattened output of one InteractingLayer(scaling=True) across
the field embeddings, and a bit-wise part, Dense(F) over a DNN on the same embeddings; no softmax.  Everything else is IFM's: the factor
multiplies every field's embedding and, BY POSITION, every first-order weight (see models/ifm.py for the pairing rule, the deep-only
DenseFeat and the refused linear counts).

Forward: fused gather -> dnn_in -> ``dctr_interacting_fwd`` (flattened attention output to HBM) -> the DNN kernel (last hidden layer to
HBM) -> ONE ``dctr_ifm_fwd`` launch with both as factor sources: the two projections summed on chip, refined FM and linear terms, bias,
sigmoid.  ``vector_part_in_kernel = False`` computes the vector-wise product (K = F * d_att * heads, 2,496 at the Criteo defaults) with
``dctr_sgemm`` in front and hands it over as m': faster at small batches, but that GEMM splits K over workgroups with float atomics
there, so the last bits change from run to run (DESIGN.md 4.12 has the figures)"""
import torch

from .. import ops
from .. import training as tops
from ..layers.base import name_scope
from ..layers.core import Dense, PredictionLayer
from ..layers.interaction import InteractingLayer
from .ifm import InputAwareModel, position_order


class _DIFM(InputAwareModel):
    def __init__(self, linear_feature_columns, dnn_feature_columns, att_embedding_size, att_head_num, att_res, dnn_hidden_units, seed,
                 dnn_dropout, dnn_activation, dnn_use_bn, task, device):
        linear_feature_columns, dnn_feature_columns = list(linear_feature_columns or []), list(dnn_feature_columns or [])
        if not len(dnn_hidden_units) > 0:
            raise ValueError("dnn_hidden_units is null!")
        if not position_order(dnn_feature_columns):
            raise ValueError("there are no sparse features")
        super(_DIFM, self).__init__("DIFM", linear_feature_columns + dnn_feature_columns, device, task)
        self.att_embedding_size, self.att_head_num, self.att_res = int(att_embedding_size), int(att_head_num), bool(att_res)
        with name_scope():
            self._build_common("DIFM", linear_feature_columns, dnn_feature_columns, dnn_hidden_units, dnn_activation, dnn_use_bn,
                               dnn_dropout, seed)
            self.att = self._add(InteractingLayer(att_embedding_size, att_head_num, att_res, scaling=True,
                                                  device=self.device).build_for(self.emb_dim))
            self.att_out_dim = self.n_fields * self.att_embedding_size * self.att_head_num
            # creation order of the reference: Dense over the attention output ("dense"), then Dense over the DNN ("dense_1")
            self.dense = self._add(Dense(self.n_fields, use_bias=False, seed=seed, device=self.device).build_for(self.att_out_dim))
            self.dense_1 = self._add(Dense(self.n_fields, use_bias=False, seed=seed, device=self.device).build_for(self.hidden_dim))
            self.prediction = self._add(PredictionLayer(task, device=self.device).build_for())

    vector_part_in_kernel = True       # False: dctr_sgemm computes m_vec in front of the launch (class docstring)

    def _more_buffers(self, B, bufs):
        bufs["att"] = torch.zeros(B, self.att_out_dim, dtype=torch.float32, device=self.device)
        bufs["m_vec"] = torch.zeros(B, self.n_fields, dtype=torch.float32, device=self.device)

    def _autograd_factor(self, x, h):
        att = tops.interacting_stack([self.att], x)
        return att.reshape(att.shape[0], -1) @ self.dense.w("kernel") + h @ self.dense_1.w("kernel")

    def _factor_sources(self, x, h):
        att = tops.interacting_stack([self.att], x)
        return [(att.reshape(att.shape[0], -1), self.dense.w("kernel")), (h, self.dense_1.w("kernel"))], False

    def _hip_min_rows(self):
        return tops.DIFM_HIP_MIN_ROWS

    def _forward(self, staged, lo, hi, out):
        ws, bufs, add, desc = self._stage_run(staged, lo, hi)
        ops.interacting(ws["dnn_in"], [self.att.weights_qkvr], self.att_embedding_size, self.att_head_num, self.att_res, True,
                        fields=self.n_fields, dim=self.emb_dim, out=bufs["att"])
        hidden = self._dnn_hidden(ws, bufs)
        sources, m_vec = [(hidden, self.dense_1.w('kernel'))], None
        if self.vector_part_in_kernel:
            sources.insert(0, (bufs["att"], self.dense.w('kernel')))
        else:
            m_vec = ops.sgemm(bufs["att"], self.dense.w('kernel'), out=bufs["m_vec"])
        ops.ifm(ws["dnn_in"], self.n_fields, self.emb_dim, sources=sources, mprime=m_vec, softmax=False, lin=self.lin_positions,
                lin_desc=desc, add=add, global_bias=self.prediction.w('global_bias'), sigmoid_out=self.task == "binary", out=out,
                status=self.stage_plan.status())


def DIFM(linear_feature_columns, dnn_feature_columns, att_embedding_size=8, att_head_num=8, att_res=True, dnn_hidden_units=(256, 128, 64),
         l2_reg_linear=0.00001, l2_reg_embedding=0.00001, l2_reg_dnn=0, seed=1024, dnn_dropout=0, dnn_activation='relu', dnn_use_bn=False,
         task='binary', device=None):
    """Instantiates the DIFM Network architecture on the MI355X forward path."""
    m = _DIFM(linear_feature_columns, dnn_feature_columns, att_embedding_size, att_head_num, att_res, dnn_hidden_units, seed, dnn_dropout,
              dnn_activation, dnn_use_bn, task, device)
    m.regularizers = {"embedding": float(l2_reg_embedding), "linear": float(l2_reg_linear), "dnn": float(l2_reg_dnn)}
    return m
