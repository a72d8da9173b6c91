"""DCNMix — same signature as ``deepctr.models.dcnmix.DCNMix`` (reference deepctr/models/dcnmix.py:22-78): DCN with the
cross part replaced by ``CrossNetMix`` (mixture of low-rank experts).  SURVEY §8(f) rank 4 sibling: DCN's launches with
``dctr_crossnet_mix_fwd`` in place of ``dctr_crossnet_fwd``."""
import torch

from .. import ops
from ..layers.interaction import CrossNetMix
from .dcn import _DCN


class _DCNMix(_DCN):
    fuse_head = False       # (dctr_crossnet_mix_fwd has no fused head: the [cross, deep] stack goes through the Dense(1) launch)

    def __init__(self, linear_feature_columns, dnn_feature_columns, cross_num, dnn_hidden_units, low_rank, num_experts, seed,
                 dnn_dropout, dnn_use_bn, dnn_activation, task, device):
        self._mix = (low_rank, num_experts)
        super(_DCNMix, self).__init__(linear_feature_columns, dnn_feature_columns, cross_num, None, dnn_hidden_units, seed,
                                      dnn_dropout, dnn_use_bn, dnn_activation, task, device, name="DCNMix")

    def _make_cross(self, cross_num, cross_parameterization):
        # the reference passes no seed here: CrossNetMix keeps its default 1024 (dcnmix.py:56-57)
        return CrossNetMix(low_rank=self._mix[0], num_experts=self._mix[1], layer_num=cross_num, device=self.device)

    def _run_cross(self, dnn_in, B, d, stack):
        ops.crossnet_mix(dnn_in, *self._cross_packed, dim=d, out=stack)

    def _autograd_cross(self, x0):                  # CrossNetMix (interaction.py:511-549)
        cr = self.cross
        xl = x0
        for i in range(cr.layer_num):
            U, V, C, b = cr.w("U_list%d" % i), cr.w("V_list%d" % i), cr.w("C_list%d" % i), cr.w("bias%d" % i).reshape(-1)
            gate = torch.softmax(torch.cat([xl @ g.w("kernel") for g in cr.gating], dim=-1), dim=-1)       # [B,experts]
            moe = torch.zeros_like(xl)
            for e in range(cr.num_experts):
                v = torch.tanh(torch.tanh(xl @ V[e]) @ C[e].t())
                moe = moe + gate[:, e:e + 1] * (x0 * (v @ U[e].t() + b))
            xl = moe + xl
        return xl

    # ---- the HIP training step: _DCN's, on CrossNetMix's five packed parameter tensors and dctr_crossnet_mix_fwd / _bwd ---------------
    def _hip_supported(self):
        # dctr_crossnet_mix_fwd takes any number of experts, dctr_crossnet_mix_bwd sixteen: past that the autograd step
        cr = self.cross
        return super(_DCNMix, self)._hip_supported() and (
            cr is None or ops.crossnet_mix_bwd_supported(self.stage_plan.in_dim, cr.layer_num, cr.num_experts, cr.low_rank))

    def _hip_pack_cross(self, tr, l2):
        # U / V / C stacked over layers, the experts' gating kernels, the biases, in the C ABI's layout.  l2 on U / V / C only (the
        # reference regularises U_list / V_list / C_list, interaction.py:481-500)
        U, V, C, G, Bb = self.cross.packed()
        return [tr.param(U.clone(), l2), tr.param(V.clone(), l2), tr.param(C.clone(), l2), tr.param(G.clone()), tr.param(Bb.clone())]

    def _bind_cross_views(self, U, V, C, G, Bb):
        cr = self.cross
        for i in range(cr.layer_num):
            cr._weights['U_list%d' % i], cr._weights['V_list%d' % i], cr._weights['C_list%d' % i] = U[i], V[i], C[i]
            cr._weights['bias%d' % i] = Bb[i].view(cr.dim, 1)
        for e, dense in enumerate(cr.gating):
            dense._weights['kernel'] = G[e].view(cr.dim, 1)

    def _hip_cross_fwd(self, tr, dnn_in, d, stack, buf):
        ops.crossnet_mix(dnn_in, *[p.w for p in tr.own["cross"]], dim=d, out=stack)

    def _hip_cross_bwd(self, tr, dnn_in, d, dstack, buf, accumulate):
        ps = tr.own["cross"]
        ops.crossnet_mix_bwd(dnn_in, d, [p.w for p in ps], dstack, [p.g for p in ps], buf["dx"], accumulate=accumulate)


def DCNMix(linear_feature_columns, dnn_feature_columns, cross_num=2, dnn_hidden_units=(256, 128, 64), l2_reg_linear=1e-5,
           l2_reg_embedding=1e-5, low_rank=32, num_experts=4, l2_reg_cross=1e-5, l2_reg_dnn=0, seed=1024, dnn_dropout=0,
           dnn_use_bn=False, dnn_activation='relu', task='binary', device=None):
    """Instantiates the Deep&Cross Network with mixture of experts architecture on the MI355X forward path."""
    if len(dnn_hidden_units) == 0 and cross_num == 0:
        raise ValueError("Either hidden_layer or cross layer must > 0")
    m = _DCNMix(linear_feature_columns, dnn_feature_columns, cross_num, dnn_hidden_units, low_rank, num_experts, seed,
                dnn_dropout, dnn_use_bn, dnn_activation, task, device)
    m.regularizers = {"embedding": float(l2_reg_embedding), "linear": float(l2_reg_linear), "dnn": float(l2_reg_dnn),
                      "cross": float(l2_reg_cross)}
    return m
