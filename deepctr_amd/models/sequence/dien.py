"""DIEN — same signature as ``deepctr.models.sequence.dien.DIEN`` (reference deepctr/models/sequence/dien.py:112-219): DIN's wiring with
an interest-extractor GRU and an interest-evolution GRU around the attention unit (``interest_evolution``, dien.py:66-109).

Per batch: DIN's staging (pooled non-history sequences + fused gather of every SparseFeat into the DNN input), the query / key
lookups (``dctr_embed_lookup_multi``; DIEN builds its embeddings with seq_mask_zero=False and takes the mask from ``seq_length``,
dien.py:166-173), then per ``gru_type``:
  GRU                   gru1 -> gru2 as ONE two-layer ``dctr_gru_fwd`` launch (gru1's [B, T, E] never reaches HBM), then
                        ``dctr_din_attn_pool_fwd`` with the length mask into its slot of the DNN input;
  AIGRU / AGRU / AUGRU  gru1 (sequence), the attention scores (``dctr_din_attn_pool_fwd`` with return_score), gru2 — plain with its input
                        scaled by the scores, or the attention-gated cell — whose final state goes straight into the DNN slot;
and ``dctr_mlp_fwd`` (DNN + Dense(1) + sigmoid).  fit() takes the autograd step over the torch restatement below, in which every GRU
layer is one differentiable HIP op (``dctr_gru_fwd`` / ``dctr_gru_bwd``, training.dynamic_gru); with ``use_negsampling`` it adds ``alpha`` times the auxiliary loss of dien.py:22-63 over the ``neg_hist_*`` columns,
which predict() ignores."""
import torch

from ... import ops
from ... import training as tops
from ...feature_column import VarLenSparseFeat
from ...layers.core import DNN
from ...layers.sequence import DynamicGRU
from .din import _DIN

GRU_TYPES = ("GRU", "AIGRU", "AGRU", "AUGRU")


class _DIEN(_DIN):
    model_name = "DIEN"
    key_hash_mode = 1            # Hash(mask_zero=False): embedding_lookup without a mask_feat_list (dien.py:169-173)
    key_mask_from_ids = False    # the mask is sequence_mask(seq_length, T)

    def __init__(self, dnn_feature_columns, history_feature_list, gru_type, use_negsampling, alpha, use_bn, dnn_hidden_units,
                 dnn_activation, att_hidden_units, att_activation, att_weight_normalization, dnn_dropout, seed, task, device):
        if gru_type not in GRU_TYPES:
            raise ValueError("gru_type error ")
        self.gru_type, self.use_negsampling, self.alpha = gru_type, bool(use_negsampling), float(alpha)
        if self.use_negsampling and gru_type != "AUGRU":
            # (the reference forms the auxiliary loss for AUGRU only, dien.py:76, and fails on alpha * None otherwise, :213)
            raise ValueError("use_negsampling needs gru_type='AUGRU': the reference forms the auxiliary loss for that type only")
        neg_names = ["neg_hist_" + n for n in history_feature_list]
        self.skip_varlen_extra = tuple(neg_names)
        self.neg_cols = [fc for fc in dnn_feature_columns if isinstance(fc, VarLenSparseFeat) and fc.name in neg_names]
        if self.use_negsampling and len(self.neg_cols) != len(neg_names):
            raise ValueError("use_negsampling needs a 'neg_hist_<name>' sequence column for every history feature")
        self._added = None
        super(_DIEN, self).__init__(dnn_feature_columns, history_feature_list, use_bn, dnn_hidden_units, dnn_activation, att_hidden_units,
                                    att_activation, att_weight_normalization, dnn_dropout, seed, task, device)
        self.attention.return_score = gru_type != "GRU"
        if self.use_negsampling and sum(fc.embedding_dim for fc in self.neg_cols) != self.key_dim:
            raise ValueError("the neg_hist_* columns must have the widths of the hist_* columns")

    def _build_sequence_block(self, seed, dnn_dropout):
        if not any(fc.length_name == "seq_length" for fc in self.history_cols):
            raise ValueError("DIEN reads the behaviour length from the input 'seq_length': give a history column length_name='seq_length'")
        E = self.key_dim
        self.gru1 = self._add(DynamicGRU(None, return_sequence=True, name="gru1", device=self.device).build_for(E))
        self.aux_dnn = None
        if self.use_negsampling:            # auxiliary_loss's DNN([100, 50, 1], 'sigmoid') over [h_t | e_{t+1}] (dien.py:39)
            self.aux_dnn = self._add(DNN([100, 50, 1], activation='sigmoid', device=self.device).build_for(2 * E))
        cell = self.gru_type if self.gru_type in ("AGRU", "AUGRU") else "GRU"
        self.gru2 = self._add(DynamicGRU(None, gru_type=cell, return_sequence=self.gru_type == "GRU", name="gru2",
                                         device=self.device).build_for(E))

    def _stage_inputs(self, feed, staged):
        super(_DIEN, self)._stage_inputs(feed, staged)
        if all(fc.name in feed for fc in self.neg_cols):           # fit() with use_negsampling; predict() may leave them out
            for fc in self.neg_cols:
                self.stage_plan.stage_varlen(feed, staged, fc)

    def _forward(self, staged, lo, hi, out):
        sp = self.stage_plan
        ws = sp.run(staged, lo, hi)
        bufs = self._attention_inputs(staged, lo, hi, ws)
        q, k, m = bufs["q"], bufs["k"], bufs["m"]
        if "h" not in bufs:
            bufs["h"] = torch.empty_like(k)
        lens = staged.length["seq_length"][lo:hi]
        torch.lt(torch.arange(self.T, device=lens.device, dtype=torch.int32)[None, :], lens[:, None], out=m.view(torch.bool))
        dst = ws["dnn_in"][:, sp.extra_offsets["hist"]:]
        if self.gru_type == "GRU":
            seq = ops.dynamic_gru(k, lens, [self.gru1.operands(), self.gru2.operands()], out=bufs["h"])
            self.attention.run(q, seq, m, out=dst, out_stride=sp.out_stride)
        else:
            seq = ops.dynamic_gru(k, lens, [self.gru1.operands()], out=bufs["h"])
            scores = self.attention.run(q, seq, m)
            ops.dynamic_gru(seq, lens, [self.gru2.operands()], cell=self.gru2.cell, att_scores=scores, scale_input=self.gru_type == "AIGRU",
                            return_sequence=False, out=dst, out_stride=sp.out_stride)
        ops.mlp(ws["dnn_in"], self.dnn.kernels, self.dnn.biases, self.dnn.activation, dice=self.dnn.dice_params(), bn=self.dnn.bn_params(),
                head_w=self.dense.w('kernel'), global_bias=self.prediction.w('global_bias'),
                sigmoid_out=self.task == "binary", in_dim=sp.in_dim, out=out)

    # ---- the forward in differentiable torch ops ----------------------------------------------------------------------------------
    def _embed(self, cols, staged, lo, hi):
        return torch.cat([self.tables[fc.embedding_name].embeddings[tops._rows_for(fc, staged.seq[fc.name][lo:hi], False)] for fc in cols],
                         dim=-1)

    def _scores(self, q, k, km, training):
        """AttentionSequencePoolingLayer's scores [B, T] (reference sequence.py:261-298) in torch ops."""
        la = self.attention.local_att
        qq = q.unsqueeze(1).expand(-1, k.shape[1], -1)
        att = tops.dnn_forward(la.dnn, torch.cat([qq, k, qq - k, qq * k], dim=-1), training)
        score = (att @ la.w("kernel") + la.w("bias")).squeeze(-1)
        if self.attention.weight_normalization:
            return torch.softmax(torch.where(km, score, torch.full_like(score, float(-2 ** 32 + 1))), dim=-1)
        return torch.where(km, score, torch.zeros_like(score))

    def auxiliary_loss(self, h_states, click_seq, noclick_seq, lengths, training=False):
        """dien.py:22-63: -log p([h_t | e_{t+1}]) - log(1 - p([h_t | neg e_{t+1}])) under sequence_mask(lengths, T - 1), the mean over
        ALL B (T - 1) entries.  h_states, click_seq, noclick_seq [B, T - 1, E]; lengths [B] = seq_length - 1."""
        T1 = click_seq.shape[1]
        mask = (torch.arange(T1, device=lengths.device)[None, :] < lengths.reshape(-1, 1)).to(h_states.dtype)
        click = tops.dnn_forward(self.aux_dnn, torch.cat([h_states, click_seq], dim=-1), training)[:, :, 0]
        noclick = tops.dnn_forward(self.aux_dnn, torch.cat([h_states, noclick_seq], dim=-1), training)[:, :, 0]
        return (-torch.log(click) * mask - torch.log(1.0 - noclick) * mask).mean()

    def _autograd_added_loss(self):
        """What keras' Model.add_loss adds to the step's loss (dien.py:212-213): alpha x the auxiliary loss of the batch the last
        autograd forward ran, None when that forward had no neg_hist_* inputs."""
        added, self._added = self._added, None
        return added

    def _autograd_logit(self, staged, lo, hi, parts, extra, training):       # dien.py:169-205
        q = torch.cat([self.tables[fc.embedding_name].embeddings[tops._rows_for(fc, staged.ids[row, lo:hi], False)]
                       for fc, row in zip(self.query_cols, self._query_rows)], dim=-1)
        k = self._embed(self.history_cols, staged, lo, hi)
        lens = staged.length["seq_length"][lo:hi].reshape(-1)
        km = torch.arange(k.shape[1], device=k.device)[None, :] < lens[:, None]
        h1 = tops.dynamic_gru(k, lens, [self.gru1.operands()])
        self._added = None
        if self.use_negsampling and k.shape[1] > 1 and all(fc.name in staged.seq for fc in self.neg_cols):
            neg = self._embed(self.neg_cols, staged, lo, hi)
            self._added = self.alpha * self.auxiliary_loss(h1[:, :-1], k[:, 1:], neg[:, 1:], lens - 1, training)
        if self.gru_type == "GRU":
            h2 = tops.dynamic_gru(h1, lens, [self.gru2.operands()])
            parts[extra["hist"]] = (self._scores(q, h2, km, training).unsqueeze(1) @ h2).squeeze(1)
        else:
            score = self._scores(q, h1, km, training)
            parts[extra["hist"]] = tops.dynamic_gru(h1, lens, [self.gru2.operands()], cell=self.gru2.cell, att_scores=score,
                                             scale_input=self.gru_type == "AIGRU", return_sequence=False)
        return super(_DIN, self)._autograd_logit(staged, lo, hi, parts, extra, training)

    def _hip_supported(self):
        return False                # fit() takes the autograd step; its GRUs run on dctr_gru_fwd / dctr_gru_bwd


def DIEN(dnn_feature_columns, history_feature_list, gru_type="GRU", use_negsampling=False, alpha=1.0, use_bn=False,
         dnn_hidden_units=(256, 128, 64), dnn_activation='relu', att_hidden_units=(64, 16), att_activation="dice",
         att_weight_normalization=True, l2_reg_dnn=0, l2_reg_embedding=1e-6, dnn_dropout=0, seed=1024, task='binary', device=None):
    """Instantiates the Deep Interest Evolution Network architecture on the MI355X forward path."""
    m = _DIEN(dnn_feature_columns, history_feature_list, gru_type, use_negsampling, alpha, use_bn, dnn_hidden_units, dnn_activation,
              att_hidden_units, att_activation, att_weight_normalization, dnn_dropout, seed, task, device)
    # l2 regularisers of the reference constructor (dien.py:166, :206); the GRUs, the attention unit and the auxiliary DNN have none
    m.regularizers = {"embedding": float(l2_reg_embedding), "linear": 0.0, "dnn": float(l2_reg_dnn)}
    return m
