"""DSIN — same signature as ``deepctr.models.sequence.dsin.DSIN`` (reference deepctr/models/sequence/dsin.py:26-167): the behaviour
history cut into ``sess_max_count`` sessions that share the SparseFeats' embeddings and one Transformer, a bidirectional LSTM over
the session interests, and two attention poolings against the query.

Per batch: DIN's staging (fused gather of every SparseFeat into the DNN input; DSIN pools no sequence column, dsin.py:100-106), the
query lookups and ONE lookup per session feature over its [B, S, T] ids into a [B, S, T, E] buffer (``dctr_embed_lookup_multi``,
which also writes the position mask: every feature's id non-zero, keras' ``Concat.compute_mask``), ``dctr_bias_encoding_fwd`` in
place when ``bias_encoding``, ONE ``dctr_transformer_fwd`` launch over the [B S, T, E] view whose mean output is the session
interests [B, S, E], ``dctr_din_attn_pool_fwd`` over them, ``dctr_bilstm_fwd`` and a second ``dctr_din_attn_pool_fwd`` over its
output, both under ``sequence_mask(sess_length, S)`` and each into its slot of the DNN input, and ``dctr_mlp_fwd`` (DNN + Dense(1) +
sigmoid).  fit() takes the autograd step over the torch restatement below, in which the BiLSTM is one differentiable HIP op
(``dctr_bilstm_train_fwd`` / ``dctr_bilstm_bwd``, training.bilstm) and so is the Transformer over all sessions
(``dctr_transformer_train_fwd`` / ``dctr_transformer_bwd``, training.transformer); the poolings stay torch ops."""
from collections import OrderedDict

import numpy as np
import torch

from ... import ops
from ... import training as tops
from ...engine import EmbeddingStage, prehashed_on_host
from ...feature_column import InputSpec, SparseFeat, VarLenSparseFeat
from ...inputs import Embedding
from ...layers.base import name_scope
from ...layers.core import DNN, Dense, PredictionLayer
from ...layers.sequence import AttentionSequencePoolingLayer, BiLSTM, BiasEncoding, Transformer
from .._common import FeatureModel


class _DSIN(FeatureModel):
    def __init__(self, dnn_feature_columns, sess_feature_list, sess_max_count, bias_encoding, att_embedding_size, att_head_num,
                 dnn_hidden_units, dnn_activation, dnn_dropout, dnn_use_bn, seed, task, device):
        dnn_feature_columns = list(dnn_feature_columns)
        self.sess_feature_list = list(sess_feature_list)
        hist_emb_size = sum(fc.embedding_dim for fc in dnn_feature_columns if fc.name in self.sess_feature_list)
        if att_embedding_size * att_head_num != hist_emb_size:
            raise ValueError("hist_emb_size must equal to att_embedding_size * att_head_num ,got %d != %d *%d" % (
                hist_emb_size, att_embedding_size, att_head_num))
        super(_DSIN, self).__init__("DSIN", dnn_feature_columns, device, task)
        if "sess_length" not in self.inputs:                # dsin.py:87, after every feature's input (:140)
            self.inputs["sess_length"] = InputSpec("sess_length", (1,), "float32")
            self.input_names = list(self.inputs.keys())
        self.S, self.E = int(sess_max_count), int(hist_emb_size)
        sparse = [fc for fc in dnn_feature_columns if isinstance(fc, SparseFeat)]
        varlen = {fc.name: fc for fc in dnn_feature_columns if isinstance(fc, VarLenSparseFeat)}
        # the session features in the SparseFeats' order (get_embedding_vec_list walks those, inputs.py:74-86)
        self.sess_cols = [fc for fc in sparse if fc.name in self.sess_feature_list]
        if not self.sess_cols:
            raise ValueError("DSIN needs the SparseFeats named in sess_feature_list")
        if len(self.sess_cols) > 6:     # one lookup writes the mask and takes (id != 0) of at most five more id tensors
            raise NotImplementedError("DSIN with more than six session features is outside the fused lookup's limits")
        # sess_{i}_{feat}: looked up through the SparseFeat's table and hash settings (dsin.py:80-85, :151-152)
        self.sess_inputs, T = [], set()
        for i in range(self.S):
            for fc in self.sess_cols:
                name = "sess_%d_%s" % (i, fc.name)
                if name not in varlen:
                    raise KeyError(name)
                T.add(varlen[name].maxlen)
                self.sess_inputs.append(VarLenSparseFeat(fc._replace(name=name), maxlen=varlen[name].maxlen))
        if len(T) != 1:
            raise ValueError("the session columns must share one maxlen")
        self.T = int(T.pop())
        with name_scope():
            self.linear_tables, self.linear = {}, None
            self.tables = OrderedDict()
            for i, fc in enumerate(sparse):                 # dsin.py:89-96: one table per SparseFeat, mask_zero for the session features
                emb = Embedding(fc.vocabulary_size, fc.embedding_dim, embeddings_initializer=fc.embeddings_initializer,
                                name="sparse_emb_%d-%s" % (i, fc.name), mask_zero=fc.name in self.sess_feature_list, device=self.device)
                emb.trainable = fc.trainable
                self.tables[fc.embedding_name] = self._add(emb)
            # DNN input = [all SparseFeat embeddings, session-interest attention, LSTM attention, dense] (dsin.py:126-129); the other
            # sequence columns are computed by no part of it
            self.stage_plan = EmbeddingStage(self.tables, {}, [], dnn_feature_columns, mask_feat_list=tuple(self.sess_feature_list),
                                             extra_dims=(("sess", self.E), ("lstm", self.E)), skip_varlen=tuple(varlen), device=self.device)
            # rows of the id matrix (= positions in the DNN input's parts) that hold the session features' own ids: the query
            self._query_rows = [next(i for i, f in enumerate(self.stage_plan.fields) if f.kind == "sparse" and f.fc.name == fc.name)
                                for fc in self.sess_cols]
            self.bias_enc = None
            if bias_encoding:
                self.bias_enc = self._add(BiasEncoding(self.S, device=self.device).build_for(self.T, self.E))
            self.transformer = self._add(Transformer(att_embedding_size, att_head_num, dropout_rate=0, use_layer_norm=False,
                                                     use_positional_encoding=not bias_encoding, seed=seed, supports_masking=True,
                                                     blinding=True, output_type="mean", device=self.device).build_for(self.T, self.E))
            self.sess_attention = self._add(AttentionSequencePoolingLayer((64, 16), weight_normalization=True, supports_masking=False,
                                                                          device=self.device).build_for(self.E))
            self.bilstm = self._add(BiLSTM(self.E, layers=2, res_layers=0, dropout_rate=0.2, device=self.device).build_for(self.E))
            self.lstm_attention = self._add(AttentionSequencePoolingLayer((64, 16), weight_normalization=True, device=self.device)
                                            .build_for(self.E))
            self.dnn = self._add(DNN(dnn_hidden_units, dnn_activation, 0, dnn_dropout, dnn_use_bn, seed=seed,
                                     device=self.device).build_for(self.stage_plan.in_dim))
            last = dnn_hidden_units[-1] if len(dnn_hidden_units) else self.stage_plan.in_dim
            self.dense = self._add(Dense(1, use_bias=False, device=self.device).build_for(last))
            self.prediction = self._add(PredictionLayer(task, device=self.device).build_for())

    def _stage_inputs(self, feed, staged):
        sp = self.stage_plan
        sp.stage(feed, staged)
        for fc in self.sess_inputs:
            sp.stage_varlen(feed, staged, fc)
        # one [N, S, T] id tensor per session feature: its lookup is then one launch over all sessions
        nf = len(self.sess_cols)
        for j, fc in enumerate(self.sess_cols):
            per = [staged.seq[self.sess_inputs[i * nf + j].name] for i in range(self.S)]
            dt = torch.int64 if any(t.dtype == torch.int64 for t in per) else torch.int32
            staged.seq["sess:" + fc.name] = torch.stack([t.to(dt) for t in per], dim=1).contiguous()
        lens = np.ceil(np.asarray(feed["sess_length"], dtype=np.float64).reshape(-1)).astype(np.int32)     # sequence_mask: t < length
        staged.length["sess_length"] = torch.from_numpy(np.ascontiguousarray(lens)).to(self.device)

    def _hash_mode(self, fc):
        return 2 if (fc.use_hash and not prehashed_on_host(fc)) else 0       # Hash(mask_zero=True): dsin.py:98-99, :151-152

    def _session_inputs(self, staged, lo, hi, ws):
        """Query [B, E], the session embeddings [B, S, T, E] and their position mask [B, S, T] of rows [lo, hi)."""
        B, S, T, E, dev = hi - lo, self.S, self.T, self.E, self.device
        bufs = self._per_batch(B, lambda: dict(
            q=torch.zeros(B, E, dtype=torch.float32, device=dev), k=torch.zeros(B, S, T, E, dtype=torch.float32, device=dev),
            m=torch.ones(B, S, T, dtype=torch.uint8, device=dev), sm=torch.ones(B, S, dtype=torch.uint8, device=dev),
            sess_fea=torch.empty(B, S, E, dtype=torch.float32, device=dev), lstm=torch.empty(B, S, E, dtype=torch.float32, device=dev)))
        lookups, col = [], 0
        kflat = bufs["k"].view(B * S * T, E)
        ids = [staged.seq["sess:" + fc.name][lo:hi] for fc in self.sess_cols]
        for j, (fc, row) in enumerate(zip(self.sess_cols, self._query_rows)):
            table, hm = self.tables[fc.embedding_name].embeddings, self._hash_mode(fc)
            lookups.append(dict(idx=staged.ids[row, lo:hi], table=table, hash_mode=hm, out=bufs["q"][:, col:]))
            lk = dict(idx=ids[j], table=table, hash_mode=hm, out=kflat[:, col:])
            if j == 0:          # every session feature masks zero: the first lookup writes the conjunction of all (id != 0)
                lk["mask"] = bufs["m"]
            lookups.append(lk)
            col += fc.embedding_dim
        for c0 in range(0, len(lookups), 8):            # eight lookups per launch
            ops.embed_lookup_multi(lookups[c0:c0 + 8], extra_mask_ids=ids[1:], status=ws["status"])
        lens = staged.length["sess_length"][lo:hi]
        torch.lt(torch.arange(S, device=dev, dtype=torch.int32)[None, :], lens[:, None], out=bufs["sm"].view(torch.bool))
        return bufs

    def _forward(self, staged, lo, hi, out):
        sp = self.stage_plan
        ws = sp.run(staged, lo, hi)
        B, S, T, E = hi - lo, self.S, self.T, self.E
        bufs = self._session_inputs(staged, lo, hi, ws)
        q, k, sm = bufs["q"], bufs["k"], bufs["sm"]
        if self.bias_enc is not None:
            self.bias_enc.run(k)
        m = bufs["m"].view(B * S, T)
        self.transformer.run(k.view(B * S, T, E), query_mask=m, key_mask=m, out=bufs["sess_fea"].view(B * S, E))
        self.sess_attention.run(q, bufs["sess_fea"], sm, out=ws["dnn_in"][:, sp.extra_offsets["sess"]:], out_stride=sp.out_stride)
        self.bilstm.run(bufs["sess_fea"], out=bufs["lstm"])
        self.lstm_attention.run(q, bufs["lstm"], sm, out=ws["dnn_in"][:, sp.extra_offsets["lstm"]:], out_stride=sp.out_stride)
        ops.mlp(ws["dnn_in"], self.dnn.kernels, self.dnn.biases, self.dnn.activation, dice=self.dnn.dice_params(), bn=self.dnn.bn_params(),
                head_w=self.dense.w('kernel'), global_bias=self.prediction.w('global_bias'),
                sigmoid_out=self.task == "binary", in_dim=sp.in_dim, out=out)

    # ---- the forward in differentiable torch ops ----------------------------------------------------------------------------------
    def _pool(self, layer, q, keys, km, training):
        la = layer.local_att
        qq = q.unsqueeze(1).expand(-1, keys.shape[1], -1)
        att = tops.dnn_forward(la.dnn, torch.cat([qq, keys, qq - keys, qq * keys], dim=-1), training)
        score = (att @ la.w("kernel") + la.w("bias")).squeeze(-1)
        score = torch.softmax(torch.where(km, score, torch.full_like(score, float(-2 ** 32 + 1))), dim=-1)
        return (score.unsqueeze(1) @ keys).squeeze(1)

    def _autograd_logit(self, staged, lo, hi, parts, extra, training):       # dsin.py:98-129
        B, S, T, E = hi - lo, self.S, self.T, self.E
        q = torch.cat([parts[i] for i in self._query_rows], dim=-1)
        keys, m = [], None
        for fc in self.sess_cols:
            rows = tops._rows_for(fc, staged.seq["sess:" + fc.name][lo:hi], True)
            keys.append(self.tables[fc.embedding_name].embeddings[rows])
            m = (rows != 0) if m is None else (m & (rows != 0))
        k = torch.cat(keys, dim=-1)                                           # [B,S,T,E]
        if self.bias_enc is not None:
            be = self.bias_enc
            k = k + be.w("item_bias_embedding") + be.w("seq_bias_embedding") + be.w("sess_bias_embedding").reshape(1, S, 1, 1)
        k, m = k.reshape(B * S, T, E), m.reshape(B * S, T)
        sess_fea = tops.transformer([self.transformer], k, m, m, training).reshape(B, S, E)      # mask form, output mean
        sm = torch.arange(S, device=k.device)[None, :] < staged.length["sess_length"][lo:hi].reshape(-1, 1)
        parts[extra["sess"]] = self._pool(self.sess_attention, q, sess_fea, sm, training)
        lstm = tops.bilstm(sess_fea, self.bilstm.operands(), self.bilstm.res_layers, self.bilstm.merge_mode,
                           self.bilstm.recurrent_activation, self.bilstm.dropout_rate, training)
        parts[extra["lstm"]] = self._pool(self.lstm_attention, q, lstm, sm, training)
        return super(_DSIN, self)._autograd_logit(staged, lo, hi, parts, extra, training)

    def _hip_supported(self):
        return False                # fit() takes the autograd step (the poolings have no HIP step); in it the Transformer runs on
                                    # dctr_transformer_train_fwd / dctr_transformer_bwd and the BiLSTM on dctr_bilstm_train_fwd /
                                    # dctr_bilstm_bwd


def DSIN(dnn_feature_columns, sess_feature_list, sess_max_count=5, bias_encoding=False, att_embedding_size=1, att_head_num=8,
         dnn_hidden_units=(256, 128, 64), dnn_activation='relu', dnn_dropout=0, dnn_use_bn=False, l2_reg_dnn=0, l2_reg_embedding=1e-6,
         seed=1024, task='binary', device=None):
    """Instantiates the Deep Session Interest Network architecture on the MI355X forward path."""
    m = _DSIN(dnn_feature_columns, sess_feature_list, sess_max_count, bias_encoding, att_embedding_size, att_head_num, dnn_hidden_units,
              dnn_activation, dnn_dropout, dnn_use_bn, seed, task, device)
    # l2 regularisers of the reference constructor (dsin.py:89-92, :130); the Transformer, the LSTMs and the attention units have none
    m.regularizers = {"embedding": float(l2_reg_embedding), "linear": 0.0, "dnn": float(l2_reg_dnn)}
    return m
