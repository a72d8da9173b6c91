"""BST — same signature as ``deepctr.models.sequence.bst.BST`` (reference deepctr/models/sequence/bst.py:21-107): DIN's wiring with the
history embeddings passed through ``transformer_num`` Transformer layers before the attention pooling.

Per batch: DIN's staging (pooled non-history sequences + fused gather of every SparseFeat into the DNN input), the query / key
lookups (``dctr_embed_lookup_multi``; BST hashes them without mask_zero, bst.py:68-71), ``dctr_transformer_fwd`` over the [B, T, E] key
buffer IN PLACE for all layers in one launch — it also emits the ``sequence_mask(seq_length, T)`` key mask the pooling needs —
``dctr_din_attn_pool_fwd`` (AttentionSequencePoolingLayer((64, 16), 'sigmoid', weight_normalization=True)) into its slot of the DNN
input, and ``dctr_mlp_fwd`` (DNN + Dense(1) + sigmoid).  fit() takes the autograd step over the torch restatement below, in which the
Transformer stack is one differentiable HIP op (``dctr_transformer_train_fwd`` / ``dctr_transformer_bwd``, training.transformer)."""
import torch

from ... import ops
from ... import training as tops
from ...layers.sequence import Transformer
from .din import _DIN


class _BST(_DIN):
    model_name = "BST"
    key_hash_mode = 1            # Hash(mask_zero=False): embedding_lookup without a mask_feat_list (bst.py:68-71)
    key_mask_from_ids = False    # the mask is sequence_mask(seq_length, T): dctr_transformer_fwd writes it (key_mask_out)

    def __init__(self, dnn_feature_columns, history_feature_list, transformer_num, att_head_num, use_bn, dnn_hidden_units, dnn_activation,
                 dnn_dropout, seed, task, device):
        self.transformer_num, self.att_head_num = int(transformer_num), int(att_head_num)
        super(_BST, self).__init__(dnn_feature_columns, history_feature_list, use_bn, dnn_hidden_units, dnn_activation, (64, 16), "sigmoid",
                                   True, dnn_dropout, seed, task, device)

    def _build_sequence_block(self, seed, dnn_dropout):
        if not any(fc.length_name == "seq_length" for fc in self.history_cols):
            raise ValueError("BST reads the behaviour length from the input 'seq_length': give a history column length_name='seq_length'")
        if self.att_head_num <= 0:
            raise ValueError('head_num must be a int > 0')
        if self.key_dim % self.att_head_num:
            raise ValueError("att_embedding_size * head_num must equal the last dimension size of inputs,got %d * %d != %d"
                             % (self.key_dim // self.att_head_num, self.att_head_num, self.key_dim))
        self.transformers = []
        for _ in range(self.transformer_num):
            layer = Transformer(att_embedding_size=self.key_dim // self.att_head_num, head_num=self.att_head_num, dropout_rate=dnn_dropout,
                                use_positional_encoding=True, use_res=True, use_feed_forward=True, use_layer_norm=True, blinding=False,
                                seed=seed, supports_masking=False, output_type=None, device=self.device)
            self.transformers.append(self._add(layer.build_for(self.T, self.key_dim)))

    def _forward(self, staged, lo, hi, out):
        sp = self.stage_plan
        ws = sp.run(staged, lo, hi)
        bufs = self._attention_inputs(staged, lo, hi, ws)
        k = bufs["k"]
        if self.transformers:
            lens = staged.length["seq_length"][lo:hi]
            ops.transformer(k, [t.operands() for t in self.transformers], self.att_head_num, query_lengths=lens, key_lengths=lens,
                            output_type=None, out=k, key_mask_out=bufs["m"], **self.transformers[0].flags())
        else:
            self._length_mask(staged, lo, hi, bufs["m"])
        hist_off = sp.extra_offsets["hist"]
        self.attention.run(bufs["q"], k, bufs["m"], out=ws["dnn_in"][:, hist_off:], out_stride=sp.out_stride)
        ops.mlp(ws["dnn_in"], self.dnn.kernels, self.dnn.biases, self.dnn.activation, dice=self.dnn.dice_params(), bn=self.dnn.bn_params(),
                head_w=self.dense.w('kernel'), global_bias=self.prediction.w('global_bias'),
                sigmoid_out=self.task == "binary", in_dim=sp.in_dim, out=out)

    def _length_mask(self, staged, lo, hi, m):
        """transformer_num = 0: the pooling's sequence_mask(seq_length, T) (bst.py:94-96) without a Transformer launch to emit it."""
        lens = staged.length["seq_length"][lo:hi]
        torch.lt(torch.arange(self.T, device=lens.device, dtype=torch.int32)[None, :], lens[:, None], out=m.view(torch.bool))

    def _autograd_logit(self, staged, lo, hi, parts, extra, training):       # bst.py:68-97
        q = torch.cat([self.tables[fc.embedding_name].embeddings[tops._rows_for(fc, staged.ids[row, lo:hi], False)]
                       for fc, row in zip(self.query_cols, self._query_rows)], dim=-1)
        k = torch.cat([self.tables[fc.embedding_name].embeddings[tops._rows_for(fc, staged.seq[fc.name][lo:hi], False)]
                       for fc in self.history_cols], dim=-1)
        lens = staged.length["seq_length"][lo:hi].reshape(-1, 1)
        km = torch.arange(k.shape[1], device=k.device)[None, :] < lens
        # every layer as one differentiable HIP op (dctr_transformer_train_fwd / dctr_transformer_bwd), lengths form
        k = tops.transformer(self.transformers, k, km, km, training, lengths=staged.length["seq_length"][lo:hi])
        la = self.attention.local_att
        qq = q.unsqueeze(1).expand(-1, k.shape[1], -1)
        att = tops.dnn_forward(la.dnn, torch.cat([qq, k, qq - k, qq * k], dim=-1), training)
        score = (att @ la.w("kernel") + la.w("bias")).squeeze(-1)
        score = torch.softmax(torch.where(km, score, torch.full_like(score, float(-2 ** 32 + 1))), dim=-1)
        parts[extra["hist"]] = (score.unsqueeze(1) @ k).squeeze(1)
        return super(_DIN, self)._autograd_logit(staged, lo, hi, parts, extra, training)

    def _hip_supported(self):
        return False                # fit() takes the autograd step (DIN's pooling over the Transformer output has no HIP step); in it
                                    # the Transformer stack runs on dctr_transformer_train_fwd / dctr_transformer_bwd


def BST(dnn_feature_columns, history_feature_list, transformer_num=1, att_head_num=8, use_bn=False, dnn_hidden_units=(256, 128, 64),
        dnn_activation='relu', l2_reg_dnn=0, l2_reg_embedding=1e-6, dnn_dropout=0.0, seed=1024, task='binary', device=None):
    """Instantiates the Behavior Sequence Transformer architecture on the MI355X forward path."""
    m = _BST(dnn_feature_columns, history_feature_list, transformer_num, att_head_num, use_bn, dnn_hidden_units, dnn_activation,
             dnn_dropout, seed, task, device)
    # l2 regularisers of the reference constructor (bst.py:65-66, :101); the Transformer and the attention unit have none
    m.regularizers = {"embedding": float(l2_reg_embedding), "linear": 0.0, "dnn": float(l2_reg_dnn)}
    return m
