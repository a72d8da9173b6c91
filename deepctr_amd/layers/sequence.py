"""Host mirror of the in-scope layers of the reference's ``deepctr/layers/sequence.py``:
``SequencePoolingLayer`` (:41-120), ``WeightedSequenceLayer`` (:123-197), ``AttentionSequencePoolingLayer``
(:200-315), ``BiLSTM`` (:318-428), ``Transformer`` (:431-651), ``PositionEncoding`` (:654-703), ``BiasEncoding`` (:706-757) and
``DynamicGRU`` (:760-815).  In the model path pooling is fused INTO the embedding gather (``dctr_embed_pool``: ids ->
pooled vector, the [B,T,E] tensor never exists); these classes are the stand-alone layer API over an
already gathered [B,T,E] tensor.  Stand-alone pooling of a materialised tensor is pure data movement, done
here with the same kernel by treating the sequence tensor as its own table."""
import numpy as np
import torch

from .. import ops
from ..initializers import Constant, GlorotUniform, Orthogonal, TruncatedNormal
from .activation import require_base_activation
from .base import Layer, next_auto_name
from .core import LocalActivationUnit
from .normalization import LayerNormalization


def _pool_materialised(seq, mode, mask=None, lengths=None, weight=None, weight_norm=True):
    """seq [B,T,E] -> [B,1,E] through dctr_embed_pool: row (b,t) of the flattened tensor is 'table' row b*T+t+1
    (row 0 is a zero row so that the kernel's mask_zero rule 'id != 0' encodes the mask)."""
    B, T, E = seq.shape
    table = torch.cat([torch.zeros(1, E, device=seq.device), seq.reshape(B * T, E)], dim=0)
    ids = torch.arange(1, B * T + 1, device=seq.device, dtype=torch.int64).reshape(B, T)
    length = None
    if lengths is not None:
        length = lengths.reshape(-1).to(torch.int32)
    else:
        ids = ids * mask.reshape(B, T).to(torch.int64)
    out, _ = ops.embed_pool(ids, table, mode, length=length, weight=weight, weight_norm=weight_norm)
    return out.reshape(B, 1, E)


class SequencePoolingLayer(Layer):
    def __init__(self, mode='mean', supports_masking=False, **kwargs):
        if mode not in ['sum', 'mean', 'max']:
            raise ValueError("mode must be sum or mean")
        self.mode = mode
        self.eps = 1e-8
        super(SequencePoolingLayer, self).__init__(**kwargs)
        self.supports_masking = supports_masking

    def build(self, input_shape):
        if not self.supports_masking:
            self.seq_len_max = int(input_shape[0][1])
        super(SequencePoolingLayer, self).build(input_shape)

    def call(self, seq_value_len_list, mask=None, **kwargs):
        if self.supports_masking:
            if mask is None:
                raise ValueError("When supports_masking=True,input must support masking")
            return _pool_materialised(seq_value_len_list, self.mode, mask=mask)
        seq, lengths = seq_value_len_list
        return _pool_materialised(seq, self.mode, lengths=lengths)

    def compute_output_shape(self, input_shape):
        if self.supports_masking:
            return (None, 1, input_shape[-1])
        return (None, 1, input_shape[0][-1])

    def compute_mask(self, inputs, mask):
        return None

    def get_config(self):
        config = {'mode': self.mode, 'supports_masking': self.supports_masking}
        base = super(SequencePoolingLayer, self).get_config()
        return dict(list(base.items()) + list(config.items()))


class WeightedSequenceLayer(Layer):
    """[B,T,E] * per-position weight (softmax-normalised over valid positions when weight_normalization):
    dctr_seq_weight_fwd on a materialised tensor; the model path fuses the weighting into dctr_embed_pool."""

    def __init__(self, weight_normalization=True, supports_masking=False, **kwargs):
        super(WeightedSequenceLayer, self).__init__(**kwargs)
        self.weight_normalization = weight_normalization
        self.supports_masking = supports_masking

    def build(self, input_shape):
        if not self.supports_masking:
            self.seq_len_max = int(input_shape[0][1])
        super(WeightedSequenceLayer, self).build(input_shape)

    def call(self, input_list, mask=None, **kwargs):
        if self.supports_masking:
            if mask is None:
                raise ValueError("When supports_masking=True,input must support masking")
            key_input, value_input = input_list
            return ops.seq_weight(key_input, value_input, mask=mask[0], weight_norm=self.weight_normalization)
        key_input, key_length_input, value_input = input_list
        return ops.seq_weight(key_input, value_input, length=key_length_input, weight_norm=self.weight_normalization)

    def compute_output_shape(self, input_shape):
        return input_shape[0]

    def compute_mask(self, inputs, mask):
        if self.supports_masking:
            return mask[0]
        return None

    def get_config(self):
        config = {'weight_normalization': self.weight_normalization, 'supports_masking': self.supports_masking}
        base = super(WeightedSequenceLayer, self).get_config()
        return dict(list(base.items()) + list(config.items()))


class AttentionSequencePoolingLayer(Layer):
    def __init__(self, att_hidden_units=(80, 40), att_activation='sigmoid', weight_normalization=False,
                 return_score=False, supports_masking=False, **kwargs):
        self.att_hidden_units = att_hidden_units
        self.att_activation = att_activation
        self.weight_normalization = weight_normalization
        self.return_score = return_score
        super(AttentionSequencePoolingLayer, self).__init__(**kwargs)
        self.supports_masking = supports_masking
        require_base_activation("AttentionSequencePoolingLayer", att_activation)     # (as its LocalActivationUnit)

    def build(self, input_shape):
        if not self.supports_masking:
            if not isinstance(input_shape, list) or len(input_shape) != 3:
                raise ValueError('A `AttentionSequencePoolingLayer` layer should be called on a list of 3 inputs')
            if len(input_shape[0]) != 3 or len(input_shape[1]) != 3 or len(input_shape[2]) != 2:
                raise ValueError("Unexpected inputs dimensions,the 3 tensor dimensions are %d,%d and %d , expect to be "
                                 "3,3 and 2" % (len(input_shape[0]), len(input_shape[1]), len(input_shape[2])))
            if input_shape[0][-1] != input_shape[1][-1] or input_shape[0][1] != 1 or input_shape[2][1] != 1:
                raise ValueError('A `AttentionSequencePoolingLayer` layer requires inputs of a 3 tensor with shape '
                                 '(None,1,embedding_size),(None,T,embedding_size) and (None,1)'
                                 'Got different shapes: %s' % (input_shape,))
        self.build_for(int(input_shape[0][-1]))

    def build_for(self, emb):
        if self.built:
            return self
        self.local_att = LocalActivationUnit(self.att_hidden_units, self.att_activation, l2_reg=0, dropout_rate=0,
                                             use_bn=False, seed=1024)
        self.local_att.build_for(emb)
        self._sublayers.append(self.local_att)
        self.built = True
        return self

    # masked positions are skipped by the score kernel (csrc/din_chain_kernels.hip); False scores every position (A/B switch)
    compact_positions = True

    def run(self, queries, keys, key_masks, out=None, out_stride=None):
        la = self.local_att
        return ops.din_attention(queries, keys, key_masks, la.dnn.kernels, la.dnn.biases, la.w("kernel"), la.w("bias"),
                                 self.att_activation, la.dnn.dice_params(), weight_normalization=self.weight_normalization,
                                 return_score=self.return_score, out=out, out_stride=out_stride, compact=self.compact_positions)

    def call(self, inputs, mask=None, training=None, **kwargs):
        if self.supports_masking:
            if mask is None:
                raise ValueError("When supports_masking=True,input must support masking")
            queries, keys = inputs
            key_masks = mask[-1]
        else:
            queries, keys, keys_length = inputs
            T = keys.shape[1]
            key_masks = torch.arange(T, device=keys.device)[None, :] < keys_length.reshape(-1, 1)
        return self.run(queries, keys, key_masks)

    def compute_output_shape(self, input_shape):
        if self.return_score:
            return (None, 1, input_shape[1][1])
        return (None, 1, input_shape[0][-1])

    def compute_mask(self, inputs, mask):
        return None

    def get_config(self):
        config = {'att_hidden_units': self.att_hidden_units, 'att_activation': self.att_activation,
                  'weight_normalization': self.weight_normalization, 'return_score': self.return_score,
                  'supports_masking': self.supports_masking}
        base = super(AttentionSequencePoolingLayer, self).get_config()
        return dict(list(base.items()) + list(config.items()))


class Transformer(Layer):
    """Multi-head self-attention block with positional encodings, residual, LayerNormalization and feed-forward (reference
    sequence.py:431-651): every flag, both input forms, ``attention_type='scaled_dot_product'``.  One launch of
    ``dctr_transformer_fwd``; BST stacks its layers into a single launch through ``operands``.  In a training step a stack over
    self-attention without an active dropout is one differentiable op, ``dctr_transformer_train_fwd`` / ``dctr_transformer_bwd``
    (training.transformer); everything else trains on the torch ops of training._transformer."""

    def __init__(self, att_embedding_size=1, head_num=8, dropout_rate=0.0, use_positional_encoding=True, use_res=True,
                 use_feed_forward=True, use_layer_norm=False, blinding=True, seed=1024, supports_masking=False,
                 attention_type="scaled_dot_product", output_type="mean", **kwargs):
        if head_num <= 0:
            raise ValueError('head_num must be a int > 0')
        if attention_type in ("cos", "ln", "additive"):
            raise NotImplementedError("Transformer attention_type=%r is outside this build: only 'scaled_dot_product' has a kernel"
                                      % (attention_type,))
        if attention_type != "scaled_dot_product":
            raise ValueError("attention_type must be [scaled_dot_product,cos,ln,additive]")
        self.att_embedding_size = att_embedding_size
        self.head_num = head_num
        self.num_units = att_embedding_size * head_num
        self.use_res = use_res
        self.use_feed_forward = use_feed_forward
        self.seed = seed
        self.use_positional_encoding = use_positional_encoding
        self.dropout_rate = dropout_rate
        self.use_layer_norm = use_layer_norm
        self.blinding = blinding
        self.attention_type = attention_type
        self.output_type = output_type
        super(Transformer, self).__init__(**kwargs)
        self.supports_masking = supports_masking

    def build(self, input_shape):
        return self.build_for(int(input_shape[0][-2]), int(input_shape[0][-1]))

    def build_for(self, seq_len_max, embedding_size):
        if self.built:
            return self
        if self.num_units != embedding_size:
            raise ValueError("att_embedding_size * head_num must equal the last dimension size of inputs,got %d * %d != %d" % (
                self.att_embedding_size, self.head_num, embedding_size))
        self.seq_len_max = int(seq_len_max)
        shape = (embedding_size, self.num_units)
        self.add_weight('query', shape, TruncatedNormal(seed=self.seed))
        self.add_weight('key', shape, TruncatedNormal(seed=self.seed + 1))
        self.add_weight('value', shape, TruncatedNormal(seed=self.seed + 2))
        if self.use_feed_forward:
            self.add_weight('fw1', (self.num_units, 4 * self.num_units), GlorotUniform(seed=self.seed))
            self.add_weight('fw2', (4 * self.num_units, self.num_units), GlorotUniform(seed=self.seed))
        # one LayerNormalization serves both applications (sequence.py:516, :619, :628); keras builds it at its first call
        self.ln = LayerNormalization(device=self.device)
        if self.use_layer_norm:
            self.ln.build_for(self.num_units)
        self._sublayers.append(self.ln)
        if self.use_positional_encoding:
            self.query_pe = PositionEncoding(device=self.device).build_for(self.seq_len_max, embedding_size)
            self.key_pe = PositionEncoding(device=self.device).build_for(self.seq_len_max, embedding_size)
            self._sublayers += [self.query_pe, self.key_pe]
        self.built = True
        return self

    def operands(self):
        """The layer's weights as ops.transformer takes them; the positional tables are folded with float32(sqrt(E)) from the live
        tables on every call (one multiply each, the rounding of sequence.py:687-688)."""
        w = {k: self.w(k) for k in ("query", "key", "value")}
        if self.use_feed_forward:
            w["fw1"], w["fw2"] = self.w("fw1"), self.w("fw2")
        if self.use_layer_norm:
            w["ln_gamma"], w["ln_beta"] = self.ln.w("gamma"), self.ln.w("beta")
        if self.use_positional_encoding:
            w["pe_q"], w["pe_k"] = self.query_pe.scaled_table(), self.key_pe.scaled_table()
        return w

    def flags(self):
        return dict(use_positional_encoding=self.use_positional_encoding, use_res=self.use_res, use_feed_forward=self.use_feed_forward,
                    use_layer_norm=self.use_layer_norm, blinding=self.blinding, ln_eps=self.ln.eps)

    def run(self, queries, keys=None, query_lengths=None, key_lengths=None, query_mask=None, key_mask=None, out=None,
            key_mask_out=None):
        return ops.transformer(queries, [self.operands()], self.head_num, keys=keys, query_lengths=query_lengths,
                               key_lengths=key_lengths, query_mask=query_mask, key_mask=key_mask, output_type=self.output_type, out=out,
                               key_mask_out=key_mask_out, **self.flags())

    def call(self, inputs, mask=None, training=None, **kwargs):
        if self.supports_masking:
            queries, keys = inputs
            if mask is None:
                raise ValueError("When supports_masking=True,input must support masking")
            query_masks, key_masks = mask
            kw = dict(query_mask=query_masks.reshape(queries.shape[0], -1) != 0, key_mask=key_masks.reshape(keys.shape[0], -1) != 0)
        else:
            queries, keys, query_masks, key_masks = inputs
            kw = dict(query_lengths=query_masks.reshape(-1).to(torch.int32), key_lengths=key_masks.reshape(-1).to(torch.int32))
        if queries.dim() != 3 or keys.shape != queries.shape:
            raise ValueError("Transformer takes queries and keys of one shape (batch_size, timesteps, input_dim), got %s and %s"
                             % (tuple(queries.shape), tuple(keys.shape)))
        q = queries if queries.dtype == torch.float32 and queries.stride(-1) == 1 else queries.to(torch.float32).contiguous()
        k = None if keys is queries else (keys if keys.dtype == torch.float32 and keys.stride(-1) == 1 else keys.to(torch.float32).contiguous())
        y = self.run(q, k, **kw)
        return y if self.output_type is None else y.reshape(y.shape[0], 1, y.shape[1])

    def compute_output_shape(self, input_shape):
        return (None, 1, self.att_embedding_size * self.head_num)

    def compute_mask(self, inputs, mask=None):
        return None

    def get_config(self):
        config = {'att_embedding_size': self.att_embedding_size, 'head_num': self.head_num, 'dropout_rate': self.dropout_rate,
                  'use_res': self.use_res, 'use_positional_encoding': self.use_positional_encoding,
                  'use_feed_forward': self.use_feed_forward, 'use_layer_norm': self.use_layer_norm, 'seed': self.seed,
                  'supports_masking': self.supports_masking, 'blinding': self.blinding, 'attention_type': self.attention_type,
                  'output_type': self.output_type}
        base = super(Transformer, self).get_config()
        return dict(list(base.items()) + list(config.items()))


class PositionEncoding(Layer):
    """Trainable sinusoid positional table added to the inputs, scaled by sqrt(width) (reference sequence.py:654-703).  Inside
    Transformer the addition is fused into ``dctr_transformer_fwd``; stand-alone it is one elementwise addition."""

    def __init__(self, pos_embedding_trainable=True, zero_pad=False, scale=True, **kwargs):
        self.pos_embedding_trainable = pos_embedding_trainable
        self.zero_pad = zero_pad
        self.scale = scale
        super(PositionEncoding, self).__init__(**kwargs)

    def build(self, input_shape):
        return self.build_for(int(input_shape[-2]), int(input_shape[-1]))

    def build_for(self, T, num_units):
        if self.built:
            return self
        # pe[t, i] = sin(t / 10000^(2 floor(i / 2) / width)) for even i, cos of the same angle for odd i
        column = np.arange(int(num_units))
        angle = np.arange(int(T), dtype=np.float64)[:, None] / 10000.0 ** (2.0 * (column // 2) / num_units)[None, :]
        table = np.where(column[None, :] % 2 == 0, np.sin(angle), np.cos(angle))
        if self.zero_pad:
            table[0] = 0.0
        self.add_weight("lookup_table", (T, num_units), Constant(table), trainable=self.pos_embedding_trainable)
        self.built = True
        return self

    def scaled_table(self):
        """lookup_table * float32(sqrt(width)) (sequence.py:687-688), from the live table."""
        t = self.w("lookup_table")
        return t * float(np.float32(t.shape[1] ** 0.5)) if self.scale else t

    def call(self, inputs, mask=None, **kwargs):
        return self.scaled_table() + inputs

    def compute_output_shape(self, input_shape):
        return input_shape

    def compute_mask(self, inputs, mask=None):
        return mask

    def get_config(self):
        config = {'pos_embedding_trainable': self.pos_embedding_trainable, 'zero_pad': self.zero_pad, 'scale': self.scale}
        base = super(PositionEncoding, self).get_config()
        return dict(list(base.items()) + list(config.items()))


class DynamicGRU(Layer):
    """GRU / AGRU / AUGRU over a [B, T, E] sequence under dynamic_rnn's sequence_length rule (reference sequence.py:760-815 with the
    cells of contrib/utils.py): one launch of ``dctr_gru_fwd`` for the whole time loop; DIEN's plain stack gru1 -> gru2 goes out as
    a single launch through ``operands``.  Weight names are TensorFlow's variable names below the layer's scope: tf's GRUCell opens a
    ``gru_cell`` scope (``gru_cell/gates/kernel`` ...), the contrib cells override ``__call__`` and do not (``gates/kernel`` ...).
    Initial values as there: gate bias 1, candidate bias 0, kernels from get_variable's default glorot_uniform."""

    def __init__(self, num_units=None, gru_type='GRU', return_sequence=True, **kwargs):
        self.num_units = num_units
        self.return_sequence = return_sequence
        self.gru_type = gru_type
        super(DynamicGRU, self).__init__(**kwargs)

    def build(self, input_shape):
        return self.build_for(int(input_shape[0][-1]))

    def build_for(self, embedding_size):
        if self.built:
            return self
        if self.num_units is None:
            self.num_units = int(embedding_size)
        if self.num_units != int(embedding_size):
            raise NotImplementedError("DynamicGRU(num_units=%d) over inputs of width %d is outside this build: the kernel takes inputs and "
                                      "units of one width (the reference's models pass num_units=None)" % (self.num_units, embedding_size))
        E = self.num_units
        self._scope = "" if self.gru_type in ("AGRU", "AUGRU") else "gru_cell/"
        self.add_weight(self._scope + "gates/kernel", (2 * E, 2 * E), GlorotUniform())
        self.add_weight(self._scope + "gates/bias", (2 * E,), Constant(1.0))
        self.add_weight(self._scope + "candidate/kernel", (2 * E, E), GlorotUniform())
        self.add_weight(self._scope + "candidate/bias", (E,), Constant(0.0))
        self.built = True
        return self

    @property
    def cell(self):
        """The kernel's cell kind: 'AGRU' / 'AUGRU', and 'GRU' for every other gru_type (the reference's else branch, :777-781)."""
        return self.gru_type if self.gru_type in ("AGRU", "AUGRU") else "GRU"

    def operands(self):
        """(gate kernel, gate bias, candidate kernel, candidate bias) as ops.dynamic_gru and training._gru take a layer."""
        s = self._scope
        return (self.w(s + "gates/kernel"), self.w(s + "gates/bias"), self.w(s + "candidate/kernel"), self.w(s + "candidate/bias"))

    def run(self, x, lengths, att_scores=None, scale_input=False, out=None, out_stride=None):
        return ops.dynamic_gru(x, lengths, [self.operands()], cell=self.cell, att_scores=att_scores, scale_input=scale_input,
                               return_sequence=self.return_sequence, out=out, out_stride=out_stride)

    def call(self, input_list, **kwargs):
        if self.cell == "GRU":
            rnn_input, sequence_length = input_list
            att_score = None
        else:
            rnn_input, sequence_length, att_score = input_list
            att_score = att_score.to(torch.float32).contiguous()
        x = rnn_input if rnn_input.dtype == torch.float32 and rnn_input.stride(-1) == 1 else rnn_input.to(torch.float32).contiguous()
        y = self.run(x, sequence_length.reshape(-1).to(torch.int32).contiguous(), att_score)
        return y if self.return_sequence else y.reshape(y.shape[0], 1, y.shape[1])

    def compute_output_shape(self, input_shape):
        rnn_input_shape = input_shape[0]
        if self.return_sequence:
            return rnn_input_shape
        return (None, 1, rnn_input_shape[2])

    def get_config(self):
        config = {'num_units': self.num_units, 'gru_type': self.gru_type, 'return_sequence': self.return_sequence}
        base_config = super(DynamicGRU, self).get_config()
        return dict(list(base_config.items()) + list(config.items()))


class _LSTMWeights(Layer):
    """The weights of one tf.keras.layers.LSTM under keras' names: ``kernel`` [D, 4u], ``recurrent_kernel`` [u, 4u], ``bias`` [4u], gate
    order i | f | c~ | o.  Initial values as BiLSTM builds them (reference sequence.py:365-370): kernel glorot_uniform, recurrent kernel
    orthogonal, bias ones (``bias_initializer='ones'``; keras' unit_forget_bias then leaves every quarter at one)."""

    def __init__(self, input_dim, units, **kwargs):
        super(_LSTMWeights, self).__init__(name=next_auto_name("lstm"), **kwargs)
        self.add_weight("kernel", (input_dim, 4 * units), GlorotUniform())
        self.add_weight("recurrent_kernel", (units, 4 * units), Orthogonal())
        self.add_weight("bias", (4 * units,), Constant(1.0))
        self.built = True

    def operands(self):
        return (self.w("kernel"), self.w("recurrent_kernel"), self.w("bias"))


class BiLSTM(Layer):
    """A multiple layer bidirectional residual LSTM (reference sequence.py:318-428): one launch of ``dctr_bilstm_fwd`` for both stacks.
    ``dropout_rate`` is the LSTMs' input dropout: inactive at inference; under fit() training.bilstm draws one mask per LSTM and
    runs both stacks as one differentiable HIP op (``dctr_bilstm_train_fwd`` / ``dctr_bilstm_bwd``), or the torch restatement
    training._bilstm where that op does not apply (the CPU, no_grad, float64, a refused shape).  keras' masked-step rule (a masked step copies the state through) is outside this build: a mask raises
    NotImplementedError; in DSIN none reaches the layer (Transformer.compute_mask returns None)."""

    def __init__(self, units, layers=2, res_layers=0, dropout_rate=0.2, merge_mode='ave', **kwargs):
        if merge_mode not in ['fw', 'bw', 'sum', 'mul', 'ave', 'concat', None]:
            raise ValueError('Invalid merge mode. '
                             'Merge mode should be one of '
                             '{"fw","bw","sum", "mul", "ave", "concat", None}')
        self.units = units
        self.layers = layers
        self.res_layers = res_layers
        self.dropout_rate = dropout_rate
        self.merge_mode = merge_mode
        self.recurrent_activation = "sigmoid"       # the TF 2.x default; 'hard_sigmoid' serves weights trained under TF 1.x
        super(BiLSTM, self).__init__(**kwargs)
        self.supports_masking = True

    def build(self, input_shape):
        if len(input_shape) != 3:
            raise ValueError("Unexpected inputs dimensions %d, expect to be 3 dimensions" % (len(input_shape)))
        return self.build_for(int(input_shape[-1]))

    def build_for(self, input_dim):
        if self.built:
            return self
        if self.res_layers >= self.layers and int(input_dim) != int(self.units):
            raise ValueError("BiLSTM: a residual over layer 0 needs inputs of the units' width, got %d and %d" % (input_dim, self.units))
        self.fw_lstm, self.bw_lstm = [], []
        for i in range(self.layers):
            D = int(input_dim) if i == 0 else int(self.units)
            self.fw_lstm.append(_LSTMWeights(D, int(self.units), device=self.device))
            self.bw_lstm.append(_LSTMWeights(D, int(self.units), device=self.device))
            self._sublayers += [self.fw_lstm[-1], self.bw_lstm[-1]]
        self.built = True
        return self

    def operands(self):
        """Per layer (fw kernel, fw recurrent kernel, fw bias, bw kernel, bw recurrent kernel, bw bias) as ops.bilstm and
        training._bilstm take it."""
        return [f.operands() + b.operands() for f, b in zip(self.fw_lstm, self.bw_lstm)]

    def run(self, x, out=None):
        return ops.bilstm(x, self.operands(), res_layers=self.res_layers, merge_mode=self.merge_mode,
                          recurrent_activation=self.recurrent_activation, out=out)

    def call(self, inputs, mask=None, **kwargs):
        if mask is not None:
            raise NotImplementedError("BiLSTM over masked inputs is outside this build: keras' masked-step rule has no kernel")
        x = inputs if inputs.dtype == torch.float32 and inputs.stride(-1) == 1 else inputs.to(torch.float32).contiguous()
        y = self.run(x)
        return list(y) if self.merge_mode is None else y

    def compute_output_shape(self, input_shape):
        if self.merge_mode is None:
            return [input_shape, input_shape]
        elif self.merge_mode == 'concat':
            return input_shape[:-1] + (input_shape[-1] * 2,)
        return input_shape

    def compute_mask(self, inputs, mask=None):
        return mask

    def get_config(self):
        config = {'units': self.units, 'layers': self.layers, 'res_layers': self.res_layers, 'dropout_rate': self.dropout_rate,
                  'merge_mode': self.merge_mode}
        base_config = super(BiLSTM, self).get_config()
        return dict(list(base_config.items()) + list(config.items()))


class BiasEncoding(Layer):
    """Session, position and item biases added to every session's [B, T, E] embeddings (reference sequence.py:706-757).  Inside DSIN
    ``dctr_bias_encoding_fwd`` adds them in place over the [B, S, T, E] lookup buffer; stand-alone the layer takes the reference's
    list of ``sess_max_count`` tensors (one tensor when ``sess_max_count`` is 1) and returns a list."""

    def __init__(self, sess_max_count, seed=1024, **kwargs):
        self.sess_max_count = sess_max_count
        self.seed = seed
        super(BiasEncoding, self).__init__(**kwargs)

    def build(self, input_shape):
        shape = input_shape if self.sess_max_count == 1 and not isinstance(input_shape, list) else input_shape[0]
        return self.build_for(int(shape[1]), int(shape[2]))

    def build_for(self, seq_len_max, embed_size):
        if self.built:
            return self
        init = lambda: TruncatedNormal(mean=0.0, stddev=0.0001, seed=self.seed)    # noqa: E731
        self.add_weight('sess_bias_embedding', (self.sess_max_count, 1, 1), init())
        self.add_weight('seq_bias_embedding', (1, seq_len_max, 1), init())
        self.add_weight('item_bias_embedding', (1, 1, embed_size), init())
        self.built = True
        return self

    def run(self, x):
        """In place over a float32 [B, S, T, E] view."""
        return ops.bias_encoding(x, self.w('sess_bias_embedding'), self.w('seq_bias_embedding'), self.w('item_bias_embedding'))

    def call(self, inputs, mask=None):
        seqs = [inputs] if isinstance(inputs, torch.Tensor) else list(inputs)
        x = torch.stack([t.to(torch.float32) for t in seqs[:self.sess_max_count]], dim=1).contiguous()
        self.run(x)
        return [x[:, i] for i in range(self.sess_max_count)]

    def compute_output_shape(self, input_shape):
        return input_shape

    def compute_mask(self, inputs, mask=None):
        return mask

    def get_config(self):
        config = {'sess_max_count': self.sess_max_count, 'seed': self.seed}
        base_config = super(BiasEncoding, self).get_config()
        return dict(list(base_config.items()) + list(config.items()))


class KMaxPooling(Layer):
    """K Max pooling that selects the k biggest value along the specific axis (reference sequence.py:818-874): nD tensor -> the same
    tensor with ``k`` entries on ``axis``, in descending order of value (tf.nn.top_k(sorted=True)); one ``dctr_kmax_pool_fwd`` launch."""

    def __init__(self, k=1, axis=-1, **kwargs):
        self.k = k
        self.axis = axis
        super(KMaxPooling, self).__init__(**kwargs)

    def build(self, input_shape):
        if self.axis < 1 or self.axis > len(input_shape):
            raise ValueError("axis must be 1~%d,now is %d" % (len(input_shape), self.axis))
        if self.k < 1 or self.k > input_shape[self.axis]:
            raise ValueError("k must be in 1 ~ %d,now k is %d" % (input_shape[self.axis], self.k))
        self.dims = len(input_shape)
        super(KMaxPooling, self).build(input_shape)

    def call(self, inputs):
        return ops.kmax_pool(inputs, self.k, self.axis)

    def compute_output_shape(self, input_shape):
        output_shape = list(input_shape)
        output_shape[self.axis] = self.k
        return tuple(output_shape)

    def get_config(self, ):
        config = {'k': self.k, 'axis': self.axis}
        base_config = super(KMaxPooling, self).get_config()
        return dict(list(base_config.items()) + list(config.items()))
