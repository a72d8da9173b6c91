"""Host mirror of the ten in-scope layers of the reference's ``deepctr/layers/interaction.py``:
``AFMLayer`` (:39-160), ``CIN`` (:209-341), ``CrossNet`` (:344-435), ``FM`` (:563-607),
``InnerProductLayer`` (:610-694), ``InteractingLayer`` (:697-790), ``SENETLayer`` (:1067-1139), ``BilinearInteraction`` (:1142-1221),
``FwFMLayer`` (:1351-1425), ``FEFMLayer`` (:1428-1499), ``FieldWiseBiInteraction`` (:1224-1348, fieldwise_kernels.hip) and
``FGCNNLayer`` (:937-1064, fieldconv_kernels.hip).
Same constructor kwargs, ``get_config`` and weight names/shapes; ``call`` launches the HIP kernels
(deepctr_amd/csrc/interaction_kernels.hip, cin_kernels.hip, interacting_kernels.hip, bilinear_kernels.hip,
bilinear_bwd_kernels.hip, fieldpair_kernels.hip).  The other six interaction layers of the reference are out of scope."""
import itertools

import torch

from .. import ops
from ..initializers import GlorotNormal, GlorotUniform, Ones, TruncatedNormal, Zeros
from .base import Layer, next_auto_name


def _stack_fields(inputs):
    """list of F tensors [B,1,E] -> [B,F,E] (the reference concatenates on axis 1 before pairing)."""
    return torch.cat(list(inputs), dim=1)


class AFMLayer(Layer):
    def __init__(self, attention_factor=4, l2_reg_w=0, dropout_rate=0, seed=1024, **kwargs):
        self.attention_factor = attention_factor
        self.l2_reg_w = l2_reg_w
        self.dropout_rate = dropout_rate
        self.seed = seed
        super(AFMLayer, self).__init__(**kwargs)

    def build(self, input_shape):
        if not isinstance(input_shape, list) or len(input_shape) < 2:
            raise ValueError('A `AttentionalFM` layer should be called on a list of at least 2 inputs')
        shape_set = set(tuple(s) for s in input_shape)
        if len(shape_set) > 1:
            raise ValueError('A `AttentionalFM` layer requires inputs with same shapes '
                             'Got different shapes: %s' % (shape_set))
        if len(input_shape[0]) != 3 or input_shape[0][1] != 1:
            raise ValueError('A `AttentionalFM` layer requires inputs of a list with same shape tensor like '
                             '(None, 1, embedding_size)Got different shapes: %s' % (input_shape[0],))
        embedding_size = int(input_shape[0][-1])
        self.add_weight("attention_W", (embedding_size, self.attention_factor), GlorotNormal(seed=self.seed))
        self.add_weight("attention_b", (self.attention_factor,), Zeros())
        self.add_weight("projection_h", (self.attention_factor, 1), GlorotNormal(seed=self.seed))
        self.add_weight("projection_p", (embedding_size, 1), GlorotNormal(seed=self.seed))
        super(AFMLayer, self).build(input_shape)

    def call(self, inputs, training=None, **kwargs):
        if inputs[0].dim() != 3:
            raise ValueError("Unexpected inputs dimensions %d, expect to be 3 dimensions" % (inputs[0].dim()))
        if training and self.dropout_rate > 0:
            raise NotImplementedError("dropout is a training-time op; the HIP path is inference (forward) only")
        return ops.afm(_stack_fields(inputs), self.w("attention_W"), self.w("attention_b"), self.w("projection_h"),
                       self.w("projection_p"))

    def compute_output_shape(self, input_shape):
        if not isinstance(input_shape, list):
            raise ValueError('A `AFMLayer` layer should be called on a list of inputs.')
        return (None, 1)

    def get_config(self):
        config = {'attention_factor': self.attention_factor, 'l2_reg_w': self.l2_reg_w,
                  'dropout_rate': self.dropout_rate, 'seed': self.seed}
        base = super(AFMLayer, self).get_config()
        base.update(config)
        return base


class CIN(Layer):
    def __init__(self, layer_size=(128, 128), activation='relu', split_half=True, l2_reg=1e-5, seed=1024, **kwargs):
        if len(layer_size) == 0:
            raise ValueError("layer_size must be a list(tuple) of length greater than 1")
        self.layer_size = layer_size
        self.split_half = split_half
        self.activation = activation
        self.l2_reg = l2_reg
        self.seed = seed
        super(CIN, self).__init__(**kwargs)

    def build(self, input_shape):
        if len(input_shape) != 3:
            raise ValueError("Unexpected inputs dimensions %d, expect to be 3 dimensions" % (len(input_shape)))
        self.build_for(int(input_shape[1]))

    def build_for(self, field_num):
        if self.built:
            return self
        self.field_nums = [int(field_num)]
        for i, size in enumerate(self.layer_size):
            self.add_weight('filter' + str(i), (1, self.field_nums[-1] * self.field_nums[0], size),
                            GlorotUniform(seed=self.seed + i))
            self.add_weight('bias' + str(i), (size,), Zeros())
            if self.split_half:
                if i != len(self.layer_size) - 1 and size % 2 > 0:
                    raise ValueError("layer_size must be even number except for the last layer when split_half=True")
                self.field_nums.append(size // 2)
            else:
                self.field_nums.append(size)
        self.built = True
        return self

    @property
    def filters(self):
        return [self.w('filter%d' % i) for i in range(len(self.layer_size))]

    @property
    def biases(self):
        return [self.w('bias%d' % i) for i in range(len(self.layer_size))]

    def call(self, inputs, **kwargs):
        if inputs.dim() != 3:
            raise ValueError("Unexpected inputs dimensions %d, expect to be 3 dimensions" % (inputs.dim()))
        return ops.cin(inputs, self.filters, self.biases, list(self.layer_size), self.split_half, self.activation)

    def compute_output_shape(self, input_shape):
        return (None, ops.cin_output_dim(list(self.layer_size), self.split_half))

    def get_config(self):
        config = {'layer_size': self.layer_size, 'split_half': self.split_half, 'activation': self.activation,
                  'seed': self.seed}
        base = super(CIN, self).get_config()
        base.update(config)
        return base


class InteractingLayer(Layer):
    """Multi-head self-attention across the fields (reference interaction.py:697-790): x [B,F,E] -> [B,F,d*H]."""

    def __init__(self, att_embedding_size=8, head_num=2, use_res=True, scaling=False, seed=1024, **kwargs):
        if head_num <= 0:
            raise ValueError('head_num must be a int > 0')
        self.att_embedding_size = att_embedding_size
        self.head_num = head_num
        self.use_res = use_res
        self.seed = seed
        self.scaling = scaling
        super(InteractingLayer, self).__init__(**kwargs)

    def build(self, input_shape):
        if len(input_shape) != 3:
            raise ValueError("Unexpected inputs dimensions %d, expect to be 3 dimensions" % (len(input_shape)))
        return self.build_for(int(input_shape[-1]))

    def build_for(self, embedding_size):
        if self.built:
            return self
        shape = (int(embedding_size), self.att_embedding_size * self.head_num)
        self.add_weight('query', shape, TruncatedNormal(seed=self.seed))
        self.add_weight('key', shape, TruncatedNormal(seed=self.seed + 1))
        self.add_weight('value', shape, TruncatedNormal(seed=self.seed + 2))
        if self.use_res:
            self.add_weight('res', shape, TruncatedNormal(seed=self.seed))
        self.built = True
        return self

    @property
    def weights_qkvr(self):
        """(query, key, value, res or None): the operands of one layer of ops.interacting."""
        return (self.w('query'), self.w('key'), self.w('value'), self.w('res') if self.use_res else None)

    def call(self, inputs, **kwargs):
        if inputs.dim() != 3:
            raise ValueError("Unexpected inputs dimensions %d, expect to be 3 dimensions" % (inputs.dim()))
        qkvr = self.weights_qkvr
        if inputs.is_cuda and torch.is_grad_enabled() and (inputs.requires_grad or any(w is not None and w.requires_grad for w in qkvr)):
            # differentiable: the same forward launch, dctr_interacting_bwd behind it
            y = ops.InteractingFunction.apply(inputs, self.att_embedding_size, self.head_num, self.use_res, self.scaling, *qkvr)
        else:
            y = ops.interacting(inputs, [qkvr], self.att_embedding_size, self.head_num, self.use_res, self.scaling)
        return y.reshape(inputs.shape[0], inputs.shape[1], self.att_embedding_size * self.head_num)

    def compute_output_shape(self, input_shape):
        return (None, input_shape[1], self.att_embedding_size * self.head_num)

    def get_config(self):
        # (the reference's omits scaling)
        config = {'att_embedding_size': self.att_embedding_size, 'head_num': self.head_num, 'use_res': self.use_res,
                  'seed': self.seed}
        base = super(InteractingLayer, self).get_config()
        base.update(config)
        return base


class SENETLayer(Layer):
    """Squeeze-excitation reweighting of the fields (reference interaction.py:1067-1139): a list of F tensors [B,1,E] -> the same
    list, each field scaled by A2[f] = relu(relu(mean_E(x) W_1) W_2)[f]."""

    def __init__(self, reduction_ratio=3, seed=1024, **kwargs):
        self.reduction_ratio = reduction_ratio
        self.seed = seed
        super(SENETLayer, self).__init__(**kwargs)

    def build(self, input_shape):
        if not isinstance(input_shape, list) or len(input_shape) < 2:
            raise ValueError('A `AttentionalFM` layer should be called on a list of at least 2 inputs')
        return self.build_for(len(input_shape), int(input_shape[0][-1]))

    def build_for(self, field_size, embedding_size):
        if self.built:
            return self
        self.filed_size = int(field_size)
        self.embedding_size = int(embedding_size)
        reduction_size = max(1, self.filed_size // self.reduction_ratio)
        self.add_weight("W_1", (self.filed_size, reduction_size), GlorotNormal(seed=self.seed))
        self.add_weight("W_2", (reduction_size, self.filed_size), GlorotNormal(seed=self.seed))
        self.built = True
        return self

    @property
    def weights_w12(self):
        return (self.w("W_1"), self.w("W_2"))

    def call(self, inputs, training=None, **kwargs):
        if inputs[0].dim() != 3:
            raise ValueError("Unexpected inputs dimensions %d, expect to be 3 dimensions" % (inputs[0].dim()))
        x = _stack_fields(inputs)
        B, F, E = x.shape
        w12 = self.weights_w12
        if x.is_cuda and torch.is_grad_enabled() and (x.requires_grad or any(w.requires_grad for w in w12)):
            # differentiable: the same forward launch, dctr_bilinear_bwd behind it
            y = ops.SenetBilinearFunction.apply(x.reshape(B, F * E), F, E, 0, "interaction", "senet", *w12)
        else:
            y = ops.senet_bilinear(x, senet_w=w12)
        return list(torch.split(y.reshape(B, F, E), 1, dim=1))

    def compute_output_shape(self, input_shape):
        return input_shape

    def compute_mask(self, inputs, mask=None):
        return [None] * self.filed_size

    def get_config(self):
        config = {'reduction_ratio': self.reduction_ratio, 'seed': self.seed}
        base = super(SENETLayer, self).get_config()
        base.update(config)
        return base


class BilinearInteraction(Layer):
    """Bilinear interaction of every field pair (reference interaction.py:1142-1221): a list of F tensors [B,1,E] -> [B, F(F-1)/2, E],
    p_ij = (x_i W) * x_j over i < j in itertools.combinations order, W shared ('all'), per i ('each') or per pair ('interaction')."""

    def __init__(self, bilinear_type="interaction", seed=1024, **kwargs):
        self.bilinear_type = bilinear_type
        self.seed = seed
        super(BilinearInteraction, self).__init__(**kwargs)

    def build(self, input_shape):
        if not isinstance(input_shape, list) or len(input_shape) < 2:
            raise ValueError('A `AttentionalFM` layer should be called on a list of at least 2 inputs')
        return self.build_for(len(input_shape), int(input_shape[0][-1]))

    def build_for(self, field_size, embedding_size):
        if self.built:
            return self
        F, E = int(field_size), int(embedding_size)
        shape, init = (E, E), (lambda: GlorotNormal(seed=self.seed))
        if self.bilinear_type == "all":
            self.add_weight("bilinear_weight", shape, init())
        elif self.bilinear_type == "each":
            for i in range(F - 1):
                self.add_weight("bilinear_weight" + str(i), shape, init())
        elif self.bilinear_type == "interaction":
            for i, j in itertools.combinations(range(F), 2):
                self.add_weight("bilinear_weight" + str(i) + '_' + str(j), shape, init())
        else:
            raise NotImplementedError("bilinear_type %r: expected 'all', 'each' or 'interaction'" % (self.bilinear_type,))
        self.filed_size = F
        self.built = True
        return self

    @property
    def matrices(self):
        """The layer's [E,E] weights in the order ops.senet_bilinear takes them (creation order = the reference's)."""
        return list(self._weights.values())

    def call(self, inputs, **kwargs):
        if inputs[0].dim() != 3:
            raise ValueError("Unexpected inputs dimensions %d, expect to be 3 dimensions" % (inputs[0].dim()))
        x = _stack_fields(inputs)
        B, F, E = x.shape
        ws = self.matrices
        if x.is_cuda and torch.is_grad_enabled() and (x.requires_grad or any(w.requires_grad for w in ws)):
            # differentiable: the same forward launch, dctr_bilinear_bwd behind it
            y = ops.SenetBilinearFunction.apply(x.reshape(B, F * E), F, E, 0, self.bilinear_type, "layer", *ws)
        else:
            y = ops.senet_bilinear(x, bilinear_w=ws, bilinear_type=self.bilinear_type)
        return y.reshape(B, F * (F - 1) // 2, E)

    def compute_output_shape(self, input_shape):
        filed_size = len(input_shape)
        return (None, filed_size * (filed_size - 1) // 2, input_shape[0][-1])

    def get_config(self):
        config = {'bilinear_type': self.bilinear_type, 'seed': self.seed}
        base = super(BilinearInteraction, self).get_config()
        base.update(config)
        return base


class FieldWiseBiInteraction(Layer):
    """FLEN's field-wise bi-interaction (reference interaction.py:1224-1348): a list of G >= 2 tensors [B, n_g, E], one per field
    group -> [B, E].  With s_g / q_g the sum / the sum of squares of group g's embeddings:
    (sum_{i<j} kernel_mf[p(i,j)] s_i s_j + bias_mf) + (sum_g kernel_fm[g] (s_g^2 - q_g) + bias_fm), pairs in
    itertools.combinations order.  One ``dctr_fieldwise_fwd`` launch."""

    def __init__(self, use_bias=True, seed=1024, **kwargs):
        self.use_bias = use_bias
        self.seed = seed
        super(FieldWiseBiInteraction, self).__init__(**kwargs)

    def build(self, input_shape):
        if not isinstance(input_shape, list) or len(input_shape) < 2:
            raise ValueError('A `Field-Wise Bi-Interaction` layer should be called on a list of at least 2 inputs')
        return self.build_for(len(input_shape), int(input_shape[0][-1]))

    def build_for(self, num_fields, embedding_size):
        if self.built:
            return self
        if int(num_fields) < 2:
            raise ValueError('A `Field-Wise Bi-Interaction` layer should be called on a list of at least 2 inputs')
        self.num_fields = int(num_fields)           # (the reference's name for the number of field GROUPS)
        self.add_weight('kernel_mf', (self.num_fields * (self.num_fields - 1) // 2, 1), Ones())
        self.add_weight('kernel_fm', (self.num_fields, 1), lambda shape: torch.full(shape, 0.5))
        if self.use_bias:
            self.add_weight('bias_mf', (int(embedding_size),), Zeros())
            self.add_weight('bias_fm', (int(embedding_size),), Zeros())
        self.built = True
        return self

    @property
    def biases(self):
        return (self.w('bias_mf'), self.w('bias_fm')) if self.use_bias else (None, None)

    def call(self, inputs, **kwargs):
        if inputs[0].dim() != 3:
            raise ValueError("Unexpected inputs dimensions %d, expect to be 3 dimensions" % (inputs[0].dim()))
        if len(inputs) != self.num_fields:
            raise ValueError("FieldWiseBiInteraction was built for %d field groups, got %d" % (self.num_fields, len(inputs)))
        B, dim = inputs[0].shape[0], inputs[0].shape[2]
        x = torch.cat([t.reshape(B, -1) for t in inputs], dim=1)
        groups, first = [], 0
        for t in inputs:
            groups.append((first, t.shape[1]))
            first += t.shape[1] * dim
        bias_mf, bias_fm = self.biases
        y, _ = ops.fieldwise(x, groups, dim, self.w('kernel_mf'), self.w('kernel_fm'), bias_mf, bias_fm)
        return y

    def compute_output_shape(self, input_shape):
        return (None, input_shape[0][-1])

    def get_config(self):
        config = {'use_bias': self.use_bias, 'seed': self.seed}
        base = super(FieldWiseBiInteraction, self).get_config()
        base.update(config)
        return base


class FwFMLayer(Layer):
    """Field-weighted factorization machine (reference interaction.py:1351-1425): x [B,F,E] -> [B,1],
    sum_{i<j} field_pair_strengths[i][j] <x_i, x_j>."""

    def __init__(self, num_fields=4, regularizer=0.000001, **kwargs):
        self.num_fields = num_fields
        self.regularizer = regularizer
        super(FwFMLayer, self).__init__(**kwargs)

    def build(self, input_shape):
        if len(input_shape) != 3:
            raise ValueError("Unexpected inputs dimensions %d, expect to be 3 dimensions" % (len(input_shape)))
        if input_shape[1] != self.num_fields:
            raise ValueError("Mismatch in number of fields {} and concatenated embeddings dims {}".format(self.num_fields,
                                                                                                         input_shape[1]))
        return self.build_for()

    def build_for(self):
        if self.built:
            return self
        self.add_weight('field_pair_strengths', (self.num_fields, self.num_fields), TruncatedNormal())
        self.built = True
        return self

    @property
    def field_strengths(self):
        return self.w('field_pair_strengths')

    def call(self, inputs, **kwargs):
        if inputs.dim() != 3:
            raise ValueError("Unexpected inputs dimensions %d, expect to be 3 dimensions" % (inputs.dim()))
        if inputs.shape[1] != self.num_fields:
            raise ValueError("Mismatch in number of fields {} and concatenated embeddings dims {}".format(self.num_fields,
                                                                                                         inputs.shape[1]))
        r = self.field_strengths
        if inputs.is_cuda and torch.is_grad_enabled() and (inputs.requires_grad or r.requires_grad):
            # differentiable: the same forward launch, dctr_fieldpair_bwd behind it
            _, logit = ops.FieldPairFunction.apply(inputs, "fwfm", False, True, r)
        else:
            _, logit = ops.fieldpair(inputs, r, kind="fwfm")
        return logit.reshape(-1, 1)

    def compute_output_shape(self, input_shape):
        return (None, 1)

    def get_config(self):
        config = {'num_fields': self.num_fields, 'regularizer': self.regularizer}
        base = super(FwFMLayer, self).get_config()
        base.update(config)
        return base


class FEFMLayer(Layer):
    """Field-embedded factorization machine (reference interaction.py:1428-1499): x [B,F,E] -> [B, F(F-1)/2], per pair i < j
    (itertools.combinations order) x_i^T (W_ij + W_ij^T) x_j with one [E,E] matrix ``field_embeddings<i>-<j>`` per pair."""

    def __init__(self, regularizer, **kwargs):
        self.regularizer = regularizer
        super(FEFMLayer, self).__init__(**kwargs)

    def build(self, input_shape):
        if len(input_shape) != 3:
            raise ValueError("Unexpected inputs dimensions %d, expect to be 3 dimensions" % (len(input_shape)))
        return self.build_for(int(input_shape[1]), int(input_shape[2]))

    def build_for(self, num_fields, embedding_size):
        if self.built:
            return self
        self.num_fields = int(num_fields)
        shape = (int(embedding_size), int(embedding_size))
        # (the reference's TruncatedNormal() is unseeded: every matrix its own draw — here the pair index seeds it)
        for p, (fi, fj) in enumerate(itertools.combinations(range(self.num_fields), 2)):
            self.add_weight('field_embeddings' + str(fi) + "-" + str(fj), shape, TruncatedNormal(seed=p))
        self.built = True
        return self

    @property
    def matrices(self):
        """The pair matrices in the order ops.fieldpair takes them (creation order = itertools.combinations)."""
        return list(self._weights.values())

    def call(self, inputs, **kwargs):
        if inputs.dim() != 3:
            raise ValueError("Unexpected inputs dimensions %d, expect to be 3 dimensions" % (inputs.dim()))
        ws = self.matrices
        if inputs.is_cuda and torch.is_grad_enabled() and (inputs.requires_grad or any(w.requires_grad for w in ws)):
            # differentiable: the same forward launch, dctr_fieldpair_bwd behind it
            pairs, _ = ops.FieldPairFunction.apply(inputs, "fefm", True, False, *ws)
        else:
            pairs, _ = ops.fieldpair(inputs, ws, kind="fefm", pairs=True)
        return pairs

    def compute_output_shape(self, input_shape):
        num_fields = int(input_shape[1])
        return (None, (num_fields * (num_fields - 1)) / 2)

    def get_config(self):
        config = {'regularizer': self.regularizer}
        base = super(FEFMLayer, self).get_config()
        base.update(config)
        return base


class CrossNet(Layer):
    def __init__(self, layer_num=2, parameterization='vector', l2_reg=0, seed=1024, **kwargs):
        self.layer_num = layer_num
        self.parameterization = parameterization
        self.l2_reg = l2_reg
        self.seed = seed
        print('CrossNet parameterization:', self.parameterization)
        super(CrossNet, self).__init__(**kwargs)

    def build(self, input_shape):
        if len(input_shape) != 2:
            raise ValueError("Unexpected inputs dimensions %d, expect to be 2 dimensions" % (len(input_shape),))
        self.build_for(int(input_shape[-1]))

    def build_for(self, dim):
        if self.built:
            return self
        if self.parameterization == 'vector':
            shape = (dim, 1)
        elif self.parameterization == 'matrix':
            shape = (dim, dim)
        else:
            raise ValueError("parameterization should be 'vector' or 'matrix'")
        for i in range(self.layer_num):
            self.add_weight('kernel' + str(i), shape, GlorotNormal(seed=self.seed))
        for i in range(self.layer_num):
            self.add_weight('bias' + str(i), (dim, 1), Zeros())
        self.dim = dim
        self.built = True
        return self

    def packed(self):
        """kernels [L,d] / [L,d,d] and bias [L,d] as the C ABI wants them (a gather of small tensors)."""
        if self.layer_num == 0:
            return None, None
        ks = torch.stack([self.w('kernel%d' % i).reshape(self.dim, -1) for i in range(self.layer_num)])
        if self.parameterization == 'vector':
            ks = ks.reshape(self.layer_num, self.dim)
        bs = torch.stack([self.w('bias%d' % i).reshape(self.dim) for i in range(self.layer_num)])
        return ks.contiguous(), bs.contiguous()

    def call(self, inputs, **kwargs):
        if inputs.dim() != 2:
            raise ValueError("Unexpected inputs dimensions %d, expect to be 2 dimensions" % (inputs.dim()))
        ks, bs = self.packed()
        return ops.crossnet(inputs, ks, bs, self.parameterization)

    def get_config(self):
        config = {'layer_num': self.layer_num, 'parameterization': self.parameterization, 'l2_reg': self.l2_reg,
                  'seed': self.seed}
        base = super(CrossNet, self).get_config()
        base.update(config)
        return base

    def compute_output_shape(self, input_shape):
        return input_shape


class CrossNetMix(Layer):
    """Mirror of deepctr.layers.interaction.CrossNetMix (:438-560): the cross part of DCN-Mix (mixture of low-rank experts)."""

    def __init__(self, low_rank=32, num_experts=4, layer_num=2, l2_reg=0, seed=1024, **kwargs):
        self.low_rank = low_rank
        self.num_experts = num_experts
        self.layer_num = layer_num
        self.l2_reg = l2_reg
        self.seed = seed
        super(CrossNetMix, self).__init__(**kwargs)

    def build(self, input_shape):
        if len(input_shape) != 2:
            raise ValueError("Unexpected inputs dimensions %d, expect to be 2 dimensions" % (len(input_shape),))
        self.build_for(int(input_shape[-1]))

    def build_for(self, dim):
        if self.built:
            return self
        from .core import Dense
        for k in ('U_list', 'V_list'):
            for i in range(self.layer_num):
                self.add_weight(k + str(i), (self.num_experts, dim, self.low_rank), GlorotNormal(seed=self.seed))
        for i in range(self.layer_num):
            self.add_weight('C_list' + str(i), (self.num_experts, self.low_rank, self.low_rank), GlorotNormal(seed=self.seed))
        # one Dense(1, use_bias=False) per expert, shared by every cross layer (:502, :524)
        self.gating = [Dense(1, use_bias=False, device=self.device).build_for(dim) for _ in range(self.num_experts)]
        self._sublayers.extend(self.gating)
        for i in range(self.layer_num):
            self.add_weight('bias' + str(i), (dim, 1), Zeros())
        self.dim = dim
        self.built = True
        return self

    def packed(self):
        """(U, V [L,experts,d,r], C [L,experts,r,r], gating [experts,d], bias [L,d]) as the C ABI takes them."""
        if self.layer_num == 0:
            return None, None, None, None, None
        st = lambda k: torch.stack([self.w(k + str(i)) for i in range(self.layer_num)]).contiguous()   # noqa: E731
        g = torch.stack([d.w('kernel').reshape(self.dim) for d in self.gating]).contiguous()
        b = torch.stack([self.w('bias%d' % i).reshape(self.dim) for i in range(self.layer_num)]).contiguous()
        return st('U_list'), st('V_list'), st('C_list'), g, b

    def call(self, inputs, **kwargs):
        if inputs.dim() != 2:
            raise ValueError("Unexpected inputs dimensions %d, expect to be 2 dimensions" % (inputs.dim()))
        return ops.crossnet_mix(inputs, *self.packed())

    def get_config(self):
        config = {'low_rank': self.low_rank, 'num_experts': self.num_experts, 'layer_num': self.layer_num,
                  'l2_reg': self.l2_reg, 'seed': self.seed}
        base = super(CrossNetMix, self).get_config()
        base.update(config)
        return base

    def compute_output_shape(self, input_shape):
        return input_shape


class FM(Layer):
    def build(self, input_shape):
        if len(input_shape) != 3:
            raise ValueError("Unexpected inputs dimensions % d, expect to be 3 dimensions" % (len(input_shape)))
        super(FM, self).build(input_shape)

    def call(self, inputs, **kwargs):
        if inputs.dim() != 3:
            raise ValueError("Unexpected inputs dimensions %d, expect to be 3 dimensions" % (inputs.dim()))
        return ops.fm(inputs)

    def compute_output_shape(self, input_shape):
        return (None, 1)


class BiInteractionPooling(Layer):
    """Mirror of deepctr.layers.interaction.BiInteractionPooling (:170-211)."""

    def build(self, input_shape):
        if len(input_shape) != 3:
            raise ValueError("Unexpected inputs dimensions %d, expect to be 3 dimensions" % (len(input_shape)))
        super(BiInteractionPooling, self).build(input_shape)

    def call(self, inputs, **kwargs):
        if inputs.dim() != 3:
            raise ValueError("Unexpected inputs dimensions %d, expect to be 3 dimensions" % (inputs.dim()))
        return ops.bi_interaction(inputs)

    def compute_output_shape(self, input_shape):
        return (None, 1, input_shape[-1])


class OutterProductLayer(Layer):
    """Weight holder only: PNN (reference models/pnn.py:49) instantiates this layer, and thereby its kernel, even with
    use_outter=False, so Keras weight lists of a reference PNN contain it.  The outer-product arithmetic
    (interaction.py:866-924) is outside SURVEY §8 and calling the layer raises."""

    def __init__(self, kernel_type='mat', seed=1024, **kwargs):
        if kernel_type not in ['mat', 'vec', 'num']:
            raise ValueError("kernel_type must be mat,vec or num")
        self.kernel_type = kernel_type
        self.seed = seed
        super(OutterProductLayer, self).__init__(**kwargs)

    def build_for(self, num_inputs, embed_size):
        if self.built:
            return self
        num_pairs = int(num_inputs * (num_inputs - 1) / 2)
        shape = {'mat': (embed_size, num_pairs, embed_size), 'vec': (num_pairs, embed_size), 'num': (num_pairs, 1)}[self.kernel_type]
        self.add_weight('kernel', shape, GlorotUniform(seed=self.seed))
        self.built = True
        return self

    def call(self, inputs, **kwargs):
        raise NotImplementedError("OutterProductLayer arithmetic is outside the MI355X hot-path scope (SURVEY.md §8)")

    def get_config(self):
        base = super(OutterProductLayer, self).get_config()
        base.update({'kernel_type': self.kernel_type, 'seed': self.seed})
        return base


class InnerProductLayer(Layer):
    def __init__(self, reduce_sum=True, **kwargs):
        self.reduce_sum = reduce_sum
        super(InnerProductLayer, self).__init__(**kwargs)

    def build(self, input_shape):
        if not isinstance(input_shape, list) or len(input_shape) < 2:
            raise ValueError('A `InnerProductLayer` layer should be called on a list of at least 2 inputs')
        shape_set = set(tuple(s) for s in input_shape)
        if len(shape_set) > 1:
            raise ValueError('A `InnerProductLayer` layer requires inputs with same shapes '
                             'Got different shapes: %s' % (shape_set))
        if len(input_shape[0]) != 3 or input_shape[0][1] != 1:
            raise ValueError('A `InnerProductLayer` layer requires inputs of a list with same shape tensor like '
                             '(None,1,embedding_size)Got different shapes: %s' % (input_shape[0],))
        super(InnerProductLayer, self).build(input_shape)

    def call(self, inputs, **kwargs):
        if inputs[0].dim() != 3:
            raise ValueError("Unexpected inputs dimensions %d, expect to be 3 dimensions" % (inputs[0].dim()))
        return ops.inner_product(_stack_fields(inputs), self.reduce_sum)

    def compute_output_shape(self, input_shape):
        num_inputs = len(input_shape)
        num_pairs = int(num_inputs * (num_inputs - 1) / 2)
        input_shape = input_shape[0]
        if self.reduce_sum:
            return (input_shape[0], num_pairs, 1)
        return (input_shape[0], num_pairs, input_shape[-1])

    def get_config(self):
        config = {'reduce_sum': self.reduce_sum}
        base = super(InnerProductLayer, self).get_config()
        base.update(config)
        return base


class BridgeModule(Layer):
    """Bridge module of EDCN (reference interaction.py:1502-1565): [x, h], two [B, D] tensors -> [B, D] by 'pointwise_addition',
    'hadamard_product', 'concatenation' (a Dense(D, activation) over [x, h]) or 'attention_pooling' (softmax-DNN(x) * x +
    softmax-DNN(h) * h, two DNN([D, D], activation, output_activation='softmax')).  As in the reference an unknown ``bridge_type``
    builds no weights; here it is refused when the layer is called (the reference returns None)."""
    TYPES = ("pointwise_addition", "hadamard_product", "concatenation", "attention_pooling")

    def __init__(self, bridge_type='hadamard_product', activation='relu', **kwargs):
        self.bridge_type = bridge_type
        self.activation = activation
        super(BridgeModule, self).__init__(**kwargs)

    def build(self, input_shape):
        if not isinstance(input_shape, list) or len(input_shape) < 2:
            raise ValueError('A `BridgeModule` layer should be called on a list of 2 inputs')
        self.build_for(int(input_shape[0][-1]))

    def build_for(self, dnn_dim):
        if self.built:
            return self
        from .core import DNN, Dense
        self.dnn_dim = D = int(dnn_dim)
        self.dense = self.dense_x = self.dense_h = None
        if self.bridge_type == "concatenation":
            if self.activation not in ("relu", "sigmoid", "tanh", "linear", None):
                raise ValueError("BridgeModule: the Dense of 'concatenation' takes relu / sigmoid / tanh / linear, got %r" % (self.activation,))
            self.dense = Dense(D, device=self.device).build_for(2 * D)
            self._sublayers.append(self.dense)
        elif self.bridge_type == "attention_pooling":
            # (the softmax of the last layer is the bridge kernel's: the DNNs end linear here and keep the reference's names)
            self.dense_x = DNN([D, D], self.activation, device=self.device).build_for(D)
            self.dense_h = DNN([D, D], self.activation, device=self.device).build_for(D)
            self._sublayers += [self.dense_x, self.dense_h]
        self.built = True
        return self

    def weights_for_op(self):
        """This round's ``bridge_weights`` entry of ops.edcn (None for the weightless bridges)."""
        if self.bridge_type == "concatenation":
            return (self.dense.w('kernel'), self.dense.w('bias'))
        if self.bridge_type == "attention_pooling":
            return tuple((dn.w('kernel0'), dn.w('bias0'), dn.w('kernel1'), dn.w('bias1')) for dn in (self.dense_x, self.dense_h))
        return None

    def call(self, inputs, **kwargs):
        x, h = inputs
        if self.bridge_type not in self.TYPES:
            raise ValueError("BridgeModule: unknown bridge_type %r" % (self.bridge_type,))
        if self.bridge_type == "concatenation":
            return ops.mlp(torch.cat([x, h], dim=-1), [self.dense.w('kernel')], [self.dense.w('bias')], self.activation or "linear")
        if self.bridge_type == "attention_pooling":
            ax, ah = (self._scores(dn, t) for dn, t in ((self.dense_x, x), (self.dense_h, h)))
            return ops.edcn_bridge(x.contiguous(), h.contiguous(), self.bridge_type, ax=ax, ah=ah)
        return ops.edcn_bridge(x.contiguous(), h.contiguous(), self.bridge_type)

    def _scores(self, dn, t):
        hid = ops.mlp(t, [dn.w('kernel0')], [dn.w('bias0')], dn.activation, dice=None if not dn.dice_layers else [dn.dice_layers[0].params()])
        return ops.mlp(hid, [dn.w('kernel1')], [dn.w('bias1')], "linear")

    def compute_output_shape(self, input_shape):
        return (None, self.dnn_dim)

    def get_config(self):
        base = super(BridgeModule, self).get_config()
        base.update({'bridge_type': self.bridge_type, 'activation': self.activation})
        return base


class _Conv2DWeights(Layer):
    """The weights of one tf.keras.layers.Conv2D(filters, (width, 1)) under keras' names: ``kernel`` [width, 1, C_in, filters]
    (glorot_uniform over fan_in = width C_in, fan_out = width filters) and ``bias`` [filters] (zeros)."""

    def __init__(self, width, in_channels, filters, **kwargs):
        super(_Conv2DWeights, self).__init__(name=next_auto_name("conv2d"), **kwargs)
        self.add_weight("kernel", (int(width), 1, int(in_channels), int(filters)), GlorotUniform())
        self.add_weight("bias", (int(filters),), Zeros())
        self.built = True


class FGCNNLayer(Layer):
    """Feature Generation Layer used in FGCNN, including Convolution, MaxPooling and Recombination (reference interaction.py:937-1064):
    [B, F, E] -> the new features [B, sum_i rows_i new_maps_i, E].  The conv / pool stack is ONE ``dctr_fieldconv_fwd`` launch that also
    hands out every stage's pooled map; each stage's recombination Dense(rows E new_maps, tanh) reads its map in place through the DNN
    kernel and writes its new fields straight into the output at their field offset (the reference's reshape of the flat row to
    (rows new_maps, E) is a reinterpretation)."""

    def __init__(self, filters=(14, 16,), kernel_width=(7, 7,), new_maps=(3, 3,), pooling_width=(2, 2), **kwargs):
        if not (len(filters) == len(kernel_width) == len(new_maps) == len(pooling_width)):
            raise ValueError("length of argument must be equal")
        self.filters = filters
        self.kernel_width = kernel_width
        self.new_maps = new_maps
        self.pooling_width = pooling_width
        super(FGCNNLayer, self).__init__(**kwargs)

    def build(self, input_shape):
        if len(input_shape) != 3:
            raise ValueError("Unexpected inputs dimensions %d, expect to be 3 dimensions" % (len(input_shape)))
        return self.build_for(int(input_shape[1]), int(input_shape[2]))

    def build_for(self, field_size, embedding_size):
        if self.built:
            return self
        from .core import Dense
        self.field_size, self.embedding_size = int(field_size), int(embedding_size)
        self.conv_layers, self.dense_layers, self.rows = [], [], []
        rows, cin = self.field_size, 1
        for filters, width, new, pool in zip(self.filters, self.kernel_width, self.new_maps, self.pooling_width):
            if int(pool) < 1 or rows // int(pool) < 1:
                raise ValueError("FGCNNLayer: pooling width %d over %d rows leaves an empty feature map" % (pool, rows))
            conv = _Conv2DWeights(width, cin, filters, device=self.device)
            rows, cin = rows // int(pool), int(filters)
            dense = Dense(rows * self.embedding_size * int(new), device=self.device).build_for(rows * self.embedding_size * cin)
            self.conv_layers.append(conv)
            self.dense_layers.append(dense)
            self.rows.append(rows)
            self._sublayers += [conv, dense]
        self.new_features = sum(r * int(n) for r, n in zip(self.rows, self.new_maps))
        self._maps = {}
        self.built = True
        return self

    @property
    def pools(self):
        return [("max", int(p)) for p in self.pooling_width]

    @property
    def conv_kernels(self):
        return [c.w("kernel") for c in self.conv_layers]

    @property
    def conv_biases(self):
        return [c.w("bias") for c in self.conv_layers]

    def _stage_maps(self, B, device):
        """Per batch size, the buffers that receive the stages' pooled maps (rows padded to 4 floats with zeros: the DNN kernel may
        read the padding)."""
        key = (B, str(device))
        bufs = self._maps.pop(key, None)
        if bufs is None:
            while len(self._maps) >= 4:                     # least recently used out
                self._maps.pop(next(iter(self._maps)))
            E = self.embedding_size
            bufs = [torch.zeros(B, (r * E * int(c) + 3) // 4 * 4, dtype=torch.float32, device=device) for r, c in zip(self.rows, self.filters)]
        self._maps[key] = bufs                              # (dicts keep insertion order: most recently used last)
        return bufs

    def run(self, x, out, out_offset=0, fields=None, dim=None, x_offset=0):
        """x: [B, F, E], or with ``fields`` / ``dim`` a [B, stride] buffer read in place from ``x_offset``; the new features go to the
        columns [out_offset, out_offset + new_features E) of the float32 [B, stride] buffer ``out``."""
        B, E = int(x.shape[0]), self.embedding_size
        maps = self._stage_maps(B, x.device)
        ops.field_conv(x, self.conv_kernels, self.conv_biases, self.pools, fields=fields, dim=dim, x_offset=x_offset, out=maps[-1],
                       stage_outs=maps[:-1] + [None])
        off = int(out_offset)
        for m, dense, r, c, new in zip(maps, self.dense_layers, self.rows, self.filters, self.new_maps):
            n = r * E * int(new)
            ops.mlp(m, [dense.w("kernel")], [dense.w("bias")], "tanh", in_dim=r * E * int(c), out=out[:, off:off + n])
            off += n
        return out

    def call(self, inputs, **kwargs):
        if inputs.dim() != 3:
            raise ValueError("Unexpected inputs dimensions %d, expect to be 3 dimensions" % (inputs.dim()))
        B, E = int(inputs.shape[0]), self.embedding_size
        out = torch.empty(B, self.new_features * E, dtype=torch.float32, device=inputs.device)
        return self.run(inputs, out).reshape(B, self.new_features, E)

    def compute_output_shape(self, input_shape):
        new_features_num = 0
        features_num = input_shape[1]
        for i in range(0, len(self.kernel_width)):
            pooled_features_num = features_num // self.pooling_width[i]
            new_features_num += self.new_maps[i] * pooled_features_num
            features_num = pooled_features_num
        return (None, new_features_num, input_shape[-1])

    def get_config(self, ):
        config = {'kernel_width': self.kernel_width, 'filters': self.filters, 'new_maps': self.new_maps,
                  'pooling_width': self.pooling_width}
        base_config = super(FGCNNLayer, self).get_config()
        base_config.update(config)
        return base_config
