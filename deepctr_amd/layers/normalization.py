"""``LayerNormalization`` under the reference's name (deepctr/layers/normalization.py:18-51): normalisation over the last axis with a
trainable gain and bias.  Inside the Transformer block it is fused into ``dctr_transformer_fwd``; stand-alone it is one launch of
``dctr_layer_norm_fwd``."""
from .. import ops
from ..initializers import Ones, Zeros
from .base import Layer


class LayerNormalization(Layer):
    def __init__(self, axis=-1, eps=1e-9, center=True, scale=True, **kwargs):
        self.axis = axis
        self.eps = eps
        self.center = center
        self.scale = scale
        super(LayerNormalization, self).__init__(**kwargs)

    def build(self, input_shape):
        return self.build_for(int(input_shape[-1]))

    def build_for(self, dim):
        if self.built:
            return self
        self.add_weight('gamma', (int(dim),), Ones())
        self.add_weight('beta', (int(dim),), Zeros())
        self.built = True
        return self

    def call(self, inputs, **kwargs):
        if self.axis not in (-1, inputs.dim() - 1):
            raise NotImplementedError("LayerNormalization normalises the last axis; axis=%r is outside the kernel" % (self.axis,))
        return ops.layer_norm(inputs, self.w('gamma') if self.scale else None, self.w('beta') if self.center else None, self.eps)

    def compute_output_shape(self, input_shape):
        return input_shape

    def get_config(self):
        config = {'axis': self.axis, 'eps': self.eps, 'center': self.center, 'scale': self.scale}
        base = super(LayerNormalization, self).get_config()
        return dict(list(base.items()) + list(config.items()))
