"""``Dice`` (reference deepctr/layers/activation.py:28-72) and ``activation_layer`` (:75-85), inference form:
BatchNormalization(center=False, scale=False, epsilon=1e-9) uses its moving statistics.

The reference hands any other string to ``tf.keras.layers.Activation(name)`` (:75-85; layers/core.py:176-184).  Of tf.keras 2.x's
names this build runs relu / sigmoid / tanh / linear and ``KERAS_ACTIVATIONS`` — elu (alpha 1), selu, softplus, softsign, exponential,
hard_sigmoid (clip(0.2 z + 0.5, 0, 1), the Keras 2 form), swish (alias silu) and gelu (approximate=False) — in the DNN's kernels
(csrc/act_device.h); softmax and the names only Keras 3 knows raise the ValueError they always did."""
import torch

from ..initializers import Ones, Zeros
from .base import Layer


class Dice(Layer):
    def __init__(self, axis=-1, epsilon=1e-9, **kwargs):
        self.axis = axis
        self.epsilon = epsilon
        super(Dice, self).__init__(**kwargs)

    def build(self, input_shape):
        n = int(input_shape[-1])
        # keras creates Dice's BatchNormalization here (activation.py:51-53); its auto-name shares the counter with the
        # BatchNormalization layers of DNN(use_bn=True).  The statistics live on this layer; `bn_name` is the keras name.
        from .base import next_auto_name
        self.bn_name = next_auto_name("batch_normalization")
        self.add_weight('dice_alpha', (n,), Zeros())
        self.add_weight('moving_mean', (n,), Zeros())
        self.add_weight('moving_variance', (n,), Ones())
        super(Dice, self).build(input_shape)

    def params(self):
        return (self.w('dice_alpha'), self.w('moving_mean'), self.w('moving_variance'))

    def call(self, inputs, training=None, **kwargs):
        # stand-alone use: the fused MLP / attention kernels apply Dice in their epilogue instead
        from .. import ops
        x2 = inputs.reshape(-1, inputs.shape[-1])
        eye = torch.eye(x2.shape[1], device=x2.device)
        y = ops.mlp(x2, [eye], [None], "dice", dice=[self.params()], dice_eps=self.epsilon)
        return y.reshape(inputs.shape)

    def compute_output_shape(self, input_shape):
        return input_shape

    def get_config(self):
        config = {'axis': self.axis, 'epsilon': self.epsilon}
        base = super(Dice, self).get_config()
        return dict(list(base.items()) + list(config.items()))


# what every kernel that reads an activation code takes (EDCN's tower, the multi-task level / tower kernels, DIN's attention unit)
BASE_ACTIVATIONS = ("relu", "sigmoid", "tanh", "linear", "dice", "Dice", None)
# the tf.keras 2.x names the DNN kernels take beside them (dctr_mlp_fwd / dctr_mlp_bwd / dctr_dnn_train_layer_*)
KERAS_ACTIVATIONS = ("elu", "selu", "softplus", "softsign", "exponential", "hard_sigmoid", "swish", "silu", "gelu")
SUPPORTED = BASE_ACTIVATIONS + KERAS_ACTIVATIONS


def require_base_activation(who, activation):
    """For the callers of ``DNN`` whose own kernels read the activation code and take ``BASE_ACTIVATIONS`` only: refuse the other
    names at construction, as ``DNN`` itself refuses a name it does not know."""
    if (isinstance(activation, str) or activation is None) and activation not in BASE_ACTIVATIONS:
        raise ValueError("Invalid activation,found %s.%s runs relu / sigmoid / tanh / linear / dice (its kernels do not take the "
                         "other tf.keras names a plain DNN does)." % (activation, who))


def activation_layer(activation):
    if activation in ("dice", "Dice"):
        return Dice()
    if isinstance(activation, str) or activation is None:
        if activation not in SUPPORTED:
            raise ValueError("Invalid activation,found %s.You should use a str or a Activation Layer Class." % (activation,))
        return activation
    if isinstance(activation, type) and issubclass(activation, Layer):
        return activation()
    raise ValueError("Invalid activation,found %s.You should use a str or a Activation Layer Class." % (activation,))
