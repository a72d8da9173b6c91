"""Optimizer objects for ``model.compile`` — tf.keras' ``optimizer_v2`` classes restated as plain Python.

    from deepctr_amd.optimizers import Adagrad, Ftrl
    model.compile(Adagrad(0.1024), "binary_crossentropy")
    model.compile(Ftrl(0.05, l1_regularization_strength=1e-4), "binary_crossentropy")

Argument names, order and defaults are tf.keras'; ``lr`` is accepted for ``learning_rate``; ``clipnorm``, ``clipvalue``,
``global_clipnorm`` and ``decay`` are the common keyword arguments.  The objects hold hyper-parameters and ``iterations`` only: the
update itself runs in ``dctr_opt_apply`` (training_hip.HipTrainer) or in ``training.KerasOptimizer`` (the autograd step), both of which
read ``_rule()`` below.  Nothing here imports torch or TensorFlow, and instances are NOT callable — a callable handed to ``compile``
is a ``torch.optim`` factory.  The update rules are written out in DESIGN.md §7.
"""
import math
import sys

from . import optimizer_schedules as schedules  # (optimizers.schedules.ExponentialDecay, ...)
from .optimizer_schedules import LearningRateSchedule

# `from deepctr_amd.optimizers.schedules import ExponentialDecay` works as tf.keras' spelling does, the way os.path does
sys.modules[__name__ + ".schedules"] = schedules

# dctr_opt_apply's kinds (include/dctr.h: DCTR_OPT_*)
KIND_ADAM, KIND_ADAGRAD, KIND_RMSPROP, KIND_SGD, KIND_ADAMAX, KIND_ADADELTA, KIND_FTRL = range(7)


class Optimizer(object):
    """What the seven classes share: the learning rate (a float, a schedule or any callable step -> float), Keras' legacy ``decay``,
    the three clipping arguments, ``iterations`` and the config protocol."""
    _hyper = ()                     # (name, default) in constructor order, after learning_rate

    def _init_common(self, learning_rate, name, kwargs):
        if "lr" in kwargs:
            learning_rate = kwargs.pop("lr")
        self.clipnorm = kwargs.pop("clipnorm", None)
        self.clipvalue = kwargs.pop("clipvalue", None)
        self.global_clipnorm = kwargs.pop("global_clipnorm", None)
        self.decay = float(kwargs.pop("decay", 0.0) or 0.0)
        if kwargs:
            raise TypeError("Unexpected keyword argument passed to optimizer: %s" % sorted(kwargs)[0])
        if self.clipnorm is not None and self.global_clipnorm is not None:
            raise ValueError("Cannot accept both `clipnorm` and `global_clipnorm`, got %r and %r" % (self.clipnorm, self.global_clipnorm))
        for k in ("clipnorm", "clipvalue", "global_clipnorm"):
            v = getattr(self, k)
            if v is not None:
                if float(v) <= 0:
                    raise ValueError("`%s` must be positive, got %r" % (k, v))
                setattr(self, k, float(v))
        if self.decay < 0:
            raise ValueError("decay cannot be less than 0: %r" % self.decay)
        if isinstance(learning_rate, dict):
            learning_rate = schedules.deserialize(learning_rate)
        if not (isinstance(learning_rate, LearningRateSchedule) or callable(learning_rate)):
            learning_rate = float(learning_rate)
        self.learning_rate = learning_rate
        self.name = name
        self.iterations = 0

    @property
    def lr(self):
        return self.learning_rate

    def current_lr(self, iterations=None):
        """The rate of the update that follows ``iterations`` applied ones (evaluated on the host, once per update)."""
        it = self.iterations if iterations is None else iterations
        lr = self.learning_rate
        lr = float(lr(it)) if callable(lr) else float(lr)
        if self.decay:
            lr = lr / (1.0 + self.decay * it)
        return lr

    def get_config(self):
        lr = self.learning_rate
        if isinstance(lr, LearningRateSchedule):
            lr = schedules.serialize(lr)
        elif callable(lr):
            raise ValueError("a plain callable learning rate has no config")
        cfg = {"name": self.name, "learning_rate": lr, "decay": self.decay}
        for k in ("clipnorm", "clipvalue", "global_clipnorm"):
            if getattr(self, k) is not None:
                cfg[k] = getattr(self, k)
        for k, _ in self._hyper:
            cfg[k] = getattr(self, k)
        return cfg

    @classmethod
    def from_config(cls, config):
        cfg = dict(config)
        if "lr" in cfg:
            cfg["learning_rate"] = cfg.pop("lr")
        return cls(**cfg)

    def __repr__(self):
        return "%s(%s)" % (type(self).__name__, ", ".join("%s=%r" % (k, getattr(self, k)) for k in ("learning_rate",) + tuple(
            k for k, _ in self._hyper)))

    # ---- what the two training steps read ----------------------------------------------------------------------------------
    def _rule(self):
        """dict(kind, slots=[initial value per state slot, in dctr_opt_seg_t order], + the launch scalars that do not change)."""
        raise NotImplementedError

    def _step_lr(self, t):
        """The ``lr`` scalar of update number ``t`` (1-based): the scheduled rate, with Adam's / Adamax' bias correction folded in
        as dctr_adam_multi's callers do."""
        return self.current_lr(t - 1)


class SGD(Optimizer):
    _hyper = (("momentum", 0.0), ("nesterov", False))

    def __init__(self, learning_rate=0.01, momentum=0.0, nesterov=False, name="SGD", **kwargs):
        self._init_common(learning_rate, name, kwargs)
        if not 0.0 <= float(momentum) <= 1.0:
            raise ValueError("`momentum` must be between [0, 1].")
        self.momentum, self.nesterov = float(momentum), bool(nesterov)

    def _rule(self):
        return dict(kind=KIND_SGD, slots=[0.0] if self.momentum else [], momentum=self.momentum, nesterov=self.nesterov)


class Adagrad(Optimizer):
    _hyper = (("initial_accumulator_value", 0.1), ("epsilon", 1e-7))

    def __init__(self, learning_rate=0.001, initial_accumulator_value=0.1, epsilon=1e-7, name="Adagrad", **kwargs):
        self._init_common(learning_rate, name, kwargs)
        if float(initial_accumulator_value) < 0.0:
            raise ValueError("initial_accumulator_value must be non-negative: %s" % initial_accumulator_value)
        self.initial_accumulator_value, self.epsilon = float(initial_accumulator_value), float(epsilon)

    def _rule(self):
        return dict(kind=KIND_ADAGRAD, slots=[self.initial_accumulator_value], eps=self.epsilon)


class RMSprop(Optimizer):
    _hyper = (("rho", 0.9), ("momentum", 0.0), ("epsilon", 1e-7), ("centered", False))

    def __init__(self, learning_rate=0.001, rho=0.9, momentum=0.0, epsilon=1e-7, centered=False, name="RMSprop", **kwargs):
        self._init_common(learning_rate, name, kwargs)
        if not 0.0 <= float(momentum) <= 1.0:
            raise ValueError("`momentum` must be between [0, 1].")
        self.rho, self.momentum, self.epsilon, self.centered = float(rho), float(momentum), float(epsilon), bool(centered)

    def _rule(self):
        # slots: ms, then mg when centered, then mom when momentum > 0
        return dict(kind=KIND_RMSPROP, slots=[0.0] * (1 + int(self.centered) + int(self.momentum > 0)), beta2=self.rho, eps=self.epsilon,
                    momentum=self.momentum, centered=self.centered)


class Adam(Optimizer):
    _hyper = (("beta_1", 0.9), ("beta_2", 0.999), ("epsilon", 1e-7), ("amsgrad", False))

    def __init__(self, learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7, amsgrad=False, name="Adam", **kwargs):
        self._init_common(learning_rate, name, kwargs)
        self.beta_1, self.beta_2, self.epsilon, self.amsgrad = float(beta_1), float(beta_2), float(epsilon), bool(amsgrad)

    def _rule(self):
        return dict(kind=KIND_ADAM, slots=[0.0] * (3 if self.amsgrad else 2), beta1=self.beta_1, beta2=self.beta_2, eps=self.epsilon,
                    amsgrad=self.amsgrad)

    def _step_lr(self, t):
        return self.current_lr(t - 1) * math.sqrt(1.0 - self.beta_2 ** t) / (1.0 - self.beta_1 ** t)


class Adamax(Optimizer):
    _hyper = (("beta_1", 0.9), ("beta_2", 0.999), ("epsilon", 1e-7))

    def __init__(self, learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7, name="Adamax", **kwargs):
        self._init_common(learning_rate, name, kwargs)
        self.beta_1, self.beta_2, self.epsilon = float(beta_1), float(beta_2), float(epsilon)

    def _rule(self):
        return dict(kind=KIND_ADAMAX, slots=[0.0, 0.0], beta1=self.beta_1, beta2=self.beta_2, eps=self.epsilon)

    def _step_lr(self, t):
        return self.current_lr(t - 1) / (1.0 - self.beta_1 ** t)


class Adadelta(Optimizer):
    _hyper = (("rho", 0.95), ("epsilon", 1e-7))

    def __init__(self, learning_rate=0.001, rho=0.95, epsilon=1e-7, name="Adadelta", **kwargs):
        self._init_common(learning_rate, name, kwargs)
        self.rho, self.epsilon = float(rho), float(epsilon)

    def _rule(self):
        return dict(kind=KIND_ADADELTA, slots=[0.0, 0.0], beta2=self.rho, eps=self.epsilon)


class Ftrl(Optimizer):
    _hyper = (("learning_rate_power", -0.5), ("initial_accumulator_value", 0.1), ("l1_regularization_strength", 0.0),
              ("l2_regularization_strength", 0.0), ("l2_shrinkage_regularization_strength", 0.0), ("beta", 0.0))

    def __init__(self, learning_rate=0.001, learning_rate_power=-0.5, initial_accumulator_value=0.1, l1_regularization_strength=0.0,
                 l2_regularization_strength=0.0, name="Ftrl", l2_shrinkage_regularization_strength=0.0, beta=0.0, **kwargs):
        self._init_common(learning_rate, name, kwargs)
        if float(initial_accumulator_value) < 0.0:
            raise ValueError("`initial_accumulator_value` needs to be positive or zero. Received: %s" % initial_accumulator_value)
        if float(learning_rate_power) > 0.0:
            raise ValueError("`learning_rate_power` needs to be negative or zero. Received: %s" % learning_rate_power)
        for k, v in (("l1_regularization_strength", l1_regularization_strength), ("l2_regularization_strength", l2_regularization_strength),
                     ("l2_shrinkage_regularization_strength", l2_shrinkage_regularization_strength)):
            if float(v) < 0.0:
                raise ValueError("`%s` needs to be positive or zero. Received: %s" % (k, v))
        self.learning_rate_power, self.initial_accumulator_value = float(learning_rate_power), float(initial_accumulator_value)
        self.l1_regularization_strength, self.l2_regularization_strength = float(l1_regularization_strength), float(l2_regularization_strength)
        self.l2_shrinkage_regularization_strength, self.beta = float(l2_shrinkage_regularization_strength), float(beta)

    def _rule(self):
        # slots: n (the accumulator), z (the linear term)
        return dict(kind=KIND_FTRL, slots=[self.initial_accumulator_value, 0.0], lr_power=self.learning_rate_power,
                    l1=self.l1_regularization_strength, l2_ftrl=self.l2_regularization_strength,
                    l2_shrinkage=self.l2_shrinkage_regularization_strength, beta=self.beta)


_CLASSES = {c.__name__.lower(): c for c in (SGD, Adagrad, RMSprop, Adam, Adamax, Adadelta, Ftrl)}


# keys of a foreign config (newer Keras) that do not change the rule, and keys that do not while they hold one of these values
_CONFIG_IGNORED = {"jit_compile", "is_legacy_optimizer", "ema_momentum", "ema_overwrite_frequency"}
_CONFIG_NEUTRAL = {"weight_decay": (None, 0, 0.0), "use_ema": (None, False), "loss_scale_factor": (None,),
                   "gradient_accumulation_steps": (None,)}


def _from_class_config(class_name, config):
    cls = _CLASSES.get(str(class_name).lower())
    if cls is None:
        raise ValueError("Unknown optimizer: %r (SGD, Adagrad, RMSprop, Adam, Adamax, Adadelta, Ftrl)" % (class_name,))
    import inspect
    known = set(inspect.signature(cls.__init__).parameters) | {"lr", "clipnorm", "clipvalue", "global_clipnorm", "decay"}
    kept = {}
    for k, v in dict(config).items():
        if k in known:
            kept[k] = v
        elif k in _CONFIG_NEUTRAL and v in _CONFIG_NEUTRAL[k] or k in _CONFIG_IGNORED:
            continue
        else:       # a setting this build does not have: training on without it would be another rule
            raise ValueError("%s config: %s=%r is not supported" % (cls.__name__, k, v))
    return cls.from_config(kept)


def get(identifier):
    """An optimizer object from a name (either case), one of this module's objects, a Keras-style config dict
    {"class_name": ..., "config": {...}}, or any foreign object whose ``get_config()`` carries ``name`` and Keras' keys (a tf.keras
    optimizer instance: read through its config, TensorFlow is not imported).  ValueError for anything else."""
    if isinstance(identifier, Optimizer):
        return identifier
    if isinstance(identifier, str):
        cls = _CLASSES.get(identifier.lower())
        if cls is None:
            raise ValueError("Unknown optimizer: %r (SGD, Adagrad, RMSprop, Adam, Adamax, Adadelta, Ftrl)" % (identifier,))
        return cls()
    if isinstance(identifier, dict):
        if "class_name" not in identifier or "config" not in identifier:
            raise ValueError("an optimizer config dict needs `class_name` and `config`: %r" % (identifier,))
        return _from_class_config(identifier["class_name"], identifier["config"])
    cfg_of = getattr(identifier, "get_config", None)
    if cfg_of is not None and not isinstance(identifier, type):
        cfg = cfg_of()
        if isinstance(cfg, dict) and "name" in cfg:
            # (`name` is the class name unless the user renamed the instance: then the foreign class's own name decides)
            return _from_class_config(cfg["name"] if str(cfg["name"]).lower() in _CLASSES else type(identifier).__name__, cfg)
    raise ValueError("Could not interpret optimizer identifier: %r" % (identifier,))
