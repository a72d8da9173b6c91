"""tf.keras.optimizers.schedules restated as plain Python (reached as ``deepctr_amd.optimizers.schedules``): callables step -> float,
evaluated on the host once per update — the learning rate is a launch scalar of the optimizer kernel."""
import math


class LearningRateSchedule(object):
    def __call__(self, step):
        raise NotImplementedError

    def get_config(self):
        raise NotImplementedError

    @classmethod
    def from_config(cls, config):
        return cls(**config)


class ExponentialDecay(LearningRateSchedule):
    """initial_learning_rate * decay_rate ^ (step / decay_steps); ``staircase``: the exponent is floored."""

    def __init__(self, initial_learning_rate, decay_steps, decay_rate, staircase=False, name=None):
        self.initial_learning_rate, self.decay_steps, self.decay_rate = float(initial_learning_rate), decay_steps, float(decay_rate)
        self.staircase, self.name = bool(staircase), name

    def __call__(self, step):
        p = float(step) / float(self.decay_steps)
        if self.staircase:
            p = math.floor(p)
        return self.initial_learning_rate * self.decay_rate ** p

    def get_config(self):
        return {"initial_learning_rate": self.initial_learning_rate, "decay_steps": self.decay_steps, "decay_rate": self.decay_rate,
                "staircase": self.staircase, "name": self.name}


class InverseTimeDecay(LearningRateSchedule):
    """initial_learning_rate / (1 + decay_rate * step / decay_steps); ``staircase``: the quotient is floored."""

    def __init__(self, initial_learning_rate, decay_steps, decay_rate, staircase=False, name=None):
        self.initial_learning_rate, self.decay_steps, self.decay_rate = float(initial_learning_rate), decay_steps, float(decay_rate)
        self.staircase, self.name = bool(staircase), name

    def __call__(self, step):
        p = float(step) / float(self.decay_steps)
        if self.staircase:
            p = math.floor(p)
        return self.initial_learning_rate / (1.0 + self.decay_rate * p)

    def get_config(self):
        return {"initial_learning_rate": self.initial_learning_rate, "decay_steps": self.decay_steps, "decay_rate": self.decay_rate,
                "staircase": self.staircase, "name": self.name}


class PiecewiseConstantDecay(LearningRateSchedule):
    """values[0] while step <= boundaries[0], values[i] while boundaries[i-1] < step <= boundaries[i], values[-1] beyond."""

    def __init__(self, boundaries, values, name=None):
        if len(boundaries) != len(values) - 1:
            raise ValueError("The length of boundaries should be 1 less than the length of values")
        self.boundaries, self.values, self.name = list(boundaries), [float(v) for v in values], name

    def __call__(self, step):
        for b, v in zip(self.boundaries, self.values):
            if step <= b:
                return v
        return self.values[-1]

    def get_config(self):
        return {"boundaries": self.boundaries, "values": self.values, "name": self.name}


_CLASSES = {c.__name__: c for c in (ExponentialDecay, InverseTimeDecay, PiecewiseConstantDecay)}


def serialize(schedule):
    return {"class_name": type(schedule).__name__, "config": schedule.get_config()}


def deserialize(config):
    cls = _CLASSES.get(config.get("class_name"))
    if cls is None:
        raise ValueError("Unknown learning rate schedule: %r" % (config,))
    return cls.from_config(config["config"])
