"""float64 NumPy restatement of the optimizer rules of DESIGN.md §7 (tf.keras' optimizer_v2 as the issue states them), of the three
clipping arguments and of the learning-rate schedules.  Written from the formulas, independently of training.KerasOptimizer and of
csrc/opt_kernels.hip; every test of the optimizer objects measures against this."""
import math

import numpy as np


# ---- schedules -------------------------------------------------------------------------------------------------------------------
def exponential_decay(lr0, decay_steps, decay_rate, step, staircase=False):
    e = step / decay_steps
    return lr0 * decay_rate ** (math.floor(e) if staircase else e)


def inverse_time_decay(lr0, decay_steps, decay_rate, step, staircase=False):
    e = step / decay_steps
    return lr0 / (1.0 + decay_rate * (math.floor(e) if staircase else e))


def piecewise_constant(boundaries, values, step):
    i = 0
    while i < len(boundaries) and step > boundaries[i]:
        i += 1
    return values[i]


# ---- clipping --------------------------------------------------------------------------------------------------------------------
def clip_scales(grads, clipnorm=None, global_clipnorm=None):
    """One factor per gradient: clip / max(norm, clip), the norm per gradient or over all of them."""
    sq = [float(np.sum(np.asarray(g, dtype=np.float64) ** 2)) for g in grads]
    if clipnorm is not None:
        return [clipnorm / max(math.sqrt(s), clipnorm) for s in sq]
    if global_clipnorm is not None:
        return [global_clipnorm / max(math.sqrt(sum(sq)), global_clipnorm)] * len(grads)
    return [1.0] * len(grads)


# ---- the rules -------------------------------------------------------------------------------------------------------------------
class Oracle(object):
    """rule: "sgd" | "adagrad" | "rmsprop" | "adam" | "adamax" | "adadelta" | "ftrl"; hp: tf.keras' argument names.  ``lr`` of
    update(): the scheduled rate of that update.  State per parameter index; weights are updated in place (float64 arrays)."""
    DEFAULTS = {
        "sgd": dict(momentum=0.0, nesterov=False),
        "adagrad": dict(initial_accumulator_value=0.1, epsilon=1e-7),
        "rmsprop": dict(rho=0.9, momentum=0.0, epsilon=1e-7, centered=False),
        "adam": dict(beta_1=0.9, beta_2=0.999, epsilon=1e-7, amsgrad=False),
        "adamax": dict(beta_1=0.9, beta_2=0.999, epsilon=1e-7),
        "adadelta": dict(rho=0.95, epsilon=1e-7),
        "ftrl": dict(learning_rate_power=-0.5, initial_accumulator_value=0.1, l1_regularization_strength=0.0,
                     l2_regularization_strength=0.0, l2_shrinkage_regularization_strength=0.0, beta=0.0),
    }

    def __init__(self, rule, clipnorm=None, clipvalue=None, global_clipnorm=None, **hp):
        self.rule = rule
        self.hp = dict(self.DEFAULTS[rule], **hp)
        self.clipnorm, self.clipvalue, self.global_clipnorm = clipnorm, clipvalue, global_clipnorm
        self.t = 0
        self.state = {}

    def update(self, ws, g_raw, l2s, lr):
        """ws: list of float64 arrays (updated in place); g_raw: data gradients; l2s: one l2 per parameter."""
        self.t += 1
        t, hp = self.t, self.hp
        gs = [np.asarray(g, dtype=np.float64) + 2.0 * l2 * w for w, g, l2 in zip(ws, g_raw, l2s)]
        gs = [g * s for g, s in zip(gs, clip_scales(gs, self.clipnorm, self.global_clipnorm))]
        if self.clipvalue is not None:
            gs = [np.clip(g, -self.clipvalue, self.clipvalue) for g in gs]
        for i, (w, g) in enumerate(zip(ws, gs)):
            st = self.state.setdefault(i, {})
            z = lambda k, v=0.0: st.setdefault(k, np.full_like(w, v))       # noqa: E731
            if self.rule == "sgd":
                mu = hp["momentum"]
                if mu == 0:
                    w -= lr * g
                else:
                    a = z("a")
                    a[...] = mu * a - lr * g
                    w += (mu * a - lr * g) if hp["nesterov"] else a
            elif self.rule == "adagrad":
                v = z("v", hp["initial_accumulator_value"])
                v += g * g
                w -= lr * g / (np.sqrt(v) + hp["epsilon"])
            elif self.rule == "rmsprop":
                rho, mu, eps = hp["rho"], hp["momentum"], hp["epsilon"]
                ms = z("ms")
                ms[...] = rho * ms + (1 - rho) * g * g
                den = ms
                if hp["centered"]:
                    mg = z("mg")
                    mg[...] = rho * mg + (1 - rho) * g
                    den = ms - mg * mg
                if mu > 0:
                    mom = z("mom")
                    mom[...] = mu * mom + lr * g / np.sqrt(den + eps)
                    w -= mom
                else:
                    w -= lr * g / (np.sqrt(den) + eps)
            elif self.rule == "adam":
                b1, b2, eps = hp["beta_1"], hp["beta_2"], hp["epsilon"]
                m, v = z("m"), z("v")
                m[...] = b1 * m + (1 - b1) * g
                v[...] = b2 * v + (1 - b2) * g * g
                lr_t = lr * math.sqrt(1 - b2 ** t) / (1 - b1 ** t)
                if hp["amsgrad"]:
                    vh = z("vhat")
                    vh[...] = np.maximum(vh, v)
                    w -= lr_t * m / (np.sqrt(vh) + eps)
                else:
                    w -= lr_t * m / (np.sqrt(v) + eps)
            elif self.rule == "adamax":
                b1, b2, eps = hp["beta_1"], hp["beta_2"], hp["epsilon"]
                m, u = z("m"), z("u")
                m[...] = b1 * m + (1 - b1) * g
                u[...] = np.maximum(b2 * u, np.abs(g))
                w -= lr / (1 - b1 ** t) * m / (u + eps)
            elif self.rule == "adadelta":
                rho, eps = hp["rho"], hp["epsilon"]
                a, s = z("a"), z("s")
                a[...] = rho * a + (1 - rho) * g * g
                d = np.sqrt(s + eps) / np.sqrt(a + eps) * g
                s[...] = rho * s + (1 - rho) * d * d
                w -= lr * d
            elif self.rule == "ftrl":
                p = -hp["learning_rate_power"]
                l1, l2, l2s, beta = (hp["l1_regularization_strength"], hp["l2_regularization_strength"],
                                     hp["l2_shrinkage_regularization_strength"], hp["beta"])
                n, zz = z("n", hp["initial_accumulator_value"]), z("z")
                gsh = g + 2 * l2s * w
                n1 = n + g * g
                pw = (lambda x: np.sqrt(x)) if p == 0.5 else (lambda x: x ** p)
                zz += gsh - (pw(n1) - pw(n)) / lr * w
                q = pw(n1) / lr + 2 * (l2 + beta / (2 * lr))
                w[...] = np.where(np.abs(zz) > l1, (np.sign(zz) * l1 - zz) / q, 0.0)
                n[...] = n1
            else:
                raise ValueError(self.rule)


# ---- the cases both test files run: (id, deepctr_amd.optimizers class name, constructor kwargs, oracle rule, oracle kwargs) ----------
CASES = [
    ("sgd", "SGD", dict(learning_rate=0.05), "sgd", {}),
    ("sgd_momentum", "SGD", dict(learning_rate=0.05, momentum=0.9), "sgd", dict(momentum=0.9)),
    ("sgd_nesterov", "SGD", dict(learning_rate=0.05, momentum=0.9, nesterov=True), "sgd", dict(momentum=0.9, nesterov=True)),
    ("adagrad", "Adagrad", dict(learning_rate=0.1), "adagrad", {}),
    ("rmsprop", "RMSprop", dict(learning_rate=0.01), "rmsprop", {}),
    ("rmsprop_centered", "RMSprop", dict(learning_rate=0.01, centered=True), "rmsprop", dict(centered=True)),
    ("rmsprop_momentum", "RMSprop", dict(learning_rate=0.01, momentum=0.5), "rmsprop", dict(momentum=0.5)),
    ("rmsprop_momentum_centered", "RMSprop", dict(learning_rate=0.01, momentum=0.5, centered=True), "rmsprop",
     dict(momentum=0.5, centered=True)),
    ("adam", "Adam", dict(learning_rate=0.01), "adam", {}),
    ("adam_amsgrad", "Adam", dict(learning_rate=0.01, amsgrad=True), "adam", dict(amsgrad=True)),
    ("adamax", "Adamax", dict(learning_rate=0.01), "adamax", {}),
    ("adadelta", "Adadelta", dict(learning_rate=0.5), "adadelta", {}),
    ("ftrl_l1", "Ftrl", dict(learning_rate=0.05, l1_regularization_strength=0.05), "ftrl", dict(l1_regularization_strength=0.05)),
    ("ftrl_shrinkage", "Ftrl", dict(learning_rate=0.05, l1_regularization_strength=0.01, l2_regularization_strength=0.02,
                                    l2_shrinkage_regularization_strength=0.1), "ftrl",
     dict(l1_regularization_strength=0.01, l2_regularization_strength=0.02, l2_shrinkage_regularization_strength=0.1)),
    ("ftrl_beta", "Ftrl", dict(learning_rate=0.05, beta=0.3), "ftrl", dict(beta=0.3)),
    ("ftrl_power", "Ftrl", dict(learning_rate=0.05, learning_rate_power=-0.3, l1_regularization_strength=0.01), "ftrl",
     dict(learning_rate_power=-0.3, l1_regularization_strength=0.01)),
    ("adam_clipvalue", "Adam", dict(learning_rate=0.01, clipvalue=0.05), "adam", dict(clipvalue=0.05)),
    ("sgd_clipnorm", "SGD", dict(learning_rate=0.05, momentum=0.9, clipnorm=0.5), "sgd", dict(momentum=0.9, clipnorm=0.5)),
    ("adagrad_global_clipnorm", "Adagrad", dict(learning_rate=0.1, global_clipnorm=1.0), "adagrad", dict(global_clipnorm=1.0)),
]
CASE_IDS = [c[0] for c in CASES]


def ftrl_draw(rng, shapes, l2s, steps, lr, oracle_kw, margin=1e-6, tries=50, transform=None):
    """Weights and per-step gradients for an Ftrl case on which no element's |z| comes within ``margin`` of l1 at any step (a float32
    evaluation could land on the other side of the threshold there): such draws are taken again, here on the CPU.  z == 0 exactly — an
    element no gradient has reached yet — is 0 in float32 too and does not count.  ``transform``: applied to the drawn gradients
    (a list per step) before they are judged, e.g. the zeroing of a table's untouched groups."""
    l1 = oracle_kw.get("l1_regularization_strength", 0.0)
    for _ in range(tries):
        ws = [rng.uniform(-0.5, 0.5, s).astype(np.float32) for s in shapes]
        gs = [[rng.normal(0, 0.1, s).astype(np.float32) for s in shapes] for _ in range(steps)]
        if transform is not None:
            gs = transform(gs)
        o = Oracle("ftrl", **oracle_kw)
        w64 = [w.astype(np.float64) for w in ws]
        ok = True
        for g in gs:
            o.update(w64, g, l2s, lr)
            if any(np.any((np.abs(np.abs(o.state[i]["z"]) - l1) < margin) & (o.state[i]["z"] != 0)) for i in range(len(ws))):
                ok = False
                break
        if ok:
            return ws, gs
    raise RuntimeError("no draw clear of the l1 threshold in %d tries" % tries)
