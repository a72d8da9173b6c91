"""NumPy oracle of the multi-task training step's kernels (dctr_mtl_mix_bwd, dctr_mtl_loss_grad; DESIGN.md §4.15 "Training"), float64 by
default, ``dtype=`` selectable.

``mix_bwd`` is the backward of the gated mixture O_g = sum_j softmax(z_g Wg_g)[j] h_{m_j}: from the forward's operands and d_out it
returns dh and ds (what the kernel writes), the gate logits, and dz / dWg (what the one-layer linear ops.mlp_bwd behind the kernel
makes of ds).  ``absolute=True`` is the magnitude mode for tests.util.assert_close_terms: the same sums over |d_out| and |h| with the
TRUE gate weights (they lie in (0, 1) and sum to one), an upper bound of the magnitude every sum was taken at.

``loss_grad`` restates models/multitask/_fit.py:task_losses and its derivative in closed form.

The bar of the op test: assert_close_terms with rtol = 1e-4 and rtol_terms = OP_RTOL_TERMS, measured on the CPU
(tests/test_mtl_train_cpu.py::test_float32_oracle_against_float64_sets_the_bar over the sweep of tests/test_gpu_mtl_train.py): the float32
NumPy run of ``mix_bwd`` sits at most 6.66e-7 of the summed magnitude off the float64 run (a lone p_j d_out term of dh whose gate
weight exp(l_j - max) / sum carries the rounding of a logit difference of 6).  Twice that, since the kernel sums a wave's partial products
in another order than NumPy, is 1.33e-6; rounded up: 1.4e-6.  Below assert_close_terms' default 2e-6."""
import numpy as np

OP_RTOL_TERMS = 1.4e-6
LO, HI = 1e-7, 1.0 - 1e-7
HI32 = float(np.float32(1.0 - 1e-7))        # the upper clip bound as a float32 computation holds it: 1 - 2^-23


def _softmax(v):
    e = np.exp(v - v.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def mix_bwd(h, width, z, gate_kernels, members, d_out, dtype=np.float64, absolute=False):
    """h [B, E * width]; z[g] [B, dz]; gate_kernels[g] [dz, n_g]; members[g]; d_out [B, G * width].  Returns a dict: dh [B, E * width],
    ds [B, sum n_g], logits [B, sum n_g], dz [g] -> [B, dz], dWg [g] -> [dz, n_g]."""
    dt = np.dtype(dtype).type
    ab = np.abs if absolute else (lambda v: v)
    H = int(width)
    h, d_out = np.asarray(h).astype(dt), np.asarray(d_out).astype(dt)
    dh = np.zeros_like(h)
    ds, logits, dzs, dws = [], [], [], []
    for g, ms in enumerate(members):
        zg, W = np.asarray(z[g]).astype(dt), np.asarray(gate_kernels[g]).astype(dt)
        l = zg @ W
        p = _softmax(l)
        dg = ab(d_out[:, g * H:(g + 1) * H])
        a = np.stack([(dg * ab(h[:, m * H:(m + 1) * H])).sum(-1) for m in ms], axis=1)
        mean = (p * a).sum(-1, keepdims=True)
        s = p * (a + mean) if absolute else p * (a - mean)
        for j, m in enumerate(ms):
            dh[:, m * H:(m + 1) * H] += p[:, j:j + 1] * dg
        ds.append(s)
        logits.append(l)
        dzs.append(ab(s) @ ab(W).T)
        dws.append(ab(zg).T @ ab(s))
    return dict(dh=dh, ds=np.concatenate(ds, axis=1), logits=np.concatenate(logits, axis=1), dz=dzs, dWg=dws)


def loss_grad(pred, y, losses, binary, loss_weights=None, esmm=False, dtype=np.float64, hi=HI):
    """pred [T, B]: sigmoid(logit_t) where binary[t] else logit_t (esmm: row 1 = sigmoid(l_cvr)); y [T, B].  Returns (dlogit [T, B] =
    d(sum_t w_t mean_b loss_t) / d logit_t, loss_sum [T] = sum_b of the reported loss, dbias [T] = sum_b dlogit).  ``hi``: the upper
    clip bound (HI32 for a float32 computation)."""
    dt = np.dtype(dtype).type
    pred, y = np.asarray(pred).astype(dt), np.asarray(y).astype(dt)
    T, B = pred.shape
    w = np.ones(T, dtype=dt) if loss_weights is None else np.asarray(loss_weights).astype(dt)
    lo, hi = dt(LO), dt(hi)
    clipped = lambda pc, yy: -(yy * np.log(pc) + (1 - yy) * np.log(1 - pc))       # noqa: E731
    dl, loss = np.zeros((T, B), dtype=dt), np.zeros(T, dtype=dt)
    for t in range(T):
        if losses[t] in ("mse", "mean_squared_error"):
            assert not binary[t]
            dl[t] = 2 * w[t] * (pred[t] - y[t]) / B
            loss[t] = ((pred[t] - y[t]) ** 2).sum()
        else:
            assert binary[t]
            dl[t] = w[t] * (pred[t] - y[t]) / B
            loss[t] = clipped(np.clip(pred[t], lo, hi), y[t]).sum()
    if esmm:
        assert T == 2 and all(binary)
        p0, c = pred[0], pred[1]
        p1 = p0 * c
        pc = np.clip(p1, lo, hi)
        inside = (p1 >= lo) & (p1 <= hi)
        g = np.where(inside, w[1] * (-y[1] / pc + (1 - y[1]) / (1 - pc)) / B, 0)
        dl[0] = w[0] * (p0 - y[0]) / B + g * p1 * (1 - p0)
        dl[1] = g * p1 * (1 - c)
        loss[1] = clipped(pc, y[1]).sum()
    return dl, loss, dl.sum(-1)
