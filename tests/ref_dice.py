"""Dice.call restated in torch for the checkers of dctr_mlp_bwd's Dice branch (tests/test_gpu_din_train.py, tests/test_gpu_mlp_bwd.py):
autograd over these formulas is the reference, in whatever dtype and on whatever device the leaves live; and the bar both files
compare at."""
import torch

from tests.util import assert_close


def scaled_close(got, ref, what, rtol=2e-4, atol=2e-6):
    """assert_close on tensors divided by the reference's largest magnitude."""
    scale = max(float(ref.abs().max()), 1e-4)
    assert_close(got.cpu().numpy() / scale, ref.cpu().numpy() / scale, rtol=rtol, atol=atol, what=what)


def dice_dnn(h, kernels, biases, alphas, means=None, variances=None, eps=1e-9):
    """DNN with Dice activations: z = h W + b;  p = sigmoid((z - mean) / sqrt(var + eps));  h = alpha (1 - p) z + p z.
    ``means`` / ``variances`` None: this batch's statistics (biased variance), differentiated through, as BatchNormalization does under
    training=True.  Returns (h_last, [(mean, var) per layer], detached)."""
    stats = []
    for i in range(len(kernels)):
        z = h @ kernels[i] + biases[i]
        if means is None:
            m, v = z.mean(dim=0), z.var(dim=0, unbiased=False)
        else:
            m, v = means[i], variances[i]
        stats.append((m.detach(), v.detach()))
        p = torch.sigmoid((z - m) / torch.sqrt(v + eps))
        h = alphas[i] * (1 - p) * z + p * z
    return h, stats
