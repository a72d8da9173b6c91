"""GPU: training.field_conv_selected in float32 on the device against the float64 oracle of tests/ref_fieldconv_bwd.py.  Its selection
equals the oracle's on every line whose deciding gap exceeds RB.GAP (a forward within its bar cannot order those differently); its
gradients are the oracle's on the tape it made itself, within assert_close_terms(rtol=1e-4, rtol_terms=RB.BWD_RTOL_TERMS); exact
ties go to the lower row on the device as on the CPU."""
import numpy as np
import pytest
import torch

from tests import ref_fieldconv_bwd as RB
from tests.util import assert_close_terms

pytestmark = pytest.mark.gpu

NAMES = [RB.CASES[i].name for i in (2, 3, 9, 13, 22, 28, 33, 38, 39, 40)]


@pytest.mark.parametrize("name", NAMES)
def test_selection_and_gradients_against_the_oracle(device, name):
    from deepctr_amd import training
    case = RB.CASE_BY_NAME[name]
    x, kernels, biases, d_out, dso = RB.case_inputs(case)
    dev = lambda a: torch.tensor(np.asarray(a), device=device)       # noqa: E731
    xt = dev(x).requires_grad_(True)
    ks, bs = [dev(k).requires_grad_(True) for k in kernels], [dev(b).requires_grad_(True) for b in biases]
    last, maps, sels = training.field_conv_selected(xt, ks, bs, list(case.pools))
    gaps = RB.min_selection_gap(x, kernels, biases, case.pools)
    for s, (sel, (_, sel64), gap) in enumerate(zip(sels, RB.case_tape(case), gaps)):
        clear = gap > RB.GAP
        assert 1.0 - clear.mean() <= RB.GAP_SHARE_MAX
        same = (sel.cpu().numpy() == sel64).all(axis=1)
        assert same[clear].all(), "%s stage %d: %d clear lines select differently" % (name, s, int((~same[clear]).sum()))
    loss = 0.0
    if d_out is not None:
        loss = loss + (last * dev(d_out)).sum()
    for m, d in zip(maps, dso or []):
        if d is not None:
            loss = loss + (m * dev(d)).sum()
    loss.backward()
    tape = [(m.detach().cpu().numpy(), sel.cpu().numpy()) for m, sel in zip(maps, sels)]
    G = RB.field_conv_bwd(x, kernels, tape, d_out, dso)
    T = RB.field_conv_bwd(x, kernels, tape, d_out, dso, absolute=True)
    got = {"dx": xt.grad.cpu().numpy(), "d_kernels": [k.grad.cpu().numpy() for k in ks], "d_biases": [b.grad.cpu().numpy() for b in bs]}
    for (k, g), (_, r), (_, t) in zip(RB.outputs(got), RB.outputs(G), RB.outputs(T)):
        assert_close_terms(g, r, t, rtol=1e-4, rtol_terms=RB.BWD_RTOL_TERMS, what="%s %s" % (name, k))


def test_exact_ties_go_to_the_lower_row_on_the_device(device):
    from deepctr_amd import training
    rng = np.random.RandomState(5)
    x = rng.standard_normal((33, 6, 5)).astype(np.float32)
    x[:, 2] = x[:, 1]
    x[:, 5] = x[:, 4]
    kern, bias = [(np.abs(rng.standard_normal((1, 1, 3))) + 0.1).astype(np.float32)], [np.zeros(3, np.float32)]
    for pools in ([("max", 3)], [("kmax", 6)], [("kmax", 2)]):
        sel = training.field_conv_selected(torch.tensor(x, device=device), [torch.tensor(kern[0], device=device)],
                                           [torch.tensor(bias[0], device=device)], pools)[2][0].cpu().numpy()
        want = RB.forward_tape(x, kern, bias, pools, np.float32)[0][1]
        assert np.array_equal(sel, want), pools
