"""CPU: the float64 oracle of the field-conv stack's backward (tests/ref_fieldconv_bwd.py) against torch double autograd through a torch
restatement whose pooling is ``gather`` with the tape's selection, and against training._field_conv where no line sits at a near-tie;
the room the bar leaves a float32 implementation; the near-tie condition of the case table; and training.field_conv_selected, the
stack with its pooling as an explicit selection, against the oracle: its selection, its gradients, a given tape, exact ties."""
import numpy as np
import pytest
import torch

from tests import ref_fieldconv as RF
from tests import ref_fieldconv_bwd as RB

IDS = [c.name for c in RB.CASES]


def test_case_table_covers_what_was_agreed():
    cs = RB.CASES
    assert 38 <= len(cs) <= 48
    assert {c.F for c in cs} == {1, 2, 5, 7, 13} and {c.E for c in cs} == {1, 4, 5, 17} and {c.B for c in cs} == {1, 17, 33}
    assert {(1, 3), (1, 16, 17), (4, 20, 1)} <= {c.chans for c in cs}
    assert {len(c.widths) for c in cs} >= {1, 2, 4}
    widths = {(w if w in (1, 2, 6, 7) else "F+3") for c in cs for w in c.widths if w in (1, 2, 6, 7) or w == c.F + 3}
    assert widths == {1, 2, 6, 7, "F+3"}
    ks, ps, ragged, full, mixed = set(), set(), False, False, False
    for c in cs:
        rows = c.F
        for kind, arg in c.pools:
            if kind == "kmax":
                ks.add(arg)
                full |= arg == rows and rows > 3
                rows = arg
            else:
                ps.add(arg)
                ragged |= rows % arg != 0
                rows //= arg
        mixed |= len({k for k, _ in c.pools}) == 2
    assert {1, 3} <= ks and full and ps == {1, 2, 3} and ragged and mixed
    assert any(c.dso for c in cs) and any(not c.dso for c in cs) and any(not c.d_out for c in cs)
    assert any(c.max_blocks and -(-c.B * c.E // 16) > c.max_blocks for c in cs)       # a workgroup walks several tiles
    assert any(c.E == 17 and c.B > 1 for c in cs)                                       # a tile straddles samples


def _torch_grads(case, tape, dtype):
    x, kernels, biases, d_out, dso = RB.case_inputs(case)
    xt = torch.tensor(x, dtype=dtype, requires_grad=True)
    ks = [torch.tensor(k, dtype=dtype, requires_grad=True) for k in kernels]
    bs = [torch.tensor(b, dtype=dtype, requires_grad=True) for b in biases]
    maps = RB.torch_stack(xt, ks, bs, [torch.tensor(sel) for _, sel in tape])
    seeds = [None] * len(maps)
    if d_out is not None:
        seeds[-1] = torch.tensor(d_out, dtype=dtype)
    for s, d in enumerate(dso or []):
        if d is not None:
            seeds[s] = torch.tensor(d, dtype=dtype) if seeds[s] is None else seeds[s] + torch.tensor(d, dtype=dtype)
    loss = sum((m * d).sum() for m, d in zip(maps, seeds) if d is not None)
    loss.backward()
    zero = lambda t: (torch.zeros_like(t) if t.grad is None else t.grad).numpy()      # noqa: E731
    return maps, {"dx": zero(xt), "d_kernels": [zero(k) for k in ks], "d_biases": [zero(b) for b in bs]}


@pytest.mark.parametrize("name", IDS)
def test_oracle_matches_torch_double_autograd(name):
    case = RB.CASE_BY_NAME[name]
    x, kernels, biases, d_out, dso = RB.case_inputs(case)
    tape = RB.case_tape(case)
    maps, ref = _torch_grads(case, tape, torch.float64)
    for (P, sel), m, rows, c in zip(tape, maps, RB.stage_rows(case), case.chans[1:]):
        assert P.shape == sel.shape == (case.B, rows, case.E, c) and sel.dtype == np.int32
        assert np.abs(m.detach().numpy() - P).max() <= 1e-14
    last, every = RF.field_conv(x, kernels, biases, case.pools, np.float64)       # the forward oracle's values are the tape's
    assert all(np.array_equal(a, P) for a, (P, _) in zip(every, tape))
    G = RB.field_conv_bwd(x, kernels, tape, d_out, dso)
    for (k, g), (_, r) in zip(RB.outputs(G), RB.outputs(ref)):
        assert g.shape == r.shape, k
        assert np.abs(g - r).max() <= 1e-12 * max(1.0, float(np.abs(r).max())), (name, k, float(np.abs(g - r).max()))


def test_selection_rules():
    y = np.array([0.5, 0.9, 0.5, 0.9, -1.0, 0.1, 0.1]).reshape(1, 7, 1, 1)
    assert RB.select(y, "kmax", 4)[0, :, 0, 0].tolist() == [1, 3, 0, 2]               # ties to the lower row
    assert RB.select(y, "max", 2)[0, :, 0, 0].tolist() == [1, 3, 5]                    # rows % p dropped
    assert RB.select(y, "max", 3)[0, :, 0, 0].tolist() == [1, 3]                       # the lowest row that holds the maximum
    assert RB.select(y[:, 5:], "max", 2)[0, :, 0, 0].tolist() == [0]


def test_float32_backward_against_float64_sets_the_bar():
    """The float32 NumPy run of the oracle against its float64 run, the float64 tape handed to both: twice the worst ratio to the summed
    magnitude, rounded up to one digit, is the op's rtol_terms — unless that is at or below assert_close_terms' default, which is kept."""
    worst = 0.0
    for case in RB.CASES:
        x, kernels, biases, d_out, dso = RB.case_inputs(case)
        tape = RB.case_tape(case)
        G = RB.field_conv_bwd(x, kernels, tape, d_out, dso)
        T = RB.field_conv_bwd(x, kernels, tape, d_out, dso, absolute=True)
        tape32 = [(P.astype(np.float32), sel) for P, sel in tape]
        G32 = RB.field_conv_bwd(x, kernels, tape32, d_out, dso, dtype=np.float32)
        for (k, g), (_, t), (_, g32) in zip(RB.outputs(G), RB.outputs(T), RB.outputs(G32)):
            assert g32.dtype == np.float32 and (t >= np.abs(g) - 1e-12).all(), (case.name, k)
            ratio = float((np.abs(g32.astype(np.float64) - g) / np.maximum(t, 1e-30)).max())
            worst = max(worst, ratio)
    print("[fieldconv_bwd] float32 oracle vs float64: worst err / summed magnitude %.3g" % worst)
    derived = 2.0 * worst
    assert derived <= RB.BWD_RTOL_TERMS, "the bar %.3g leaves a float32 implementation less than twice its own error %.3g" % (
        RB.BWD_RTOL_TERMS, worst)
    # the recorded bar is the default because the derivation came out below it, not a looser one
    assert RB.BWD_RTOL_TERMS == 2e-6 and derived <= 2e-6


@pytest.mark.parametrize("name", IDS)
def test_at_most_a_quarter_of_the_lines_sit_at_a_near_tie(name):
    case = RB.CASE_BY_NAME[name]
    x, kernels, biases, _, _ = RB.case_inputs(case)
    assert RB.GAP == pytest.approx(2.04e-4)
    for s, g in enumerate(RB.min_selection_gap(x, kernels, biases, case.pools)):
        assert g.shape == (case.B, case.E, case.chans[s + 1])
        share = float((g <= RB.GAP).mean())
        assert share <= RB.GAP_SHARE_MAX, "%s stage %d: %.3g of the lines under GAP" % (name, s, share)


def test_min_selection_gap_on_a_known_map():
    x = np.array([0.1, 0.4, 0.35, -0.2, 0.0]).reshape(1, 5, 1)
    k, b = [np.ones((1, 1, 1))], [np.zeros(1)]
    t = np.tanh(x.reshape(-1))
    g = RB.min_selection_gap(x, k, b, [("kmax", 2)])[0]
    assert g.shape == (1, 1, 1) and g[0, 0, 0] == pytest.approx(min(t[1] - t[2], t[2] - t[0]))
    g = RB.min_selection_gap(x, k, b, [("kmax", 5)])[0]
    assert g[0, 0, 0] == pytest.approx(min(t[1] - t[2], t[2] - t[0], t[0] - t[4], t[4] - t[3]))
    g = RB.min_selection_gap(x, k, b, [("max", 2)])[0]
    assert g[0, 0, 0] == pytest.approx(min(t[1] - t[0], t[2] - t[3]))
    assert np.isinf(RB.min_selection_gap(x, k, b, [("max", 1)])[0]).all()


@pytest.mark.parametrize("name", IDS)
def test_oracle_matches_the_training_paths_own_autograd(name):
    """training._field_conv selects for itself (topk / amax) and spreads amax's gradient over exact ties.  Both sides are float64 here,
    so their selections agree wherever no two candidates tie to within float64 rounding: every case must clear 1e-9, and then the
    training path's gradients are the oracle's."""
    from deepctr_amd import training
    case = RB.CASE_BY_NAME[name]
    x, kernels, biases, d_out, dso = RB.case_inputs(case)
    gap = min(float(g.min()) for g in RB.min_selection_gap(x, kernels, biases, case.pools))
    assert gap > 1e-9, "%s: a float64 tie: change the seed" % name
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    ks = [torch.tensor(k, dtype=torch.float64, requires_grad=True) for k in kernels]
    bs = [torch.tensor(b, dtype=torch.float64, requires_grad=True) for b in biases]
    last, maps = training._field_conv(xt, ks, bs, list(case.pools))
    loss = 0.0
    if d_out is not None:
        loss = loss + (last * torch.tensor(d_out, dtype=torch.float64)).sum()
    for m, d in zip(maps, dso or []):
        if d is not None:
            loss = loss + (m * torch.tensor(d, dtype=torch.float64)).sum()
    loss.backward()
    G = RB.field_conv_bwd(x, kernels, RB.case_tape(case), d_out, dso)
    ref = {"dx": xt.grad.numpy(), "d_kernels": [k.grad.numpy() for k in ks], "d_biases": [b.grad.numpy() for b in bs]}
    for (k, g), (_, r) in zip(RB.outputs(G), RB.outputs(ref)):
        assert np.abs(g - r).max() <= 1e-12 * max(1.0, float(np.abs(r).max())), (name, k)


# ---------------------------------------------------------------------------------------------------
# training.field_conv_selected: the stack with its pooling as an explicit selection, ties by the reference's rules
# ---------------------------------------------------------------------------------------------------
def _selected_grads(case, dtype, sels=None):
    from deepctr_amd import training
    x, kernels, biases, d_out, dso = RB.case_inputs(case)
    xt = torch.tensor(x, dtype=dtype, requires_grad=True)
    ks = [torch.tensor(k, dtype=dtype, requires_grad=True) for k in kernels]
    bs = [torch.tensor(b, dtype=dtype, requires_grad=True) for b in biases]
    last, maps, chosen = training.field_conv_selected(xt, ks, bs, list(case.pools), sels=sels)
    assert last is maps[-1] and last.grad_fn is not None
    loss = 0.0
    if d_out is not None:
        loss = loss + (last * torch.tensor(d_out, dtype=dtype)).sum()
    for m, d in zip(maps, dso or []):
        if d is not None:
            loss = loss + (m * torch.tensor(d, dtype=dtype)).sum()
    loss.backward()
    zero = lambda t: (torch.zeros_like(t) if t.grad is None else t.grad).numpy()      # noqa: E731
    return maps, chosen, {"dx": zero(xt), "d_kernels": [zero(k) for k in ks], "d_biases": [zero(b) for b in bs]}


@pytest.mark.parametrize("name", IDS)
def test_field_conv_selected_selects_and_differentiates_as_the_oracle(name):
    from deepctr_amd import training
    case = RB.CASE_BY_NAME[name]
    x, kernels, biases, d_out, dso = RB.case_inputs(case)
    tape = RB.case_tape(case)
    maps, chosen, got = _selected_grads(case, torch.float64)
    for (P, sel), m, c in zip(tape, maps, chosen):
        assert c.dtype == torch.int64 and np.array_equal(c.numpy(), sel), name
        assert np.abs(m.detach().numpy() - P).max() <= 1e-14
    G = RB.field_conv_bwd(x, kernels, tape, d_out, dso)
    for (k, g), (_, r) in zip(RB.outputs(got), RB.outputs(G)):
        assert g.shape == r.shape and np.abs(g - r).max() <= 1e-12 * max(1.0, float(np.abs(r).max())), (name, k)
    # the values are training._field_conv's up to rounding, in float32 too
    with torch.no_grad():
        xt = torch.tensor(x)
        ks, bs = [torch.tensor(k) for k in kernels], [torch.tensor(b) for b in biases]
        want = training._field_conv(xt, ks, bs, list(case.pools))[1]
        have = training.field_conv_selected(xt, ks, bs, list(case.pools))[1]
    for a, b in zip(have, want):
        assert a.shape == b.shape and float((a - b).abs().max()) <= 2e-6


@pytest.mark.parametrize("name", [IDS[3], IDS[9], IDS[28]])
def test_field_conv_selected_pools_by_a_given_selection(name):
    """Handed a tape's selection the float32 run makes no choice of its own: its gradients are the oracle's on that tape, within the
    bar, and the selection comes back as given."""
    from tests.util import assert_close_terms
    case = RB.CASE_BY_NAME[name]
    x, kernels, biases, d_out, dso = RB.case_inputs(case)
    tape = RB.case_tape(case)
    maps, chosen, got = _selected_grads(case, torch.float32, sels=[torch.tensor(sel) for _, sel in tape])
    assert all(np.array_equal(c.numpy(), sel) for c, (_, sel) in zip(chosen, tape))
    tape32 = [(m.detach().numpy(), sel) for m, (_, sel) in zip(maps, tape)]
    G = RB.field_conv_bwd(x, kernels, tape32, d_out, dso)
    T = RB.field_conv_bwd(x, kernels, tape32, d_out, dso, absolute=True)
    for (k, g), (_, r), (_, t) in zip(RB.outputs(got), RB.outputs(G), RB.outputs(T)):
        assert_close_terms(g, r, t, rtol=1e-4, rtol_terms=RB.BWD_RTOL_TERMS, what="%s %s" % (name, k))


def test_field_conv_selected_routes_a_tie_to_one_row_as_the_reference_does():
    """Rows 1 and 2 of the input are equal, so every conv output of width 1 ties exactly.  tf.nn.top_k puts the lower row first and
    MaxPool's gradient goes to the first maximum: one row receives the gradient.  _field_conv's amax splits it over the tied rows."""
    from deepctr_amd import training
    rng = np.random.RandomState(5)
    x = rng.standard_normal((3, 4, 2))
    x[:, 2] = x[:, 1]
    x[:, 1:3] += 3.0                                    # the tied pair is the maximum of its window and the top of the k-max
    kern, bias = [np.abs(rng.standard_normal((1, 1, 2))) + 0.1], [np.zeros(2)]
    for pools, rows in ([("max", 4)], [1]), ([("kmax", 2)], [1, 2]):
        xt = torch.tensor(x, requires_grad=True)
        ks, bs = [torch.tensor(kern[0], requires_grad=True)], [torch.tensor(bias[0], requires_grad=True)]
        last, maps, sels = training.field_conv_selected(xt, ks, bs, pools)
        assert all((sels[0][:, i] == r).all() for i, r in enumerate(rows))
        tape = RB.forward_tape(x, kern, bias, pools)
        assert np.array_equal(sels[0].numpy(), tape[0][1])
        d = rng.standard_normal(tuple(last.shape))
        (last * torch.tensor(d)).sum().backward()
        G = RB.field_conv_bwd(x, kern, tape, d)
        assert np.abs(xt.grad.numpy() - G["dx"]).max() <= 1e-14 and np.abs(ks[0].grad.numpy() - G["d_kernels"][0]).max() <= 1e-13
        if pools[0][0] == "max":
            assert (xt.grad[:, 2] == 0).all() and (xt.grad[:, 1] != 0).all()       # the first maximum alone
            x2 = torch.tensor(x, requires_grad=True)
            (training._field_conv(x2, [torch.tensor(kern[0])], [torch.tensor(bias[0])], pools)[0] * torch.tensor(d)).sum().backward()
            assert (x2.grad[:, 2] != 0).all() and torch.allclose(x2.grad[:, 1] + x2.grad[:, 2], xt.grad[:, 1], rtol=1e-12, atol=0)
