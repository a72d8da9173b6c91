"""Pins, without a GPU, what tests/test_gpu_cin_bwd.py checks the CIN backward against (tests/ref_cin_bwd.py): the float64 oracle
against torch double autograd over the reference formulation, its ``terms`` against its values, the restated routes and the case table
against dctr_cin_bwd_workspace_bytes (host arithmetic of the library; the CU count falls back to 256 without a device), the branches the
table must name, and that the shapes of the hole-* cases carry enough signal for a staging hole to miss the bar by a wide margin."""
import functools

import numpy as np
import pytest
import torch

from tests import ref_cin_bwd as RC

CASE = {c.id: c for c in RC.CASES}
HOLE_IDS = [i for i in RC.CASE_IDS if i.startswith("hole-")]
KS_IDS = [i for i in RC.CASE_IDS if i.startswith("ks-")]


@functools.lru_cache(maxsize=None)
def _reference(case_id):
    case, rt = RC.resolve(CASE[case_id])
    d = RC.make_data(case)
    g, t = RC.oracle(case, d)
    return case, rt, d, g, t


def _ratio(got, ref, terms):
    """Worst error in units of tests.util.assert_close_terms' default bar."""
    return float((np.abs(got - ref) / (1e-4 * np.abs(ref) + 2e-6 * np.abs(terms) + 1e-30)).max())


@pytest.mark.parametrize("layers", [(6,), (6, 5), (6, 5, 4)])
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("act", RC.ACTS)
def test_the_oracle_matches_double_autograd(act, split, layers):
    """The reference formulation (interaction.py:277-325) in torch float64 with autograd, against the oracle fed the UNROUNDED saved
    outputs of the same forward: 1e-12 of each gradient's largest element."""
    rng = np.random.RandomState(len(layers) + 10 * split + 100 * RC.ACTS.index(act))
    B, F0, D = 5, 4, 3
    plan, out_dim = RC.layer_plan(F0, layers, split)
    x = rng.standard_normal((B, F0 * D))
    fs = [rng.standard_normal((F0 * fk, H)) / np.sqrt(F0 * fk) for fk, H, _, _, _ in plan]
    bs = [rng.standard_normal(H) * 0.1 for _, H, _, _, _ in plan]
    d_out = rng.standard_normal((B, out_dim))
    xt = torch.tensor(x, requires_grad=True)
    ft = [torch.tensor(f, requires_grad=True) for f in fs]
    bt = [torch.tensor(b, requires_grad=True) for b in bs]
    f_act = {"relu": torch.relu, "linear": lambda z: z, "sigmoid": torch.sigmoid, "tanh": torch.tanh}[act]
    x0 = xt.reshape(B, F0, D)
    hidden, finals = x0, []
    for k, h in enumerate(layers):
        z = torch.einsum("bid,bjd->bdij", x0, hidden).reshape(B, D, -1)
        y = f_act(z @ ft[k] + bt[k]).transpose(1, 2)                                  # [B, H, D]
        if split and k != len(layers) - 1:
            hidden, direct = y[:, :h // 2], y[:, h // 2:]
        else:
            hidden, direct = y, y
        finals.append(direct)
    (torch.cat(finals, dim=1).sum(-1) * torch.tensor(d_out)).sum().backward()
    x0t = RC.to_rows(x, F0, D)
    ys, _ = RC.forward(x0t, fs, bs, layers, split, act, round32=False)
    g, t = RC.cin_bwd(x0t, fs, ys, layers, split, act, d_out, D)

    def close(got, ref, what):
        ref = ref.numpy()
        assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max(), "%s: %.3g of %.3g" % (what, np.abs(got - ref).max(), np.abs(ref).max())
    close(RC.from_rows(g["dx"], B, F0, D), xt.grad, "dx")
    for k in range(len(layers)):
        close(g["dW"][k], ft[k].grad, "dW%d" % k)
        close(g["db"][k], bt[k].grad, "db%d" % k)
        assert (np.abs(g["dW"][k]) <= t["dW"][k] * (1 + 1e-12)).all() and (np.abs(g["db"][k]) <= t["db"][k] * (1 + 1e-12)).all()


@pytest.mark.parametrize("case_id", RC.CASE_IDS)
def test_terms_dominate_the_values_and_the_case_reaches_its_route(case_id):
    """resolve() raises when the restated routes of a case no longer satisfy what it was made for; the terms are an upper bound."""
    case, rt, d, g, t = _reference(case_id)
    for key in ("dx", "dx0"):
        assert (np.abs(g[key]) <= t[key] * (1 + 1e-12) + 1e-300).all(), key
    for key in ("dW", "db", "dxk", "dpre"):
        for k in range(len(case.layers)):
            assert (np.abs(g[key][k]) <= t[key][k] * (1 + 1e-12) + 1e-300).all(), "%s%d" % (key, k)
    assert case.tags <= set(RC.BRANCHES), case.tags - set(RC.BRANCHES)


@pytest.mark.parametrize("case_id", RC.CASE_IDS)
def test_the_restated_routes_reproduce_the_workspace_size(case_id):
    """The size depends on which layers carry z (non-fused) and on the dW kernel's slice count (fused): a disagreement means the table
    no longer describes the code.  No device here: the library's CU count is the 256 the restatement defaults to."""
    case, rt = RC.resolve(CASE[case_id])
    need, fwd_ws = RC.library_bytes(case.B, case.F0, case.D, case.layers, case.split)
    assert need == 4 * RC.workspace_floats(case.B, case.F0, case.D, case.layers, case.split, fwd_ws), (case.id, rt)


def test_a_wrong_route_would_change_the_workspace_size():
    """The pin above is decisive: one more slice, or a layer taken for fused that is not, moves the restated size."""
    c, _ = RC.resolve(CASE["mixed-f-nf-f"])
    need, fwd_ws = RC.library_bytes(c.B, c.F0, c.D, c.layers, c.split)
    assert need != 4 * RC.workspace_floats(c.B, c.F0, c.D, (32, 16, 16), c.split, fwd_ws)
    c, rt = RC.resolve(CASE["slices-2"])
    need, fwd_ws = RC.library_bytes(c.B, c.F0, c.D, c.layers, c.split)
    assert need == 4 * RC.workspace_floats(c.B, c.F0, c.D, c.layers, c.split, fwd_ws)
    assert need != 4 * RC.workspace_floats(c.B, c.F0, c.D, c.layers, c.split, fwd_ws, cus=128)


def test_every_branch_is_named_by_a_case():
    covered = set().union(*(c.tags for c in RC.CASES))
    assert set(RC.BRANCHES) <= covered, sorted(set(RC.BRANCHES) - covered)
    # both fused dW endings and both non-fused ones, every activation on a fused and on a non-fused case, and the issue's families
    for act in RC.ACTS:
        assert {"act-%s-fused" % act, "act-%s-nonfused" % act} <= set(CASE)
    for fk in (4, 12, 16, 17, 26, 32, 36, 48, 64):
        for F0 in (1, 2, 3, 5, 32):
            for how in ("split", "whole"):
                assert "tpi-%d-Fk%d-F%d-%s" % (-(-fk // 16), fk, F0, how) in CASE
    # Fk = 17 and 26 without split-half come from a non-fused first layer whose row pitch is no multiple of 4
    for cid in ("tpi-2-Fk17-F5-whole", "tpi-2-Fk26-F5-whole", "tpi-2-Fk17-F5-split"):
        rt = RC.resolve(CASE[cid])[1]
        assert not rt[0].fused and rt[1].fused and not rt[1].XK4 and rt[1].ldk % 4 != 0
    assert len(set(RC.CASE_IDS)) == len(RC.CASE_IDS)


@pytest.mark.parametrize("cus", [64, 104, 256, 304])
def test_the_slices_cases_resolve_at_other_cu_counts(cus):
    for tiles in (2, 3):
        case, rt = RC.resolve(CASE["slices-%d" % tiles], cus)
        assert rt[1].tiles == tiles and rt[1].last_rows % RC.RB != 0 and rt[1].splits >= 2
        assert RC.routes(case.F0, case.layers, case.split, (case.B - 1) * case.D, cus)[1].tiles <= tiles
    assert RC.resolve(CASE["slices-2"])[0].B * 3 < 5000 and RC.resolve(CASE["slices-3"])[0].B * 3 < 9000      # ~4.5 k and ~8.3 k rows at 256 CUs


def test_the_staging_maps():
    """What the row-stepped dpre staging left unwritten (enumerated on the CPU), and that the flat index writes every float4 of the tile
    exactly once for every H the kernels take."""
    for H in range(16, 129, 16):
        old, new = RC.old_dpre_stage_map(H), RC.dpre_stage_map(H)
        assert (new == 1).all(), H
        assert old.all() == (256 % (H // 4) == 0), H
    hole = {H: ~RC.old_dpre_stage_map(H) for H in (48, 80, 96, 112)}
    assert [tuple(x) for x in np.argwhere(hole[48])] == [(63, c) for c in range(4, 12)]
    assert [tuple(x) for x in np.argwhere(hole[112])] == [(63, c) for c in range(4, 28)]
    for H in (80, 96):
        H4 = H // 4
        assert [tuple(x) for x in np.argwhere(hole[H])] == [(60, c) for c in range(16, H4)] + [(r, c) for r in (61, 62, 63) for c in range(H4)]


@pytest.mark.parametrize("mode", ["zero", "stale"])
@pytest.mark.parametrize("case_id", HOLE_IDS)
def test_a_staging_hole_misses_the_bar_by_a_wide_margin(case_id, mode):
    """Do the hole-* shapes carry enough signal (under ReLU part of dpre is zero anyway)?  A NumPy emulation of the hole — the unstaged
    dpre entries of every 64-row block read as zeros, or as the previous block's values — against the clean oracle, in units of
    assert_close_terms' default bar.  A correct fp32 kernel sits below 1; required here: above 100 for dx and for dW.
    Measured over the sixteen cases (run with -s for each figure): dx 8.1e3 .. 3.6e4 x the bar with zeros and 1.2e4 .. 7.3e4 with stale
    values; dW 3.9e3 .. 1.2e5 with zeros and 5.3e3 .. 3.0e5 with stale values.  The lowest dW figures and the lowest dx with zeros are
    hole-H48-ks3-R128-F3's: 8 of 12 float4 columns of two rows in 128."""
    case, rt, d, g, t = _reference(case_id)
    gc, _ = RC.oracle(case, d, corrupt=RC.hole_emulation(case.layers[0], mode))
    r_dx, r_dw = _ratio(gc["dx"], g["dx"], t["dx"]), _ratio(gc["dW"][0], g["dW"][0], t["dW"][0])
    print("%s %s: dx %.3g  dW %.3g x the bar" % (case_id, mode, r_dx, r_dw))
    assert r_dx > 100 and r_dw > 100, (r_dx, r_dw)
    assert _ratio(gc["db"][0], g["db"][0], t["db"][0]) == 0.0            # (the column sums never went through the staged tile)


@pytest.mark.parametrize("case_id", KS_IDS)
def test_the_emulation_is_a_no_op_where_the_staging_had_no_hole(case_id):
    case, rt, d, g, t = _reference(case_id)
    assert 256 % (case.layers[0] // 4) == 0
    for mode in ("zero", "stale"):
        gc, _ = RC.oracle(case, d, corrupt=RC.hole_emulation(case.layers[0], mode))
        assert _ratio(gc["dx"], g["dx"], t["dx"]) <= 1.0 and _ratio(gc["dW"][0], g["dW"][0], t["dW"][0]) <= 1.0
