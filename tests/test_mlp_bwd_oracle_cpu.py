"""CPU: pins tests/ref_mlp_bwd.py, the checker of tests/test_gpu_mlp_bwd.py — the float64 oracle against torch double autograd, its
``terms`` against the values, and the form (chained / layered) of every GPU case against dctr_mlp_bwd_workspace_bytes, which is host
arithmetic and runs without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

from tests import ref_mlp_bwd as RM


def _flat(g):
    out = [("dx", g["dx"])] + [("dW%d" % l, a) for l, a in enumerate(g["dW"])] + [("db%d" % l, a) for l, a in enumerate(g["db"])]
    return out + ([("d_head_w", g["d_head_w"])] if g["d_head_w"] is not None else [])


@pytest.mark.parametrize("head", [True, False])
@pytest.mark.parametrize("act", RM.ACTS)
def test_oracle_equals_double_autograd_on_the_unrounded_forward(act, head):
    """With the saved outputs = the float64 forward itself, "act' from the outputs" and autograd are the same function: 1e-12 relative,
    headed and headless; switching dx / the bias gradients off only drops outputs (the oracle always returns all of them), so the
    comparison covers those forms element for element."""
    rng = np.random.RandomState(11)
    B, w = 37, [13, 8, 6, 5]
    x = rng.standard_normal((B, w[0]))
    ks = [rng.standard_normal((k, n)) / np.sqrt(k) for k, n in zip(w[:-1], w[1:])]
    bs = [rng.standard_normal(n) * 0.1 for n in w[1:]]
    hw, dl, dout = rng.standard_normal(w[-1]) * 0.3, rng.standard_normal(B), rng.standard_normal((B, w[-1]))
    f = {"relu": torch.relu, "tanh": torch.tanh, "sigmoid": torch.sigmoid, "linear": lambda z: z}[act]
    for want_dx in (True, False):
        for want_db in (True, False):
            xt = torch.tensor(x, requires_grad=want_dx)
            kt = [torch.tensor(k, requires_grad=True) for k in ks]
            bt = [torch.tensor(b, requires_grad=want_db) for b in bs]
            ht = torch.tensor(hw, requires_grad=True)
            h, saved = xt, []
            for k, b in zip(kt, bt):
                h = f(h @ k + b)
                saved.append(h.detach().numpy())
            loss = ((h @ ht) * torch.tensor(dl)).sum() if head else (h * torch.tensor(dout)).sum()
            loss.backward()
            mine = RM.saved_acts(x, ks, bs, act, round32=False)
            for a, b in zip(mine, saved):
                np.testing.assert_allclose(a, b, rtol=1e-13, atol=0)
            g, t = RM.mlp_bwd(x, ks, saved, act, head_w=hw if head else None, dlogit=dl if head else None, d_out=None if head else dout)
            ref = {"dx": xt.grad} if want_dx else {}
            ref.update(("dW%d" % l, k.grad) for l, k in enumerate(kt))
            if want_db:
                ref.update(("db%d" % l, b.grad) for l, b in enumerate(bt))
            if head:
                ref["d_head_w"] = ht.grad
            got = dict(_flat(g))
            assert set(ref) <= set(got)
            for name, r in ref.items():
                r = r.numpy()
                assert got[name].shape == r.shape and got[name].dtype == np.float64
                err = np.abs(got[name] - r)
                assert (err <= 1e-12 * np.abs(r)).all(), "%s %s: worst relative error %.3g" % (act, name, float((err / np.abs(r)).max()))
            for (name, v), (_, tv) in zip(_flat(g), _flat(t)):
                assert (tv >= np.abs(v)).all(), "terms < |value| in " + name


@pytest.mark.parametrize("act", RM.ACTS)
def test_terms_bound_the_values_on_float32_saved_outputs(act):
    """terms >= |value| elementwise on what the GPU test feeds (saved outputs rounded to float32, relu with exact zeros)."""
    for case in (c for c in RM.CASES if c.id in ("chain-B33", "chain-pad64", "headless3-chain-B37", "layer-B33")):
        d = RM.make_data(case, act)
        g, t = RM.oracle(case, d, act)
        for (name, v), (_, tv) in zip(_flat(g), _flat(t)):
            assert v.shape == tv.shape and np.isfinite(v).all()
            assert (tv >= np.abs(v)).all(), "%s %s: terms < |value|" % (case.id, name)
        assert all(a.dtype == np.float32 for a in d["acts"])
        if act == "relu":
            assert all((a == 0).any() and (a > 0).any() for a in d["acts"])


def test_saved_acts_refuses_a_relu_layer_without_zeros():
    x = np.ones((3, 2))
    with pytest.raises(AssertionError):
        RM.saved_acts(x, [np.ones((2, 2))], [np.zeros(2)], "relu")


def _library_bytes(batch, widths, act="relu"):
    from deepctr_amd import _C
    units = (ctypes.c_int32 * (len(widths) - 1))(*widths[1:])
    a = _C.MlpBwdArgs(x=ctypes.c_void_p(4096), batch=batch, x_stride=widths[0] + 3, in_dim=widths[0], n_layers=len(widths) - 1,
                      units=ctypes.cast(units, ctypes.c_void_p), activation=_C.ACT_CODES[act])
    return int(_C.lib().dctr_mlp_bwd_workspace_bytes(ctypes.byref(a)))


def test_width_1216_is_chained_and_1217_is_layered():
    """The threshold between the two forms, from the layouts in the comments of mlp_bwd_chain_floats and mlp_bwd_main_floats
    (deepctr_amd/csrc/dnn_train_kernels.hip): chained = per layer
    dZ [B, N] + W^T [K N] + slices x (K + 1) N, each 4-float aligned; layered = two buffers [B, widest] + the largest sliced dW."""
    B = 37                                                   # one slice, one part
    for k0, chained in ((1216, True), (1217, False)):
        w = [k0, 8]
        lay = (2 * B * k0 + 3) // 4 * 4
        cha = (B * 8 + 3) // 4 * 4 + (k0 * 8 + 3) // 4 * 4 + ((k0 + 1) * 8 + 3) // 4 * 4
        assert cha != lay and RM.is_chained(w) == chained
        assert _library_bytes(B, w) == 4 * (max(lay, cha) if chained else lay)
        assert RM.workspace_bytes(B, w) == _library_bytes(B, w)
    # the same threshold where the wide layer is an inner one, and where the chained layout is the larger of the two
    for n, chained in ((1216, True), (1217, False)):
        w, B = [8, n, 8], 16
        assert RM.is_chained(w) == chained and RM.chained_floats(B, w) > RM.layered_floats(B, w)
        assert _library_bytes(B, w) == 4 * (RM.chained_floats(B, w) if chained else RM.layered_floats(B, w))


def test_every_gpu_case_takes_the_form_the_table_states():
    """Each case of the table names its form; the restated host arithmetic agrees, and the library's workspace size is the one of that
    form for every activation — decisive wherever the chained layout is larger than the layered one, which the table says per case."""
    assert len(set(RM.CASE_IDS)) == len(RM.CASES)
    decided = 0
    for c in RM.CASES:
        w = list(c.widths)
        assert c.route in ("chained", "layered")
        assert RM.is_chained(w) == (c.route == "chained"), c.id
        assert (max(w) <= 1216) == (c.route == "chained"), c.id
        for act in RM.ACTS:
            assert _library_bytes(c.batch, w, act) == RM.workspace_bytes(c.batch, w), (c.id, act)
        cha, lay = RM.chained_floats(c.batch, w), RM.layered_floats(c.batch, w)
        assert _library_bytes(c.batch, w) == 4 * (max(cha, lay) if c.route == "chained" else lay), c.id
        decided += cha > lay                      # the size tells the two forms apart
        # Dice never takes the chain
        assert _library_bytes(c.batch, w, "dice") == 4 * RM.layered_floats(c.batch, w, dice=True), c.id
    assert decided >= 10, decided                # (small batches under wide layers: the slices outweigh the ping-pong buffers)
    # the slice and tile counts the table's comments promise
    assert [RM.k_slices(b) for b in (256, 257, 513, 4097, 8193)] == [1, 2, 3, 17, 29]
    assert [RM.chain_rt(b, [13, 8, 5]) for b in (8192, 8193, 65536, 65600)] == [1, 2, 2, 4]      # (restated only: see chain_rt)
    assert [RM.dw_parts(b, 1217 * 8) for b in (33, 1024, 1031, 1536)] == [1, 2, 1, 3]
    assert RM.dw_parts(1024, 24 * 1300) == 2 and RM.dw_parts(1024, 1300 * 8) == 2
    assert _library_bytes(0, [13, 8, 5]) == 0


def test_nine_layers_and_an_empty_batch_are_decided_by_the_host():
    """The size checks come first: nine layers are DCTR_E_DIM, an empty batch returns at once — the GPU test asserts that neither
    changes a buffer.  Every pointer is NULL, so a reorder of those checks shows as DCTR_E_NULL here, not as a read."""
    from deepctr_amd import _C
    a = _C.MlpBwdArgs(x=None, batch=37, x_stride=14, in_dim=11, n_layers=9, units=None, kernels=None, acts=None,
                      activation=_C.ACT_CODES["relu"], dx_stride=13, workspace=None, workspace_bytes=0)
    assert _C.lib().dctr_mlp_bwd(ctypes.byref(a), None) == -2 and b"bad sizes" in _C.lib().dctr_last_error()
    a.n_layers, a.batch = 8, 0
    assert _C.lib().dctr_mlp_bwd(ctypes.byref(a), None) == 0


def test_the_workspace_guard_is_decisive_for_these_chained_cases():
    """The GPU test's guard tail starts at max(layered, chained) floats: it sees an overrun of the chained carving only where the chained
    layout is the larger one.  These cases are the ones, one of them with more than one dW slice."""
    tight = [c for c in RM.CASES if c.route == "chained" and RM.chained_floats(c.batch, list(c.widths)) >= RM.layered_floats(c.batch, list(c.widths))]
    assert len(tight) >= 10, [c.id for c in tight]
    assert {"chain-B1", "chain-B17", "chain-pad64", "chain-8layers", "headless3-chain-B37", "nodx3-chain-B37", "chain-tight-B257"} <= {c.id for c in tight}
    assert any(RM.k_slices(c.batch) > 1 for c in tight)
