"""GPU: dctr_ffm_bwd (deepctr_amd/csrc/ffm_bwd_kernels.hip) against the float64 oracle of tests/ref_ffm_bwd.py on every case of the
table there, on both routes and with reduce_sum off and on; out-of-range ids; the differentiable ops.FieldAwareFunction against the
torch ops; ONN on the autograd step with its pair products on HIP.  The oracle and the room the bar leaves are pinned without a GPU by
tests/test_ffm_bwd_oracle_cpu.py.

Bar of the op: tests.util.assert_close_terms' defaults — 1e-4 of the result plus 2e-6 of the summed magnitude — for every case and
field; none has a bar of its own.  Table gradients ACCUMULATE, so each starts at a random non-zero g0 of the result's magnitude and
``g - g0`` is compared, |g0| added to ``terms``.  A pre-pooled field's d_rows is written onto NaN inside rows PAD floats wider, whose
sentinel padding comes back bit-identical; d_out sits at column 3 of rows wider than its data; ids, tables, pooled rows and d_out come
back bit-identical, and a frozen field gets no buffer at all (its table, like every input, is unchanged).

Worst err / bar per case, largest over routes, reduce_sum and fields, on an MI355X (MEASURED_GPU below; table gradients vary in the
last bits with the order of the atomics; most of each figure is the rounding of ``g0 + gradient`` in float32):
      smallest 0.00006, ragged 0.025, vec 0.013, dup 0.059, tiles 0.063, pooled 0.032, frozen 0.015, criteo4 0.048, criteo16 0.061,
      direct 0.028
  float32 products added in sample order on the CPU, from zero (test_ffm_bwd_oracle_cpu.py -s): 0.0005 to 0.048, criteo16 0.027.

ONN's autograd step has no row threshold (training.ONN_HIP_MIN_ROWS = 0, profiles/onn_ffm_bwd.txt); one test pins that default."""
import functools

import numpy as np
import pytest
import torch

from tests import ref_ffm_bwd as RB
from tests.util import TERMS_REPORT, assert_close, assert_close_terms

pytestmark = pytest.mark.gpu

MEASURED_GPU = {"smallest": 0.00006, "ragged": 0.025, "vec": 0.013, "dup": 0.059, "tiles": 0.063, "pooled": 0.032, "frozen": 0.015,
                "criteo4": 0.048, "criteo16": 0.061, "direct": 0.028}  # case -> worst err / bar over its routes, reduce_sum and fields, on an MI355X

SENTINEL = 0.75
G_OFF, G_PAD = 3, 2


def dev(a, device):
    return torch.tensor(np.asarray(a), device=device)       # (a copy: the cases' arrays are read-only)


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


@functools.lru_cache(maxsize=None)
def _g0(name, reduce_sum):
    """Per table field the gradient table's starting value: random, non-zero, of the result's magnitude.  Computed once, read-only."""
    case = RB.CASE_BY_NAME[name]
    G, _ = RB.oracle(case, reduce_sum)
    rng = np.random.RandomState(11 + len(name))
    out = []
    for j, a in enumerate(G):
        if a is None or j in case.pooled:
            out.append(None)
            continue
        g0 = (rng.standard_normal(a.shape) * max(float(np.sqrt(np.mean(np.square(a)))), 1e-3)).astype(np.float32)
        g0.setflags(write=False)
        out.append(g0)
    return out


def _operands(device, case, reduce_sum, ids=None):
    ids_h, masters, g, pooled = RB.case_inputs(case, reduce_sum)
    F, d, B = case.shape
    ids_d = dev(ids_h if ids is None else ids, device)
    ms = [(dev(pooled[j], device),) if j in pooled else dev(masters[j], device) for j in range(F)]
    gbuf = np.full((B, G_OFF + g.shape[1] + G_PAD), -3.5, dtype=np.float32)
    gbuf[:, G_OFF:G_OFF + g.shape[1]] = g
    return ids_d, ms, dev(gbuf, device)


def _call(device, name, route, reduce_sum, max_blocks, calls=1):
    """``calls`` identical calls from g0; returns (the pooled fields' d_rows of each call, worst err / bar)."""
    from deepctr_amd import ops
    case = RB.CASE_BY_NAME[name]
    F, d, B = case.shape
    R = (F - 1) * d
    G, T = RB.oracle(case, reduce_sum)
    g0 = _g0(name, reduce_sum)
    ids_d, ms, gd = _operands(device, case, reduce_sum)
    assert ops.ffm_bwd_route(B, F, d, reduce_sum, route=route) == ("direct" if route == "direct" else case.route)
    assert ops.ffm_bwd_workspace_bytes(B, F, d, reduce_sum, route=route) == 0
    ins = [ids_d, gd] + [m[0] if isinstance(m, tuple) else m for m in ms]
    snap = [bits(t) for t in ins]
    drows, first = [], None
    for _ in range(calls):
        grads = []
        for j in range(F):
            if j in case.frozen:
                grads.append(None)
            elif j in case.pooled:
                buf = torch.full((B, R + RB.PAD), SENTINEL, device=device)
                buf[:, :R] = float("nan")
                grads.append(buf)
            else:
                grads.append(dev(g0[j], device))
        status = ops.new_status(device)
        ops.ffm_bwd(ids_d, ms, gd, grads, dim=d, reduce_sum=reduce_sum, d_out_offset=G_OFF, status=status, route=route,
                    max_blocks=max_blocks)
        torch.cuda.synchronize()
        assert int(status.item()) == 0
        for j in case.pooled:
            assert (bits(grads[j][:, R:]) == bits(torch.full_like(grads[j][:, R:], SENTINEL))).all(), "%s: d_rows' padding changed" % name
        drows.append([grads[j][:, :R].cpu().numpy() for j in case.pooled])
        first = grads if first is None else first
    for t, s in zip(ins, snap):
        assert (bits(t) == s).all(), "%s: an input changed" % name
    worst = 0.0
    print("[ffm_bwd] %s route=%s reduce=%d max_blocks=%d" % (name, route, reduce_sum, max_blocks), end=" ")
    try:
        for j in range(F):
            if j in case.frozen:
                continue
            got = first[j].cpu().numpy().astype(np.float64)
            n0 = len(TERMS_REPORT)
            try:
                if j in case.pooled:
                    assert np.isfinite(got[:, :R]).all(), "%s: d_rows of field %d holds what it held before (NaN)" % (name, j)
                    assert_close_terms(got[:, :R], G[j].reshape(B, R), T[j].reshape(B, R), what="%s d_rows of field %d" % (name, j))
                else:
                    assert_close_terms(got - g0[j], G[j], T[j] + np.abs(g0[j]), what="%s gradient of table %d" % (name, j))
            finally:
                worst = max(worst, TERMS_REPORT[n0][4]) if len(TERMS_REPORT) > n0 else worst
    finally:
        print("worst err / bar %.3g" % worst)
    return drows, worst


@pytest.mark.parametrize("name,route,reduce_sum,max_blocks", RB.RUNS, ids=RB.RUN_IDS)
def test_op_against_the_oracle(device, name, route, reduce_sum, max_blocks):
    _call(device, name, route, reduce_sum, max_blocks)


@pytest.mark.parametrize("route", [None, "direct"])
def test_d_rows_is_bit_identical_from_call_to_call(device, route):
    drows, _ = _call(device, "pooled", route, False, 0, calls=2)
    assert len(drows[0]) == 2
    for a, b in zip(drows[0], drows[1]):
        assert (a.view(np.int32) == b.view(np.int32)).all()


@pytest.mark.parametrize("all_equal", [False, True])
def test_duplicate_ids(device, all_equal):
    """Every sample of a column on one row (``dup``'s vocabulary of 1; with ``all_equal`` every column of ``tiles``): all of a
    field's atomics meet on one row."""
    from deepctr_amd import ops
    if not all_equal:
        _call(device, "dup", None, False, 0)
        return
    case = RB.CASE_BY_NAME["tiles"]
    F, d, B = case.shape
    ids_h, masters, g, _ = RB.case_inputs(case, False)
    same = np.full_like(ids_h, 5)
    G, T = RB.ffm_bwd(same, masters, g)
    ids_d, ms, gd = _operands(device, case, False, ids=same)
    grads = [torch.zeros(m.shape, device=device) for m in ms]
    ops.ffm_bwd(ids_d, ms, gd, grads, d_out_offset=G_OFF)
    for j in range(F):
        got = grads[j].cpu().numpy()
        assert (np.delete(got, 5, axis=0) == 0).all()
        assert_close_terms(got, G[j], T[j], what="all ids equal, table %d" % j)


@pytest.mark.parametrize("route", [None, "direct"])
def test_out_of_range_id_sets_the_status_word_and_touches_no_other_row(device, route):
    from deepctr_amd import ops
    case = RB.CASE_BY_NAME["pooled"]
    F, d, B = case.shape
    R = (F - 1) * d
    ids_h, masters, g, pooled = RB.case_inputs(case, False)
    bad = ids_h.copy()
    bad[1, 17] = RB.case_vocab(case)[1]             # == the vocabulary size of field 1
    G, T = RB.ffm_bwd(bad, masters, g, False, {j: v[:, :R] for j, v in pooled.items()})
    clean, _ = RB.oracle(case, False)
    ids_d, ms, gd = _operands(device, case, False, ids=bad)
    rng = np.random.RandomState(2)
    g0 = [None if j in pooled else rng.standard_normal(masters[j].shape).astype(np.float32) for j in range(F)]
    grads = [torch.full((B, R), float("nan"), device=device) if j in pooled else dev(g0[j], device) for j in range(F)]
    guard = [(m[0] if isinstance(m, tuple) else m).clone() for m in ms]
    status = ops.new_status(device)
    ops.ffm_bwd(ids_d, ms, gd, grads, d_out_offset=G_OFF, status=status, route=route)
    torch.cuda.synchronize()
    assert int(status.item()) & 1                                     # DCTR_STATUS_INDEX_OOR
    with pytest.raises(IndexError):
        ops.check_status(status)
    assert all(torch.equal(a, m[0] if isinstance(m, tuple) else m) for a, m in zip(guard, ms))
    for j in range(F):
        got = grads[j].cpu().numpy()
        if j in pooled:
            assert np.isfinite(got).all()
            assert_close_terms(got, G[j].reshape(B, R), T[j].reshape(B, R), what="d_rows of field %d beside an out-of-range id" % j)
            # sample 17's row towards field 1 is the product with a row of zeros
            assert (got[17].reshape(F - 1, d)[1] == 0).all() and (got[16].reshape(F - 1, d)[1] != 0).any()
            continue
        assert_close_terms(got.astype(np.float64) - g0[j], G[j], T[j] + np.abs(g0[j]), what="table %d beside an out-of-range id" % j)
        used = np.zeros(masters[j].shape[0], dtype=bool)
        ok = (bad[j] >= 0) & (bad[j] < masters[j].shape[0])
        used[bad[j][ok]] = True
        assert (got[~used].view(np.int32) == g0[j][~used].view(np.int32)).all(), "a row no id names changed"
    # the sample adds nothing to its own field: field 1's gradient is the clean one less sample 17's share
    r = int(ids_h[1, 17])
    assert np.abs(clean[1][r] - G[1][r]).max() > 0
    others = np.delete(np.arange(masters[1].shape[0]), r)
    assert (clean[1][others] == G[1][others]).all()


# ---------------------------------------------------------------------------------------------------
# the differentiable op
# ---------------------------------------------------------------------------------------------------
def _torch_pairs(views, ids, pooled, F, reduce_sum):
    """The torch ops of _ONN.field_aware_rows / _autograd_logit over per-name views (a pooled field: its [B, F-1, d] rows)."""
    from deepctr_amd import training
    from tests.ref_onn import slot
    embs = []
    for j in range(F):
        if j in pooled:
            embs.append({i: pooled[j][:, slot(j, i), :] for i in range(F) if i != j})
        else:
            embs.append({i: views[j][slot(j, i)][ids[j].to(torch.int64)] for i in range(F) if i != j})
    prods = []
    for i, j in zip(*training._pair_indices(F)):
        pr = embs[i][j] * embs[j][i]
        prods.append(pr.sum(-1, keepdim=True) if reduce_sum else pr)
    return torch.cat(prods, dim=-1)


@pytest.mark.parametrize("reduce_sum", [False, True])
@pytest.mark.parametrize("with_seq", [False, True])
def test_function_against_the_torch_ops(device, with_seq, reduce_sum):
    from deepctr_amd import ops
    case = RB.CASE_BY_NAME["pooled" if with_seq else "ragged"]
    F, d, B = case.shape
    R = (F - 1) * d
    ids_h, masters_h, g, pooled_h = RB.case_inputs(case, reduce_sum)
    G, T = RB.oracle(case, reduce_sum)
    ids_d, gd = dev(ids_h, device), dev(g, device)
    masters = [None if j in pooled_h else dev(masters_h[j], device) for j in range(F)]
    views = [None if m is None else [m[:, k, :].requires_grad_(True) for k in range(F - 1)] for m in masters]
    leaves = {j: dev(np.ascontiguousarray(pooled_h[j][:, :R]), device).requires_grad_(True) for j in pooled_h}
    # a pooled field reaches the op through torch ops (the model pools there): its gradient flows on through them
    spec = [(lambda j=j: leaves[j] * 1.0) if m is None else views[j] for j, m in enumerate(masters)]
    inputs = ops.FieldAwareFunction.inputs_of(masters, spec)
    assert inputs is not None and len(inputs) == sum(1 if m is None else F - 1 for m in masters)
    out = ops.FieldAwareFunction.apply(ids_d, masters, d, reduce_sum, None, *inputs)
    assert out.grad_fn is not None and tuple(out.shape) == g.shape
    params = [v for vs in views if vs is not None for v in vs] + [leaves[j] for j in sorted(leaves)]
    got = torch.autograd.grad(out, params, gd)
    ref = _torch_pairs(views, ids_d, {j: leaves[j].reshape(B, F - 1, d) for j in leaves}, F, reduce_sum)
    if reduce_sum:      # the kernel sums a pair's d products in one fma chain, torch in its own order: the bar, not the bits
        x64 = _torch_pairs([None if vs is None else [v.detach().double() for v in vs] for vs in views], ids_d,
                           {j: leaves[j].detach().double().reshape(B, F - 1, d) for j in leaves}, F, True)
        a64 = _torch_pairs([None if vs is None else [v.detach().double().abs() for v in vs] for vs in views], ids_d,
                           {j: leaves[j].detach().double().abs().reshape(B, F - 1, d) for j in leaves}, F, True)
        assert_close_terms(out.detach().cpu().numpy(), x64.cpu().numpy(), a64.cpu().numpy(), what="forward with reduce_sum")
    else:               # one fp32 product per output on both sides
        assert torch.equal(out.detach(), ref.detach())
    want = torch.autograd.grad(ref, params, gd)
    at = 0
    for j in range(F):
        if masters[j] is None:
            continue
        mine = np.stack([t.cpu().numpy() for t in got[at:at + F - 1]], axis=1)
        theirs = np.stack([t.cpu().numpy() for t in want[at:at + F - 1]], axis=1)
        at += F - 1
        assert_close_terms(mine, G[j], T[j], what="FieldAwareFunction: table %d" % j)
        assert_close_terms(theirs, G[j], T[j], what="torch ops: table %d" % j)
    for k, j in enumerate(sorted(leaves)):
        assert_close_terms(got[at + k].cpu().numpy(), G[j].reshape(B, R), T[j].reshape(B, R), what="FieldAwareFunction: pooled rows %d" % j)
    # a frozen field: its views get no gradient and the others are what they were
    for v in views[1]:
        v.requires_grad_(False)
    out = ops.FieldAwareFunction.apply(ids_d, masters, d, reduce_sum, None, *ops.FieldAwareFunction.inputs_of(masters, spec))
    live = [v for v in params if v.requires_grad]
    again = torch.autograd.grad(out, live, gd)
    assert len(live) == len(params) - (F - 1)
    assert_close_terms(again[0].cpu().numpy(), G[0][:, 0, :], T[0][:, 0, :], what="FieldAwareFunction with field 1 frozen")


def test_a_view_that_is_not_the_slot_of_its_table_is_refused(device):
    from deepctr_amd import ops
    F, d, V = 3, 4, 9
    m = [torch.randn(V, F - 1, d, device=device) for _ in range(F)]
    views = [[t[:, k, :] for k in range(F - 1)] for t in m]
    ok = ops.FieldAwareFunction.inputs_of(m, views)
    assert ok is not None and all(a is b for a, b in zip(ok, [v for vs in views for v in vs]))
    for broken in ([views[0][1], views[0][0]],                                # slots swapped
                   [views[0][0], views[1][1]],                                # a slot of another table
                   [views[0][0], views[0][1].clone()],                        # a copy
                   [views[0][0], views[0][1][:V - 1]],                        # fewer rows
                   [views[0][0]]):                                            # a slot missing
        assert ops.FieldAwareFunction.inputs_of(m, [broken] + views[1:]) is None
    assert ops.FieldAwareFunction.inputs_of([m[0].double()] + m[1:], views) is None


# ---------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------
def _normalised(got, ref, gmax, what, rtol=5e-4, atol=1e-5):
    """The bar of tests/test_gpu_flen.py:_normalised: relative to the tensor's largest gradient, at least 1e-2 of the step's."""
    scale = max(float(np.abs(ref).max()), 1e-2 * gmax)
    assert_close(np.asarray(got) / scale, np.asarray(ref) / scale, rtol=rtol, atol=atol, what=what)


def _small(rng, n, d=8, frozen=False):
    from deepctr_amd.feature_column import DenseFeat, SparseFeat, VarLenSparseFeat
    cols = [SparseFeat("C%d" % i, 50, d, trainable=not (frozen and i == 2)) for i in range(5)]
    cols += [VarLenSparseFeat(SparseFeat("S", 30, d), maxlen=4, combiner="mean"), DenseFeat("I0", 1)]
    feed = {"C%d" % i: rng.randint(0, 50, n).astype(np.int32) for i in range(5)}
    feed["S"] = rng.randint(0, 30, (n, 4)).astype(np.int32)
    feed["S"][:, 0] = np.maximum(feed["S"][:, 0], 1)
    feed["I0"] = rng.rand(n).astype(np.float32)
    return cols, feed


def _count_calls(monkeypatch):
    from deepctr_amd import ops
    seen = []
    real = ops.ffm_bwd
    monkeypatch.setattr(ops, "ffm_bwd", lambda *a, **k: (seen.append(1), real(*a, **k))[1])
    return seen


def _loss_and_grads(model, staged, n, y, params):
    from deepctr_amd import training
    model._begin()
    logit = training.model_logits(model, staged, 0, n, training=True)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(logit, y)
    grads = torch.autograd.grad(loss, params, allow_unused=True)
    return float(loss.detach()), [None if g is None else g.cpu().numpy() for g in grads]


@pytest.mark.parametrize("reduce_sum", [False, True])
@pytest.mark.parametrize("use_bn", [False, True])
def test_model_gradients_with_the_switch_on_and_off(device, use_bn, reduce_sum, monkeypatch):
    from deepctr_amd import engine, models, training, training_hip
    rng = np.random.RandomState(8)
    n = 211
    cols, feed = _small(rng, n, frozen=True)
    model = models.ONN(cols, cols, dnn_hidden_units=(32, 16), use_bn=use_bn, reduce_sum=reduce_sum, seed=5, device=device)
    assert not training_hip.supported(model)
    y = dev(rng.randint(0, 2, n).astype(np.float32), device)
    staged = engine.Staged(n)
    model._stage_inputs(feed, staged)
    frozen = training.frozen_weights(model)
    named = [(k, t) for k, t in model.named_weights() if "moving_" not in k and t.data_ptr() not in frozen]
    assert not any(k.startswith("sparse_emb_C2_") for k, _ in named) and any(k.startswith("sparse_emb_S_") for k, _ in named)
    params = [t for _, t in named]
    seen = _count_calls(monkeypatch)
    monkeypatch.setattr(training, "ONN_HIP_MIN_ROWS", 0)
    moving = [t.clone() for k, t in model.named_weights() if "moving_" in k]
    try:
        for t in params:
            t.requires_grad_(True)
        monkeypatch.setattr(training, "HIP_AUTOGRAD_OPS", False)
        loss_off, g_off = _loss_and_grads(model, staged, n, y, params)
        assert not seen
        for t, m in zip([t for k, t in model.named_weights() if "moving_" in k], moving):
            t.copy_(m)                       # (the BatchNormalization's moving statistics: both runs start from the same)
        monkeypatch.setattr(training, "HIP_AUTOGRAD_OPS", True)
        loss_on, g_on = _loss_and_grads(model, staged, n, y, params)
        assert len(seen) == 1
    finally:
        for t in params:
            t.requires_grad_(False)
    assert abs(loss_on - loss_off) <= 1e-5 * abs(loss_off)
    gmax = max(float(np.abs(g).max()) for g in g_off if g is not None)
    live = 0
    for (k, _), a, b in zip(named, g_on, g_off):
        assert (a is None) == (b is None), k
        if a is not None:
            _normalised(a, b, gmax, "use_bn=%d reduce_sum=%d: d %s" % (use_bn, reduce_sum, k))
            live += k.startswith("sparse_emb_") and float(np.abs(a).max()) > 0
    assert live >= 20


def test_fit_runs_the_pair_products_backward_on_hip(device, monkeypatch):
    from deepctr_amd import models, training, training_hip
    rng = np.random.RandomState(9)
    n = 512
    cols, feed = _small(rng, n)
    y = ((feed["C0"] % 2) ^ (feed["C1"] % 3 == 0)).astype(np.float32)
    seen = _count_calls(monkeypatch)
    monkeypatch.setattr(training, "ONN_HIP_MIN_ROWS", 0)
    ends = {}
    w0 = None
    for on in (True, False):
        model = models.ONN(cols, cols, dnn_hidden_units=(32, 16), seed=5, device=device)
        assert not training_hip.supported(model)
        if w0 is None:
            w0 = model.get_weights_by_name()
        else:
            model.set_weights_by_name(w0)
        monkeypatch.setattr(training, "HIP_AUTOGRAD_OPS", on)
        del seen[:]
        model.compile("adam", "binary_crossentropy")
        hist = model.fit(feed, y, batch_size=256, epochs=1, shuffle=False, verbose=0)          # two steps
        assert np.isfinite(hist.history["loss"]).all()
        assert len(seen) == (2 if on else 0)
        ends[on] = model.get_weights_by_name()
    moved = 0
    for k in sorted(w0):
        # two Adam steps move a weight by at most 2e-3: the two runs agree to half a percent of that
        assert_close(ends[True][k], ends[False][k], rtol=1e-4, atol=1e-5, what="after two steps: " + k)
        moved += k.startswith("sparse_emb_") and not np.array_equal(ends[True][k], w0[k])
    assert moved >= 20


def test_default_row_threshold(device, monkeypatch):
    """profiles/onn_ffm_bwd.txt: the HIP op wins at every row count measured, so ONN's autograd step has no row threshold; the
    mechanism stays (training.ONN_HIP_MIN_ROWS), and below it the torch ops run."""
    from deepctr_amd import engine, models, training
    assert training.ONN_HIP_MIN_ROWS == 0
    rng = np.random.RandomState(6)
    cols, feed = _small(rng, 32)
    model = models.ONN(cols, cols, dnn_hidden_units=(8,), device=device)
    seen = _count_calls(monkeypatch)
    monkeypatch.setattr(training, "ONN_HIP_MIN_ROWS", 32)
    params = [t for k, t in model.named_weights() if k.startswith("sparse_emb_")]
    staged = engine.Staged(32)
    model._stage_inputs(feed, staged)
    try:
        for t in params:
            t.requires_grad_(True)
        for B, want in ((31, 0), (32, 1)):
            del seen[:]
            model._begin()
            training.model_logits(model, staged, 0, B, training=True).sum().backward()
            assert len(seen) == want, (B, seen)
    finally:
        for t in params:
            t.requires_grad_(False)
            t.grad = None
