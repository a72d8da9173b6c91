"""GPU: dctr_mlr_bwd (deepctr_amd/csrc/mlr_bwd_kernels.hip) against the float64 oracle of tests/ref_mlr.py over the forward's sweep (at
B <= 700), its edge cases, the differentiable ops.MLRFunction against training._mlr_output under autograd, and fit() with
HIP_AUTOGRAD_OPS on against off.

Bar of the op: tests.util.assert_close_terms' defaults — 1e-4 of the result plus 2e-6 of the summed magnitude — for dz, the table
gradients and the pooled-row gradients.  The backward is given the z the oracle's forward produced, rounded to float32, and the oracle
differentiates at that same z.  Table gradients ACCUMULATE, so each starts at a random non-zero g0 of the result's magnitude and
``g - g0`` is compared, |g0| added to ``terms``; the masters' padding columns start at a sentinel and must come back bit-identical.

Worst err / bar over the sweep on an MI355X: 0.12 .. 0.21 per (F, bias) (printed by the sweep test; table gradients vary in the last
bits with the order of the atomics)."""
import numpy as np
import pytest
import torch

from tests import ref_mlr as RM
from tests.test_gpu_ffm_bwd import _normalised
from tests.test_gpu_mlr import dev, dev_fields
from tests.util import assert_close, assert_close_terms

pytestmark = pytest.mark.gpu

SENTINEL = 0.75


def _backward(device, case, R, bias, task, B, seed, frozen=(), fields=None):
    """One dctr_mlr_bwd call on the case (``fields``: the case's with other ids); checks everything against the oracle and returns the
    worst err / bar it saw."""
    from deepctr_amd import ops
    K = case["K"]
    rng = np.random.RandomState(seed)
    fields = case["fields"] if fields is None else fields
    fwd = RM.mlr_op(fields, B, R, bias, task, case["dense"], case["dense_w"])
    z32 = fwd["z"].astype(np.float32)
    d_out = rng.standard_normal(B).astype(np.float32)
    res = RM.mlr_op(fields, B, R, bias, task, case["dense"], case["dense_w"], d_out=d_out, z=z32)
    dfields, owners = dev_fields(dict(case, fields=fields), device)
    snap = [o.clone() for o in owners]
    # gradient buffers shaped like the owners: tables start at g0 with a sentinel in the columns the field does not own
    g0, gbufs, grads = [], [], []
    for j, (f, (own, first)) in enumerate(zip(fields, case["owners"])):
        if j in frozen:
            g0.append(None)
            gbufs.append(None)
            grads.append(None)
            continue
        scale = max(float(np.sqrt(np.mean(np.square(res["grads"][j])))), 1e-3)
        buf = np.full(own.shape, SENTINEL, dtype=np.float32)
        if f["ids"] is None:
            buf[:, first:first + f["width"]] = np.nan
            g0.append(None)
        else:
            start = (rng.standard_normal((own.shape[0], f["width"])) * scale).astype(np.float32)
            buf[:, first:first + f["width"]] = start
            g0.append(start)
        t = dev(buf, device)
        gbufs.append(t)
        grads.append(t[:, first:])
    dzbuf = torch.full((B, K + 3), float("nan"), device=device)
    status = ops.new_status(device)
    dz = ops.mlr_bwd(dfields, R, dev(z32, device), dev(d_out, device), bias=bias, task=task, grads=grads, dz=dzbuf, status=status, batch=B)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(owners, snap)), "an input changed"
    got_dz = dzbuf.cpu().numpy()
    assert np.isnan(got_dz[:, K:]).all()
    worst = 0.0

    def close(got, ref, terms, what):
        nonlocal worst
        err = np.abs(np.asarray(got, dtype=np.float64) - ref)
        bar = 1e-4 * np.abs(ref) + 2e-6 * np.abs(terms) + 1e-30
        worst = max(worst, float((err / bar).max()) if err.size else 0.0)
        assert_close_terms(got, ref, terms, what=what)

    close(got_dz[:, :K], res["dz"], res["dz_terms"], "dz")
    for j, (f, (own, first)) in enumerate(zip(fields, case["owners"])):
        if j in frozen:
            continue
        got = gbufs[j].cpu().numpy()
        w = f["width"]
        pad = np.ones(own.shape[1], dtype=bool)
        pad[first:first + w] = False
        assert (got[:, pad].view(np.int32) == np.float32(SENTINEL).view(np.int32)).all(), "field %d: a column outside its range changed" % j
        mine = got[:, first:first + w]
        if f["ids"] is None:
            assert np.isfinite(mine[:B]).all()
            close(mine[:B], res["grads"][j][:B], res["grad_terms"][j][:B], "d_rows of field %d" % j)
        else:
            close(mine.astype(np.float64) - g0[j], res["grads"][j], res["grad_terms"][j] + np.abs(g0[j]), "gradient of field %d" % j)
            used = np.zeros(own.shape[0], dtype=bool)
            ok = (f["ids"] >= 0) & (f["ids"] < own.shape[0])
            used[f["ids"][ok]] = True
            assert (mine[~used].view(np.int32) == g0[j][~used].view(np.int32)).all(), "field %d: a row no id names changed" % j
    return worst, int(status.item()), dz


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("F", [1, 2, 5, 26])
def test_op_sweep_against_the_oracle(device, F, bias):
    worst, seed = 0.0, 100 * F + int(bias)
    for R in (2, 3, 4, 7, 16, 31):
        for B in (1, 5, 17, 33, 700):
            for n_dense in (0, 3):
                for i64 in (False, True):
                    seed += 1
                    task = "binary" if (seed % 3) else "regression"
                    case = RM.op_case(F, R, bias, B, n_dense, i64, seed)
                    w, st, _ = _backward(device, case, R, bias, task, B, seed)
                    assert st == 0
                    worst = max(worst, w)
    print("[mlr_bwd] F=%d bias=%d: worst err / bar %.3g" % (F, bias, worst))


def test_all_ids_equal_every_sample_adds_into_one_row(device):
    R, B = 4, 700
    case = RM.op_case(5, R, True, B, 0, False, 21)
    fields = [dict(f, ids=None if f["ids"] is None else np.full_like(f["ids"], 5)) for f in case["fields"]]
    _, st, _ = _backward(device, case, R, True, "binary", B, 21, fields=fields)
    assert st == 0


def test_frozen_field_is_left_untouched(device):
    R, B = 3, 33
    case = RM.op_case(5, R, True, B, 3, True, 22)
    _, st, _ = _backward(device, case, R, True, "regression", B, 22, frozen=(0, 1, 4))
    assert st == 0


def test_no_grads_at_all_still_writes_dz(device):
    from deepctr_amd import ops
    R, B = 4, 17
    case = RM.op_case(2, R, False, B, 0, False, 23)
    fwd = RM.mlr_op(case["fields"], B, R, False, "binary")
    z32 = fwd["z"].astype(np.float32)
    d = np.linspace(-1, 1, B).astype(np.float32)
    res = RM.mlr_op(case["fields"], B, R, False, "binary", d_out=d, z=z32)
    dfields, _ = dev_fields(case, device)
    dz = ops.mlr_bwd(dfields, R, dev(z32, device), dev(d, device), batch=B)
    assert_close_terms(dz.cpu().numpy(), res["dz"], res["dz_terms"], what="dz without grads")


def test_out_of_range_id_gets_no_gradient_and_sets_the_status_bit(device):
    R, B = 3, 33
    case = RM.op_case(5, R, True, B, 0, False, 24)
    fields = [dict(f) for f in case["fields"]]
    bad = fields[0]["ids"].copy()
    bad[17] = fields[0]["rows"].shape[0]
    bad[3] = -7
    fields[0]["ids"] = bad
    _, st, _ = _backward(device, case, R, True, "binary", B, 24, fields=fields)
    assert st & 1                                                      # DCTR_STATUS_INDEX_OOR


# ---------------------------------------------------------------------------------------------------
# the differentiable op and the model
# ---------------------------------------------------------------------------------------------------
def _small(rng, n, frozen=False):
    from deepctr_amd.feature_column import DenseFeat, SparseFeat, VarLenSparseFeat
    cols = [SparseFeat("C%d" % i, 50, 4, trainable=not (frozen and i == 2)) for i in range(5)]
    cols += [VarLenSparseFeat(SparseFeat("S", 30, 4), maxlen=4, combiner="mean"),
             VarLenSparseFeat(SparseFeat("T", 20, 4, embedding_name="C1"), maxlen=3, combiner="sum", weight_name="tw"), DenseFeat("I0", 2)]
    feed = {"C%d" % i: rng.randint(0, 50 if i != 1 else 20, n).astype(np.int32) for i in range(5)}
    cols[1] = SparseFeat("C1", 20, 4)
    feed["S"] = rng.randint(0, 30, (n, 4)).astype(np.int32)
    feed["S"][:, 0] = np.maximum(feed["S"][:, 0], 1)
    feed["T"] = rng.randint(0, 20, (n, 3)).astype(np.int32)
    feed["tw"] = rng.rand(n, 3, 1).astype(np.float32)
    feed["I0"] = rng.rand(n, 2).astype(np.float32)
    return cols, feed


def _model(device, rng, cols, task, with_bias, R=3):
    from deepctr_amd.models.mlr import MLR
    bias = [cols[0], cols[3], cols[-1]] if with_bias else None
    base = cols[1:]                                     # C0: region (+ bias) only — with a bias part the two-entry feature
    model = MLR(cols, base, region_num=R, task=task, bias_feature_columns=bias, l2_reg_linear=1e-4, seed=5, device=device)
    model.set_weights_by_name({k: (0.5 * rng.standard_normal(v.shape)).astype(np.float32) for k, v in model.get_weights_by_name().items()})
    return model


def _count_calls(monkeypatch):
    from deepctr_amd import ops
    seen = []
    real = ops.mlr_bwd
    monkeypatch.setattr(ops, "mlr_bwd", lambda *a, **k: (seen.append(1), real(*a, **k))[1])
    return seen


@pytest.mark.parametrize("task,with_bias", [("binary", True), ("regression", False), ("binary", False)])
def test_function_against_the_torch_ops_under_autograd(device, task, with_bias, monkeypatch):
    """ops.MLRFunction inside the model's autograd forward against training._mlr_output: the forward to 1e-4 / 2e-5, every gradient
    to the _normalised bar; a frozen feature's views get none."""
    from deepctr_amd import engine, training
    rng = np.random.RandomState(8)
    n = 211
    cols, feed = _small(rng, n, frozen=True)
    model = _model(device, rng, cols, task, with_bias)
    staged = engine.Staged(n)
    model._stage_inputs(feed, staged)
    frozen = training.frozen_weights(model)
    named = [(k, t) for k, t in model.named_weights() if t.data_ptr() not in frozen]
    assert not any("_C2/" in k for k, _ in named) and any("_S/" in k for k, _ in named)
    params = [t for _, t in named]
    gy = dev(rng.standard_normal(n).astype(np.float32), device)
    seen = _count_calls(monkeypatch)
    outs, grads = {}, {}
    try:
        for t in params:
            t.requires_grad_(True)
        for on in (False, True):
            monkeypatch.setattr(training, "HIP_AUTOGRAD_OPS", on)
            del seen[:]
            model._begin()
            out = training.model_logits(model, staged, 0, n, training=True)
            g = torch.autograd.grad(out, params, gy, allow_unused=True)
            assert len(seen) == int(on)
            outs[on] = out.detach().cpu().numpy()
            grads[on] = [None if t is None else t.cpu().numpy() for t in g]
        with torch.no_grad():
            ref = training._mlr_output(model, staged, 0, n, dtype=torch.float64).cpu().numpy()
    finally:
        for t in params:
            t.requires_grad_(False)
    for on in (False, True):
        assert_close(outs[on], ref, rtol=1e-4, atol=2e-5, what="forward, HIP op %s" % on)
    gmax = max(float(np.abs(g).max()) for g in grads[False] if g is not None)
    live = 0
    for (k, _), a, b in zip(named, grads[True], grads[False]):
        assert (a is None) == (b is None), k
        if a is not None:
            _normalised(a, b, gmax, "%s bias=%d: d %s" % (task, with_bias, k))
            live += float(np.abs(a).max()) > 0
    assert live >= len(named) - 2


def test_a_view_that_is_not_the_column_of_its_master_is_refused(device):
    from deepctr_amd import ops
    m = torch.randn(9, 8, device=device)
    ids = torch.zeros(4, dtype=torch.int32, device=device)
    plan = [dict(master=m, ids=ids, first=1, col0=1, width=3)]
    views = [m[:, 1 + k:2 + k] for k in range(3)]
    ok = ops.MLRFunction.inputs_of(plan, [views])
    assert ok is not None and all(a is b for a, b in zip(ok, views))
    for broken in ([views[1], views[0], views[2]], [views[0], views[1], views[2].clone()], [views[0], views[1], views[2][:8]],
                   views[:2], [m[:, k:k + 1] for k in range(3)]):
        assert ops.MLRFunction.inputs_of(plan, [broken]) is None
    assert ops.MLRFunction.inputs_of([dict(plan[0], master=m.double())], [views]) is None


@pytest.mark.parametrize("task,with_bias", [("binary", True), ("regression", False)])
def test_fit_with_the_switch_on_against_off(device, task, with_bias, monkeypatch):
    """Three batches from the same weights: the loss and every updated tensor with MLR's forward and backward on HIP against the torch
    ops."""
    from deepctr_amd import training, training_hip
    rng = np.random.RandomState(9)
    n = 768
    cols, feed = _small(rng, n)
    y = ((feed["C0"] % 2) ^ (feed["C1"] % 3 == 0)).astype(np.float32)
    if task == "regression":
        y = y + 0.1 * rng.standard_normal(n).astype(np.float32)
    seen = _count_calls(monkeypatch)
    ends, losses, w0 = {}, {}, None
    for on in (True, False):
        model = _model(device, np.random.RandomState(10), cols, task, with_bias)
        assert not training_hip.supported(model)
        w0 = model.get_weights_by_name()
        monkeypatch.setattr(training, "HIP_AUTOGRAD_OPS", on)
        del seen[:]
        model.compile("adam", "binary_crossentropy" if task == "binary" else "mse")
        hist = model.fit(feed, y, batch_size=256, epochs=1, shuffle=False, verbose=0)          # three steps
        assert len(seen) == (3 if on else 0)
        losses[on] = float(hist.history["loss"][0])
        ends[on] = model.get_weights_by_name()
    assert np.isfinite(losses[True]) and abs(losses[True] - losses[False]) <= 1e-5 * abs(losses[False])
    wmax = max(float(np.abs(ends[False][k]).max()) for k in w0)
    moved = 0
    for k in sorted(w0):
        _normalised(ends[True][k], ends[False][k], wmax, "after three steps: " + k)
        moved += not np.array_equal(ends[True][k], w0[k])
    assert moved == len(w0)


def test_default_row_threshold(device, monkeypatch):
    """training.MLR_HIP_MIN_ROWS = 0 until profiles/mlr.txt says otherwise; the mechanism is there: below it the torch ops run."""
    from deepctr_amd import engine, training
    assert training.MLR_HIP_MIN_ROWS == 0
    rng = np.random.RandomState(6)
    cols, feed = _small(rng, 32)
    model = _model(device, rng, cols, "binary", True)
    seen = _count_calls(monkeypatch)
    monkeypatch.setattr(training, "MLR_HIP_MIN_ROWS", 32)
    params = [t for k, t in model.named_weights()]
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
