"""GPU: the training GEMM (deepctr_amd/csrc/gemm_kernels.hip) through the C ABI on raw pointers, against the float64 oracle of
tests/ref_gemm.py — every tiling (64 x 64, 64 x 64 with the reduction split, 128 x 128), padded leading dimensions, pointers 0 - 3
floats off a 16-byte boundary, batch strides, transposes, beta 0 / 1, and the grouped launch.

Every run asserts: the route dctr_sgemm_plan reports is the one the case is for; the m x n window is bit-equal to the exact product
(integer data) / within 2e-6 of the summed magnitude (normal data) and holds no NaN; every other float of the C allocation, and
both inputs, are bit for bit what they were (the guards and paddings hold NaN, so a load that is not masked shows in the result)."""
import ctypes
import itertools

import numpy as np
import pytest

from tests import ref_gemm as R

pytestmark = pytest.mark.gpu

NO_SPLIT, SPLIT = False, True


def _lib():
    from deepctr_amd import _C
    return _C.lib()


def _plan(m, n, k, batch):
    lib = _lib()
    t, s, c = (ctypes.c_int32(-1) for _ in range(3))
    assert lib.dctr_sgemm_plan(m, n, k, batch, 0, ctypes.byref(t), ctypes.byref(s), ctypes.byref(c)) == 0, lib.dctr_last_error()
    return t.value, s.value, c.value


def _upload(device, x):
    import torch
    t = torch.from_numpy(x.buf).to(device)
    assert t.data_ptr() % 16 == 0                      # so that the data's alignment is the operand's offset alone
    return t, t.data_ptr() + 4 * x.off


def _stride_pad(rows, cols, ld_pad):
    """A gap between batches that leaves the batch stride no multiple of 4."""
    per = (max(rows, 1) + ld_pad) * cols
    return 5 if (per + 5) % 4 else 6


def run_sgemm(device, rng, kind, ta, tb, m, n, k, beta, route, pads=(0, 0, 0), offs=(0, 0, 0), batch=1, gaps=False, broadcast=None):
    """One dctr_sgemm call on fresh guarded buffers, checked.  gaps: batch strides larger than the matrices and no multiple of 4;
    broadcast: "a" / "b" — that operand is one matrix with batch stride 0."""
    import torch
    from deepctr_amd import _C
    lib = _lib()
    what = "%s ta=%d tb=%d m=%d n=%d k=%d beta=%g batch=%d pads=%s offs=%s gaps=%s broadcast=%s" % (kind, ta, tb, m, n, k, beta, batch, pads, offs, gaps, broadcast)
    shape_a, shape_b = ((k, m) if ta else (m, k)), ((n, k) if tb else (k, n))
    sp = [_stride_pad(r, c, p) if gaps else 0 for (r, c), p in zip((shape_a, shape_b, (m, n)), pads)]
    A = R.build_operand(rng, kind, *shape_a, ld_pad=pads[0], offset=offs[0], count=batch, stride_pad=sp[0], broadcast=broadcast == "a")
    B = R.build_operand(rng, kind, *shape_b, ld_pad=pads[1], offset=offs[1], count=batch, stride_pad=sp[1], broadcast=broadcast == "b")
    C = R.build_operand(rng, kind, m, n, ld_pad=pads[2], offset=offs[2], count=batch, stride_pad=sp[2], fill=beta == 1.0)
    if gaps and batch > 1:
        assert all(x.stride % 4 != 0 for x in (A, B, C) if x.stride)
    exp = R.gemm_ref(A, B, C, ta, tb, m, n, k, batch=batch, beta=beta)
    tile, slices, _ = _plan(m, n, k, batch)
    assert (tile, slices > 1) == route, "%s: planned tile %d, %d slices; the case is for tile %d, split %s" % (what, tile, slices, route[0], route[1])
    (ta_, pa), (tb_, pb), (tc_, pc) = (_upload(device, x) for x in (A, B, C))
    rc = lib.dctr_sgemm(ta, tb, m, n, k, pa, A.ld, A.stride, pb, B.ld, B.stride, beta, pc, C.ld, C.stride, batch, _C.stream_ptr())
    assert rc == 0, (what, lib.dctr_last_error())
    torch.cuda.synchronize()
    worst = R.check_result(tc_.cpu().numpy(), C.buf, exp, kind, what)
    R.check_untouched(ta_.cpu().numpy(), A.buf, what + ": A")
    R.check_untouched(tb_.cpu().numpy(), B.buf, what + ": B")
    return worst


def all_forms(seed, kinds=R.KINDS):
    """(rng, kind, ta, tb, beta, i): both data kinds x the four transposes x beta 0 / 1, with i in 0 .. 3 such that a case which
    rotates its layouts by i gives every transpose four different ones over the two kinds."""
    rng = np.random.RandomState(seed)
    for kind in kinds:
        ki = R.KINDS.index(kind)
        for ti, (ta, tb) in enumerate(R.TRANS):
            for bi, beta in enumerate((0.0, 1.0)):
                yield rng, kind, ta, tb, beta, (ti + bi + 2 * ki) % 4


# ------------------------------------------------------------------------------------------------------------------------------
# 64 x 64 tiles, one slice
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", R.EDGE_MN)
def test_tile64_edges(device, m, n):
    for rng, kind, ta, tb, beta, _ in all_forms(1000 * m + n):
        run_sgemm(device, rng, kind, ta, tb, m, n, 37, beta, (64, NO_SPLIT))


@pytest.mark.parametrize("k", R.K_DEPTH)
@pytest.mark.parametrize("m,n", R.K_DEPTH_MN)
def test_tile64_pipeline_depth_and_k_tail(device, m, n, k):
    """0 - 5 k-blocks through the registers -> LDS -> MFMA pipeline and every tail length.  k = 0 is C = beta * C: zeros over a
    NaN-filled C with beta = 0 (the oracle's product of an m x 0 and a 0 x n matrix), C unchanged with beta = 1."""
    for rng, kind, ta, tb, beta, i in all_forms(100 * k + m):
        run_sgemm(device, rng, kind, ta, tb, m, n, k, beta, (64, NO_SPLIT))
        run_sgemm(device, rng, kind, ta, tb, m, n, k, beta, (64, NO_SPLIT), pads=(4, 4, 4))
        # every leading dimension a multiple of 4: the 16-byte loads, whose last one along k must fall back to single floats when
        # k % 4 != 0 (what lies behind a row's k is NaN padding)
        rows = (k if ta else m, n if tb else k, m)
        run_sgemm(device, rng, kind, ta, tb, m, n, k, beta, (64, NO_SPLIT), pads=tuple(-r % 4 for r in rows))


@pytest.mark.parametrize("pad", R.LD_PADS)
@pytest.mark.parametrize("m,n,k", R.LAYOUT_SHAPES)
def test_tile64_leading_dimensions_and_pointer_offsets(device, m, n, k, pad):
    """lda / ldb / ldc tight, + 1, + 3, + 4 against A, B, C each 0 - 3 floats off a 16-byte boundary: the 16-byte load path and the
    scalar path with either, both or neither operand on it."""
    for rng, kind, ta, tb, beta, _ in all_forms(10 * m + pad):
        for offs in R.OFFSETS:
            run_sgemm(device, rng, kind, ta, tb, m, n, k, beta, (64, NO_SPLIT), pads=(pad, pad, pad), offs=offs)


@pytest.mark.parametrize("m,n,k", R.LAYOUT_SHAPES)
def test_tile64_mixed_leading_dimensions(device, m, n, k):
    for rng, kind, ta, tb, beta, _ in all_forms(10 * m + 7):
        for pads in itertools.permutations((0, 3, 4)):
            run_sgemm(device, rng, kind, ta, tb, m, n, k, beta, (64, NO_SPLIT), pads=pads, offs=(0, 0, 0))


@pytest.mark.parametrize("batch", [3, 5])
@pytest.mark.parametrize("m,n,k", R.LAYOUT_SHAPES)
def test_tile64_batch_strides_and_broadcast_operands(device, m, n, k, batch):
    for rng, kind, ta, tb, beta, i in all_forms(10 * m + batch):
        pads, offs = R.ROTATING_LAYOUTS[i]
        run_sgemm(device, rng, kind, ta, tb, m, n, k, beta, (64, NO_SPLIT), pads=pads, offs=offs, batch=batch, gaps=True)
        for w in ("a", "b"):                           # a weight shared by every batch: stride 0
            run_sgemm(device, rng, kind, ta, tb, m, n, k, beta, (64, NO_SPLIT), pads=pads, offs=offs, batch=batch, gaps=True, broadcast=w)


# ------------------------------------------------------------------------------------------------------------------------------
# 64 x 64 tiles, the reduction split over workgroups (float atomics into C; C cleared first with beta = 0)
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", R.SPLIT_K)
@pytest.mark.parametrize("m,n", R.SPLIT_MN)
def test_tile64_split_k(device, m, n, k):
    """k = 1025: a short last slice; k = 8193: the slice count is lowered so that none is empty.  ldc is padded in three of four
    runs (the clear may touch the m x n window only), beta = 1 adds to what is there, batch 2 and 3 use blockIdx.z = batch x slice."""
    for batch in (1, 2, 3):
        for rng, kind, ta, tb, beta, i in all_forms(k + 10 * m + batch):
            pads, offs = R.ROTATING_LAYOUTS[(i + 1) % 4]
            run_sgemm(device, rng, kind, ta, tb, m, n, k, beta, (64, SPLIT), pads=pads, offs=offs, batch=batch, gaps=batch > 1)


# ------------------------------------------------------------------------------------------------------------------------------
# 128 x 128 tiles
# ------------------------------------------------------------------------------------------------------------------------------
def _smallest(pred, hi):
    for v in range(1, hi + 1):
        if pred(v):
            return v
    raise AssertionError("nothing up to %d reaches the 128 x 128 tiling" % hi)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("k", R.TILE128_K)
@pytest.mark.parametrize("m,n", R.TILE128_MN)
def test_tile128_batched(device, m, n, k, kind):
    """The smallest batch at which the launcher takes 128 x 128 tiles on this part (512 tiles on an MI355X: batch 256 / 256 / 512)."""
    batch = _smallest(lambda b: _plan(m, n, k, b)[0] == 128, 4096)
    assert _plan(m, n, k, batch - 1)[0] == 64
    for rng, kind, ta, tb, beta, i in all_forms(k + 10 * m, (kind,)):
        pads, offs = R.ROTATING_LAYOUTS[i]
        run_sgemm(device, rng, kind, ta, tb, m, n, k, beta, (128, NO_SPLIT), pads=pads, offs=offs, batch=batch, gaps=i % 2 == 1)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("k", R.FLAT_K)
@pytest.mark.parametrize("m", R.FLAT_SMALL)
def test_tile128_flat(device, m, k, kind):
    """dH = dZ W^T of a large batch: one long dimension, the smallest count of 128-row tiles that reaches the 128 x 128 tiling on
    this part, the last of them ragged (37 rows)."""
    rows = lambda t: (t - 1) * 128 + 37
    t = _smallest(lambda t: _plan(m, rows(t), k, 1)[0] == 128, 65535)
    n = rows(t)
    assert _plan(m, n - 37, k, 1)[0] == 64               # one tile row fewer stays on 64 x 64
    for rng, kind, ta, tb, beta, i in all_forms(k + m, (kind,)):
        pads, offs = R.ROTATING_LAYOUTS[i]
        run_sgemm(device, rng, kind, ta, tb, m, n, k, beta, (128, NO_SPLIT), pads=pads, offs=offs)


def test_the_tables_take_all_three_routes(device):
    """The three routes of dctr_sgemm on this part, each from the table that is there for it (every case above asserts its own)."""
    def route(m, n, k, batch):
        tile, slices, _ = _plan(m, n, k, batch)
        return tile, slices > 1

    assert {route(m, n, 37, 1) for m, n in R.EDGE_MN} == {(64, NO_SPLIT)}
    assert {route(m, n, k, b) for (m, n), k, b in itertools.product(R.SPLIT_MN, R.SPLIT_K, (1, 2, 3))} == {(64, SPLIT)}
    batches = [_smallest(lambda b: _plan(m, n, 16, b)[0] == 128, 4096) for m, n in R.TILE128_MN]
    assert {route(m, n, 16, b) for (m, n), b in zip(R.TILE128_MN, batches)} == {(128, NO_SPLIT)}
    print("dctr_sgemm routes on this part: 64, 64 + split (%s), 128 from batch %s" % (
        sorted({_plan(m, n, k, 1)[1] for (m, n), k in itertools.product(R.SPLIT_MN, R.SPLIT_K)}), batches))


# ------------------------------------------------------------------------------------------------------------------------------
# the grouped launch
# ------------------------------------------------------------------------------------------------------------------------------
def run_grouped(device, kind, n_groups, seed):
    """The first n_groups entries of ref_gemm.grouped_table() in ONE dctr_sgemm_grouped launch, every group checked against its
    oracle (a stored slice against the product of its own k range).  Returns [(call, C, downloaded C buffer)]."""
    import torch
    from deepctr_amd import _C
    lib = _lib()
    rng = np.random.RandomState(seed)
    built = [R.build_group(rng, kind, g) for g in R.grouped_table()[:n_groups]]
    arr = (_C.gemm.Group * n_groups)()
    keep = []
    for i, (A, B, C, call) in enumerate(built):
        for f in ("trans_a", "trans_b", "m", "n", "k", "lda", "ldb", "ldc", "batch", "stride_a", "stride_b", "stride_c", "slice_stride_c",
                  "ones_last", "accumulate", "k_slices"):
            setattr(arr[i], f, call[f])
        if "rows_per_slice" in R.grouped_table()[i]:
            assert lib.dctr_gemm_k_slices(call["k"], R.grouped_table()[i]["rows_per_slice"]) == call["k_slices"] > 1
        if call["m"] == 0:                                  # an empty group: skipped, its pointers are never looked at
            keep.append(None)
            continue
        ups = [_upload(device, x) for x in (A, B, C)]
        arr[i].A, arr[i].B, arr[i].C = (p for _, p in ups)
        keep.append(ups)
    rc = lib.dctr_sgemm_grouped(arr, n_groups, _C.stream_ptr())
    assert rc == 0, lib.dctr_last_error()
    torch.cuda.synchronize()
    out = []
    for i, ((A, B, C, call), ups) in enumerate(zip(built, keep)):
        if ups is None:
            out.append((call, C, None))
            continue
        what = "%s, %d groups, group %d" % (kind, n_groups, i)
        got = ups[2][0].cpu().numpy()
        exp = R.gemm_ref(A, B, C, **call["ref"])
        R.check_result(got, C.buf, exp, kind, what)
        R.check_untouched(ups[0][0].cpu().numpy(), A.buf, what + ": A")
        R.check_untouched(ups[1][0].cpu().numpy(), B.buf, what + ": B")
        if call["slice_stride_c"]:                          # the caller's sum over the stored slices is the whole product
            whole = zip(R.slice_sum(got, C, call), R.slice_sum(exp.c, C, call), R.slice_sum(exp.terms, C, call))
            for b, (s, want, terms) in enumerate(whole):
                err = np.abs(s - want)
                assert (err == 0).all() if kind == "int" else (err <= R.RTOL_TERMS * terms + 1e-30).all(), "%s: sum of the slices, batch %d" % (what, b)
        if call["ones_last"]:                               # the last output column is the k-sum of op(A), whatever op(B) holds
            for s in range(call["k_slices"] if call["slice_stride_c"] else 1):
                col = R.window(got, C.off + s * call["slice_stride_c"], call["m"], call["n"], C.ld)[:, -1]
                assert not np.isnan(col).any(), what
        out.append((call, C, got))
    return out


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("n_groups", [1, 2, 3, 8])
def test_grouped_launch_at_several_group_counts(device, kind, n_groups):
    """The walk from workgroup to (group, tile, batch, slice) at 1, 2, 3 and 8 groups; the full table has empty groups in the middle
    and at the end, ones_last with and without slices, slices stored per k range, slices added atomically to a filled C, and a
    batch together with slices."""
    run_grouped(device, kind, n_groups, seed=40 + n_groups)


def test_grouped_stored_slices_give_the_same_bits_twice(device):
    """The stored-slice form has no atomics: two launches give the same bits (the BiLSTM backward relies on it)."""
    first, second = (run_grouped(device, "normal", 8, seed=77) for _ in range(2))
    seen = 0
    for (call, _, a), (_, _, b) in zip(first, second):
        if a is not None and call["slice_stride_c"]:
            assert np.array_equal(R.bits(a), R.bits(b))
            seen += 1
    assert seen == 2
