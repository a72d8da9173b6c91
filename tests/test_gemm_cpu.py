"""CPU: the GEMM oracle and its guarded buffers (tests/ref_gemm.py) against numpy, dctr_sgemm_plan / dctr_gemm_k_slices against
their Python restatements, and the argument contract of dctr_sgemm_grouped (everything that returns before a device call)."""
import ctypes

import numpy as np
import pytest

from tests import ref_gemm as R


def _lib():
    import os
    from deepctr_amd import _C
    if not os.path.exists(_C.LIB_PATH):
        from deepctr_amd import build
        build.build(verbose=False)
    return _C.lib()


# ------------------------------------------------------------------------------------------------------------------------------
# the oracle and the buffers
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ta,tb", R.TRANS)
def test_oracle_matches_numpy_matmul_on_padded_offset_batched_layouts(ta, tb):
    rng = np.random.RandomState(3 + 2 * ta + tb)
    m, n, k, batch = 7, 5, 11, 3
    a = rng.standard_normal((batch, m, k))
    b = rng.standard_normal((batch, k, n))
    c = rng.standard_normal((batch, m, n))
    # by hand, without the builder: column-major with lda / ldb / ldc and batch strides, written element by element
    lda, ldb, ldc = (k if ta else m) + 2, (n if tb else k) + 1, m + 3
    sa, sb, sc = lda * (m if ta else k) + 5, ldb * (k if tb else n) + 1, ldc * n + 2
    off = (9, 2, 6)
    abuf, bbuf, cbuf = (np.full(400, np.nan, dtype=np.float32) for _ in range(3))
    for z in range(batch):
        for i in range(m):
            for kk in range(k):
                abuf[off[0] + z * sa + (kk + lda * i if ta else i + lda * kk)] = a[z, i, kk]
        for kk in range(k):
            for j in range(n):
                bbuf[off[1] + z * sb + (j + ldb * kk if tb else kk + ldb * j)] = b[z, kk, j]
        for i in range(m):
            for j in range(n):
                cbuf[off[2] + z * sc + i + ldc * j] = c[z, i, j]
    A = R.Operand(abuf, off[0], k if ta else m, m if ta else k, lda, sa, batch)
    B = R.Operand(bbuf, off[1], n if tb else k, k if tb else n, ldb, sb, batch)
    C = R.Operand(cbuf, off[2], m, n, ldc, sc, batch)
    a32, b32, c32 = (x.astype(np.float32).astype(np.float64) for x in (a, b, c))
    for beta in (0.0, 1.0):
        e = R.gemm_ref(A, B, C, ta, tb, m, n, k, batch=batch, beta=beta)
        want = a32 @ b32 + beta * c32
        mag = np.abs(a32) @ np.abs(b32) + beta * np.abs(c32)
        assert e.mask.sum() == batch * m * n
        for z in range(batch):
            for j in range(n):
                s = off[2] + z * sc + ldc * j
                assert np.array_equal(e.c[s:s + m], want[z, :, j]) and np.array_equal(e.terms[s:s + m], mag[z, :, j]) and e.mask[s:s + m].all()
                assert not e.mask[s + m:s + ldc].any() and np.isnan(e.c[s + m:s + ldc]).all()        # the row padding stays what it was
        assert np.array_equal(R.bits(e.c[~e.mask]), R.bits(cbuf[~e.mask]))
    # a broadcast operand (stride 0) is the same matrix in every batch
    B0 = R.Operand(bbuf, off[1], B.rows, B.cols, ldb, 0, batch)
    e = R.gemm_ref(A, B0, C, ta, tb, m, n, k, batch=batch)
    for z in range(batch):
        assert np.array_equal(C.view(z, e.c), a32[z] @ b32[0])


def test_oracle_slices_ones_column_and_k_zero():
    rng = np.random.RandomState(5)
    m, n, k = 6, 4, 100
    A = R.build_operand(rng, "int", m, k, ld_pad=1)
    B = R.build_operand(rng, "int", k, n - 1, ld_pad=2)                     # ones_last: n - 1 columns in memory
    a, b = A.view().astype(np.float64), np.concatenate([B.view().astype(np.float64), np.ones((k, 1))], axis=1)
    C = R.build_operand(rng, "int", m, n, ld_pad=3, count=4, stride_pad=7, fill=False)
    e = R.gemm_ref(A, B, C, 0, 0, m, n, k, ones_last=True, k_slices=4, slice_stride_c=C.stride)
    assert R.slice_chunk(k, 4) == (32, 4)                                   # 32 + 32 + 32 + 4
    for s, (k0, k1) in enumerate(((0, 32), (32, 64), (64, 96), (96, 100))):
        assert np.array_equal(C.view(s, e.c), a[:, k0:k1] @ b[k0:k1])
        assert np.array_equal(C.view(s, e.c)[:, n - 1], a[:, k0:k1].sum(1))  # the ones column: the k-sum of op(A)
    whole = R.gemm_ref(A, B, C, 0, 0, m, n, k, ones_last=True, k_slices=4, slice_stride_c=0)      # slices that add up in one C
    assert np.array_equal(C.view(0, whole.c), a @ b) and whole.mask.sum() == m * n
    with pytest.raises(AssertionError):
        R.gemm_ref(A, B, C, 0, 0, m, n, k, ones_last=True, k_slices=3, slice_stride_c=C.stride)  # 3 slices of 64 would be 2
    # k = 0: C = beta * C
    A0, B0 = R.build_operand(rng, "int", m, 0), R.build_operand(rng, "int", 0, n)
    C1 = R.build_operand(rng, "int", m, n, ld_pad=1)
    assert (R.gemm_ref(A0, B0, C1, 0, 0, m, n, 0, beta=0.0).c[C1.data_mask()] == 0).all()
    assert np.array_equal(R.gemm_ref(A0, B0, C1, 0, 0, m, n, 0, beta=1.0).c[C1.data_mask()], C1.buf[C1.data_mask()])


def test_buffer_builder_puts_nan_everywhere_but_the_data():
    rng = np.random.RandomState(6)
    for kind in R.KINDS:
        for rows, cols, pad, off, count, spad in ((5, 3, 0, 0, 1, 0), (5, 3, 2, 3, 1, 0), (4, 6, 1, 1, 3, 5), (1, 1, 4, 2, 2, 1), (0, 4, 0, 1, 1, 0)):
            x = R.build_operand(rng, kind, rows, cols, ld_pad=pad, offset=off, count=count, stride_pad=spad)
            assert x.off == R.GUARD + off and x.ld == max(rows, 1) + pad and x.stride == x.ld * cols + spad
            assert x.buf.size == R.GUARD + off + (count - 1) * x.stride + x.ld * cols + R.GUARD
            data = np.zeros(x.buf.size, dtype=bool)
            for z in range(count):
                for j in range(cols):
                    s = x.off + z * x.stride + j * x.ld
                    data[s:s + rows] = True
            assert np.array_equal(data, x.data_mask())
            assert np.isnan(x.buf[~data]).all() and not np.isnan(x.buf[data]).any()
            assert np.isnan(x.buf[:x.off]).all() and np.isnan(x.buf[-R.GUARD:]).all()
            if kind == "int":
                assert (np.abs(x.buf[data]) <= 4).all() and (x.buf[data] == np.round(x.buf[data])).all()
    c = R.build_operand(rng, "normal", 5, 3, ld_pad=1, fill=False)
    assert np.isnan(c.buf).all()
    w = R.build_operand(rng, "normal", 5, 3, count=4, broadcast=True)
    assert w.stride == 0 and w.buf.size == 2 * R.GUARD + 15 and np.array_equal(w.view(3), w.view(0))


def test_result_check_sees_one_wrong_element_a_touched_guard_and_a_nan():
    rng = np.random.RandomState(7)
    m, n, k = 9, 6, 40
    for kind in R.KINDS:
        A, B = R.build_operand(rng, kind, m, k, ld_pad=1), R.build_operand(rng, kind, k, n)
        C = R.build_operand(rng, kind, m, n, ld_pad=2, offset=1, fill=False)
        e = R.gemm_ref(A, B, C, 0, 0, m, n, k)
        good = np.where(e.mask, e.c, C.buf).astype(np.float32)
        R.check_result(good, C.buf, e, kind)
        inside, pad = C.off + 3 + 2 * C.ld, C.off + m + 2 * C.ld
        assert e.mask[inside] and not e.mask[pad]
        for at, val in ((inside, good[inside] + (1.0 if kind == "int" else 1e-3 * e.terms[inside])), (pad, 0.0), (3, 0.0), (inside, np.nan)):
            bad = good.copy()
            bad[at] = val
            with pytest.raises(AssertionError):
                R.check_result(bad, C.buf, e, kind)
    # one term of ordinary size left out of one output: the integer data sees it whatever its size
    A, B = R.build_operand(rng, "int", m, k), R.build_operand(rng, "int", k, n)
    A.view()[3, 7], B.view()[7, 2] = 1.0, -1.0
    C = R.build_operand(rng, "int", m, n, fill=False)
    e = R.gemm_ref(A, B, C, 0, 0, m, n, k)
    dropped = np.where(e.mask, e.c, C.buf).astype(np.float32)
    dropped[C.off + 3 + 2 * C.ld] += 1.0
    with pytest.raises(AssertionError):
        R.check_result(dropped, C.buf, e, "int")


def test_case_tables_reach_what_they_are_for():
    # (the route of every GPU case is asserted there through dctr_sgemm_plan; this is the arithmetic behind the shapes, at 256 CUs)
    assert len(set(R.EDGE_MN)) == 24 and {m for m, _ in R.EDGE_MN} == {n for _, n in R.EDGE_MN} == set(R.EDGES)
    assert {R.ceil_div(k, 16) for k in R.K_DEPTH} == {0, 1, 2, 3, 4, 5} and {k % 4 for k in R.K_DEPTH} == {0, 1, 2, 3}
    assert len(set(R.OFFSETS)) == 16 and {o[:2] for o in R.OFFSETS} == {(a, b) for a in range(4) for b in range(4)}
    assert all({o[i] for o in R.OFFSETS} == {0, 1, 2, 3} for i in range(3))
    for m, n in R.EDGE_MN + R.K_DEPTH_MN:
        assert R.plan(m, n, 65, 1, 256) == (64, 1, 65)
    for k in R.SPLIT_K:
        for m, n in R.SPLIT_MN:
            for batch in (1, 2, 3):
                tile, slices, chunk = R.plan(m, n, k, batch, 256)
                assert tile == 64 and slices > 1 and chunk % 32 == 0 and (slices - 1) * chunk < k <= slices * chunk
    assert R.plan(5, 7, 1025, 1, 256) == (64, 4, 288)         # 288 + 288 + 288 + 161: a short last slice
    assert R.plan(5, 7, 8193, 1, 256) == (64, 29, 288)        # 32 wanted; 32 slices of 288 would leave three empty
    for m, n in R.TILE128_MN:
        per = R.ceil_div(m, 128) * R.ceil_div(n, 128)
        assert R.plan(m, n, 16, 512 // per, 256)[0] == 128 and R.plan(m, n, 16, 512 // per - 1, 256)[0] == 64
    table = R.grouped_table()
    assert len(table) == R.MAX_GROUPS and [i for i, g in enumerate(table) if g["m"] == 0] == [3, 7]
    rng = np.random.RandomState(0)
    calls = [R.build_group(rng, "int", g)[3] for g in table]
    assert [c["k_slices"] for c in calls] == [1, 1, 4, 1, 5, 3, 1, 1]
    assert any(c["ones_last"] and c["k_slices"] > 1 for c in calls) and any(c["batch"] > 1 and c["slice_stride_c"] for c in calls)
    assert any(c["accumulate"] and c["k_slices"] > 1 and c["slice_stride_c"] == 0 for c in calls)
    assert len({(c["trans_a"], c["trans_b"]) for c in calls if c["m"]}) == 4


# ------------------------------------------------------------------------------------------------------------------------------
# the library's host side
# ------------------------------------------------------------------------------------------------------------------------------
def _plan(lib, m, n, k, batch, cus):
    t, s, c = (ctypes.c_int32(-1) for _ in range(3))
    assert lib.dctr_sgemm_plan(m, n, k, batch, cus, ctypes.byref(t), ctypes.byref(s), ctypes.byref(c)) == 0, lib.dctr_last_error()
    return t.value, s.value, c.value


@pytest.mark.parametrize("cus", [256, 80, 1])
def test_sgemm_plan_equals_its_restatement(cus):
    lib = _lib()
    dims = (0, 1, 5, 64, 65, 127, 128, 129, 130, 429, 1000, 4096, 70000)
    ks = (0, 1, 16, 255, 256, 1023, 1024, 1025, 2049, 4096, 8193, 16384, 100000)
    seen = set()
    for m in dims:
        for n in dims:
            for k in ks:
                for batch in (0, 1, 2, 3, 37, 512):
                    got = _plan(lib, m, n, k, batch, cus)
                    assert got == R.plan(m, n, k, batch, cus), (m, n, k, batch, cus, got)
                    seen.add((got[0], got[1] > 1))
    assert seen == {(64, False), (64, True), (128, False)} if cus > 1 else (64, True) not in seen


def test_sgemm_plan_of_the_deepfm_step_and_its_argument_errors():
    """DESIGN.md's DeepFM step (DNN 429 -> 256 -> 128 -> 64): the dW products at B = 4096 and B = 16,384 on 256 CUs, worked out by
    hand from the launcher's rule as it stood before the plan query existed."""
    lib = _lib()
    # dW0 (429 x 256, reduction B): 4 x 2 = 8 tiles of 128 < 512 -> 64 tiling, 7 x 4 = 28 tiles, 2 * 28 <= 256, want = min(512 / 28, B / 256, 32)
    assert _plan(lib, 429, 256, 4096, 1, 256) == (64, 16, 256)         # min(18, 16, 32) = 16 slices of 256
    assert _plan(lib, 429, 256, 16384, 1, 256) == (64, 18, 928)        # min(18, 64, 32) = 18: ceil(911 / 32) * 32 = 928, ceil(16384 / 928) = 18
    assert _plan(lib, 256, 128, 4096, 1, 256) == (64, 16, 256)         # 8 tiles: min(64, 16, 32)
    assert _plan(lib, 128, 64, 16384, 1, 256) == (64, 32, 512)         # 2 tiles: min(256, 64, 32)
    # dH = dZ W^T (429 x B, k = 256): 4 x 32 = 128 tiles of 128 at B = 4096 (64 tiling, no split), 512 at B = 16,384 (128 tiling)
    assert _plan(lib, 429, 4096, 256, 1, 256) == (64, 1, 256)
    assert _plan(lib, 429, 16384, 256, 1, 256) == (128, 1, 256)
    t = ctypes.c_int32()
    assert lib.dctr_sgemm_plan(-1, 4, 4, 1, 256, ctypes.byref(t), ctypes.byref(t), ctypes.byref(t)) == -2
    assert lib.dctr_sgemm_plan(4, 4, 4, 1, -3, ctypes.byref(t), ctypes.byref(t), ctypes.byref(t)) == -2
    assert lib.dctr_sgemm_plan(4, 4, 4, 1, 256, None, ctypes.byref(t), ctypes.byref(t)) == -1


def test_k_slices_equals_its_restatement():
    lib = _lib()
    for rows in (0, 1, 32, 64, 100, 128, 256, 512, 4096):
        for k in list(range(0, 70)) + [127, 128, 129, 255, 256, 257, 513, 1000, 1024, 1025, 4097, 8193, 16384, 100001]:
            got = lib.dctr_gemm_k_slices(k, rows)
            assert got == R.k_slices(k, rows), (k, rows, got)
            assert 1 <= got <= 32 and (k == 0 or R.slice_chunk(k, got)[1] == got)      # a count the grouped call accepts
    assert [lib.dctr_gemm_k_slices(b, 256) for b in (256, 257, 513, 4097, 8193)] == [1, 2, 3, 17, 29]
    assert lib.dctr_gemm_k_slices(-5, 256) == 1


def test_group_mirror_has_the_layout_the_c_compiler_gives_the_header(tmp_path):
    import os
    import shutil
    import subprocess
    from deepctr_amd import _C
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    cls = _C.gemm.Group
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dctr.h"', "int main(void) {",
             '    printf("sizeof %zu\\n", sizeof(dctr_gemm_group_t));']
    for fname, _ in cls._fields_:
        lines.append('    printf("%s %%zu\\n", offsetof(dctr_gemm_group_t, %s));' % (fname, fname))
    lines += ["    return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    seen = 0
    for line in filter(None, out):
        field, val = line.split()
        want = ctypes.sizeof(cls) if field == "sizeof" else getattr(cls, field).offset
        assert int(val) == want, "dctr_gemm_group_t.%s: C says %s, ctypes %d" % (field, val, want)
        seen += 1
    assert seen == len(cls._fields_) + 1 and ctypes.sizeof(cls) == 3 * 8 + 4 * 8 + 12 * 4


def test_sgemm_grouped_argument_errors_are_reported_without_a_gpu():
    """Everything dctr_sgemm_grouped answers before a device call; the pointers are never dereferenced."""
    from deepctr_amd import _C
    lib = _lib()
    fake = 4096

    def group(**kw):
        f = dict(A=fake, B=fake, C=fake, trans_a=0, trans_b=0, m=8, n=8, k=8, lda=8, ldb=8, ldc=8, batch=1)
        f.update(kw)
        return _C.gemm.Group(**f)

    def call(*gs, n=None):
        arr = (_C.gemm.Group * max(len(gs), 1))(*gs)
        return lib.dctr_sgemm_grouped(arr, len(gs) if n is None else n, None)

    empty = group(m=0)
    assert call(empty, n=0) == -2 and b"groups" in lib.dctr_last_error()
    assert call(*[empty] * 9) == -2                                            # more than 8
    assert lib.dctr_sgemm_grouped(None, 1, None) == -1
    assert call(*[empty] * 8) == 0 and call(group(n=0), group(batch=0)) == 0  # nothing to launch
    for bad in (dict(m=-1, ldc=8), dict(n=-1), dict(k=-1), dict(batch=-1)):
        assert call(empty, group(**bad)) == -2, bad
    assert call(group(ldc=7)) == -2 and call(group(lda=0)) == -2 and call(group(ldb=0)) == -2
    for ptr in ("A", "B", "C"):
        assert call(empty, group(**{ptr: None})) == -1 and b"null" in lib.dctr_last_error()
    assert call(group(A=None, B=None, C=None, n=0)) == 0                       # an empty group needs no pointers
    # k_slices: the count must be what the slicing rule gives for k
    assert lib.dctr_gemm_k_slices(1000, 256) == 4
    assert call(group(k=1000, k_slices=9, slice_stride_c=64)) == -2 and b"slices" in lib.dctr_last_error()   # ceil(112 / 32) * 32 = 128 -> 8 slices
    assert call(group(k=100, k_slices=3, slice_stride_c=64)) == -2             # ceil(34 / 32) * 32 = 64 -> 2 slices
    assert call(group(k=100, k_slices=33, slice_stride_c=64)) == -2            # chunk 32 -> 4 slices
    # stored slices need their own C each and no accumulate; atomically added slices need accumulate
    assert call(group(k=1000, k_slices=4, slice_stride_c=0, accumulate=0)) == _C.E_UNSUPPORTED
    assert call(group(k=1000, k_slices=4, slice_stride_c=64, accumulate=1)) == _C.E_UNSUPPORTED
    assert b"k_slices" in lib.dctr_last_error()
