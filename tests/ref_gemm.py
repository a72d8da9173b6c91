"""float64 oracle, guarded buffers and case tables for the training GEMM (deepctr_amd/csrc/gemm_kernels.hip: dctr_sgemm,
dctr_sgemm_grouped) — numpy only, no GPU and no torch.

The oracle takes what the C ABI takes: flat float32 buffers, element offsets, column-major leading dimensions, batch strides.
It returns the whole expected C buffer, so that a test compares the window the call may write with the product and everything
else (row padding, guards, the gaps between batches) bit for bit with what was there before.

Every operand sits inside a larger allocation whose guards and padding hold NaN: a load that is not masked drags a NaN into
the result (NaN * 0 is NaN), a store outside the window changes a guard, and nothing leaves memory the test owns.
"""
import numpy as np

RTOL_TERMS = 2e-6        # tests.util.assert_close_terms' rtol_terms: the bar of tests/test_gpu_train.py::test_own_sgemm_matches_float64
GUARD = 64               # floats of NaN before and after every operand (a multiple of 4: the data's alignment is its offset alone)
MAX_GROUPS = 8
KINDS = ("int", "normal")
TRANS = ((0, 0), (0, 1), (1, 0), (1, 1))


def ceil_div(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------------------------------
# the launcher's rules, restated
# ------------------------------------------------------------------------------------------------------------------------------
def plan(m, n, k, batch, n_cus):
    """(tile, k_slices, k_chunk) of a dctr_sgemm call on a part with n_cus compute units (gemm_kernels.hip: dctr_sgemm_plan)."""
    if m == 0 or n == 0 or batch == 0:
        return 64, 1, k
    t128 = ceil_div(m, 128) * ceil_div(n, 128) * batch
    tile = 64 if t128 < 2 * n_cus else 128
    tiles = ceil_div(m, tile) * ceil_div(n, tile) * batch
    want = 1
    if tiles * 2 <= n_cus and k >= 1024:
        want = max(1, min(2 * n_cus // tiles, k // 256, 32))
    if want == 1:
        return tile, 1, k
    chunk = ceil_div(ceil_div(k, want), 32) * 32
    return tile, ceil_div(k, chunk), chunk


def slice_chunk(k, slices):
    """(chunk, slices the chunk gives) for a reduction cut into `slices`: chunk = ceil(ceil(k / s) / 32) * 32, ceil(k / chunk)."""
    chunk = ceil_div(ceil_div(k, slices), 32) * 32
    return chunk, ceil_div(k, chunk)


def k_slices(k, rows_per_slice):
    """gemm_kernels.hip: dctr_gemm::k_slices (dctr_gemm_k_slices)."""
    if k <= 0:
        return 1
    want = max(1, min(32, ceil_div(k, rows_per_slice if rows_per_slice > 0 else k)))
    return slice_chunk(k, want)[1]


# ------------------------------------------------------------------------------------------------------------------------------
# buffers
# ------------------------------------------------------------------------------------------------------------------------------
class Operand(object):
    """A column-major matrix (or `count` of them `stride` elements apart) inside a NaN-guarded float32 allocation.
    buf: the allocation; off: element offset of the first matrix; rows x cols with leading dimension ld."""

    def __init__(self, buf, off, rows, cols, ld, stride, count):
        self.buf, self.off, self.rows, self.cols, self.ld, self.stride, self.count = buf, off, rows, cols, ld, stride, count

    def view(self, i=0, buf=None):
        return window(self.buf if buf is None else buf, self.off + i * self.stride, self.rows, self.cols, self.ld)

    def data_mask(self):
        mask = np.zeros(self.buf.shape, dtype=bool)
        for i in range(self.count):
            self.view(i, mask)[...] = True
        return mask


def window(buf, off, rows, cols, ld):
    """rows x cols view of the column-major matrix at buf[off] with leading dimension ld (no copy; writes go to buf)."""
    if rows == 0 or cols == 0:
        return np.zeros((rows, cols), dtype=buf.dtype)
    assert off >= 0 and ld >= rows and off + (cols - 1) * ld + rows <= buf.size, (off, rows, cols, ld, buf.size)
    return np.lib.stride_tricks.as_strided(buf[off:], shape=(rows, cols), strides=(buf.itemsize, ld * buf.itemsize))


def draw(rng, kind, shape):
    if kind == "int":            # products and partial sums of these are exact in fp32 for k * 16 < 2^24: any summation order gives the same bits
        return rng.randint(-4, 5, size=shape).astype(np.float32)
    assert kind == "normal"
    return rng.standard_normal(shape).astype(np.float32)


def build_operand(rng, kind, rows, cols, ld_pad=0, offset=0, count=1, stride_pad=0, broadcast=False, fill=True, tail=0):
    """`count` rows x cols matrices, leading dimension max(rows, 1) + ld_pad, the first one `offset` (0 - 3) floats past a 16-byte
    boundary of the allocation, consecutive ones (ld * cols + stride_pad) apart — or all the same one (stride 0) with broadcast.
    Guards, row padding and the gaps between matrices hold NaN; so does the data itself with fill=False (a C that beta = 0 may
    not read).  tail: that many more NaN floats behind the last matrix (the column an operand with ones_last does not have)."""
    assert 0 <= offset < 4 and GUARD % 4 == 0
    ld = max(rows, 1) + ld_pad
    per = ld * cols
    stride = 0 if broadcast else per + stride_pad
    stored = 1 if broadcast else count
    buf = np.full(GUARD + offset + (stored - 1) * stride + per + tail + GUARD, np.nan, dtype=np.float32)
    op = Operand(buf, GUARD + offset, rows, cols, ld, stride, stored)
    if fill:
        data = draw(rng, kind, (stored, cols, rows))
        for i in range(stored):
            op.view(i)[...] = data[i].T
    op.count = count
    return op


# ------------------------------------------------------------------------------------------------------------------------------
# the oracle
# ------------------------------------------------------------------------------------------------------------------------------
def op_matrix(x, trans, rows, cols, i=0):
    """float64 op(X) (rows x cols) of matrix i of operand x, which stores cols x rows when trans."""
    r, c = (cols, rows) if trans else (rows, cols)
    v = window(x.buf, x.off + i * x.stride, r, c, x.ld).astype(np.float64)
    return v.T if trans else v


class Expected(object):
    """c: the expected C buffer in float64 (everything outside `mask` is what the buffer held before the call);
    terms: sum |a| |b| (+ |c| with beta = 1) inside mask, 0 outside; mask: what the call may write."""

    def __init__(self, c, terms, mask):
        self.c, self.terms, self.mask = c, terms, mask


def gemm_ref(A, B, C, trans_a, trans_b, m, n, k, batch=1, beta=0.0, stride_c=None, ones_last=False, k_slices=1, slice_stride_c=0):
    """C (m x n, ldc) = op(A) (m x k) op(B) (k x n) + beta C per batch, as dctr_sgemm / one group of dctr_sgemm_grouped define it.
    ones_last: op(B) has n - 1 columns in memory and a column of ones behind them.  k_slices > 1 with slice_stride_c != 0: slice
    s of the reduction, k in [s chunk, (s + 1) chunk) with chunk = ceil(ceil(k / k_slices) / 32) * 32, is stored on its own at
    C + s * slice_stride_c; any other k_slices does not change what is computed (the slices add up in C)."""
    assert beta in (0.0, 1.0)
    stride_c = C.stride if stride_c is None else stride_c
    exp = C.buf.astype(np.float64)
    terms = np.zeros(C.buf.shape, dtype=np.float64)
    mask = np.zeros(C.buf.shape, dtype=bool)
    ranges = [(0, k)]
    if k_slices > 1 and k > 0:
        chunk, got = slice_chunk(k, k_slices)
        assert got == k_slices, "k = %d does not cut into %d slices (chunk %d gives %d)" % (k, k_slices, chunk, got)
        if slice_stride_c != 0:
            assert beta == 0.0
            ranges = [(s * chunk, min(k, (s + 1) * chunk)) for s in range(k_slices)]
    for b in range(batch):
        a = op_matrix(A, trans_a, m, k, b)
        bm = op_matrix(B, trans_b, k, n - 1 if ones_last else n, b)
        if ones_last:
            bm = np.concatenate([bm, np.ones((k, 1))], axis=1)
        for s, (k0, k1) in enumerate(ranges):
            off = C.off + b * stride_c + s * slice_stride_c
            prod = a[:, k0:k1] @ bm[k0:k1]
            mag = np.abs(a[:, k0:k1]) @ np.abs(bm[k0:k1])
            if beta == 1.0:
                c0 = window(C.buf, off, m, n, C.ld).astype(np.float64)
                prod, mag = prod + c0, mag + np.abs(c0)
            if m and n:
                assert not window(mask, off, m, n, C.ld).any(), "C windows overlap"
                window(exp, off, m, n, C.ld)[...] = prod
                window(terms, off, m, n, C.ld)[...] = mag
                window(mask, off, m, n, C.ld)[...] = True
    return Expected(exp, terms, mask)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def check_result(got, before, exp, kind, what=""):
    """The three assertions on a C buffer after the call: nothing outside the window changed (bit for bit, NaN guards included),
    no NaN inside it, and the window is bit-equal to the oracle (int data) / within 2e-6 of the summed magnitude (normal data).
    Returns the worst err / bar."""
    got = np.asarray(got, dtype=np.float32)
    assert got.shape == before.shape == exp.mask.shape
    mask = exp.mask                                        # (whole-buffer passes: the large cases are almost all window)
    changed = (bits(got) != bits(before)) & ~mask
    assert not changed.any(), "%s: %d elements outside the m x n window changed (first: element %d of the allocation)" % (
        what, int(changed.sum()), int(np.argmax(changed)))
    nan = np.isnan(got) & mask
    assert not nan.any(), "%s: %d NaN in the result (a load that is not masked, or C read with beta = 0)" % (what, int(nan.sum()))
    assert not (np.isnan(exp.c) & mask).any(), "%s: the oracle itself read a guard" % what
    with np.errstate(invalid="ignore"):
        err = np.abs(got.astype(np.float64) - exp.c)       # (NaN outside the window, where both hold the guard)
        if kind == "int":
            bad = (err != 0) & mask
            first = int(np.argmax(bad))
            assert not bad.any(), "%s: %d of %d outputs are not bit-equal to the exact product (first: element %d, got %r, want %r)" % (
                what, int(bad.sum()), int(mask.sum()), first, got[first], exp.c[first])
            return 0.0
        bar = RTOL_TERMS * exp.terms + 1e-30
        over = (err > bar) & mask
        worst = float(np.max(np.where(mask, err / bar, 0.0))) if mask.any() else 0.0
    assert not over.any(), "%s: %d of %d outputs outside the bar, max err / (2e-6 * terms) = %.3g" % (what, int(over.sum()), int(mask.sum()), worst)
    return worst


def check_untouched(got, before, what=""):
    """An input operand after the call: the same bits everywhere."""
    assert np.array_equal(bits(got), bits(before)), "%s changed" % what


# ------------------------------------------------------------------------------------------------------------------------------
# case tables (shared by tests/test_gemm_cpu.py, which checks what they reach, and tests/test_gpu_gemm.py, which runs them)
# ------------------------------------------------------------------------------------------------------------------------------
EDGES = (1, 15, 16, 17, 63, 64, 65, 129)
# m, n crossed sparsely: every edge meets every other residue class once as m and once as n
EDGE_MN = tuple((EDGES[i], EDGES[(i + d) % 8]) for d in (0, 3, 5) for i in range(8))
K_DEPTH = (0, 1, 2, 3, 4, 5, 15, 16, 17, 18, 31, 32, 33, 47, 48, 49, 65)       # 0 - 5 k-blocks of 16, every k % 4 in the tail
K_DEPTH_MN = ((17, 65), (64, 15))
LAYOUT_SHAPES = ((77, 33, 21), (80, 36, 24))
LD_PADS = (0, 1, 3, 4)
# pointer offsets of (A, B, C): all 16 (A, B) pairs, C running through 0 - 3 against both
OFFSETS = tuple((a, b, (a + 2 * b + 1) % 4) for a in range(4) for b in range(4))
SPLIT_K = (1024, 1025, 2049, 8193)
SPLIT_MN = ((5, 7), (64, 65), (130, 33))
TILE128_MN = ((129, 127), (100, 130), (128, 128))
TILE128_K = (5, 16, 37, 64)
FLAT_SMALL = (70, 129)
FLAT_K = (19, 48)
# four layouts the large cases rotate through: (ld pads of A, B, C), (pointer offsets of A, B, C)
ROTATING_LAYOUTS = (((0, 0, 0), (0, 0, 0)), ((1, 3, 4), (1, 2, 3)), ((4, 4, 1), (0, 0, 2)), ((3, 1, 3), (3, 0, 1)))


def grouped_table():
    """The eight groups of the grouped test, in launch order.  Keys as in dctr_gemm_group_t, plus rows_per_slice (k_slices comes
    from dctr_gemm_k_slices / k_slices above) and sliced_store (each slice to its own C).  Empty groups: index 3 and 7."""
    return [
        dict(trans_a=0, trans_b=0, m=77, n=33, k=21, batch=1, pads=(0, 0, 0), offs=(0, 1, 2)),
        dict(trans_a=1, trans_b=0, m=40, n=65, k=300, batch=1, ones_last=1, pads=(4, 1, 4), offs=(0, 0, 0)),
        dict(trans_a=0, trans_b=1, m=33, n=17, k=1000, batch=1, ones_last=1, rows_per_slice=256, sliced_store=1, pads=(3, 3, 1), offs=(1, 0, 3)),
        dict(trans_a=0, trans_b=0, m=0, n=9, k=40, batch=1, pads=(0, 0, 0), offs=(0, 0, 0)),
        dict(trans_a=1, trans_b=1, m=65, n=5, k=513, batch=1, accumulate=1, rows_per_slice=128, pads=(1, 0, 3), offs=(2, 3, 1)),
        dict(trans_a=0, trans_b=0, m=16, n=70, k=130, batch=3, rows_per_slice=64, sliced_store=1, pads=(0, 4, 0), offs=(0, 0, 0)),
        dict(trans_a=1, trans_b=0, m=129, n=64, k=5, batch=2, accumulate=1, pads=(3, 1, 1), offs=(3, 2, 0)),
        dict(trans_a=0, trans_b=1, m=0, n=4, k=8, batch=2, pads=(0, 0, 0), offs=(0, 0, 0)),
    ]


def build_group(rng, kind, g):
    """Operands of one grouped_table() entry -> (A, B, C, call) with call = the dctr_gemm_group_t fields that are not pointers
    (element strides included) and the oracle's keywords under "ref"."""
    m, n, k, batch = g["m"], g["n"], g["k"], g["batch"]
    ones, acc = g.get("ones_last", 0), g.get("accumulate", 0)
    slices = k_slices(k, g["rows_per_slice"]) if "rows_per_slice" in g else 1
    stored = slices if g.get("sliced_store") else 1
    nb = n - 1 if ones else n                                   # op(B)'s columns that are in memory
    A = build_operand(rng, kind, *((k, m) if g["trans_a"] else (m, k)), ld_pad=g["pads"][0], offset=g["offs"][0], count=batch, stride_pad=5)
    B = build_operand(rng, kind, *((nb, k) if g["trans_b"] else (k, nb)), ld_pad=g["pads"][1], offset=g["offs"][1], count=batch, stride_pad=2,
                      tail=(k + g["pads"][1]) if ones and not g["trans_b"] else 0)         # (transposed, the missing row is row padding)
    C = build_operand(rng, kind, m, n, ld_pad=g["pads"][2], offset=g["offs"][2], count=batch * stored, stride_pad=3, fill=bool(acc))
    call = dict(trans_a=g["trans_a"], trans_b=g["trans_b"], m=m, n=n, k=k, lda=A.ld, ldb=B.ld, ldc=C.ld, batch=batch,
                stride_a=A.stride, stride_b=B.stride, stride_c=C.stride * stored, slice_stride_c=C.stride if stored > 1 else 0,
                ones_last=ones, accumulate=acc, k_slices=slices)
    call["ref"] = dict(trans_a=g["trans_a"], trans_b=g["trans_b"], m=m, n=n, k=k, batch=batch, beta=float(acc), stride_c=call["stride_c"],
                       ones_last=bool(ones), k_slices=slices, slice_stride_c=call["slice_stride_c"])
    return A, B, C, call


def slice_sum(buf, C, call):
    """float64 sum over the stored slices of a sliced_store group -> [batch] list of m x n."""
    out = []
    for b in range(call["batch"]):
        acc = np.zeros((call["m"], call["n"]))
        for s in range(call["k_slices"]):
            acc += window(buf, C.off + b * call["stride_c"] + s * call["slice_stride_c"], call["m"], call["n"], C.ld).astype(np.float64)
        out.append(acc)
    return out
