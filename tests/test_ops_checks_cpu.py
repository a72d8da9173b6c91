"""CPU: the operand checks the interaction ops' wrappers are written with (ops._rows2d, _vec, _x_in_place, _workspace, _route_name,
_id_stride, and what a forward and its backward share: _bilinear_operands, _fieldpair_operands, _dx_operand, _zeroed_grads), driven
directly with CPU tensors: what they refuse, what they accept, and the strides they hand to the args structs."""
import pytest
import torch

from deepctr_amd import ops

B, W = 5, 12


def _refused(t, rows=B, cols=W, **kw):
    with pytest.raises(ValueError, match=r"op: t must be a float32 \[.*\] view with unit column stride"):
        ops._rows2d("op", "t", t, rows, cols, **kw)


def test_rows2d_dtype_rank_and_column_stride():
    assert ops._rows2d("op", "t", torch.zeros(B, W), B, W) == W
    assert ops._rows2d("op", "t", torch.zeros(B, W + 4)[:, :W], B, W) == W + 4           # a view of a wider buffer: its pitch
    _refused(torch.zeros(B, W, dtype=torch.float64))
    _refused(torch.zeros(B, W, dtype=torch.int32))
    _refused(torch.zeros(B * W))
    _refused(torch.zeros(B, W, 1))
    _refused(torch.zeros(W, B).t())                                                       # [B, W] with strides (1, B)
    _refused(torch.zeros(B, 2 * W)[:, ::2])                                               # every other column


def test_rows2d_row_rules():
    for rows in (B - 1, B + 1):
        _refused(torch.zeros(rows, W))
    _refused(torch.zeros(B - 1, W), at_least_rows=True)
    assert ops._rows2d("op", "t", torch.zeros(B, W), B, W, at_least_rows=True) == W
    assert ops._rows2d("op", "t", torch.zeros(B + 1, W), B, W, at_least_rows=True) == W
    with pytest.raises(ValueError, match=r"\[>= 5, >= 12\]"):
        ops._rows2d("op", "t", torch.zeros(B - 1, W), B, W, at_least_rows=True)
    with pytest.raises(ValueError, match=r"\[5, >= 15\]"):                                # the message names offset + cols
        ops._rows2d("op", "t", torch.zeros(B, W), B, W, 3)


def test_rows2d_offsets_and_width():
    t = torch.zeros(B, W + 3)
    _refused(t, offset=-1)
    _refused(t, offset=4)                                                                 # offset + cols one past the width
    assert ops._rows2d("op", "t", t, B, W, 3) == W + 3                                    # exactly at it
    assert ops._rows2d("op", "t", t, B, W, 0) == W + 3
    _refused(torch.zeros(B, W - 1))


def test_rows2d_single_column_and_single_row():
    col = torch.zeros(1, B).t()                                                           # [B, 1] with strides (1, B)
    assert tuple(col.shape) == (B, 1) and col.stride(1) != 1
    assert ops._rows2d("op", "t", col, B, 1) == 1
    col = torch.zeros(B, 8)[:, 3:4].t().contiguous().t()
    assert tuple(col.shape) == (B, 1)
    assert ops._rows2d("op", "t", col, B, 1) == col.stride(0)
    _refused(col, cols=2)                                                                 # (one column holds one column)
    row = torch.zeros(W, 1).t().contiguous()                                              # [1, W]: torch may report stride(0) = 1
    assert tuple(row.shape) == (1, W)
    assert ops._rows2d("op", "t", row, 1, W) == W
    assert ops._rows2d("op", "t", torch.zeros(1, W + 4)[:, :W], 1, W) == W + 4


def test_rows2d_returns_row_stride():
    for t in (torch.zeros(B, W), torch.zeros(B, W + 4)[:, :W], torch.zeros(B, W + 4)[::2, 1:W], torch.zeros(W, 1).t().contiguous(),
              torch.zeros(1, W + 4)[:, :W], torch.zeros(1, B).t(), torch.zeros(1, 1), torch.zeros(B, 0)):
        assert ops._rows2d("op", "t", t, t.shape[0], t.shape[1]) == ops.row_stride(t)


def test_vec():
    ops._vec("op", "v", torch.zeros(B), B)
    ops._vec("op", "v", torch.zeros(B, 1), B)
    for bad in (torch.zeros(2 * B)[::2], torch.zeros(B, 2)[:, 0], torch.zeros(B + 1), torch.zeros(B - 1), torch.zeros(B, dtype=torch.float64)):
        with pytest.raises(ValueError, match="op: v must be a contiguous float32 tensor of 5 elements"):
            ops._vec("op", "v", bad, B)


def test_x_in_place():
    F, E = 3, 4
    x3 = torch.arange(B * F * E, dtype=torch.float32).reshape(B, F, E)
    x, *rest = ops._x_in_place("op", x3, None, None)
    assert x is x3 and tuple(rest) == (B, F, E, F * E, 0)
    x, *rest = ops._x_in_place("op", x3.transpose(1, 2), None, None)                      # made contiguous, like _f32c
    assert x.is_contiguous() and torch.equal(x, x3.transpose(1, 2)) and tuple(rest) == (B, E, F, F * E, 0)
    for bad in (torch.zeros(B, F * E), torch.zeros(B, F, E, 1)):
        with pytest.raises(ValueError, match="expect to be 3 dimensions"):
            ops._x_in_place("op", bad, None, None)
    with pytest.raises(TypeError):
        ops._x_in_place("op", x3.double(), None, None)
    buf = torch.zeros(B, F * E + 7)
    x, *rest = ops._x_in_place("op", buf, F, E, 3)
    assert x is buf and tuple(rest) == (B, F, E, F * E + 7, 3)
    assert tuple(ops._x_in_place("op", buf, F, E)[1:]) == (B, F, E, F * E + 7, 0)
    assert tuple(ops._x_in_place("op", buf, F, E, 7)[1:]) == (B, F, E, F * E + 7, 7)     # the last column is the buffer's last
    assert tuple(ops._x_in_place("op", buf[:1], F, E, 3)[1:]) == (1, F, E, F * E + 7, 3)
    for bad, off in ((buf, 8), (buf, -1), (buf.double(), 0), (torch.zeros(F * E + 7, B).t(), 0), (x3, 0), (torch.zeros(B, F * E - 1), 0)):
        with pytest.raises(ValueError, match="op: x .* must be a float32 .* view with unit column stride"):
            ops._x_in_place("op", bad, F, E, off)


def _mats(n, E=4):
    return [torch.zeros(E, E) for _ in range(n)]


@pytest.mark.parametrize("rows", [1, B])
def test_bilinear_operands_modes(rows):
    from deepctr_amd import _C
    F, E, r = 3, 4, 2
    x3 = torch.zeros(rows, F, E)
    sw = (torch.zeros(F, r), torch.zeros(r, F))
    for bilinear_type, nW in (("all", 1), ("each", 2), ("interaction", 3)):
        ws, wr = _mats(nW), _mats(nW)
        # all three weights: the model mode, W_1 / W_2, two tables of nW addresses, every tensor named for the device check
        x, *shape, mode, got_r, (w1, w2), tables, tensors = ops._bilinear_operands("op", x3, None, None, sw, ws, wr, bilinear_type, 0)
        assert x is x3 and tuple(shape) == (rows, F, E, F * E) and mode == _C.bilinear.MODE_MODEL and got_r == r
        assert w1 is sw[0] and w2 is sw[1] and len(tensors) == 3 + 2 * nW and all(a is b for a, b in zip(tensors, [x3, *sw, *ws, *wr]))
        assert [t.tolist() for t in tables] == [[w.data_ptr() for w in ws], [w.data_ptr() for w in wr]]
        # bilinear_w alone: one layer over x, no SENET operands
        *_, mode, got_r, (w1, w2), tables, tensors = ops._bilinear_operands("op", x3, None, None, None, None, wr, bilinear_type, 0)
        assert mode == _C.bilinear.MODE_LAYER and got_r == 0 and w1 is None and w2 is None and len(tensors) == 1 + nW
        assert tables[0] is None and tables[1].tolist() == [w.data_ptr() for w in wr]
    # senet_w alone
    *_, mode, got_r, (w1, w2), tables, tensors = ops._bilinear_operands("op", x3, None, None, sw, None, None, "interaction", 0)
    assert mode == _C.bilinear.MODE_SENET and got_r == r and tables == [None, None] and len(tensors) == 3
    # x read in place behind dense columns: the model mode only
    buf = torch.zeros(rows, F * E + 5)
    x, *shape, mode, _, _, _, _ = ops._bilinear_operands("op", buf, F, E, sw, _mats(3), _mats(3), "interaction", 5)
    assert x is buf and tuple(shape) == (rows, F, E, F * E + 5) and mode == _C.bilinear.MODE_MODEL


@pytest.mark.parametrize("rows", [1, B])
def test_bilinear_operands_refusals(rows):
    F, E, r = 3, 4, 2
    x3 = torch.zeros(rows, F, E)
    sw = (torch.zeros(F, r), torch.zeros(r, F))

    def refused(match, senet_w, senet_bilinear_w, bilinear_w, bilinear_type="interaction", dense_cols=0, x=x3, fields=None, dim=None):
        with pytest.raises(ValueError, match=match):
            ops._bilinear_operands("op", x, fields, dim, senet_w, senet_bilinear_w, bilinear_w, bilinear_type, dense_cols)

    give = "op: give senet_w \\+ senet_bilinear_w \\+ bilinear_w, senet_w alone, or bilinear_w alone"
    for two in ((sw, _mats(3), None), (sw, None, _mats(3)), (None, _mats(3), _mats(3)), (None, _mats(3), None), (None, None, None)):
        refused(give, *two)
    count = "op: bilinear_type 'each' over 3 fields takes 2 matrices \\[4, 4\\]"
    for n in (1, 3):                                                                     # "each" takes F - 1
        refused(count, None, None, _mats(n), "each")
        refused(count, sw, _mats(n), _mats(2), "each")
    refused(count, None, None, _mats(2, 5), "each")
    refused("op: bilinear_type 'all' over 3 fields takes 1 matrices", None, None, _mats(2), "all")
    senet = "op: senet_w must be W_1 \\[3, r\\] and W_2 \\[r, 3\\]"
    refused(senet, (torch.zeros(F), torch.zeros(r, F)), None, None)                      # a 1-D W_1
    refused(senet, (torch.zeros(F, 0), torch.zeros(0, F)), None, None)                   # r = 0
    refused(senet, (torch.zeros(F + 1, r), torch.zeros(r, F)), None, None)
    refused(senet, (torch.zeros(F, r), torch.zeros(r + 1, F)), None, None)
    dense = "op: dense_cols exist in the three-weight \\(FiBiNET\\) form only"
    buf = torch.zeros(rows, F * E + 5)
    refused(dense, sw, None, None, dense_cols=5, x=buf, fields=F, dim=E)
    refused(dense, None, None, _mats(3), dense_cols=5, x=buf, fields=F, dim=E)
    refused("op: 1 field\\(s\\): the layers need at least 2", (torch.zeros(1, r), torch.zeros(r, 1)), None, None, x=torch.zeros(rows, 1, E))
    with pytest.raises(NotImplementedError, match="bilinear_type 'some'"):
        ops._bilinear_operands("op", x3, None, None, None, None, _mats(3), "some", 0)


@pytest.mark.parametrize("rows", [1, B])
@pytest.mark.parametrize("F", [2, 3])
def test_fieldpair_operands(rows, F):
    E, P = 4, F * (F - 1) // 2
    x3 = torch.zeros(rows, F, E)
    ws = _mats(P)
    x, *rest, wptr, tensors = ops._fieldpair_operands("op", x3, ws, "fefm", None, None, 0)
    assert x is x3 and tuple(rest) == (rows, F, E, F * E, 0, P)
    assert wptr.dtype == torch.int64 and wptr.tolist() == [w.data_ptr() for w in ws]     # the table of the matrices' addresses
    assert len(tensors) == 1 + P and all(a is b for a, b in zip(tensors, [x3] + ws))
    r = torch.zeros(F, F)
    x, *rest, wptr, tensors = ops._fieldpair_operands("op", x3, r, "fwfm", None, None, 0)
    assert x is x3 and tuple(rest) == (rows, F, E, F * E, 0, P) and wptr is r and len(tensors) == 2 and tensors[1] is r
    buf = torch.zeros(rows, F * E + 7)                                                   # one group's slice of a wider row
    x, *rest, wptr, tensors = ops._fieldpair_operands("op", buf, r, "fwfm", F, E, 3)
    assert x is buf and tuple(rest) == (rows, F, E, F * E + 7, 3, P)
    with pytest.raises(ValueError, match="op: x .* must be a float32 .* view with unit column stride"):
        ops._fieldpair_operands("op", buf, r, "fwfm", F, E, 8)
    with pytest.raises(ValueError, match="op: kind 'fm': expected 'fefm' or 'fwfm'"):
        ops._fieldpair_operands("op", x3, ws, "fm", None, None, 0)
    fefm = "op: FEFM over %d fields takes %d matrices \\[4, 4\\]" % (F, P)
    for bad in (_mats(P + 1), _mats(P - 1), _mats(P, 5), [torch.zeros(E * E)] * P):
        with pytest.raises(ValueError, match=fefm):
            ops._fieldpair_operands("op", x3, bad, "fefm", None, None, 0)
    for bad in (torch.zeros(F, F + 1), torch.zeros(F * F), torch.zeros(F + 1, F + 1)):
        with pytest.raises(ValueError, match="op: FwFM over %d fields takes field_pair_strengths \\[%d, %d\\]" % (F, F, F)):
            ops._fieldpair_operands("op", x3, bad, "fwfm", None, None, 0)
    with pytest.raises(TypeError):
        ops._fieldpair_operands("op", x3, r.double(), "fwfm", None, None, 0)


@pytest.mark.parametrize("rows", [1, B])
def test_fieldpair_operands_refuse_one_field(rows):
    for kind, weights in (("fefm", []), ("fwfm", torch.zeros(1, 1))):
        with pytest.raises(ValueError, match="op: 1 field\\(s\\): a field pair needs at least 2"):
            ops._fieldpair_operands("op", torch.zeros(rows, 1, 4), weights, kind, None, None, 0)
        with pytest.raises(ValueError, match="op: 1 field\\(s\\): a field pair needs at least 2"):
            ops._fieldpair_operands("op", torch.zeros(rows, 9), weights, kind, 1, 4, 2)


@pytest.mark.parametrize("rows", [1, B])
def test_dx_operand(rows):
    F, E = 3, 4
    assert ops._dx_operand("op", None, rows, F, E, 0) == 0
    assert ops._dx_operand("op", torch.zeros(rows, F, E), rows, F, E, 0) == F * E
    buf = torch.zeros(rows, 2 * F * E + 7)
    view = buf[:, 2:F * E + 7]                                                           # a strided view: the buffer's pitch
    assert ops._dx_operand("op", view, rows, F, E, 5) == 2 * F * E + 7                   # the last column is the view's last
    assert ops._dx_operand("op", view, rows, F, E, 0) == 2 * F * E + 7
    assert ops._dx_operand("op", view, rows, F, E, 2, extra_cols=3) == 2 * F * E + 7     # the dense columns behind the embeddings
    assert ops._dx_operand("op", torch.zeros(rows, F * E), rows, F, E, 0) == F * E
    refusals = [(view, 6, 0), (view, 3, 3), (view, -1, 0), (torch.zeros(rows, F * E - 1), 0, 0),     # too narrow / a bad offset
                (torch.zeros(rows, F, E), 1, 0), (torch.zeros(rows, F, E), 0, 2),        # [B,F,E] has no offset and no extra columns
                (torch.zeros(rows, E, F), 0, 0), (torch.zeros(rows, F, 2 * E)[:, :, :E], 0, 0),
                (torch.zeros(rows, F, E, dtype=torch.float64), 0, 0), (buf.double(), 0, 0), (torch.zeros(rows + 1, F * E), 0, 0)]
    for bad, off, extra in refusals:
        with pytest.raises(ValueError, match=r"op: dx must be a float32 \[%d, >= %d\] view with unit column stride"
                           % (rows, off + F * E + extra)):
            ops._dx_operand("op", bad, rows, F, E, off, extra)


def test_zeroed_grads():
    ws = [torch.ones(2, 3), None, torch.ones(4), torch.ones(1, 5)]
    flat, views = ops._zeroed_grads(ws, [True, False, False, True], torch.device("cpu"))
    assert flat.dtype == torch.float32 and flat.numel() == 6 + 4 + 5 and not flat.any()  # a slot per weight, wanted or not
    assert views[1] is None and views[2] is None and tuple(views[0].shape) == (2, 3) and tuple(views[3].shape) == (1, 5)
    assert views[0].data_ptr() == flat.data_ptr() and views[3].data_ptr() == flat[10:].data_ptr()
    flat, views = ops._zeroed_grads(ws, [False] * 4, torch.device("cpu"))
    assert flat is None and views == [None] * 4


class _Args:
    workspace = workspace_bytes = None


def test_workspace_takes_the_callers_tensor_or_refuses_it():
    a = _Args()
    assert ops._workspace("op", a, 0, None, torch.device("cpu")) is None and a.workspace is None
    ws = torch.zeros(16)
    assert ops._workspace("op", a, 64, ws, torch.device("cpu")) is ws
    assert (a.workspace, a.workspace_bytes) == (ws.data_ptr(), 64)
    for bad in (torch.zeros(15), torch.zeros(32)[::2], torch.zeros(16, dtype=torch.float64)):
        with pytest.raises(ValueError, match="op: workspace must be a contiguous float32 tensor of >= 64 bytes"):
            ops._workspace("op", _Args(), 64, bad, torch.device("cpu"))


def test_route_name_and_id_stride():
    from deepctr_amd import _C
    assert ops._route_name("dctr_x_route", 1, {0: "lds", 1: "direct"}) == "direct"
    with pytest.raises(_C.DctrError, match="dctr_x_route"):
        ops._route_name("dctr_x_route", -4, {0: "lds"})
    ids = torch.zeros(3, 7, dtype=torch.int32)
    assert ops._id_stride(ids[1]) == 1 and ops._id_stride(ids[:, 2]) == 7 and ops._id_stride(ids[:1, 2]) == 1
