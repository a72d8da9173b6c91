"""CPU: the operand checks the interaction ops' wrappers are written with (ops._rows2d, _vec, _x_in_place, _workspace, _route_name,
_id_stride), driven directly with CPU tensors: what they refuse, what they accept, and the strides they hand to the args structs."""
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
