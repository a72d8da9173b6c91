"""Thin Python wrappers over the C ABI (include/dctr.h): argument checking, output allocation
with PyTorch (device memory + streams are plumbing), one C call per op on torch's current stream.

Every function requires HIP-resident tensors and the built extension; nothing here computes on
the CPU and nothing falls back to eager PyTorch math.
"""
import ctypes
from collections import OrderedDict

import numpy as np
import torch

from . import _C


def _dev_check(*tensors):
    """Every tensor must live on the CURRENT HIP device: launches go to torch's current stream of the current device
    (_C.stream_ptr), so a tensor of another device would be read through the wrong queue — unordered with its copies, or a
    fault.  Models switch the current device themselves (engine.on_model_device); direct callers of ops do it with
    ``torch.cuda.device(tensor.device)``."""
    cur = None
    for t in tensors:
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise _C.DctrExtensionError("deepctr_amd ops need HIP device tensors (got %s); there is no CPU path"
                                        % (type(t).__name__ if not isinstance(t, torch.Tensor) else str(t.device)))
        if cur is None:
            cur = torch.cuda.current_device()
        if t.device.index != cur:
            raise _C.DctrExtensionError("tensor on %s but the current HIP device is cuda:%d: wrap the call in "
                                        "torch.cuda.device(%d) (kernels are launched on the current device's stream)"
                                        % (t.device, cur, t.device.index))


def _f32c(t, name):
    if t.dtype != torch.float32:
        raise TypeError("%s must be float32, got %s" % (name, t.dtype))
    return t if t.is_contiguous() else t.contiguous()


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _ids(t, name):
    if t.dtype == torch.int32:
        return t if t.is_contiguous() else t.contiguous(), 0
    if t.dtype == torch.int64:
        return t if t.is_contiguous() else t.contiguous(), 1
    raise TypeError("%s must be int32 or int64, got %s" % (name, t.dtype))


def _ptr_array(tensors):
    """host array of device pointers (const float* const*)."""
    arr = (ctypes.c_void_p * max(1, len(tensors)))()
    for i, t in enumerate(tensors):
        arr[i] = None if t is None else t.data_ptr()
    return arr


def _i32_array(vals):
    arr = (ctypes.c_int32 * max(1, len(vals)))()
    for i, v in enumerate(vals):
        arr[i] = int(v)
    return arr


def row_stride(t):
    """Elements between consecutive rows of a 2-D tensor with unit column stride.  torch leaves the stride of a size-1 dimension
    arbitrary (a [1, n] result of ``.t().contiguous()`` reports stride(0) = 1): a single row gets its width."""
    return int(t.stride(0)) if t.shape[0] != 1 else max(int(t.stride(0)), int(t.shape[1]))


# The operand checks of the interaction ops' wrappers.  They raise before anything is launched and never touch the device (the one
# _dev_check per call stays with the wrapper).
def _rows2d(op, name, t, rows, cols, offset=0, at_least_rows=False):
    """``t`` is a float32 2-D view with unit column stride that holds ``rows`` rows (or more, with ``at_least_rows``) and the columns
    [offset, offset + cols).  A single column may have any column stride (torch keeps (1, n) for the [n, 1] transpose of a [1, n]
    row).  Returns the row pitch in elements (row_stride): what the op's args struct takes as the operand's stride."""
    shape = t.shape         # (each of these is a call into torch: one of each per operand, the wrappers are latency-bound)
    if len(shape) == 2 and t.dtype == torch.float32 and offset >= 0:
        (r, c), (pitch, step) = shape, t.stride()
        if (step == 1 or c <= 1) and c >= offset + cols and (r >= rows if at_least_rows else r == rows):
            return pitch if r != 1 else max(pitch, c)       # = row_stride(t)
    raise ValueError("%s: %s must be a float32 [%s%d, >= %d] view with unit column stride"
                     % (op, name, ">= " if at_least_rows else "", rows, offset + cols))


def _vec(op, name, t, n):
    """``t`` is a contiguous float32 tensor of ``n`` elements (any shape)."""
    if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n:
        raise ValueError("%s: %s must be a contiguous float32 tensor of %d elements" % (op, name, n))


def _x_in_place(op, x, fields, dim, x_offset=0):
    """The input of an interaction layer: a [B,F,E] tensor (made contiguous float32), or with ``fields`` / ``dim`` the F*E columns from
    ``x_offset`` of a float32 [B, stride] buffer read in place.  Returns (x, B, F, E, x_stride, x_offset)."""
    if fields is None:
        if x.dim() != 3:
            raise ValueError("Unexpected inputs dimensions %d, expect to be 3 dimensions" % x.dim())
        x = _f32c(x, "x")
        B, F, E = x.shape
        return x, B, F, E, F * E, 0
    B, F, E = x.shape[0], int(fields), int(dim)
    return x, B, F, E, _rows2d(op, "x (with fields / dim)", x, B, F * E, x_offset), int(x_offset)


def _dx_operand(op, dx, B, F, E, dx_offset, extra_cols=0):
    """The input gradient a backward wrapper writes: a contiguous float32 [B,F,E] tensor (no offset, no extra columns), or a float32
    2-D view that holds the F*E + ``extra_cols`` columns from ``dx_offset``.  Returns its row stride (0 for None)."""
    if dx is None:
        return 0
    if dx.dim() == 3 and dx_offset == 0 and not extra_cols and tuple(dx.shape) == (B, F, E) and dx.is_contiguous() \
            and dx.dtype == torch.float32:
        return F * E
    return _rows2d(op, "dx", dx, B, F * E + extra_cols, dx_offset)


def _bilinear_operands(op, x, fields, dim, senet_w, senet_bilinear_w, bilinear_w, bilinear_type, dense_cols):
    """What senet_bilinear() and senet_bilinear_bwd() read alike: x (_x_in_place), the mode the given weights pick, W_1 [F,r] and
    W_2 [r,F], and the device tables of the two BilinearInteractions' matrices.  Returns (x, B, F, E, x_stride, mode, r, (w1, w2),
    (senet_bilinear table, bilinear table), tensors) — None for what the mode has not, ``tensors`` for the device check."""
    x, B, F, E, x_stride, _ = _x_in_place(op, x, fields, dim)
    if senet_w is not None and bilinear_w is not None and senet_bilinear_w is not None:
        mode = _C.bilinear.MODE_MODEL
    elif senet_w is not None and bilinear_w is None and senet_bilinear_w is None:
        mode = _C.bilinear.MODE_SENET
    elif senet_w is None and bilinear_w is not None and senet_bilinear_w is None:
        mode = _C.bilinear.MODE_LAYER
    else:
        raise ValueError("%s: give senet_w + senet_bilinear_w + bilinear_w, senet_w alone, or bilinear_w alone" % op)
    if mode != _C.bilinear.MODE_MODEL and dense_cols:
        raise ValueError("%s: dense_cols exist in the three-weight (FiBiNET) form only" % op)
    if F < 2:
        raise ValueError("%s: %d field(s): the layers need at least 2" % (op, F))
    tensors = [x]
    r = 0
    w1 = w2 = None
    if senet_w is not None:
        w1, w2 = (_f32c(w, "senet_w") for w in senet_w)
        r = w1.shape[1] if w1.dim() == 2 else -1
        if r < 1 or tuple(w1.shape) != (F, r) or tuple(w2.shape) != (r, F):
            raise ValueError("%s: senet_w must be W_1 [%d, r] and W_2 [r, %d]" % (op, F, F))
        tensors += [w1, w2]
    nW = bilinear_weight_count(bilinear_type, F)
    tables = []
    for ws in (senet_bilinear_w, bilinear_w):
        if ws is None:
            tables.append(None)
            continue
        ws = [_f32c(w, "bilinear weight") for w in ws]
        if len(ws) != nW or any(tuple(w.shape) != (E, E) for w in ws):
            raise ValueError("%s: bilinear_type %r over %d fields takes %d matrices [%d, %d]" % (op, bilinear_type, F, nW, E, E))
        tensors += ws
        tables.append(bilinear_table(ws))
    return x, B, F, E, x_stride, mode, r, (w1, w2), tables, tensors


def _fieldpair_operands(op, x, weights, kind, fields, dim, x_offset):
    """What fieldpair() and fieldpair_bwd() read alike: the kind, x (_x_in_place) over at least 2 fields, and the weights — FEFM's
    P = F(F-1)/2 matrices [E,E] behind a device table of their addresses, or FwFM's field_pair_strengths [F,F].  Returns
    (x, B, F, E, x_stride, x_offset, P, wptr, tensors): ``wptr`` is the tensor dctr_fieldpair_args_t.weights points to, ``tensors``
    are for the device check."""
    if kind not in _FIELDPAIR_KINDS:
        raise ValueError("%s: kind %r: expected 'fefm' or 'fwfm'" % (op, kind))
    x, B, F, E, x_stride, x_offset = _x_in_place(op, x, fields, dim, x_offset)
    if F < 2:
        raise ValueError("%s: %d field(s): a field pair needs at least 2" % (op, F))
    P = F * (F - 1) // 2
    if kind == "fefm":
        ws = [_f32c(w, "field_embeddings") for w in weights]
        if len(ws) != P or any(tuple(w.shape) != (E, E) for w in ws):
            raise ValueError("%s: FEFM over %d fields takes %d matrices [%d, %d]" % (op, F, P, E, E))
        return x, B, F, E, x_stride, x_offset, P, bilinear_table(ws), [x] + ws
    r = _f32c(weights, "field_pair_strengths")
    if tuple(r.shape) != (F, F):
        raise ValueError("%s: FwFM over %d fields takes field_pair_strengths [%d, %d]" % (op, F, F, F))
    return x, B, F, E, x_stride, x_offset, P, r, [x, r]


def _zeroed_grads(weights, wanted, device):
    """The backward ops ACCUMULATE into their weight gradients: ONE zeroed float32 buffer (one fill) with a slot per weight, in
    order (a None weight takes none), and per weight its slot viewed in the weight's shape where ``wanted``, else None.  Returns
    (flat, views); flat is None when nothing is wanted."""
    views = [None] * len(weights)
    if not any(wanted):
        return None, views
    flat = torch.zeros(sum(w.numel() for w in weights if w is not None), dtype=torch.float32, device=device)
    at = 0
    for i, w in enumerate(weights):
        if w is None:
            continue
        if wanted[i]:
            views[i] = flat[at:at + w.numel()].view(w.shape)
        at += w.numel()
    return flat, views


def _workspace(op, a, need, workspace, device):
    """Hand the args struct ``a`` the ``need`` bytes the library asked for: the caller's tensor if it is large enough, else the
    per-stream scratch.  Returns the tensor (None when nothing is needed)."""
    if not need:
        return None
    if workspace is None:
        workspace = _scratch(device, need)   # rewritten by every call: stream order keeps calls apart
    elif workspace.dtype != torch.float32 or not workspace.is_contiguous() or workspace.numel() * 4 < need:
        raise ValueError("%s: workspace must be a contiguous float32 tensor of >= %d bytes" % (op, need))
    a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel() * 4
    return workspace


def _route_name(op, rc, names):
    """The reply of a dctr_*_route call: a negative error code, or the index of the route in ``names``."""
    rc = int(rc)
    if rc < 0:
        _C.check(rc, op)
    return names[rc]


def _upload(arr, device):
    """A ctypes array of descriptors as a uint8 device tensor (kept alive by the caller)."""
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)


def _id_stride(ids):
    """Elements between consecutive ids of a 1-D view (the stride of a single element is arbitrary)."""
    return int(ids.stride(0)) if ids.shape[0] != 1 else 1


# ---------------------------------------------------------------------------------------------
# a2 Hash
# ---------------------------------------------------------------------------------------------
def hash_bucket(x, num_buckets, mask_zero=False):
    """Hash.call for integer ids (reference layers/utils.py:89-112): int32/int64 tensor -> int64 tensor."""
    _dev_check(x)
    lib = _C.lib()
    xc, is64 = _ids(x, "x")
    out = torch.empty(xc.shape, dtype=torch.int64, device=xc.device)
    fn = lib.dctr_hash_bucket_i64 if is64 else lib.dctr_hash_bucket_i32
    _C.check(fn(_ptr(xc), xc.numel(), int(num_buckets), int(bool(mask_zero)), _ptr(out), _C.stream_ptr()),
             "dctr_hash_bucket")
    return out


def hash_fields(desc, n_fields, ids, out):
    """Hash.call over the id matrix of a gather in one launch (dctr_hash_fields): ids [F, B] -> out [F, B]; fields whose
    descriptor says hash_mode 0 are copied."""
    _dev_check(desc, ids, out)
    _C.check(_C.lib().dctr_hash_fields(_ptr(desc), int(n_fields), _ptr(ids), ids.stride(0), ids.stride(1),
                                       int(ids.dtype == torch.int64), ids.shape[1], _ptr(out), out.stride(0),
                                       int(out.dtype == torch.int64), _C.stream_ptr()), "dctr_hash_fields")
    return out


def sgemm(a, b, trans_a=False, trans_b=False, out=None, accumulate=False):
    """Row-major convenience over dctr_sgemm (the training step's own MFMA GEMM): out [M, N] (+)= op(a) @ op(b) for 2-D (or batched
    3-D) contiguous float32 tensors; op = transpose of the last two dimensions when the flag is set."""
    _dev_check(a, b, out)
    a, b = _f32c(a, "a"), _f32c(b, "b")
    batch = a.shape[0] if a.dim() == 3 else 1
    am, ak = (a.shape[-1], a.shape[-2]) if trans_a else (a.shape[-2], a.shape[-1])
    bk, bn = (b.shape[-1], b.shape[-2]) if trans_b else (b.shape[-2], b.shape[-1])
    if ak != bk:
        raise ValueError("sgemm: inner dimensions %d and %d differ" % (ak, bk))
    shape = (batch, am, bn) if a.dim() == 3 else (am, bn)
    if out is None:
        out = torch.zeros(shape, dtype=torch.float32, device=a.device)
    # row-major out = op(a) op(b)  <=>  column-major out^T (bn x am) = op(b)^T op(a)^T: the BLAS call with (A, B) = (b, a)
    _C.check(_C.lib().dctr_sgemm(int(trans_b), int(trans_a), bn, am, ak, _ptr(b), b.shape[-1], b.shape[-2] * b.shape[-1], _ptr(a),
                                 a.shape[-1], a.shape[-2] * a.shape[-1], 1.0 if accumulate else 0.0, _ptr(out), bn, am * bn, batch,
                                 _C.stream_ptr()), "dctr_sgemm")
    return out


def pack_strings(values):
    """Host-side packing of a string column: (uint8 bytes, int64 offsets[n+1]) NumPy arrays."""
    flat = [v if isinstance(v, (bytes, np.bytes_)) else str(v).encode("utf-8") for v in values]
    offsets = np.zeros(len(flat) + 1, dtype=np.int64)
    if flat:
        np.cumsum([len(b) for b in flat], out=offsets[1:])
    data = np.frombuffer(b"".join(flat), dtype=np.uint8) if offsets[-1] > 0 else np.zeros(1, np.uint8)
    return np.ascontiguousarray(data), offsets


def hash_bucket_strings(values, num_buckets, mask_zero=False, device=None):
    """Hash.call for string-dtype features: strings are packed on the host (they are host data in the
    reference too), hashed on the device.  Returns an int64 device tensor with the shape of ``values``."""
    device = device or _C.require_device()
    lib = _C.lib()
    arr = np.asarray(values, dtype=object)
    data, offsets = pack_strings(list(arr.reshape(-1)))
    d_bytes = torch.from_numpy(data.copy()).to(device)
    d_off = torch.from_numpy(offsets).to(device)
    out = torch.empty(arr.size, dtype=torch.int64, device=device)
    _C.check(lib.dctr_hash_bucket_bytes(_ptr(d_bytes), _ptr(d_off), arr.size, int(num_buckets), int(bool(mask_zero)),
                                        _ptr(out), _C.stream_ptr()), "dctr_hash_bucket_bytes")
    return out.reshape(arr.shape)


# ---------------------------------------------------------------------------------------------
# a3-a8 embedding ops
# ---------------------------------------------------------------------------------------------
def new_status(device):
    return torch.zeros(1, dtype=torch.int32, device=device)


def check_status(status, what="embedding lookup"):
    """Raise like the reference's Embedding gather on a CPU does when an index is out of range."""
    v = int(status.item())
    if v & _C.STATUS_TIMEOUT:
        status.zero_()
        raise RuntimeError("%s: an in-kernel wait of the streaming forward kernel timed out (DCTR_STATUS_TIMEOUT); the "
                           "outputs of that launch are invalid" % what)
    if v & _C.STATUS_INDEX_OOR:
        status.zero_()
        raise IndexError("%s: index out of range [0, vocabulary_size)" % what)


def embed_lookup(idx, table, hash_mode=0, out=None, out_stride=None, return_mask=False, status=None):
    """Row gather: idx [...] -> [..., dim] (keras Embedding.call, reference inputs.py:101-117).  With
    ``return_mask`` also returns the mask_zero mask (post-hash idx != 0) as a uint8 tensor."""
    _dev_check(idx, table)
    lib = _C.lib()
    ic, is64 = _ids(idx, "idx")
    table = _f32c(table, "table")
    vocab, dim = table.shape
    n = ic.numel()
    if out is None:
        out = torch.empty(tuple(ic.shape) + (dim,), dtype=torch.float32, device=table.device)
        out_stride = dim
    mask = torch.empty(ic.shape, dtype=torch.uint8, device=table.device) if return_mask else None
    a = _C.LookupArgs(idx=ic.data_ptr(), table=table.data_ptr(), vocab=vocab, n=n, idx_is_i64=is64, dim=dim,
                      hash_mode=hash_mode, out=out.data_ptr(), out_stride=out_stride,
                      mask=None if mask is None else mask.data_ptr(),
                      status=None if status is None else status.data_ptr())
    _C.check(lib.dctr_embed_lookup(ctypes.byref(a), _C.stream_ptr()), "dctr_embed_lookup")
    return (out, mask) if return_mask else out


def embed_lookup_multi(lookups, extra_mask_ids=(), status=None):
    """Several row gathers in ONE launch.  ``lookups``: list of dicts(idx, table, hash_mode, out (2-D/3-D view with the row
    stride to write at), mask (uint8 tensor or None)).  A lookup with a mask also ANDs in (id != 0) of every tensor in
    ``extra_mask_ids`` (same number of ids) — see include/dctr.h."""
    n = len(lookups)
    arr = (_C.LookupArgs * max(1, n))()
    keep = []
    for k, lk in enumerate(lookups):
        ic, is64 = _ids(lk["idx"], "idx")
        table = _f32c(lk["table"], "table")
        out, mask = lk["out"], lk.get("mask")
        keep.append((ic, table))
        arr[k] = _C.LookupArgs(idx=ic.data_ptr(), table=table.data_ptr(), vocab=table.shape[0], n=ic.numel(), idx_is_i64=is64,
                               dim=table.shape[1], hash_mode=int(lk.get("hash_mode", 0)), out=out.data_ptr(),
                               out_stride=out.stride(-2), mask=None if mask is None else mask.data_ptr(),
                               status=None if status is None else status.data_ptr())
    ex = [_ids(t, "extra_mask_ids") for t in extra_mask_ids]
    ep = (ctypes.c_void_p * max(1, len(ex)))(*[t.data_ptr() for t, _ in ex])
    ef = (ctypes.c_int32 * max(1, len(ex)))(*[f for _, f in ex])
    _C.check(_C.lib().dctr_embed_lookup_multi(arr, n, ctypes.cast(ep, ctypes.c_void_p), ctypes.cast(ef, ctypes.c_void_p), len(ex),
                                              _C.stream_ptr()), "dctr_embed_lookup_multi")
    del keep


def embed_pool(idx, table, combiner="mean", length=None, weight=None, weight_norm=True, lin_table=None, hash_mode=0,
               out=None, out_stride=None, lin_out=None, status=None, keep_args=None):
    """VarLenSparseFeat lookup + (weighted) masked pooling: idx [B,T] -> [B,dim] (reference
    inputs.py:120-158, layers/sequence.py:76-106,155-183).  ``length`` [B] selects the length-mask form,
    otherwise mask_zero on the (post-hash) index.  Returns (pooled, pooled_linear or None)."""
    _dev_check(idx, table, length, weight, lin_table)
    lib = _C.lib()
    ic, is64 = _ids(idx, "idx")
    if ic.dim() != 2:
        raise ValueError("idx must be [B, T]")
    B, T = ic.shape
    table = _f32c(table, "table")
    vocab, dim = table.shape
    if out is None:
        out = torch.empty(B, dim, dtype=torch.float32, device=table.device)
        out_stride = dim
    if lin_table is not None:
        lin_table = _f32c(lin_table, "lin_table").reshape(-1)
        if lin_out is None:
            lin_out = torch.empty(B, dtype=torch.float32, device=table.device)
    if length is not None:
        length = length.reshape(-1).to(torch.int32).contiguous()
    if weight is not None:
        weight = _f32c(weight, "weight").reshape(B, T)
    a = _C.PoolArgs(idx=ic.data_ptr(), table=table.data_ptr(), lin_table=None if lin_table is None else lin_table.data_ptr(),
                    length=None if length is None else length.data_ptr(),
                    weight=None if weight is None else weight.data_ptr(), vocab=vocab, idx_stride=T, batch=B,
                    idx_is_i64=is64, maxlen=T, dim=dim, combiner=_C.POOL_CODES[combiner], weight_norm=int(bool(weight_norm)),
                    hash_mode=hash_mode, out=out.data_ptr(), out_stride=out_stride,
                    lin_out=None if lin_out is None else lin_out.data_ptr(),
                    status=None if status is None else status.data_ptr())
    _C.check(lib.dctr_embed_pool(ctypes.byref(a), _C.stream_ptr()), "dctr_embed_pool")
    if keep_args is not None:           # training: the backward call re-uses these arguments (and their tensors)
        keep_args.append((a, (ic, table, lin_table, length, weight, out, lin_out)))
    return out, lin_out


def embed_pool_bwd(fwd_args, d_out=None, d_lin_out=None, g_table=None, g_lin_table=None, touched=None):
    """Backward of dctr_embed_pool: scatter-adds into the dense gradient tables (see include/dctr.h)."""
    a = _C.PoolBwdArgs(fwd=ctypes.pointer(fwd_args), d_out=None if d_out is None else d_out.data_ptr(),
                       d_stride=0 if d_out is None else d_out.stride(0),
                       d_lin_out=None if d_lin_out is None else d_lin_out.data_ptr(),
                       g_table=None if g_table is None else g_table.data_ptr(),
                       g_lin_table=None if g_lin_table is None else g_lin_table.data_ptr(),
                       touched=None if (touched is None or g_table is None) else touched.data_ptr())
    _C.check(_C.lib().dctr_embed_pool_bwd(ctypes.byref(a), _C.stream_ptr()), "dctr_embed_pool_bwd")


def seq_weight(seq, weight, mask=None, length=None, weight_norm=True):
    """WeightedSequenceLayer.call on a materialised [B,T,E] tensor (reference sequence.py:155-183)."""
    _dev_check(seq, weight, mask, length)
    seq = _f32c(seq, "seq")
    B, T, E = seq.shape
    weight = _f32c(weight, "weight").reshape(B, T)
    m = None if mask is None else mask.to(torch.uint8).reshape(B, T).contiguous()
    ln = None if length is None else length.reshape(-1).to(torch.int32).contiguous()
    out = torch.empty_like(seq)
    _C.check(_C.lib().dctr_seq_weight_fwd(_ptr(seq), _ptr(weight), _ptr(m), _ptr(ln), B, T, E, int(bool(weight_norm)),
                                          _ptr(out), _C.stream_ptr()), "dctr_seq_weight_fwd")
    return out


def make_field_descriptors(fields, device):
    """fields: list of dicts(table, lin_table, vocab, dim, out_offset, in_fm, hash_mode, identity) ->
    uint8 device tensor holding the dctr_field_t array (kept alive by the caller)."""
    arr = (_C.FieldDesc * max(1, len(fields)))()
    for j, f in enumerate(fields):
        arr[j].table = f["table"].data_ptr()
        arr[j].lin_table = None if f.get("lin_table") is None else f["lin_table"].data_ptr()
        arr[j].vocab = int(f["vocab"])
        arr[j].dim = int(f["dim"])
        arr[j].out_offset = int(f.get("out_offset", -1))
        arr[j].in_fm = int(bool(f.get("in_fm", False)))
        arr[j].hash_mode = int(f.get("hash_mode", 0))
        arr[j].identity = int(bool(f.get("identity", False)))
        arr[j].row_pitch = int(f.get("row_pitch", 0))
    return _upload(arr, device)


def make_gather_args(desc, n_fields, ids, ids_stride_f, ids_stride_b, batch, max_dim, all_dim4, any_hash,
                     dense=None, dense_lin_w=None, dense_out_offset=-1, dense_copy_cols=None, dnn_in=None, out_stride=0,
                     fm_logit=None, lin_logit=None, status=None, split=(0, 0), uniform_dim=0, any_identity=False, any_pitch=False,
                     pools=None, pool_row0=0, pool_pieces=0, n_pools=0, pool_flags=0):
    """Fill a dctr_gather_fm_args_t (see include/dctr.h).  The caller keeps every tensor alive.
    ``split`` = (split_col, split_field), see the header; (0, 0) = none.  ``pools``: DEVICE array of dctr_pool_seq_t (make_pool_seqs) for
    the last ``n_pools`` fields — sequences pooled inside dctr_embed_mlp_fwd; the launch's rows start at row ``pool_row0`` of their ids."""
    _dev_check(desc, ids, dense, dnn_in)
    is64 = 0
    if ids is not None:
        if ids.dtype == torch.int64:
            is64 = 1
        elif ids.dtype != torch.int32:
            raise TypeError("ids must be int32 or int64")
    n_dense = 0 if dense is None else dense.shape[1]
    return _C.GatherFmArgs(fields=None if desc is None else desc.data_ptr(), ids=None if ids is None else ids.data_ptr(),
                           ids_stride_f=ids_stride_f, ids_stride_b=ids_stride_b, ids_is_i64=is64, n_fields=n_fields,
                           max_dim=max_dim, all_dim4=int(bool(all_dim4)), any_hash=int(bool(any_hash)), n_dense=n_dense,
                           dense=None if dense is None else dense.data_ptr(),
                           dense_stride=0 if dense is None else row_stride(dense),
                           dense_lin_w=None if dense_lin_w is None else dense_lin_w.data_ptr(),
                           dense_out_offset=dense_out_offset,
                           dense_copy_cols=n_dense if dense_copy_cols is None else dense_copy_cols, batch=batch,
                           dnn_in=None if dnn_in is None else dnn_in.data_ptr(), out_stride=out_stride,
                           fm_logit=None if fm_logit is None else fm_logit.data_ptr(),
                           lin_logit=None if lin_logit is None else lin_logit.data_ptr(),
                           status=None if status is None else status.data_ptr(),
                           split_col=int(split[0]), split_field=int(split[1]), uniform_dim=int(uniform_dim),
                           any_identity=int(bool(any_identity)), any_pitch=int(bool(any_pitch)),
                           n_pools=int(n_pools), pools=None if pools is None else pools.data_ptr(), pool_row0=int(pool_row0),
                           pool_pieces=int(pool_pieces), pool_flags=int(pool_flags))


def make_pool_seqs(seqs, device):
    """DEVICE array of dctr_pool_seq_t from [(ids [N, T] int32 tensor, length [N] int32 tensor or None, combiner 'sum' | 'mean'), ...]."""
    arr = (_C.PoolSeq * max(1, len(seqs)))()
    for i, (ids, length, combiner) in enumerate(seqs):
        arr[i].idx, arr[i].length = ids.data_ptr(), (None if length is None else length.data_ptr())
        arr[i].idx_stride, arr[i].maxlen, arr[i].combiner = ids.stride(0), ids.shape[1], _C.POOL_CODES[combiner]
    return _upload(arr, device)


def embed_gather_fm(*args, **kwargs):
    """Fused multi-table gather + concat + linear term + FM (see include/dctr.h).  Low-level: the caller
    (the model plan) owns descriptor and output buffers.  Same arguments as ``make_gather_args``."""
    a = make_gather_args(*args, **kwargs)
    _C.check(_C.lib().dctr_embed_gather_fm(ctypes.byref(a), _C.stream_ptr()), "dctr_embed_gather_fm")


# ---------------------------------------------------------------------------------------------
# a8-a12 interaction layers
# ---------------------------------------------------------------------------------------------
def fm(x):
    """FM.call (reference interaction.py:588-604): x [B,F,E] -> [B,1]."""
    _dev_check(x)
    if x.dim() != 3:
        raise ValueError("Unexpected inputs dimensions %d, expect to be 3 dimensions" % x.dim())
    x = _f32c(x, "x")
    B, F, E = x.shape
    y = torch.empty(B, 1, dtype=torch.float32, device=x.device)
    _C.check(_C.lib().dctr_fm_fwd(_ptr(x), B, F * E, F, E, _ptr(y), _C.stream_ptr()), "dctr_fm_fwd")
    return y


def fm_strided(x2d, offset, fields, dim):
    """FM over columns [offset, offset + fields*dim) of a [B, stride] concat buffer, read in place."""
    _dev_check(x2d)
    B = x2d.shape[0]
    y = torch.empty(B, dtype=torch.float32, device=x2d.device)
    base = ctypes.c_void_p(x2d.data_ptr() + 4 * offset)
    _C.check(_C.lib().dctr_fm_fwd(base, B, x2d.stride(0), fields, dim, _ptr(y), _C.stream_ptr()), "dctr_fm_fwd")
    return y


def crossnet(x, kernels, bias, parameterization="vector"):
    """CrossNet.call (reference interaction.py:405-424): x [B,d]; kernels [L,d] or [L,d,d]; bias [L,d]."""
    _dev_check(x, kernels, bias)
    if x.dim() != 2:
        raise ValueError("Unexpected inputs dimensions %d, expect to be 2 dimensions" % x.dim())
    if parameterization not in ("vector", "matrix"):
        raise ValueError("parameterization should be 'vector' or 'matrix'")
    x = _f32c(x, "x")
    B, d = x.shape
    L = 0 if kernels is None else kernels.shape[0]
    y = torch.empty(B, d, dtype=torch.float32, device=x.device)
    mode = _C.CROSS_VECTOR if parameterization == "vector" else _C.CROSS_MATRIX
    kernels = None if kernels is None else _f32c(kernels, "kernels")
    bias = None if bias is None else _f32c(bias, "bias")
    need = int(_C.lib().dctr_crossnet_workspace_bytes(d, L, mode, _ptr(kernels)))
    ws = torch.empty(need // 4, dtype=torch.float32, device=x.device) if need else None     # re-packed W rows
    _C.check(_C.lib().dctr_crossnet_fwd(_ptr(x), B, d, d, _ptr(kernels), _ptr(bias), L, mode, _ptr(y), d,
                                        _ptr(ws), need, _C.stream_ptr()), "dctr_crossnet_fwd")
    return y


def crossnet_head(x, kernels, bias, parameterization, head_w, want_y=False, workspace=None, save_u=None, save_x=None):
    """CrossNet.call with the branch's share of the model's Dense(1) fused in (dctr_crossnet_head_fwd): returns (logit [B] =
    x_L . head_w, y [B,d] or None).  ``workspace``: a dict that keeps the re-packed kernel rows of the matrix form between calls —
    the caller clears it when the kernels change (``workspace_ready``)."""
    _dev_check(x, kernels, bias, head_w)
    x = _f32c(x, "x")
    B, d = x.shape
    L = 0 if kernels is None else kernels.shape[0]
    mode = _C.CROSS_VECTOR if parameterization == "vector" else _C.CROSS_MATRIX
    kernels = None if kernels is None else _f32c(kernels, "kernels")
    bias = None if bias is None else _f32c(bias, "bias")
    head_w = _f32c(head_w, "head_w")
    need = int(_C.lib().dctr_crossnet_workspace_bytes(d, L, mode, _ptr(kernels)))
    ready = 0
    ws = None
    if need:
        ws = workspace.get("ws") if workspace is not None else None
        ready = 1 if (ws is not None and ws.numel() * 4 >= need) else 0
        if not ready:
            ws = torch.empty(need // 4, dtype=torch.float32, device=x.device)
            if workspace is not None:
                workspace["ws"] = ws
    y = torch.empty(B, d, dtype=torch.float32, device=x.device) if want_y else None
    logit = torch.empty(B, dtype=torch.float32, device=x.device)
    a = _C.CrossnetArgs(x=x.data_ptr(), batch=B, x_stride=x.stride(0), dim=d, layers=L, mode=mode, workspace_ready=ready,
                        kernels=None if kernels is None else kernels.data_ptr(), bias=None if bias is None else bias.data_ptr(),
                        y=None if y is None else y.data_ptr(), y_stride=d, workspace=None if ws is None else ws.data_ptr(),
                        workspace_bytes=need, head_w=head_w.data_ptr(), logit=logit.data_ptr(), save_u=_ptr(save_u), save_x=_ptr(save_x))
    _C.check(_C.lib().dctr_crossnet_head_fwd(ctypes.byref(a), _C.stream_ptr()), "dctr_crossnet_head_fwd")
    return logit, y


def cin_output_dim(layer_size, split_half):
    if split_half:
        return sum(layer_size[:-1]) // 2 + layer_size[-1]
    return sum(layer_size)


def cin(x, filters, biases, layer_size, split_half=True, activation="relu", fields=None, dim=None, out=None, save_y=None, fold=True,
        workspace=None, workspace_ready=False):
    """CIN.call (reference interaction.py:277-325): x [B,F0,D] (or, with ``fields``/``dim`` given, the leading
    F0*D columns of a [B, stride] concat buffer read in place); filters[k] [F0*Fk, Hk]; -> [B, featuremap_num].
    ``save_y``: per layer a [B*D, H_k] float32 tensor that receives the layer's activations (training: ``cin_bwd(saved_y=)``).
    ``fold``: hand the library the workspace for layer 0's symmetry fold (x_k = x_0 there: the F0 (F0 + 1) / 2 pairs i <= j against
    W[ij] + W[ji]); False walks all F0 x F0 products (same result up to the rounding of that sum).  ``workspace``: a caller-owned
    float32 tensor of ``cin_workspace_bytes`` for the fold (default: the per-stream scratch, rewritten by every call);
    ``workspace_ready``: it still holds an earlier call's fold of the same filter values (no fold launch)."""
    _dev_check(x, *filters, *biases)
    x, B, F0, D, x_stride, _ = _x_in_place("cin", x, fields, dim)
    n = len(layer_size)
    filters = [_f32c(f, "filter").reshape(-1, h) for f, h in zip(filters, layer_size)]
    biases = [_f32c(b, "bias") for b in biases]
    if out is None:
        out = torch.empty(B, cin_output_dim(list(layer_size), split_half), dtype=torch.float32, device=x.device)
    ls = _i32_array(layer_size)
    fp, bp = _ptr_array(filters), _ptr_array(biases)
    if activation not in _C.ACT_CODES or _C.ACT_CODES[activation] == _C.ACT_DICE:
        raise ValueError("CIN activation %r is not supported" % (activation,))
    a = _C.CinArgs(x=x.data_ptr(), batch=B, x_stride=x_stride, fields=F0, dim=D, n_layers=n, split_half=int(bool(split_half)),
                   activation=_C.ACT_CODES[activation], layer_size=ctypes.cast(ls, ctypes.c_void_p),
                   filters=ctypes.cast(fp, ctypes.c_void_p), bias=ctypes.cast(bp, ctypes.c_void_p), out=out.data_ptr(),
                   workspace=None, workspace_bytes=0)
    if save_y is not None:
        _check_saved_y(save_y, B * D, layer_size, x)
        sp = _ptr_array(list(save_y))
        a.save_y = ctypes.cast(sp, ctypes.c_void_p)
    need = int(_C.lib().dctr_cin_workspace_bytes(ctypes.byref(a)))

    def with_workspace(need):
        if workspace is not None:
            if workspace.dtype != torch.float32 or not workspace.is_contiguous() or workspace.device != x.device:
                raise ValueError("cin: workspace must be a contiguous float32 tensor (dctr_cin_workspace_bytes: %d bytes) on %s" % (need, x.device))
            # (its size is the library's to judge: the fold needs all of its share, the sliced route works in any room for >= 64 samples)
            ws, a.workspace_ready, need = workspace, int(bool(workspace_ready)), workspace.numel() * 4
        else:
            ws = _scratch(x.device, need)   # rewritten by every call (the filters may have moved): stream order keeps calls apart
        a.workspace, a.workspace_bytes = ws.data_ptr(), need
        return ws
    ws = with_workspace(need) if (fold and need) else None
    rc = _C.lib().dctr_cin_fwd(ctypes.byref(a), _C.stream_ptr())
    if rc == _C.E_NULL and ws is None and need:
        # fold=False, but the arguments take a route that REQUIRES its workspace (samples in slices of d, layer by layer): the library
        # says so before it launches anything
        ws = with_workspace(need)
        rc = _C.lib().dctr_cin_fwd(ctypes.byref(a), _C.stream_ptr())
    _C.check(rc, "dctr_cin_fwd")
    return out


def cin_supported(fields, dim, layer_size, split_half=True, activation="relu", gather=None, fused_head=False, batch=4096):
    """dctr_cin_fwd_supported: would the library take this CIN (``gather`` None: dctr_cin_fwd over a materialised x; else a
    GatherFmArgs — or a dict of its summary fields n_fields / uniform_dim / all_dim4 / any_hash / any_identity / any_pitch — :
    dctr_cin_gather_fwd, ``fused_head`` with the Dense(1) on chip)?  The host asks; it does not keep a copy of the kernels' limits."""
    ls = _i32_array(layer_size)
    a = _C.CinArgs(batch=int(batch), fields=int(fields), dim=int(dim), n_layers=len(layer_size), split_half=int(bool(split_half)),
                   activation=_C.ACT_CODES.get(activation, -1), layer_size=ctypes.cast(ls, ctypes.c_void_p))
    g = None
    if gather is not None:
        if isinstance(gather, dict):
            gather = _C.GatherFmArgs(batch=int(batch), **{k: int(v) for k, v in gather.items()})
        g = ctypes.byref(gather)
    return bool(_C.lib().dctr_cin_fwd_supported(ctypes.byref(a), g, int(bool(fused_head))))


def cin_gather(gather, filters, biases, layer_size, split_half, activation, dim, head_w, logit, workspace, workspace_ready=False, out=None):
    """CIN over the embeddings of a gather with the Dense(1) head fused (dctr_cin_gather_fwd; reference models/xdeepfm.py:52-66):
    ``gather`` = the marshalled dctr_gather_fm_args_t of the batch (EmbeddingStage.gather_args), ``head_w`` [featuremap_num(, 1)],
    ``logit`` [B] float32 receives maps . head_w, ``workspace`` = the caller-owned fold workspace (cin_workspace_bytes).
    Without a head (``head_w`` / ``logit`` None) the summed maps go to ``out`` [B, featuremap_num] as ``cin`` writes them.
    Returns False when the library declines the shape (hashed / pooled fields, dim % 4 != 0): the caller takes dnn_in + ``cin``."""
    n = len(layer_size)
    filters = [_f32c(f, "filter").reshape(-1, h) for f, h in zip(filters, layer_size)]
    biases = [_f32c(b, "bias") for b in biases]
    ls = _i32_array(layer_size)
    fp, bp = _ptr_array(filters), _ptr_array(biases)
    if activation not in _C.ACT_CODES or _C.ACT_CODES[activation] == _C.ACT_DICE:
        raise ValueError("CIN activation %r is not supported" % (activation,))
    a = _C.CinArgs(x=None, batch=int(gather.batch), x_stride=0, fields=int(gather.n_fields), dim=int(dim), n_layers=n,
                   split_half=int(bool(split_half)), activation=_C.ACT_CODES[activation], layer_size=ctypes.cast(ls, ctypes.c_void_p),
                   filters=ctypes.cast(fp, ctypes.c_void_p), bias=ctypes.cast(bp, ctypes.c_void_p),
                   out=None if out is None else out.data_ptr(), workspace=None, workspace_bytes=0)
    need = int(_C.lib().dctr_cin_workspace_bytes(ctypes.byref(a)))
    if need and workspace is not None:
        if workspace.numel() * 4 < need:
            raise ValueError("cin_gather: workspace of >= %d bytes needed" % need)
        a.workspace, a.workspace_bytes, a.workspace_ready = workspace.data_ptr(), need, int(bool(workspace_ready))
    hw = None if head_w is None else _f32c(head_w, "head_w").reshape(-1)
    rc = _C.lib().dctr_cin_gather_fwd(ctypes.byref(a), ctypes.byref(gather), None if hw is None else hw.data_ptr(),
                                      None if logit is None else logit.data_ptr(), _C.stream_ptr())
    if rc == _C.E_UNSUPPORTED:
        return False
    _C.check(rc, "dctr_cin_gather_fwd")
    return True


def cin_workspace_bytes(fields, dim, layer_size, split_half=False):
    """Bytes of the workspace dctr_cin_fwd takes for a CIN over ``fields`` embeddings of width ``dim``: layer 0's fold (0: no fold), or
    the room the sliced (embedding_dim > 128 ...) / layer-by-layer (a layer of more than ~480 maps) routes REQUIRE.  split_half=False
    (the default) is the larger need of the two."""
    ls = _i32_array(layer_size)
    a = _C.CinArgs(fields=int(fields), dim=int(dim), n_layers=len(layer_size), split_half=int(bool(split_half)),
                   layer_size=ctypes.cast(ls, ctypes.c_void_p))
    return int(_C.lib().dctr_cin_workspace_bytes(ctypes.byref(a)))


def _check_saved_y(ys, rows, layer_size, x):
    if len(ys) != len(layer_size):
        raise ValueError("save_y / saved_y: one tensor per CIN layer")
    for t, h in zip(ys, layer_size):
        if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != (rows, h) or t.device != x.device:
            raise ValueError("save_y / saved_y: expected a contiguous float32 [%d, %d] tensor on %s" % (rows, h, x.device))


def _interacting_args(B, F, E, x_stride, weights, att_embedding_size, head_num, use_res, scaling):
    flat = []
    for layer in weights:
        flat += [layer[0], layer[1], layer[2], layer[3] if use_res and len(layer) > 3 else None]
    lp = _ptr_array(flat)
    a = _C.interacting.Args(batch=int(B), x_stride=int(x_stride), fields=int(F), dim=int(E), n_layers=len(weights),
                           att_embedding_size=int(att_embedding_size), head_num=int(head_num), use_res=int(bool(use_res)),
                           scaling=int(bool(scaling)), layers=ctypes.cast(lp, ctypes.c_void_p))
    return a, lp


def interacting_workspace_bytes(batch, fields, dim, n_layers, att_embedding_size, head_num, use_res=True, with_out=True):
    """Bytes of the workspace dctr_interacting_fwd needs for these shapes (0 on the LDS route; read from the library)."""
    a = _C.interacting.Args(batch=int(batch), x_stride=int(fields) * int(dim), fields=int(fields), dim=int(dim), n_layers=int(n_layers),
                           att_embedding_size=int(att_embedding_size), head_num=int(head_num), use_res=int(bool(use_res)),
                           out_stride=int(fields) * int(att_embedding_size) * int(head_num))
    if with_out:
        a.out = 16          # (only its presence is read)
    return int(_C.lib().dctr_interacting_workspace_bytes(ctypes.byref(a)))


def interacting(x, weights, att_embedding_size, head_num, use_res, scaling, fields=None, dim=None, out=None, head_w=None, logit=None,
                workspace=None):
    """InteractingLayer.call (reference interaction.py:749-779) stacked over len(weights) layers (models/autoint.py:61-64), one launch:
    x [B,F,E] (or, with ``fields``/``dim`` given, the leading F*E columns of a [B, stride] buffer read in place); ``weights``: per layer
    (query, key, value, res) [E_l, d*H] (res unused unless ``use_res``).  Writes the flattened last layer to ``out`` [B, F*d*H] (a 2-D,
    possibly strided view; allocated when neither ``out`` nor ``head_w`` is given) and / or, with ``head_w`` [F*d*H(, 1)], the Dense(1)
    over it to ``logit`` [B].  ``workspace``: a float32 tensor of >= interacting_workspace_bytes (default: the per-stream scratch).
    Returns ``out`` (or ``logit`` when only the head is asked for)."""
    x, B, F, E, x_stride, _ = _x_in_place("interacting", x, fields, dim)
    weights = [[None if w is None else _f32c(w, "weight") for w in layer] for layer in weights]
    _dev_check(x, out, logit, head_w, *[w for layer in weights for w in layer])
    dH = int(att_embedding_size) * int(head_num)
    if head_w is None and out is None:
        out = torch.empty(B, F * dH, dtype=torch.float32, device=x.device)
    if head_w is not None:
        head_w = _f32c(head_w, "head_w").reshape(-1)
        if head_w.numel() != F * dH:
            raise ValueError("interacting: head_w must hold fields*d*H = %d values" % (F * dH))
        if logit is None:
            logit = torch.empty(B, dtype=torch.float32, device=x.device)
    a, keep = _interacting_args(B, F, E, x_stride, weights, att_embedding_size, head_num, use_res, scaling)
    a.x = x.data_ptr()
    if out is not None:
        a.out, a.out_stride = out.data_ptr(), _rows2d("interacting", "out", out, B, F * dH)
    if head_w is not None:
        a.head_w, a.logit = head_w.data_ptr(), logit.data_ptr()
    _workspace("interacting", a, int(_C.lib().dctr_interacting_workspace_bytes(ctypes.byref(a))), workspace, x.device)
    _C.check(_C.lib().dctr_interacting_fwd(ctypes.byref(a), _C.stream_ptr()), "dctr_interacting_fwd")
    del keep
    return out if out is not None else logit


def _interacting_bwd_shape(fields, dim, n_layers, att_embedding_size, head_num, use_res, batch=1):
    dH = int(att_embedding_size) * int(head_num)
    b = _C.interacting.BwdArgs(dy_stride=int(fields) * dH)
    b.fwd = _C.interacting.Args(batch=int(batch), x_stride=int(fields) * int(dim), fields=int(fields), dim=int(dim),
                                n_layers=int(n_layers), att_embedding_size=int(att_embedding_size), head_num=int(head_num),
                                use_res=int(bool(use_res)))
    return b


def interacting_bwd_supported(fields, dim, n_layers, att_embedding_size, head_num, use_res=True):
    """Does dctr_interacting_bwd take these shapes (read from the library)?"""
    b = _interacting_bwd_shape(fields, dim, n_layers, att_embedding_size, head_num, use_res)
    return bool(_C.lib().dctr_interacting_bwd_supported(ctypes.byref(b)))


def interacting_bwd_workspace_bytes(batch, fields, dim, n_layers, att_embedding_size, head_num, use_res=True):
    """Bytes of the workspace dctr_interacting_bwd needs for these shapes (0 on the LDS route; read from the library)."""
    b = _interacting_bwd_shape(fields, dim, n_layers, att_embedding_size, head_num, use_res, batch)
    return int(_C.lib().dctr_interacting_bwd_workspace_bytes(ctypes.byref(b)))


def interacting_bwd(x, weights, att_embedding_size, head_num, use_res, scaling, dy, fields=None, dim=None, dx=None, accumulate=False,
                    d_weights=None, max_blocks=0, workspace=None):
    """Backward of interacting() over the whole stack, one launch (include/dctr.h: dctr_interacting_bwd); the forward saves nothing.
    ``x`` / ``weights`` / ``fields`` / ``dim`` as interacting(); ``dy``: a float32 [B, >= F*d*H] view, the gradient w.r.t. the flattened
    last layer.  ``dx`` [B, >= F*E] (2-D view): its leading F*E columns are written, or added to with ``accumulate``.  ``d_weights``: per
    layer (d_query, d_key, d_value, d_res), contiguous and of the weights' shapes, ACCUMULATED into; any entry, or the list, may be None."""
    x, B, F, E, x_stride, _ = _x_in_place("interacting_bwd", x, fields, dim)
    weights = [[None if w is None else _f32c(w, "weight") for w in layer] for layer in weights]
    dH = int(att_embedding_size) * int(head_num)
    dy_stride = _rows2d("interacting_bwd", "dy", dy, B, F * dH)
    dx_stride = 0 if dx is None else _rows2d("interacting_bwd", "dx", dx, B, F * E)
    flat_d = []
    if d_weights is not None:
        if len(d_weights) != len(weights):
            raise ValueError("interacting_bwd: d_weights must hold one entry per layer")
        for l, layer in enumerate(d_weights):
            layer = list(layer) + [None] * (4 - len(layer))
            for m in range(4):
                g = layer[m] if m < 3 or use_res else None
                if g is not None:
                    _vec("interacting_bwd", "d_weights[%d][%d]" % (l, m), g, (E if l == 0 else dH) * dH)
                flat_d.append(g)
    _dev_check(x, dy, dx, *([w for layer in weights for w in layer] + flat_d))
    b = _C.interacting.BwdArgs(dy=dy.data_ptr(), dy_stride=dy_stride, accumulate=int(bool(accumulate)), max_blocks=int(max_blocks))
    b.fwd, keep = _interacting_args(B, F, E, x_stride, weights, att_embedding_size, head_num, use_res, scaling)
    b.fwd.x = x.data_ptr()
    if dx is not None:
        b.dx, b.dx_stride = dx.data_ptr(), dx_stride
    keep_d = _ptr_array(flat_d)
    if flat_d:
        b.d_layers = ctypes.cast(keep_d, ctypes.c_void_p)
    _workspace("interacting_bwd", b.fwd, int(_C.lib().dctr_interacting_bwd_workspace_bytes(ctypes.byref(b))), workspace, x.device)
    _C.check(_C.lib().dctr_interacting_bwd(ctypes.byref(b), _C.stream_ptr()), "dctr_interacting_bwd")
    del keep, keep_d


class InteractingFunction(torch.autograd.Function):
    """The InteractingLayer stack as one differentiable op: interacting() forward and interacting_bwd() backward, one launch each.
    ``apply(x, att_embedding_size, head_num, use_res, scaling, *weights)``: x [B,F,E]; ``weights`` flat, four per layer (query, key,
    value, res — res None when ``use_res`` is off).  Returns [B, F*d*H].  Only x and the weights are saved: the backward recomputes."""

    @staticmethod
    def forward(ctx, x, att_embedding_size, head_num, use_res, scaling, *weights):
        ctx.cfg = (int(att_embedding_size), int(head_num), bool(use_res), bool(scaling))
        x = x.detach()
        ws = [None if w is None else w.detach() for w in weights]
        out = torch.empty(x.shape[0], x.shape[1] * ctx.cfg[0] * ctx.cfg[1], dtype=torch.float32, device=x.device)
        interacting(x, [ws[i:i + 4] for i in range(0, len(ws), 4)], ctx.cfg[0], ctx.cfg[1], ctx.cfg[2], ctx.cfg[3], out=out)
        ctx.present = [w is not None for w in ws]
        ctx.save_for_backward(x, *[w for w in ws if w is not None])
        return out

    @staticmethod
    def backward(ctx, dy):
        d, H, use_res, scaling = ctx.cfg
        saved = list(ctx.saved_tensors)
        x, it = saved[0], iter(saved[1:])
        ws = [next(it) if present else None for present in ctx.present]
        dy = _grad_operand(dy, True)
        dx = torch.empty_like(x, memory_format=torch.contiguous_format) if ctx.needs_input_grad[0] else None
        wanted = [w is not None and ctx.needs_input_grad[5 + i] and (i % 4 < 3 or use_res) for i, w in enumerate(ws)]
        _, grads = _zeroed_grads(ws, wanted, x.device)      # one fill for the whole stack
        interacting_bwd(x, [ws[i:i + 4] for i in range(0, len(ws), 4)], d, H, use_res, scaling, dy,
                        dx=None if dx is None else dx.view(dx.shape[0], -1),
                        d_weights=[grads[i:i + 4] for i in range(0, len(ws), 4)])
        return (dx, None, None, None, None) + tuple(grads)


_BILINEAR_TABLES = {}


def bilinear_table(matrices):
    """DEVICE int64 table of the matrices' addresses (dctr_bilinear_args_t.bilinear_w).  Cached per tuple of addresses: in-place
    updates (set_weights, the optimiser) keep a table valid, and a reallocated weight gives a new key, hence a fresh table."""
    key = tuple(m.data_ptr() for m in matrices)
    t = _BILINEAR_TABLES.get(key)
    if t is None:
        if len(_BILINEAR_TABLES) >= 64:      # (tables of freed weights must not pile up)
            _BILINEAR_TABLES.clear()
        t = _BILINEAR_TABLES[key] = torch.tensor(key, dtype=torch.int64).to(matrices[0].device)
    return t


def bilinear_weight_count(bilinear_type, fields):
    """Matrices of one BilinearInteraction over `fields` inputs (reference interaction.py:1174-1185)."""
    if bilinear_type not in _C.bilinear.TYPES:
        raise NotImplementedError("bilinear_type %r: expected 'all', 'each' or 'interaction'" % (bilinear_type,))
    return {"all": 1, "each": fields - 1, "interaction": fields * (fields - 1) // 2}[bilinear_type]


def _bilinear_args(B, F, E, x_stride, bilinear_type, mode, r, dense_cols, out_stride):
    return _C.bilinear.Args(batch=int(B), x_stride=int(x_stride), fields=int(F), dim=int(E),
                            bilinear_type=_C.bilinear.TYPES.get(bilinear_type, -1), mode=int(mode), reduction_size=int(r),
                            dense_cols=int(dense_cols), out_stride=int(out_stride))


def senet_bilinear_width(fields, dim, mode, dense_cols=0):
    P = fields * (fields - 1) // 2
    return {_C.bilinear.MODE_MODEL: 2 * P * dim + dense_cols, _C.bilinear.MODE_SENET: fields * dim,
            _C.bilinear.MODE_LAYER: P * dim}[mode]


def senet_bilinear_workspace_bytes(batch, fields, dim, bilinear_type="interaction", mode=0, reduction_size=1):
    """Bytes of the workspace dctr_bilinear_fwd needs for these shapes (0 on the LDS route; read from the library)."""
    a = _bilinear_args(batch, fields, dim, fields * dim, bilinear_type, mode, reduction_size, 0,
                       senet_bilinear_width(fields, dim, mode))
    return int(_C.lib().dctr_bilinear_workspace_bytes(ctypes.byref(a)))


def senet_bilinear(x, senet_w=None, senet_bilinear_w=None, bilinear_w=None, bilinear_type="interaction", fields=None, dim=None,
                   dense_cols=0, out=None, workspace=None):
    """SENETLayer.call and / or BilinearInteraction.call (reference interaction.py:1113-1209), one launch.  x [B,F,E] (or, with
    ``fields`` / ``dim``, the leading F*E columns of a [B, stride] buffer read in place, ``dense_cols`` more columns behind them).
    ``senet_w`` = (W_1 [F,r], W_2 [r,F]); ``senet_bilinear_w`` / ``bilinear_w``: one BilinearInteraction's matrices [E,E] each (1, F-1
    or F(F-1)/2 of them, by ``bilinear_type``).  Which are given picks the mode:
      * all three (FiBiNET, models/fibinet.py:50-58): out [B, >= 2*P*E + dense_cols] = per pair [bilinear over the SENET output,
        E floats | bilinear over x, E floats] (the two outputs concatenated on their last axis, flattened), then the dense columns;
      * ``senet_w`` alone: out [B, >= F*E] = the SENET output, flattened;
      * ``bilinear_w`` alone: out [B, >= P*E] = the bilinear interaction over x.
    ``out`` is a 2-D (possibly strided) view, allocated when not given; ``workspace``: a float32 tensor of
    >= senet_bilinear_workspace_bytes (default: the per-stream scratch).  Returns ``out``."""
    x, B, F, E, x_stride, mode, r, (w1, w2), tables, tensors = _bilinear_operands(
        "senet_bilinear", x, fields, dim, senet_w, senet_bilinear_w, bilinear_w, bilinear_type, dense_cols)
    _dev_check(out, *tensors)
    width = senet_bilinear_width(F, E, mode, dense_cols)
    if out is None:
        out = torch.empty(B, width, dtype=torch.float32, device=x.device)
    a = _bilinear_args(B, F, E, x_stride, bilinear_type, mode, max(r, 1), dense_cols, _rows2d("senet_bilinear", "out", out, B, width))
    a.x, a.out = x.data_ptr(), out.data_ptr()
    if senet_w is not None:
        a.senet_w1, a.senet_w2 = w1.data_ptr(), w2.data_ptr()
    if tables[0] is not None:
        a.senet_bilinear_w = tables[0].data_ptr()
    if tables[1] is not None:
        a.bilinear_w = tables[1].data_ptr()
    _workspace("senet_bilinear", a, int(_C.lib().dctr_bilinear_workspace_bytes(ctypes.byref(a))), workspace, x.device)
    _C.check(_C.lib().dctr_bilinear_fwd(ctypes.byref(a), _C.stream_ptr()), "dctr_bilinear_fwd")
    return out


_BILINEAR_MODES = {"model": _C.bilinear.MODE_MODEL, "senet": _C.bilinear.MODE_SENET, "layer": _C.bilinear.MODE_LAYER}


def _bilinear_bwd_shape(batch, fields, dim, bilinear_type, mode, reduction_size, dense_cols=0):
    if mode not in _BILINEAR_MODES:
        raise ValueError("senet_bilinear_bwd: mode %r: expected 'model', 'senet' or 'layer'" % (mode,))
    m = _BILINEAR_MODES[mode]
    width = senet_bilinear_width(int(fields), int(dim), m, int(dense_cols))
    b = _C.bilinear.BwdArgs(d_out_stride=width, dx_stride=int(fields) * int(dim) + int(dense_cols))
    b.fwd = _bilinear_args(batch, fields, dim, int(fields) * int(dim) + int(dense_cols), bilinear_type, m, max(int(reduction_size), 1),
                           dense_cols, width)
    return b


def senet_bilinear_bwd_supported(fields, dim, bilinear_type="interaction", mode="model", reduction_size=1):
    """Does dctr_bilinear_bwd take these shapes (read from the library)?"""
    return bool(_C.lib().dctr_bilinear_bwd_supported(ctypes.byref(_bilinear_bwd_shape(1, fields, dim, bilinear_type, mode,
                                                                                      reduction_size))))


def senet_bilinear_bwd_workspace_bytes(batch, fields, dim, bilinear_type="interaction", mode="model", reduction_size=1):
    """Bytes of the workspace dctr_bilinear_bwd needs for these shapes (0 on the LDS route; read from the library)."""
    return int(_C.lib().dctr_bilinear_bwd_workspace_bytes(ctypes.byref(_bilinear_bwd_shape(batch, fields, dim, bilinear_type, mode,
                                                                                           reduction_size))))


def senet_bilinear_bwd(x, d_out, senet_w=None, senet_bilinear_w=None, bilinear_w=None, bilinear_type="interaction", fields=None,
                       dim=None, dense_cols=0, d_out_offset=0, dx=None, dx_offset=0, accumulate=False, d_senet_w=None,
                       d_senet_bilinear_w=None, d_bilinear_w=None, max_blocks=0, workspace=None):
    """Backward of senet_bilinear(), one launch (include/dctr.h: dctr_bilinear_bwd); the forward saves nothing.  ``x`` / the weights /
    ``bilinear_type`` / ``fields`` / ``dim`` / ``dense_cols`` as senet_bilinear(): which weights are given picks the mode.  ``d_out``: a
    float32 2-D view whose row holds the gradient of the forward's output row from column ``d_out_offset``.  ``dx``: a 2-D view
    [B, >= dx_offset + F*E + dense_cols] (or [B,F,E] contiguous) whose F*E embedding columns (and, in the FiBiNET form, the
    ``dense_cols`` behind them) from ``dx_offset`` are written, or added to with ``accumulate`` — bit-identical from call to call.
    ``d_senet_w`` = (dW_1 [F,r] or None, dW_2 [r,F] or None); ``d_senet_bilinear_w`` / ``d_bilinear_w``: ONE contiguous [nW,E,E] tensor
    each.  All weight gradients are ACCUMULATED into; they leave through float atomics and may differ in the last bits from call to
    call.  Any output may be None, but not all of them."""
    op = "senet_bilinear_bwd"
    x, B, F, E, x_stride, mode, r, (w1, w2), tables, tensors = _bilinear_operands(
        op, x, fields, dim, senet_w, senet_bilinear_w, bilinear_w, bilinear_type, dense_cols)
    nW = bilinear_weight_count(bilinear_type, F)
    width = senet_bilinear_width(F, E, mode, dense_cols)
    d_out_stride = _rows2d(op, "d_out", d_out, B, width, d_out_offset)
    dx_stride = _dx_operand(op, dx, B, F, E, dx_offset, dense_cols)
    dw1, dw2 = d_senet_w if d_senet_w is not None else (None, None)
    if senet_w is None and (dw1 is not None or dw2 is not None):
        raise ValueError("senet_bilinear_bwd: d_senet_w without senet_w")
    if dw1 is not None:
        _vec(op, "d_senet_w[0]", dw1, F * r)
    if dw2 is not None:
        _vec(op, "d_senet_w[1]", dw2, r * F)
    for name, g, ws in (("d_senet_bilinear_w", d_senet_bilinear_w, senet_bilinear_w), ("d_bilinear_w", d_bilinear_w, bilinear_w)):
        if g is not None:
            if ws is None:
                raise ValueError("senet_bilinear_bwd: %s without its weights" % name)
            _vec(op, name, g, nW * E * E)
    if dx is None and dw1 is None and dw2 is None and d_senet_bilinear_w is None and d_bilinear_w is None:
        raise ValueError("senet_bilinear_bwd: no gradient asked for (dx and every d_* are None)")
    for t in [d_out, dx, dw1, dw2, d_senet_bilinear_w, d_bilinear_w] + tensors:
        if t is not None and t.device != x.device:
            raise ValueError("senet_bilinear_bwd: operands on different devices (%s and %s)" % (x.device, t.device))
    _dev_check(d_out, dx, dw1, dw2, d_senet_bilinear_w, d_bilinear_w, *tensors)
    b = _C.bilinear.BwdArgs(d_out=d_out.data_ptr(), d_out_stride=d_out_stride, d_out_offset=int(d_out_offset), dx_stride=dx_stride,
                            dx_offset=int(dx_offset), accumulate=int(bool(accumulate)), max_blocks=int(max_blocks))
    b.fwd = _bilinear_args(B, F, E, x_stride, bilinear_type, mode, max(r, 1), dense_cols, width)
    b.fwd.x = x.data_ptr()
    if senet_w is not None:
        b.fwd.senet_w1, b.fwd.senet_w2 = w1.data_ptr(), w2.data_ptr()
    if tables[0] is not None:
        b.fwd.senet_bilinear_w = tables[0].data_ptr()
    if tables[1] is not None:
        b.fwd.bilinear_w = tables[1].data_ptr()
    for name, t in (("dx", dx), ("d_senet_w1", dw1), ("d_senet_w2", dw2), ("d_senet_bilinear_w", d_senet_bilinear_w),
                    ("d_bilinear_w", d_bilinear_w)):
        if t is not None:
            setattr(b, name, t.data_ptr())
    _workspace(op, b, int(_C.lib().dctr_bilinear_bwd_workspace_bytes(ctypes.byref(b))), workspace, x.device)
    _C.check(_C.lib().dctr_bilinear_bwd(ctypes.byref(b), _C.stream_ptr()), "dctr_bilinear_bwd")


class SenetBilinearFunction(torch.autograd.Function):
    """SENETLayer / BilinearInteraction / FiBiNET's whole DNN-input row as one differentiable op: senet_bilinear() forward and
    senet_bilinear_bwd() backward, one launch each.  ``apply(x2d, fields, dim, dense_cols, bilinear_type, mode, *weights)``: x2d
    [B, F*E + dense_cols]; ``mode`` 'model' (weights = W_1, W_2, the nW SENET-side matrices, the nW raw-side matrices), 'senet' (W_1,
    W_2) or 'layer' (the nW matrices).  Returns the forward's row [B, width].  Only x and the weights are saved: the backward loads x
    again.  The per-matrix gradients are views of ONE zeroed buffer per layer.  Weight gradients leave the kernel through float atomics
    and may differ in the last bits from call to call; dx does not."""

    @staticmethod
    def _split(mode, bilinear_type, fields, ws):
        """(senet_w, senet_bilinear_w, bilinear_w) of the flat weight list."""
        nW = bilinear_weight_count(bilinear_type, fields)
        if mode == "model":
            if len(ws) != 2 + 2 * nW:
                raise ValueError("SenetBilinearFunction: mode 'model' takes W_1, W_2 and 2 x %d matrices" % nW)
            return (ws[0], ws[1]), ws[2:2 + nW], ws[2 + nW:]
        if mode == "senet":
            if len(ws) != 2:
                raise ValueError("SenetBilinearFunction: mode 'senet' takes W_1 and W_2")
            return (ws[0], ws[1]), None, None
        if mode == "layer":
            if len(ws) != nW:
                raise ValueError("SenetBilinearFunction: mode 'layer' takes %d matrices" % nW)
            return None, None, ws
        raise ValueError("SenetBilinearFunction: mode %r: expected 'model', 'senet' or 'layer'" % (mode,))

    @staticmethod
    def forward(ctx, x, fields, dim, dense_cols, bilinear_type, mode, *weights):
        ctx.cfg = (int(fields), int(dim), int(dense_cols), bilinear_type, mode)
        x = x.detach()
        if x.dtype != torch.float32 or x.stride(-1) != 1:
            x = x.float().contiguous()
        ws = [w.detach() for w in weights]
        sw, sbw, bw = SenetBilinearFunction._split(mode, bilinear_type, fields, ws)
        out = senet_bilinear(x, senet_w=sw, senet_bilinear_w=sbw, bilinear_w=bw, bilinear_type=bilinear_type, fields=fields, dim=dim,
                             dense_cols=dense_cols)
        ctx.save_for_backward(x, *ws)
        return out

    @staticmethod
    def backward(ctx, d_out):
        saved = list(ctx.saved_tensors)
        x, ws = saved[0], saved[1:]
        F, E, D, bilinear_type, mode = ctx.cfg
        sw, sbw, bw = SenetBilinearFunction._split(mode, bilinear_type, F, ws)
        need = ctx.needs_input_grad
        want_dx = need[0]
        wneed = list(need[6:])
        d_out = _grad_operand(d_out, True)
        dx = torch.empty(x.shape[0], F * E + D, dtype=torch.float32, device=x.device) if want_dx else None
        grads = [None] * len(ws)
        at = 0
        d_senet_w = None
        if sw is not None:
            # W_1 and W_2 are small: a zeroed tensor each
            pair = [torch.zeros_like(ws[k], memory_format=torch.contiguous_format) if wneed[k] else None for k in (0, 1)]
            grads[0], grads[1] = pair
            d_senet_w = tuple(pair)
            at = 2
        flats = []
        for layer in (sbw, bw):
            if layer is None:
                flats.append(None)
                continue
            n = len(layer)
            flat, grads[at:at + n] = _zeroed_grads(layer, wneed[at:at + n], x.device)     # [n,E,E] behind the per-matrix views
            flats.append(flat)
            at += n
        if want_dx or any(g is not None for g in grads):
            senet_bilinear_bwd(x, d_out, senet_w=sw, senet_bilinear_w=sbw, bilinear_w=bw, bilinear_type=bilinear_type, fields=F, dim=E,
                               dense_cols=D, dx=dx, d_senet_w=d_senet_w, d_senet_bilinear_w=flats[0], d_bilinear_w=flats[1])
        return (dx, None, None, None, None, None) + tuple(grads)


def _fieldpair_args(kind, B, F, E, x_stride, x_offset=0):
    return _C.fieldpair.Args(batch=int(B), x_stride=int(x_stride), x_offset=int(x_offset), fields=int(F), dim=int(E), kind=int(kind))


def fieldpair_workspace_bytes(batch, fields, dim, kind="fefm", pairs=True):
    """Bytes of the workspace dctr_fieldpair_fwd needs for these shapes (0 on the LDS route; read from the library)."""
    a = _fieldpair_args(_FIELDPAIR_KINDS[kind], batch, fields, dim, fields * dim)
    P = fields * (fields - 1) // 2
    if kind == "fefm" and pairs:
        a.pairs_out, a.pairs_stride = 16, P         # (only whether it is null enters the plan)
    return int(_C.lib().dctr_fieldpair_workspace_bytes(ctypes.byref(a)))


_FIELDPAIR_KINDS = {"fefm": _C.fieldpair.FEFM, "fwfm": _C.fieldpair.FWFM}


def fieldpair(x, weights, kind="fefm", fields=None, dim=None, x_offset=0, pairs=None, pairs_offset=0, logit=None, add=None,
              workspace=None):
    """FEFMLayer.call / FwFMLayer.call (reference interaction.py:1351-1499), one launch.  x [B,F,E] (or, with ``fields`` / ``dim``, the
    F*E columns from ``x_offset`` of a [B, stride] buffer read in place: one feature group's slice of dnn_in).
      * kind "fefm": ``weights`` = the P = F(F-1)/2 matrices [E,E] in itertools.combinations order (the live per-name tensors: the
        kernel forms W + W^T itself).  ``pairs``: True (a new [B,P] tensor), or a float32 2-D view whose row receives the P scalars
        from column ``pairs_offset`` (e.g. dnn_in behind its dense columns); ``logit``: True or a float32 [B] tensor = their row sum.
      * kind "fwfm": ``weights`` = field_pair_strengths [F,F] (only r[i][j], i < j is read); ``logit`` only (True by default).
    ``add`` [B] is added to the logit in the same launch.  ``workspace``: a float32 tensor of >= fieldpair_workspace_bytes (default:
    the per-stream scratch).  Returns (pairs, logit), None for an output not asked for."""
    x, B, F, E, x_stride, x_offset, P, wptr, tensors = _fieldpair_operands("fieldpair", x, weights, kind, fields, dim, x_offset)
    if kind == "fefm":
        if pairs is None and logit is None:
            pairs = True
    else:
        if pairs is not None:
            raise ValueError("fieldpair: the FwFM kind has no pair outputs")
        if logit is None:
            logit = True
    if pairs is True:
        pairs, pairs_offset = torch.empty(B, P, dtype=torch.float32, device=x.device), 0
    if logit is True:
        logit = torch.empty(B, dtype=torch.float32, device=x.device)
    pairs_stride = 0 if pairs is None else _rows2d("fieldpair", "pairs", pairs, B, P, pairs_offset)
    if logit is not None:
        _vec("fieldpair", "logit", logit, B)
    if add is not None:
        if logit is None:
            raise ValueError("fieldpair: add needs a logit output")
        add = _f32c(add, "add")
        if add.numel() != B:
            raise ValueError("fieldpair: add must hold %d elements" % B)
    _dev_check(pairs, logit, add, *tensors)
    a = _fieldpair_args(_FIELDPAIR_KINDS[kind], B, F, E, x_stride, x_offset)
    a.x, a.weights = x.data_ptr(), wptr.data_ptr()
    if pairs is not None:
        a.pairs_out, a.pairs_stride, a.pairs_offset = pairs.data_ptr(), pairs_stride, int(pairs_offset)
    if logit is not None:
        a.logit_out = logit.data_ptr()
    if add is not None:
        a.add = add.data_ptr()
    _workspace("fieldpair", a, int(_C.lib().dctr_fieldpair_workspace_bytes(ctypes.byref(a))), workspace, x.device)
    _C.check(_C.lib().dctr_fieldpair_fwd(ctypes.byref(a), _C.stream_ptr()), "dctr_fieldpair_fwd")
    return pairs, logit


def _fieldpair_bwd_shape(kind, batch, fields, dim):
    if kind not in _FIELDPAIR_KINDS:
        raise ValueError("fieldpair_bwd: kind %r: expected 'fefm' or 'fwfm'" % (kind,))
    b = _C.fieldpair.BwdArgs()
    b.fwd = _fieldpair_args(_FIELDPAIR_KINDS[kind], batch, fields, dim, int(fields) * int(dim))
    return b


def fieldpair_bwd_supported(fields, dim, kind="fefm"):
    """Does dctr_fieldpair_bwd take these shapes (read from the library)?"""
    return bool(_C.lib().dctr_fieldpair_bwd_supported(ctypes.byref(_fieldpair_bwd_shape(kind, 1, fields, dim))))


def fieldpair_bwd_workspace_bytes(batch, fields, dim, kind="fefm"):
    """Bytes of the workspace dctr_fieldpair_bwd needs for these shapes (0 on the LDS route; read from the library)."""
    return int(_C.lib().dctr_fieldpair_bwd_workspace_bytes(ctypes.byref(_fieldpair_bwd_shape(kind, batch, fields, dim))))


def fieldpair_bwd(x, weights, kind, d_pairs=None, d_pairs_offset=0, d_logit=None, fields=None, dim=None, x_offset=0, dx=None,
                  dx_offset=0, accumulate=False, d_weights=None, max_blocks=0, workspace=None):
    """Backward of fieldpair(), one launch (include/dctr.h: dctr_fieldpair_bwd); the forward saves nothing.  ``x`` / ``weights`` /
    ``kind`` / ``fields`` / ``dim`` / ``x_offset`` as fieldpair().  ``d_pairs`` (FEFM only): a float32 2-D view whose row holds the
    gradient of the P pair scalars from column ``d_pairs_offset``; ``d_logit`` [B]: the gradient of the logit; FEFM takes either or
    both, FwFM ``d_logit``.  ``dx``: a 2-D view [B, >= dx_offset + F*E] (or [B,F,E] contiguous) whose F*E columns from ``dx_offset`` are
    written, or added to with ``accumulate`` — bit-identical from call to call.  ``d_weights``: ACCUMULATED into; FEFM one contiguous
    [P,E,E] tensor, FwFM [F,F] of which only the strict upper triangle is touched.  Weight gradients leave through float atomics and
    may differ in the last bits from call to call."""
    x, B, F, E, x_stride, x_offset, P, wptr, tensors = _fieldpair_operands("fieldpair_bwd", x, weights, kind, fields, dim, x_offset)
    if kind == "fefm":
        if d_pairs is None and d_logit is None:
            raise ValueError("fieldpair_bwd: FEFM needs d_pairs and / or d_logit")
    else:
        if d_pairs is not None:
            raise ValueError("fieldpair_bwd: the FwFM kind has no pair gradients")
        if d_logit is None:
            raise ValueError("fieldpair_bwd: FwFM needs d_logit")
    d_pairs_stride = 0 if d_pairs is None else _rows2d("fieldpair_bwd", "d_pairs", d_pairs, B, P, d_pairs_offset)
    if d_logit is not None:
        _vec("fieldpair_bwd", "d_logit", d_logit, B)
    dx_stride = _dx_operand("fieldpair_bwd", dx, B, F, E, dx_offset)
    if d_weights is not None:
        _vec("fieldpair_bwd", "d_weights", d_weights, P * E * E if kind == "fefm" else F * F)
    _dev_check(d_pairs, d_logit, dx, d_weights, *tensors)
    b = _C.fieldpair.BwdArgs(d_pairs_stride=d_pairs_stride, d_pairs_offset=int(d_pairs_offset), dx_stride=dx_stride,
                             dx_offset=int(dx_offset), accumulate=int(bool(accumulate)), max_blocks=int(max_blocks))
    b.fwd = _fieldpair_args(_FIELDPAIR_KINDS[kind], B, F, E, x_stride, x_offset)
    b.fwd.x, b.fwd.weights = x.data_ptr(), wptr.data_ptr()
    if d_pairs is not None:
        b.d_pairs = d_pairs.data_ptr()
    if d_logit is not None:
        b.d_logit = d_logit.data_ptr()
    if dx is not None:
        b.dx = dx.data_ptr()
    if d_weights is not None:
        b.d_weights = d_weights.data_ptr()
    _workspace("fieldpair_bwd", b.fwd, int(_C.lib().dctr_fieldpair_bwd_workspace_bytes(ctypes.byref(b))), workspace, x.device)
    _C.check(_C.lib().dctr_fieldpair_bwd(ctypes.byref(b), _C.stream_ptr()), "dctr_fieldpair_bwd")


def _grad_operand(dy, rows2d):
    """An incoming gradient as the op reads it: float32, unit column stride, rows not broadcast by expand()."""
    if dy is None:
        return None
    if dy.dtype != torch.float32:
        dy = dy.float()
    if rows2d:
        if dy.stride(-1) != 1 or (dy.shape[0] > 1 and dy.stride(0) < dy.shape[1]):
            dy = dy.contiguous()
    elif not dy.is_contiguous():
        dy = dy.contiguous()
    return dy


class FieldPairFunction(torch.autograd.Function):
    """FEFMLayer / FwFMLayer as one differentiable op: fieldpair() forward and fieldpair_bwd() backward, one launch each.
    ``apply(x, kind, want_pairs, want_logit, *weights)``: x [B,F,E]; ``weights`` = the P pair matrices (FEFM) or field_pair_strengths
    (FwFM).  Returns (pairs [B,P] or None, logit [B] or None).  Only x and the weights are saved: the backward loads x again.  Weight
    gradients leave the kernel through float atomics and may differ in the last bits from call to call; dx does not."""

    @staticmethod
    def forward(ctx, x, kind, want_pairs, want_logit, *weights):
        ctx.set_materialize_grads(False)
        ctx.kind = kind
        x = x.detach()
        ws = [w.detach() for w in weights]
        pairs, logit = fieldpair(x, ws if kind == "fefm" else ws[0], kind=kind, pairs=True if want_pairs else None,
                                 logit=True if want_logit else None)
        ctx.save_for_backward(x, *ws)
        return pairs, logit

    @staticmethod
    def backward(ctx, d_pairs, d_logit):
        saved = list(ctx.saved_tensors)
        x, ws = saved[0], saved[1:]
        fefm = ctx.kind == "fefm"
        want_dx = ctx.needs_input_grad[0]
        if d_pairs is None and d_logit is None:
            return (None,) * (4 + len(ws))
        d_pairs, d_logit = _grad_operand(d_pairs, True), _grad_operand(d_logit, False)
        dx = torch.empty_like(x, memory_format=torch.contiguous_format) if want_dx else None
        flat, grads = _zeroed_grads(ws, ctx.needs_input_grad[4:], x.device)     # FEFM: [P,E,E] behind the per-pair views
        if want_dx or flat is not None:
            fieldpair_bwd(x, ws if fefm else ws[0], ctx.kind, d_pairs=d_pairs, d_logit=d_logit, dx=dx, d_weights=flat)
        return (dx, None, None, None) + tuple(grads)


_FFM_ROUTES = {None: _C.ffm.ROUTE_AUTO, "auto": _C.ffm.ROUTE_AUTO, "direct": _C.ffm.ROUTE_DIRECT}


def _ffm_args(batch, fields, dim, reduce_sum=False, n_dense=0, route=None, out_stride=None, out_offset=0):
    if route not in _FFM_ROUTES:
        raise ValueError("ffm: route %r: expected None / 'auto' or 'direct'" % (route,))
    F, d = int(fields), int(dim)
    P = F * (F - 1) // 2
    width = (P if reduce_sum else P * d) + int(n_dense)
    if out_stride is None:
        out_stride = (int(out_offset) + width + 3) // 4 * 4
    return _C.ffm.Args(batch=int(batch), n_fields=F, dim=d, reduce_sum=int(bool(reduce_sum)), n_dense=int(n_dense),
                       out_stride=int(out_stride), out_offset=int(out_offset), route=_FFM_ROUTES[route])


def ffm_workspace_bytes(batch, fields, dim, reduce_sum=False, route=None):
    """Bytes of workspace dctr_ffm_fwd needs for these shapes (read from the library: 0, both routes keep their state on chip)."""
    a = _ffm_args(batch, fields, dim, reduce_sum, route=route)
    return int(_C.lib().dctr_ffm_workspace_bytes(ctypes.byref(a)))


def ffm_route(batch, fields, dim, reduce_sum=False, route=None):
    """'lds' or 'direct': the route dctr_ffm_fwd takes for these shapes (the library's answer, dctr_ffm_route)."""
    a = _ffm_args(batch, fields, dim, reduce_sum, route=route)
    return _route_name("dctr_ffm_route", _C.lib().dctr_ffm_route(ctypes.byref(a)), {_C.ffm.ROUTE_LDS: "lds", _C.ffm.ROUTE_DIRECT: "direct"})


def make_ffm_fields(fields, device):
    """fields: list of dicts(rows [V, >= (F-1)*d] float32 with unit column stride, ids 1-D id view or None = pre-pooled field whose row
    is the sample index) -> uint8 device tensor holding the dctr_ffm_field_t array (kept alive by the caller)."""
    arr = (_C.ffm.Field * max(1, len(fields)))()
    for j, f in enumerate(fields):
        rows, ids = f["rows"], f.get("ids")
        arr[j].rows = rows.data_ptr()
        arr[j].vocab = int(rows.shape[0])
        arr[j].row_pitch = row_stride(rows)
        if ids is None:
            arr[j].identity = 1
        else:
            arr[j].ids = ids.data_ptr()
            arr[j].ids_stride = _id_stride(ids)
            arr[j].ids_is_i64 = int(ids.dtype == torch.int64)
    return _upload(arr, device)


def _ffm_operands(op, ids, masters, dim, desc, batch):
    """What ffm() and ffm_bwd() read alike: the ids [F, B] and per field the fused table or the pre-pooled (buffer,) 1-tuple, behind a
    dctr_ffm_field_t array — or a ready ``desc`` with ``dim`` and ``batch``.  Returns (F, dim, B, desc, the 2-D tables to keep alive)."""
    F = len(masters)
    if F < 2:
        raise ValueError("%s: %d field(s): a field pair needs at least 2" % (op, F))
    keep = []
    if desc is None:
        B = int(ids.shape[1]) if batch is None else int(batch)
        if ids.dim() != 2 or ids.shape[0] != F or ids.dtype not in (torch.int32, torch.int64):
            raise ValueError("%s: ids must be an int32 / int64 [%d, B] matrix" % (op, F))
        fields = []
        for j, m in enumerate(masters):
            pooled = isinstance(m, tuple)
            m = m[0] if pooled else m
            if m.dtype != torch.float32:
                raise TypeError("%s: tables must be float32, got %s" % (op, m.dtype))
            if m.dim() == 3:
                if dim is None:
                    dim = int(m.shape[2])
                if m.shape[1] != F - 1 or m.shape[2] != dim or not m.is_contiguous():
                    raise ValueError("%s: field %d: expected a contiguous [V, %d, %d] table, got %s" % (op, j, F - 1, dim, tuple(m.shape)))
                m = m.view(m.shape[0], -1)
            if dim is None:
                raise ValueError("%s: dim is required with 2-D tables" % op)
            if m.dim() != 2 or m.stride(1) != 1 or m.shape[1] < (F - 1) * dim:
                raise ValueError("%s: field %d: expected [rows, >= %d] with unit column stride" % (op, j, (F - 1) * dim))
            if pooled and m.shape[0] < B:
                raise ValueError("%s: pre-pooled field %d holds %d rows for a batch of %d" % (op, j, m.shape[0], B))
            keep.append(m)
            fields.append(dict(rows=m, ids=None if pooled else ids[j]))
        _dev_check(ids, *keep)
        desc = make_ffm_fields(fields, ids.device)
    else:
        if dim is None or batch is None:
            raise ValueError("%s: desc needs dim and batch" % op)
        B = int(batch)
    return F, int(dim), B, desc, keep


def ffm(ids, masters, dim=None, scale=None, shift=None, dense=None, n_dense=None, reduce_sum=False, out=None, out_offset=0,
        status=None, route=None, desc=None, batch=None):
    """ONN's field-aware lookup + pair products (reference models/onn.py:59-99), one launch: ids [F, B] (int32 / int64; row j unused
    for a pre-pooled field) and ``masters`` = per field the fused table [V_j, F-1, d] (or its [V_j, (F-1)*d] view), or for a pre-pooled
    field a (buffer [B, >= (F-1)*d],) 1-tuple -> out [B, P*d (+ n_dense)] ([B, P (+ n_dense)] with ``reduce_sum``), pairs in
    itertools.combinations order.  ``scale`` / ``shift``: the inference BatchNormalization over the pair columns; ``dense`` [B, >= n_dense]:
    copied behind them.  ``out``: a float32 2-D view with unit column stride and a row stride that is a multiple of 4, written from
    column ``out_offset``; other columns are not touched.  ``route='direct'`` forces the direct route.  ``desc``: a descriptor tensor
    from make_ffm_fields (then ``ids`` / ``masters`` are not looked at; ``dim`` and ``batch`` are required)."""
    F, dim, B, desc, keep = _ffm_operands("ffm", ids, masters, dim, desc, batch)
    P = F * (F - 1) // 2
    W = P if reduce_sum else P * dim
    if dense is not None:
        n_dense = int(dense.shape[-1] if n_dense is None else n_dense)
        dense_stride = _rows2d("ffm", "dense", dense, B, n_dense, at_least_rows=True)
    else:
        n_dense = 0
    if (scale is None) != (shift is None):
        raise ValueError("ffm: scale and shift come together")
    if scale is not None:
        scale, shift = _f32c(scale, "scale"), _f32c(shift, "shift")
        if scale.numel() != W or shift.numel() != W:
            raise ValueError("ffm: scale / shift must hold %d elements" % W)
    width = W + n_dense
    if out is None:
        out = torch.empty(B, (out_offset + width + 3) // 4 * 4, dtype=torch.float32, device=desc.device)
    out_stride = _rows2d("ffm", "out", out, B, width, out_offset, at_least_rows=True)
    _dev_check(desc, scale, shift, dense, out, status)
    a = _ffm_args(B, F, dim, reduce_sum, n_dense, route, out_stride=out_stride, out_offset=out_offset)
    a.fields, a.out = desc.data_ptr(), out.data_ptr()
    if scale is not None:
        a.scale, a.shift = scale.data_ptr(), shift.data_ptr()
    if n_dense:
        a.dense, a.dense_stride = dense.data_ptr(), dense_stride
    if status is not None:
        a.status = status.data_ptr()
    _C.check(_C.lib().dctr_ffm_fwd(ctypes.byref(a), _C.stream_ptr()), "dctr_ffm_fwd")
    del keep
    return out


_FFM_ROUTE_NAMES = {_C.ffm.ROUTE_LDS: "lds", _C.ffm.ROUTE_DIRECT: "direct"}


def _ffm_bwd_args(batch, fields, dim, reduce_sum=False, route=None, d_out_stride=None, d_out_offset=0, max_blocks=0):
    F, d = int(fields), int(dim)
    P = F * (F - 1) // 2
    if d_out_stride is None:
        d_out_stride = int(d_out_offset) + (P if reduce_sum else P * d)
    b = _C.ffm.BwdArgs(d_out_stride=int(d_out_stride), d_out_offset=int(d_out_offset), max_blocks=int(max_blocks))
    b.fwd = _ffm_args(batch, F, d, reduce_sum, route=route)
    return b


def ffm_bwd_workspace_bytes(batch, fields, dim, reduce_sum=False, route=None):
    """Bytes of workspace dctr_ffm_bwd needs for these shapes (read from the library: 0, both routes keep their state on chip)."""
    return int(_C.lib().dctr_ffm_bwd_workspace_bytes(ctypes.byref(_ffm_bwd_args(batch, fields, dim, reduce_sum, route))))


def ffm_bwd_route(batch, fields, dim, reduce_sum=False, route=None):
    """'lds' or 'direct': the route dctr_ffm_bwd takes for these shapes (the library's answer, dctr_ffm_bwd_route)."""
    b = _ffm_bwd_args(batch, fields, dim, reduce_sum, route)
    return _route_name("dctr_ffm_bwd_route", _C.lib().dctr_ffm_bwd_route(ctypes.byref(b)), _FFM_ROUTE_NAMES)


def make_ffm_grads(grads, device):
    """grads: per field a float32 2-D view with unit column stride (a table's dense gradient, a pre-pooled field's d_rows), or None for
    a field that gets no gradient -> uint8 device tensor holding the dctr_ffm_grad_t array (kept alive by the caller)."""
    arr = (_C.ffm.Grad * max(1, len(grads)))()
    for j, g in enumerate(grads):
        if g is not None:
            arr[j].grad = g.data_ptr()
            arr[j].row_stride = row_stride(g)
    return _upload(arr, device)


def ffm_bwd(ids, masters, d_out, grads, dim=None, reduce_sum=False, d_out_offset=0, status=None, route=None, max_blocks=0, desc=None,
            batch=None):
    """Backward of ffm()'s pair products, one launch (include/dctr.h: dctr_ffm_bwd); the forward saves nothing.  ``ids`` / ``masters`` /
    ``dim`` / ``reduce_sum`` / ``route`` / ``desc`` / ``batch`` as ffm() (no scale / shift, no dense columns: their backward stays with
    the caller).  ``d_out``: a float32 2-D view whose row holds the gradient of the P*d (P) pair columns from column ``d_out_offset``.
    ``grads``: per field where its gradient goes — a table field: the dense gradient [V_j, F-1, d] (or a [V_j, >= (F-1)*d] view),
    ACCUMULATED into with float atomics (zero it first; last bits may differ from call to call); a pre-pooled field: d_rows
    [>= B, >= (F-1)*d], whose first (F-1)*d columns are written (bit-identical from call to call, the others untouched); None: a frozen
    field, skipped.  An id out of range raises ``status``, gets no gradient and gives its partners zeros."""
    F, dim, B, desc, keep = _ffm_operands("ffm_bwd", ids, masters, dim, desc, batch)
    R = (F - 1) * dim
    W = F * (F - 1) // 2 * (1 if reduce_sum else dim)
    d_out_stride = _rows2d("ffm_bwd", "d_out", d_out, B, W, d_out_offset, at_least_rows=True)
    if len(grads) != F:
        raise ValueError("ffm_bwd: grads must hold one entry (a tensor or None) per field, got %d for %d fields" % (len(grads), F))
    gs = []
    for j, g in enumerate(grads):
        if g is None:
            gs.append(None)
            continue
        pooled = isinstance(masters[j], tuple)
        if g.dim() == 3 and g.is_contiguous() and tuple(g.shape[1:]) == (F - 1, dim):
            g = g.view(g.shape[0], R)
        rows = B if pooled else (keep[j].shape[0] if keep else g.shape[0] if g.dim() == 2 else 0)
        _rows2d("ffm_bwd", "grads[%d]" % j, g, rows, R, at_least_rows=pooled)
        gs.append(g)
    _dev_check(desc, d_out, status, *gs)
    gdesc = make_ffm_grads(gs, desc.device)
    b = _ffm_bwd_args(B, F, dim, reduce_sum, route, d_out_stride, d_out_offset, max_blocks)
    b.fwd.fields, b.d_out, b.grads = desc.data_ptr(), d_out.data_ptr(), gdesc.data_ptr()
    if status is not None:
        b.fwd.status = status.data_ptr()
    _C.check(_C.lib().dctr_ffm_bwd(ctypes.byref(b), _C.stream_ptr()), "dctr_ffm_bwd")
    del keep


class FieldAwareFunction(torch.autograd.Function):
    """ONN's field-aware lookup + pair products as one differentiable op: ffm() forward and ffm_bwd() backward, one launch each.
    ``apply(ids, masters, dim, reduce_sum, status, *inputs)``: ids [F, B]; ``masters`` per field the fused table [V_j, F-1, d], or None for
    a field that arrives pooled; ``inputs`` in field order — a table field's F-1 per-name views ``master[:, k, :]`` (``inputs_of`` checks
    that they are), a pooled field's [B, (F-1)*d] rows.  Returns the pair columns [B, P*d] ([B, P] with reduce_sum).  The backward zeroes
    one [V_j, F-1, d] gradient per field that wants one and hands each view its slot ``grad[:, k, :]``, a pooled field its d_rows; table
    gradients leave the kernel through float atomics and may differ in the last bits from call to call."""

    @staticmethod
    def inputs_of(masters, views):
        """The gate: ``views[j]`` = field j's F-1 per-name tensors in slot order (``masters[j]`` its fused table), or its pooled
        [B, (F-1)*d] rows (``masters[j]`` None; a callable is called for them once every table view has passed).  Returns ``inputs``
        for apply(), or None when a view is not the slot of its table (pointer, strides, shape) — the op reads the tables, so anything
        else must stay on the torch ops."""
        F = len(masters)
        flat = []
        for m, vs in zip(masters, views):
            if m is None:
                flat.append(vs)
                continue
            if not m.is_cuda:
                return None
            if m.dim() != 3 or m.shape[1] != F - 1 or not m.is_contiguous() or m.dtype != torch.float32 or len(vs) != F - 1:
                return None
            V, _, d = m.shape
            base = m.data_ptr()
            for k, v in enumerate(vs):
                if (v.data_ptr() != base + k * d * 4 or tuple(v.shape) != (V, d) or v.dtype != torch.float32 or v.device != m.device
                        or (V > 1 and v.stride(0) != (F - 1) * d) or (d > 1 and v.stride(1) != 1)):
                    return None
            flat.extend(vs)
        return [v() if callable(v) else v for v in flat]

    @staticmethod
    def forward(ctx, ids, masters, dim, reduce_sum, status, *inputs):
        ctx.set_materialize_grads(False)
        F = len(masters)
        ms, at = [], 0
        for m in masters:
            if m is None:
                ms.append((_f32c(inputs[at].detach(), "pooled rows"),))
                at += 1
            else:
                ms.append(m.detach())
                at += F - 1
        ctx.dim, ctx.reduce_sum, ctx.status = int(dim), bool(reduce_sum), status
        ctx.pooled = [m is None for m in masters]
        out = ffm(ids, ms, dim=dim, reduce_sum=reduce_sum, status=status)
        ctx.save_for_backward(ids, *[m[0] if isinstance(m, tuple) else m for m in ms])
        return out[:, :F * (F - 1) // 2 * (1 if reduce_sum else int(dim))]

    @staticmethod
    def backward(ctx, d_out):
        saved = list(ctx.saved_tensors)
        ids, rows = saved[0], saved[1:]
        F, R = len(rows), (len(rows) - 1) * ctx.dim
        needs = ctx.needs_input_grad[5:]
        none = (None,) * (5 + len(needs))
        if d_out is None:
            return none
        wanted, at = [], 0
        for pooled in ctx.pooled:
            n = 1 if pooled else F - 1
            wanted.append(any(needs[at:at + n]))
            at += n
        if not any(wanted):
            return none
        d_out = _grad_operand(d_out, True)
        _, tables = _zeroed_grads([None if p or not w else r for p, w, r in zip(ctx.pooled, wanted, rows)], wanted, ids.device)
        grads = [torch.empty(ids.shape[1], R, dtype=torch.float32, device=ids.device) if p and w else t
                 for p, w, t in zip(ctx.pooled, wanted, tables)]
        ffm_bwd(ids, [(r,) if p else r for p, r in zip(ctx.pooled, rows)], d_out, grads, dim=ctx.dim, reduce_sum=ctx.reduce_sum,
                status=ctx.status)
        ret, at = [None] * 5, 0
        for p, g in zip(ctx.pooled, grads):
            if p:
                ret.append(g if needs[at] else None)
                at += 1
            else:
                ret.extend(g[:, k, :] if g is not None and needs[at + k] else None for k in range(F - 1))
                at += F - 1
        return tuple(ret)


_MLR_LEARNERS = {"binary": _C.mlr.LEARNER_SIGMOID, "regression": _C.mlr.LEARNER_LINEAR}


def _mlr_args(batch, n_fields, region_num, bias, task):
    if task not in _MLR_LEARNERS:
        raise ValueError("mlr: task %r: expected 'binary' or 'regression'" % (task,))
    return _C.mlr.Args(batch=int(batch), n_fields=int(n_fields), region_num=int(region_num), has_bias=int(bool(bias)),
                       learner_act=_MLR_LEARNERS[task], out_stride=1)


def mlr_supported(region_num, bias=False):
    """Does dctr_mlr_fwd / dctr_mlr_bwd take K = 2 region_num (+ 1) logit columns (K <= 64)?  The library's answer, host only."""
    return bool(_C.lib().dctr_mlr_supported(ctypes.byref(_mlr_args(0, 0, region_num, bias, "binary"))))


def make_mlr_fields(fields, device):
    """fields: list of dicts(rows = float32 2-D view with unit column stride whose first ``width`` columns the field adds to the logit
    columns ``col0`` .. ``col0 + width - 1``; ids = 1-D int32 / int64 view, or None: a pre-pooled field whose row is the sample index)
    -> uint8 device tensor holding the dctr_mlr_field_t array (kept alive by the caller, with the tensors it points at)."""
    arr = (_C.mlr.Field * max(1, len(fields)))()
    for j, f in enumerate(fields):
        rows, ids = f["rows"], f.get("ids")
        arr[j].rows = rows.data_ptr()
        arr[j].vocab = int(rows.shape[0])
        arr[j].row_pitch = row_stride(rows)
        arr[j].col0, arr[j].width = int(f["col0"]), int(f["width"])
        if ids is None:
            arr[j].identity = 1
        else:
            arr[j].ids = ids.data_ptr()
            arr[j].ids_stride = _id_stride(ids)
            arr[j].ids_is_i64 = int(ids.dtype == torch.int64)
    return _upload(arr, device)


def _mlr_operands(op, fields, region_num, bias, desc, batch, n_fields):
    """What mlr() and mlr_bwd() read alike: the field list behind a dctr_mlr_field_t array, or a ready ``desc`` with ``n_fields`` and
    ``batch``.  Returns (K, B, n_fields, desc, the tensors to keep alive)."""
    K = 2 * int(region_num) + int(bool(bias))
    keep = []
    if desc is None:
        if batch is None:
            raise ValueError("%s: batch is required" % op)
        B = int(batch)
        fields = list(fields or [])           # (no sparse or sequence feature at all is legal: the dense part alone, n_fields = 0)
        for j, f in enumerate(fields):
            rows, ids = f["rows"], f.get("ids")
            col0, width = int(f["col0"]), int(f["width"])
            if not (0 <= col0 and 1 <= width and col0 + width <= K):
                raise ValueError("%s: field %d: columns [%d, %d) outside the %d logit columns" % (op, j, col0, col0 + width, K))
            _rows2d(op, "fields[%d].rows" % j, rows, B if ids is None else 0, width, at_least_rows=True)
            if ids is not None:
                if ids.dim() != 1 or ids.shape[0] != B or ids.dtype not in (torch.int32, torch.int64):
                    raise ValueError("%s: field %d: ids must be an int32 / int64 vector of %d elements" % (op, j, B))
                keep.append(ids)
            keep.append(rows)
        _dev_check(*keep)
        n_fields = len(fields)
        desc = make_mlr_fields(fields, keep[0].device) if fields else None
    else:
        if n_fields is None or batch is None:
            raise ValueError("%s: desc needs n_fields and batch" % op)
        B = int(batch)
    return K, B, int(n_fields), desc, keep


def mlr(fields, region_num, bias=False, task="binary", dense=None, dense_w=None, out=None, z=None, z_offset=0, status=None, desc=None,
        batch=None, n_fields=None, device=None):
    """MLR's forward (reference models/mlr.py:17-74), one launch: ``fields`` as make_mlr_fields takes them (or a ready ``desc`` with
    ``n_fields``), ``batch`` samples, K = 2 region_num (+ 1 with ``bias``) logit columns in the order region, learner, bias.
    ``dense`` [B, >= n_dense] with ``dense_w`` [n_dense, K] (contiguous) adds dense @ dense_w.  ``out``: a float32 vector of B
    elements (any stride), allocated when None.  ``z``: True for a fresh [B, K], or a float32 2-D view written from column ``z_offset``
    (other columns untouched), or None: z is not written.  Returns (out, z).  K > 64 raises DctrError with rc = E_UNSUPPORTED and
    writes nothing."""
    K, B, F, desc, keep = _mlr_operands("mlr", fields, region_num, bias, desc, batch, n_fields)
    dev = device or (desc.device if desc is not None else keep[0].device if keep else dense.device if dense is not None else out.device)
    a = _mlr_args(B, F, region_num, bias, task)
    if dense is not None:
        n_dense = int(dense_w.shape[0])
        a.dense_stride = _rows2d("mlr", "dense", dense, B, n_dense, at_least_rows=True)
        if tuple(dense_w.shape) != (n_dense, K):
            raise ValueError("mlr: dense_w must be [n_dense, %d], got %s" % (K, tuple(dense_w.shape)))
        _vec("mlr", "dense_w", dense_w, n_dense * K)
        a.n_dense, a.dense, a.dense_w = n_dense, dense.data_ptr(), dense_w.data_ptr()
    if out is None:
        out = torch.empty(B, dtype=torch.float32, device=dev)
    if out.dim() != 1 or out.shape[0] != B or out.dtype != torch.float32:
        raise ValueError("mlr: out must be a float32 vector of %d elements" % B)
    a.out, a.out_stride = out.data_ptr(), _id_stride(out)
    if z is True:
        z = torch.empty(B, K, dtype=torch.float32, device=dev)
    if z is not None:
        a.z_stride = _rows2d("mlr", "z", z, B, K, z_offset, at_least_rows=True)
        a.z, a.z_offset = z.data_ptr(), int(z_offset)
    _dev_check(desc, dense, dense_w, out, z, status)
    if desc is not None:
        a.fields = desc.data_ptr()
    if status is not None:
        a.status = status.data_ptr()
    _C.check(_C.lib().dctr_mlr_fwd(ctypes.byref(a), _C.stream_ptr()), "dctr_mlr_fwd")
    del keep
    return out, z


def make_mlr_grads(grads, device):
    """grads: per field a float32 2-D view with unit column stride (a table field's dense gradient, advanced to the field's first
    column; a pre-pooled field's d_rows), or None for a field that gets no gradient -> uint8 device tensor holding the dctr_mlr_grad_t
    array (kept alive by the caller)."""
    arr = (_C.mlr.Grad * max(1, len(grads)))()
    for j, g in enumerate(grads):
        if g is not None:
            arr[j].grad = g.data_ptr()
            arr[j].row_stride = row_stride(g)
    return _upload(arr, device)


def mlr_bwd(fields, region_num, z, d_out, bias=False, task="binary", grads=None, dz=None, z_offset=0, status=None, desc=None,
            batch=None, n_fields=None):
    """Backward of mlr(), one launch (include/dctr.h: dctr_mlr_bwd).  ``z``: what the forward saved (read from column ``z_offset``);
    ``d_out``: a float32 vector of B elements.  ``grads``: None, or per field where its slice of dz goes — a table field: a
    [vocab, >= width] view of the dense gradient master (advanced to the field's first column), ACCUMULATED into with float atomics (zero
    it first; last bits may differ from call to call); a pre-pooled field: d_rows [>= B, >= width], its first ``width`` columns written;
    None: a frozen field, skipped.  Returns dz [B, K] (``dz``: a float32 2-D view to write instead)."""
    K, B, F, desc, keep = _mlr_operands("mlr_bwd", fields, region_num, bias, desc, batch, n_fields)
    b = _C.mlr.BwdArgs()
    b.fwd = _mlr_args(B, F, region_num, bias, task)
    b.fwd.z_stride = _rows2d("mlr_bwd", "z", z, B, K, z_offset, at_least_rows=True)
    b.fwd.z, b.fwd.z_offset = z.data_ptr(), int(z_offset)
    if d_out.dim() != 1 or d_out.shape[0] != B or d_out.dtype != torch.float32:
        raise ValueError("mlr_bwd: d_out must be a float32 vector of %d elements" % B)
    b.d_out, b.d_out_stride = d_out.data_ptr(), _id_stride(d_out)
    if dz is None:
        dz = torch.empty(B, K, dtype=torch.float32, device=z.device)
    b.dz_stride = _rows2d("mlr_bwd", "dz", dz, B, K, at_least_rows=True)
    b.dz = dz.data_ptr()
    gdesc = None
    if grads is not None:
        if len(grads) != F:
            raise ValueError("mlr_bwd: grads must hold one entry (a tensor or None) per field, got %d for %d fields" % (len(grads), F))
        if fields is not None:
            for j, (f, g) in enumerate(zip(fields, grads)):
                if g is not None:
                    pooled = f.get("ids") is None
                    _rows2d("mlr_bwd", "grads[%d]" % j, g, B if pooled else int(f["rows"].shape[0]), int(f["width"]), at_least_rows=pooled)
        if any(g is not None for g in grads):
            gdesc = make_mlr_grads(grads, z.device)
            b.grads = gdesc.data_ptr()
    _dev_check(desc, z, d_out, dz, status, *[g for g in (grads or []) if g is not None])
    if desc is not None:
        b.fwd.fields = desc.data_ptr()
    if status is not None:
        b.fwd.status = status.data_ptr()
    _C.check(_C.lib().dctr_mlr_bwd(ctypes.byref(b), _C.stream_ptr()), "dctr_mlr_bwd")
    del keep, gdesc
    return dz


class MLRFunction(torch.autograd.Function):
    """MLR's forward as one differentiable op: mlr() forward with z kept, mlr_bwd() backward, one launch each.
    ``apply(plan, region_num, bias, task, status, dense, dense_w, *inputs)``.  ``plan``: per field a dict(master = the fused rows
    [V, pitch] or None for a field that arrives pooled, ids = its 1-D id view, first = the master column of its first logit column,
    col0, width); ``inputs`` in field order — a table field's ``width`` per-name views ``master[:, first + k : first + k + 1]``
    (``inputs_of`` checks that they are), a pooled field's [B, width] rows.  ``dense`` [B, n_dense] and ``dense_w`` [n_dense, K] (or both
    None): dense_w's gradient is dense^T dz, a torch matmul; dense gets none.  Returns the prediction [B].  The backward zeroes ONE
    [V, pitch] gradient per distinct master and hands each view its column of it (fields that share a master add into the same
    gradient; the views of the later ones get None), a pooled field its d_rows; table gradients leave the kernel through float atomics
    and may differ in the last bits from call to call."""

    @staticmethod
    def inputs_of(plan, views):
        """The gate: ``views[j]`` = field j's per-name tensors in column order, or its pooled rows (a callable is called for them once
        every table view has passed).  Returns ``inputs`` for apply(), or None when a view is not the column of its master."""
        flat = []
        for f, vs in zip(plan, views):
            m = f["master"]
            if m is None:
                flat.append(vs)
                continue
            if not m.is_cuda or m.dim() != 2 or not m.is_contiguous() or m.dtype != torch.float32 or len(vs) != f["width"]:
                return None
            V, pitch = m.shape
            for k, v in enumerate(vs):
                if (v.data_ptr() != m.data_ptr() + (f["first"] + k) * 4 or tuple(v.shape) != (V, 1) or v.dtype != torch.float32
                        or v.device != m.device or (V > 1 and v.stride(0) != pitch)):
                    return None
            flat.extend(vs)
        return [v() if callable(v) else v for v in flat]

    @staticmethod
    def _fields(plan, pooled_rows):
        fields, at = [], 0
        for f in plan:
            if f["master"] is None:
                fields.append(dict(rows=pooled_rows[at], ids=None, col0=f["col0"], width=f["width"]))
                at += 1
            else:
                fields.append(dict(rows=f["master"].detach()[:, f["first"]:], ids=f["ids"], col0=f["col0"], width=f["width"]))
        return fields

    @staticmethod
    def forward(ctx, plan, region_num, bias, task, status, dense, dense_w, *inputs):
        ctx.set_materialize_grads(False)
        pooled, at = [], 0
        for f in plan:
            if f["master"] is None:
                pooled.append(_f32c(inputs[at].detach(), "pooled rows"))
                at += 1
            else:
                at += f["width"]
        B = int(plan[0]["ids"].shape[0] if plan and plan[0]["master"] is not None else (pooled[0].shape[0] if pooled else dense.shape[0]))
        ctx.plan, ctx.meta, ctx.status = plan, (int(region_num), bool(bias), task, B), status
        dw = None if dense_w is None else _f32c(dense_w.detach(), "dense_w")
        out, z = mlr(MLRFunction._fields(plan, pooled), region_num, bias, task, dense=dense, dense_w=dw, z=True, status=status, batch=B,
                     device=(dense if dense is not None else pooled[0] if pooled else plan[0]["master"]).device)
        ctx.save_for_backward(z, *([dense] if dense is not None else []), *pooled)
        ctx.has_dense = dense is not None
        return out

    @staticmethod
    def backward(ctx, d_out):
        plan, (R, bias, task, B) = ctx.plan, ctx.meta
        needs = ctx.needs_input_grad[7:]
        none = (None,) * (7 + len(needs))
        if d_out is None:
            return none
        saved = list(ctx.saved_tensors)
        z = saved[0]
        dense = saved[1] if ctx.has_dense else None
        pooled = saved[2 if ctx.has_dense else 1:]
        d_out = _grad_operand(d_out, False)
        masters, grads, at, pat = {}, [], 0, 0           # data_ptr of a master -> its zeroed gradient
        for f in plan:
            m = f["master"]
            if m is None:
                grads.append(torch.empty(B, f["width"], dtype=torch.float32, device=z.device) if needs[at] else None)
                at += 1
                pat += 1
            else:
                if any(needs[at:at + f["width"]]):
                    g = masters.get(m.data_ptr())
                    if g is None:
                        g = masters[m.data_ptr()] = torch.zeros_like(m)
                    grads.append(g[:, f["first"]:])
                else:
                    grads.append(None)
                at += f["width"]
        dz = mlr_bwd(MLRFunction._fields(plan, pooled), R, z, d_out, bias=bias, task=task, grads=grads, status=ctx.status, batch=B)
        d_dense_w = dense.t() @ dz if (dense is not None and ctx.needs_input_grad[6]) else None
        ret, at, handed = [None] * 6 + [d_dense_w], 0, set()
        for f, g in zip(plan, grads):
            if f["master"] is None:
                ret.append(g)
                at += 1
                continue
            for k in range(f["width"]):
                key = (f["master"].data_ptr(), f["first"] + k)
                if g is not None and needs[at + k] and key not in handed:
                    handed.add(key)
                    ret.append(g[:, k:k + 1])
                else:
                    ret.append(None)
            at += f["width"]
        return tuple(ret)


_IFM_ROUTES = {None: _C.ifm.ROUTE_AUTO, "auto": _C.ifm.ROUTE_AUTO, "workspace": _C.ifm.ROUTE_WORKSPACE}


def _ifm_args(batch, fields, dim, n_src=1, route=None):
    if route not in _IFM_ROUTES:
        raise ValueError("ifm: route %r: expected None / 'auto' or 'workspace'" % (route,))
    F, d = int(fields), int(dim)
    if F < 1 or d < 1:
        raise ValueError("ifm: fields = %d, dim = %d" % (F, d))
    if not 0 <= int(n_src) <= 2:
        raise ValueError("ifm: %d factor sources: 0, 1 or 2" % int(n_src))
    a = _C.ifm.Args(batch=int(batch), n_fields=F, dim=d, x_stride=F * d, n_src=int(n_src), mprime_stride=F, route=_IFM_ROUTES[route])
    for s in range(int(n_src)):
        a.src[s].K, a.src[s].act_stride = 1, 1
    return a


def ifm_workspace_bytes(batch, fields, dim, n_src=1, route=None):
    """Bytes of workspace dctr_ifm_fwd needs for these shapes (read from the library: 0 on the LDS route and without factor sources)."""
    a = _ifm_args(batch, fields, dim, n_src, route)
    return int(_C.lib().dctr_ifm_workspace_bytes(ctypes.byref(a)))


def ifm_route(batch, fields, dim, n_src=1, route=None):
    """'lds' or 'workspace': the route dctr_ifm_fwd takes for these shapes (the library's answer, dctr_ifm_route)."""
    a = _ifm_args(batch, fields, dim, n_src, route)
    return _route_name("dctr_ifm_route", _C.lib().dctr_ifm_route(ctypes.byref(a)), {_C.ifm.ROUTE_LDS: "lds", _C.ifm.ROUTE_WORKSPACE: "workspace"})


def make_ifm_lin(terms, batch, device):
    """terms: per position either (table [V] / [V, 1] float32, ids 1-D int32 / int64 view of >= batch elements) — gathered in the
    kernel — or a float32 tensor of >= batch elements already pooled ([B] or [B, 1]; dctr_embed_pool's lin_out) -> uint8 device tensor
    holding the dctr_ifm_lin_t array (kept alive by the caller, who also keeps the tensors alive)."""
    arr = (_C.ifm.Lin * max(1, len(terms)))()
    for k, t in enumerate(terms):
        if isinstance(t, (tuple, list)):
            table, ids = t
            if table.dtype != torch.float32 or table.numel() != table.shape[0] or not table.is_contiguous():
                raise ValueError("ifm: linear term %d: the table must be a contiguous float32 [V] or [V, 1] tensor" % k)
            if ids.dim() != 1 or ids.dtype not in (torch.int32, torch.int64) or ids.shape[0] < batch:
                raise ValueError("ifm: linear term %d: ids must be a 1-D int32 / int64 view of >= %d elements" % (k, batch))
            _dev_check(table, ids)
            arr[k].table, arr[k].vocab = table.data_ptr(), int(table.shape[0])
            arr[k].ids, arr[k].ids_is_i64 = ids.data_ptr(), int(ids.dtype == torch.int64)
            arr[k].ids_stride = _id_stride(ids)
        else:
            if t.dtype != torch.float32 or t.numel() != t.shape[0] or t.shape[0] < batch:
                raise ValueError("ifm: linear term %d: a pre-pooled term must be a float32 [B] or [B, 1] tensor of >= %d rows" % (k, batch))
            _dev_check(t)
            arr[k].vec = t.data_ptr()
            arr[k].vec_stride = int(t.stride(0)) if t.shape[0] != 1 else 1
    return _upload(arr, device)


def ifm(x, fields, dim, sources=(), mprime=None, softmax=False, lin=(), add=(), global_bias=None, sigmoid_out=False, out=None,
        factor_out=None, status=None, route=None, workspace=None, lin_desc=None):
    """The input-aware FM of IFM / DIFM (reference models/ifm.py:55-72, difm.py:59-80), one launch from the factor's inputs to the
    prediction.  x: float32 [B, >= fields*dim] with unit column stride, field f's embedding in columns [f*dim, (f+1)*dim) (dnn_in, read in
    place).  ``sources``: 0, 1 or 2 pairs (act [B, K] row-strided, kernel [K, fields] Keras layout); ``mprime`` [B, fields] is added to
    their products and required without sources.  m = fields * softmax(m') with ``softmax``, else m'.  ``lin``: per position (0 or
    ``fields`` of them) a (table, ids) pair or a pre-pooled [B] vector (make_ifm_lin; ``lin_desc`` = its result, then ``lin`` is only
    counted) — refined by m BY POSITION; ``add``: up to four [B] vectors added unrefined.  Returns out [B] = fm + lin + add + bias,
    through a sigmoid with ``sigmoid_out``.  ``factor_out`` [B, >= fields]: receives m.  ``route='workspace'`` forces the route whose
    m' goes through HBM; ``workspace``: a float32 tensor of >= ifm_workspace_bytes (default: the per-stream scratch)."""
    F, d = int(fields), int(dim)
    B = int(x.shape[0])
    x_stride = _rows2d("ifm", "x", x, B, F * d)
    sources = list(sources)
    a = _ifm_args(B, F, d, len(sources), route)
    a.x, a.x_stride = x.data_ptr(), x_stride
    keep = []
    for s, (act, kernel) in enumerate(sources):
        act_stride = _rows2d("ifm", "a source's act", act, B, 1)
        K = int(act.shape[1])
        if kernel.dtype != torch.float32 or tuple(kernel.shape) != (K, F):
            raise ValueError("ifm: source %d: kernel must be float32 [%d, %d], got %s" % (s, K, F, tuple(kernel.shape)))
        kernel = _f32c(kernel, "kernel")
        keep.append(kernel)
        a.src[s].act, a.src[s].act_stride, a.src[s].K, a.src[s].kernel = act.data_ptr(), act_stride, K, kernel.data_ptr()
    if mprime is None and not sources:
        raise ValueError("ifm: neither a factor source nor mprime")
    if mprime is not None:
        a.mprime, a.mprime_stride = mprime.data_ptr(), _rows2d("ifm", "mprime", mprime, B, F)
    n_lin = len(lin)
    if n_lin not in (0, F):
        raise ValueError("ifm: %d linear terms for %d fields: the factor refines them by position, 0 or one per field" % (n_lin, F))
    if n_lin:
        if lin_desc is None:
            lin_desc = make_ifm_lin(lin, B, x.device)
        a.lin, a.n_lin = lin_desc.data_ptr(), n_lin
    add = [t for t in add if t is not None]
    if len(add) > 4:
        raise ValueError("ifm: %d add vectors: at most 4" % len(add))
    for i, t in enumerate(add):
        _vec("ifm", "an add vector", t, B)
        a.add[i] = t.data_ptr()
    a.n_add = len(add)
    if global_bias is not None:
        if global_bias.dtype != torch.float32 or global_bias.numel() != 1:
            raise ValueError("ifm: global_bias must be a float32 scalar tensor")
        a.global_bias = global_bias.data_ptr()
    if out is None:
        out = torch.empty(B, dtype=torch.float32, device=x.device)
    _vec("ifm", "out", out, B)
    if factor_out is not None:
        a.factor_out, a.factor_stride = factor_out.data_ptr(), _rows2d("ifm", "factor_out", factor_out, B, F)
    if status is not None:
        if status.dtype != torch.int32:
            raise ValueError("ifm: status must be an int32 tensor")
        a.status = status.data_ptr()
    _dev_check(x, mprime, lin_desc, global_bias, out, factor_out, status, workspace, *(add + keep + [s_[0] for s_ in sources]))
    a.softmax, a.sigmoid_out, a.out = int(bool(softmax)), int(bool(sigmoid_out)), out.data_ptr()
    _workspace("ifm", a, int(_C.lib().dctr_ifm_workspace_bytes(ctypes.byref(a))), workspace, x.device)
    _C.check(_C.lib().dctr_ifm_fwd(ctypes.byref(a), _C.stream_ptr()), "dctr_ifm_fwd")
    del keep
    return out


def _ifm_bwd_shape(batch, fields, dim, Ks=(), dmprime=False, dact=True, dkernel=True, slices=0):
    """dctr_ifm_bwd_args_t of the shapes alone, for the host-only queries: a wanted output is any non-NULL pointer."""
    F, d = int(fields), int(dim)
    if F < 1 or d < 1:
        raise ValueError("ifm_bwd: fields = %d, dim = %d" % (F, d))
    if len(Ks) > 2:
        raise ValueError("ifm_bwd: %d factor sources: 0, 1 or 2" % len(Ks))
    b = _C.ifm.BwdArgs(batch=int(batch), n_fields=F, dim=d, x_stride=F * d, factor_stride=F, n_src=len(Ks), slices=int(slices))
    if dmprime:
        b.dmprime, b.dmprime_stride = 16, F
    for s, K in enumerate(Ks):
        b.src[s].K, b.src[s].act_stride = int(K), int(K)
        if dact:
            b.dact[s], b.dact_stride[s] = 16, int(K)
        if dkernel:
            b.dkernel[s], b.dkernel_stride[s] = 16, F
    return b


def ifm_bwd_supported(fields, dim):
    """Does dctr_ifm_bwd take these shapes (read from the library: a row of ``fields`` floats has to fit the LDS)?"""
    if int(fields) < 1 or int(dim) < 1:
        return False
    return bool(_C.lib().dctr_ifm_bwd_supported(ctypes.byref(_C.ifm.BwdArgs(batch=1, n_fields=int(fields), dim=int(dim)))))


def ifm_bwd_workspace_bytes(batch, fields, dim, Ks=(), dmprime=False, dact=True, dkernel=True, slices=0):
    """Bytes of workspace dctr_ifm_bwd needs (read from the library): ``Ks`` = K per factor source; ``dmprime`` / ``dact`` / ``dkernel``:
    is that gradient wanted (dm' waits in the workspace when a source's gradient is wanted and dmprime is not; the dkernel partials
    of ``slices`` batch slices, 0 = the library's choice)."""
    return int(_C.lib().dctr_ifm_bwd_workspace_bytes(ctypes.byref(_ifm_bwd_shape(batch, fields, dim, Ks, dmprime, dact, dkernel, slices))))


def _ifm_bwd_out(name, want, rows, cols, device):
    """An output of ifm_bwd: None / False (not wanted), True (allocated here) or the caller's float32 2-D view -> (tensor, row stride)."""
    if want is None or want is False:
        return None, 0
    if want is True:
        want = torch.empty(rows, cols, dtype=torch.float32, device=device)
    return want, _rows2d("ifm_bwd", name, want, rows, cols)


def ifm_bwd(x, fields, dim, factor, d_out, sources=(), terms=None, softmax=False, dx=None, dterms=None, dmprime=None, dact=None,
            dkernel=None, slices=0, workspace=None):
    """Backward of the differentiable part of ifm() (include/dctr.h: dctr_ifm_bwd): the logit without add vectors, bias and sigmoid.
    ``x`` / ``fields`` / ``dim`` / ``sources`` / ``softmax`` as ifm(); ``factor`` [B, >= fields]: the m the forward wrote to
    factor_out; ``terms`` [B, >= fields] or None: the first-order terms by position; ``d_out`` [B].  Outputs — each None / False (not
    wanted, its work is skipped), True (allocated here) or a float32 2-D view that is OVERWRITTEN in its leading columns: ``dx``
    [B, >= fields*dim], ``dterms`` and ``dmprime`` [B, >= fields], and per source ``dact[s]`` [B, >= K_s] and ``dkernel[s]``
    [K_s, >= fields].  ``slices``: the batch slices of the dkernel sum (0: the library's choice, 1 .. 256 forces it).  No atomics:
    bit-identical from call to call.  Returns (dx, dterms, dmprime, [dact], [dkernel])."""
    F, d = int(fields), int(dim)
    B = int(x.shape[0])
    sources = list(sources)
    if len(sources) > 2:
        raise ValueError("ifm_bwd: %d factor sources: 0, 1 or 2" % len(sources))
    if not 0 <= int(slices) <= 256:
        raise ValueError("ifm_bwd: slices = %d: 0 or 1 .. 256" % int(slices))
    b = _C.ifm.BwdArgs(batch=B, n_fields=F, dim=d, n_src=len(sources), softmax=int(bool(softmax)), slices=int(slices))
    b.x, b.x_stride = x.data_ptr(), _rows2d("ifm_bwd", "x", x, B, F * d)
    b.factor, b.factor_stride = factor.data_ptr(), _rows2d("ifm_bwd", "factor", factor, B, F)
    if terms is not None:
        b.terms, b.terms_stride = terms.data_ptr(), _rows2d("ifm_bwd", "terms", terms, B, F)
    _vec("ifm_bwd", "d_out", d_out, B)
    b.d_out = d_out.data_ptr()
    dev = x.device
    dx, b.dx_stride = _ifm_bwd_out("dx", dx, B, F * d, dev)
    dterms, b.dterms_stride = _ifm_bwd_out("dterms", dterms, B, F, dev)
    dmprime, b.dmprime_stride = _ifm_bwd_out("dmprime", dmprime, B, F, dev)
    for t, n in ((dx, "dx"), (dterms, "dterms"), (dmprime, "dmprime")):
        if t is not None:
            setattr(b, n, t.data_ptr())
    dact = list(dact) if dact is not None else [None] * len(sources)
    dkernel = list(dkernel) if dkernel is not None else [None] * len(sources)
    if len(dact) != len(sources) or len(dkernel) != len(sources):
        raise ValueError("ifm_bwd: dact / dkernel take one entry per factor source (%d)" % len(sources))
    keep = []
    for s, (act, kernel) in enumerate(sources):
        act_stride = _rows2d("ifm_bwd", "a source's act", act, B, 1)
        K = int(act.shape[1])
        if kernel.dtype != torch.float32 or tuple(kernel.shape) != (K, F):
            raise ValueError("ifm_bwd: source %d: kernel must be float32 [%d, %d], got %s" % (s, K, F, tuple(kernel.shape)))
        kernel = _f32c(kernel, "kernel")
        keep.append(kernel)
        b.src[s].act, b.src[s].act_stride, b.src[s].K, b.src[s].kernel = act.data_ptr(), act_stride, K, kernel.data_ptr()
        dact[s], b.dact_stride[s] = _ifm_bwd_out("dact[%d]" % s, dact[s], B, K, dev)
        dkernel[s], b.dkernel_stride[s] = _ifm_bwd_out("dkernel[%d]" % s, dkernel[s], K, F, dev)
        if dact[s] is not None:
            b.dact[s] = dact[s].data_ptr()
        if dkernel[s] is not None:
            b.dkernel[s] = dkernel[s].data_ptr()
    _dev_check(x, factor, terms, d_out, dx, dterms, dmprime, workspace, *(dact + dkernel + keep + [s_[0] for s_ in sources]))
    _workspace("ifm_bwd", b, int(_C.lib().dctr_ifm_bwd_workspace_bytes(ctypes.byref(b))), workspace, dev)
    _C.check(_C.lib().dctr_ifm_bwd(ctypes.byref(b), _C.stream_ptr()), "dctr_ifm_bwd")
    del keep
    return dx, dterms, dmprime, dact, dkernel


_IFM_TERM_DESCS = OrderedDict()


def _ifm_term_columns(terms, F):
    """The dctr_ifm_lin_t array that hands ifm() the columns of ``terms`` [B, F] as F pre-pooled vectors at vec_stride = its row stride.
    The array is a function of (pointer, F, row stride, device) alone: cached on them."""
    stride = row_stride(terms)
    key = (terms.data_ptr(), F, stride, str(terms.device))
    desc = _IFM_TERM_DESCS.get(key)
    if desc is None:
        arr = (_C.ifm.Lin * F)()
        for k in range(F):
            arr[k].vec, arr[k].vec_stride = terms.data_ptr() + 4 * k, stride
        while len(_IFM_TERM_DESCS) >= 64:
            _IFM_TERM_DESCS.popitem(last=False)
        desc = _IFM_TERM_DESCS[key] = _upload(arr, terms.device)
    return desc


class InputAwareFMFunction(torch.autograd.Function):
    """The input-aware FM of IFM / DIFM as one differentiable op (once differentiable): ifm() forward with the factor kept, ifm_bwd()
    backward.  ``apply(x, terms, mprime, softmax, *flat)``: x [B,F,d]; ``terms`` [B,F] (the first-order terms by position) or None;
    ``mprime`` [B,F] or None; ``flat`` = act_0, kernel_0 (, act_1, kernel_1): the factor sources.  Returns the logit [B] without the
    unrefined tail (no add vectors, no bias, no sigmoid).  Gradients are formed only for the inputs that need them; none leaves
    through atomics."""

    @staticmethod
    def forward(ctx, x, terms, mprime, softmax, *flat):
        ctx.set_materialize_grads(False)
        if x.dim() != 3 or len(flat) not in (0, 2, 4):
            raise ValueError("InputAwareFMFunction: x must be [B,F,d] and the sources (act, kernel) pairs")
        B, F, d = x.shape
        x2 = _f32c(x.detach(), "x").view(B, F * d)
        srcs = [(_grad_operand(flat[i].detach(), True), _f32c(flat[i + 1].detach(), "kernel")) for i in range(0, len(flat), 2)]
        t = None if terms is None else _grad_operand(terms.detach(), True)
        mp = None if mprime is None else _grad_operand(mprime.detach(), True)
        factor = torch.empty(B, F, dtype=torch.float32, device=x.device)
        lin_desc = None if t is None else _ifm_term_columns(t, F)
        out = ifm(x2, F, d, sources=srcs, mprime=mp, softmax=softmax, lin=() if t is None else (None,) * F, lin_desc=lin_desc,
                  factor_out=factor, sigmoid_out=False)
        ctx.softmax, ctx.n_src, ctx.has_terms, ctx.shape = bool(softmax), len(srcs), t is not None, (B, F, d)
        ctx.save_for_backward(x2, factor, *([t] if t is not None else []), *[v for s in srcs for v in s])
        return out

    @staticmethod
    def backward(ctx, d_out):
        B, F, d = ctx.shape
        n = 4 + 2 * ctx.n_src
        if d_out is None:
            return (None,) * n
        saved = list(ctx.saved_tensors)
        x2, factor = saved[0], saved[1]
        t = saved[2] if ctx.has_terms else None
        flat = saved[3 if ctx.has_terms else 2:]
        srcs = [(flat[i], flat[i + 1]) for i in range(0, len(flat), 2)]
        need = ctx.needs_input_grad
        dx, dterms, dmprime, dact, dkernel = ifm_bwd(
            x2, F, d, factor, _grad_operand(d_out, False), sources=srcs, terms=t, softmax=ctx.softmax, dx=bool(need[0]),
            dterms=bool(need[1]) and t is not None, dmprime=bool(need[2]), dact=[bool(need[4 + 2 * s]) for s in range(ctx.n_src)],
            dkernel=[bool(need[5 + 2 * s]) for s in range(ctx.n_src)])
        ret = [None if dx is None else dx.view(B, F, d), dterms, dmprime, None]
        for s in range(ctx.n_src):
            ret += [dact[s], dkernel[s]]
        return tuple(ret)


_FIELDWISE_ROUTES ={None: _C.fieldwise.ROUTE_AUTO, "auto": _C.fieldwise.ROUTE_AUTO, "reread": _C.fieldwise.ROUTE_REREAD}
_FIELDWISE_TABLES = {}


def fieldwise_groups(groups, device):
    """The group table [(first column, n fields)] as dctr_fieldwise_group_t arrays: (device tensor, host array), cached per table
    and device (a model passes the same table on every call)."""
    key = (str(device), tuple((int(a), int(n)) for a, n in groups))
    hit = _FIELDWISE_TABLES.get(key)
    if hit is None:
        host = (_C.fieldwise.Group * max(1, len(key[1])))()
        for i, (a, n) in enumerate(key[1]):
            host[i].first, host[i].n_fields = a, n
        raw = np.frombuffer(host, dtype=np.uint8).copy()
        if len(_FIELDWISE_TABLES) >= 64:
            _FIELDWISE_TABLES.clear()
        hit = _FIELDWISE_TABLES[key] = (torch.from_numpy(raw).to(device), host)
    return hit


def _fieldwise_args(x, groups, dim, x_offset, route, device=None, x_stride=0):
    if route not in _FIELDWISE_ROUTES:
        raise ValueError("fieldwise: route %r: expected None, 'auto' or 'reread'" % (route,))
    groups = list(groups)
    a = _C.fieldwise.Args(n_groups=len(groups), dim=int(dim), x_offset=int(x_offset), route=_FIELDWISE_ROUTES[route])
    dev_t, host = fieldwise_groups(groups, device) if device is not None else (None, fieldwise_groups(groups, "cpu")[1])
    a.groups_host = ctypes.addressof(host)
    keep = [host, dev_t]
    if dev_t is not None:
        a.groups = dev_t.data_ptr()
    if x is not None:
        a.batch, a.x, a.x_stride = x.shape[0], x.data_ptr(), x_stride
    else:
        a.x_stride = int(x_offset) + max([f + n * int(dim) for f, n in groups] + [0])
    return a, keep


def fieldwise_route(groups, dim, route=None):
    """The route dctr_fieldwise_fwd takes for these shapes: 'on_chip' (the group sums wait in LDS) or 'reread' (read from the library)."""
    a, _keep = _fieldwise_args(None, groups, dim, 0, route)
    return _route_name("dctr_fieldwise_route", _C.lib().dctr_fieldwise_route(ctypes.byref(a)),
                       {_C.fieldwise.ROUTE_ON_CHIP: "on_chip", _C.fieldwise.ROUTE_REREAD: "reread"})


def fieldwise_bwd_supported(groups, dim):
    """Does dctr_fieldwise_bwd take these shapes (its group sums and accumulators fit the LDS)?"""
    b = _C.fieldwise.BwdArgs()
    b.fwd, _keep = _fieldwise_args(None, groups, dim, 0, None)
    return bool(_C.lib().dctr_fieldwise_bwd_supported(ctypes.byref(b)))


def _fieldwise_operands(op, x, x_offset, groups, dim, kernel_mf, kernel_fm, bias_mf, bias_fm):
    """The checks fieldwise() and fieldwise_bwd() share: (x's row pitch, the columns the groups span, the weights made contiguous)."""
    G = len(groups)
    if G < 2:
        raise ValueError("A `Field-Wise Bi-Interaction` layer should be called on a list of at least 2 inputs")
    if min(f for f, _ in groups) < 0:
        raise ValueError("%s: a group starts before column 0" % op)
    span = max(f + n * dim for f, n in groups)
    x_stride = _rows2d(op, "x", x, x.shape[0], span, x_offset)
    kernel_mf, kernel_fm = _f32c(kernel_mf, "kernel_mf"), _f32c(kernel_fm, "kernel_fm")
    if kernel_mf.numel() != G * (G - 1) // 2 or kernel_fm.numel() != G:
        raise ValueError("fieldwise: %d groups take kernel_mf [%d, 1] and kernel_fm [%d, 1]" % (G, G * (G - 1) // 2, G))
    if (bias_mf is None) != (bias_fm is None):
        raise ValueError("fieldwise: bias_mf and bias_fm come together (use_bias)")
    if bias_mf is not None:
        bias_mf, bias_fm = _f32c(bias_mf, "bias_mf"), _f32c(bias_fm, "bias_fm")
        if bias_mf.numel() != dim or bias_fm.numel() != dim:
            raise ValueError("fieldwise: the biases hold dim = %d elements" % dim)
    return x_stride, span, kernel_mf, kernel_fm, bias_mf, bias_fm


def fieldwise(x, groups, dim, kernel_mf, kernel_fm, bias_mf=None, bias_fm=None, x_offset=0, y=None, y_offset=0, head_w=None,
              add=None, logit=None, route=None):
    """FieldWiseBiInteraction.call (reference interaction.py:1283-1339), one launch.  x: a float32 [B, stride] buffer read in place;
    ``groups``: [(first column, n fields)] counted from column ``x_offset``, every field ``dim`` wide (EmbeddingStage.group_slices).
    The weights are the live tensors.  ``y``: True (a new [B, dim] tensor) or a float32 2-D view whose rows receive the dim values
    from column ``y_offset``; ``logit``: True or a float32 [B] tensor = y . head_w (+ ``add`` [B]).  Default: y.  Returns (y, logit)."""
    dim = int(dim)
    groups = [(int(a), int(n)) for a, n in groups]
    x_stride, _, kernel_mf, kernel_fm, bias_mf, bias_fm = _fieldwise_operands("fieldwise", x, x_offset, groups, dim, kernel_mf, kernel_fm,
                                                                              bias_mf, bias_fm)
    B = x.shape[0]
    if y is None and logit is None:
        y = True
    if y is True:
        y, y_offset = torch.empty(B, dim, dtype=torch.float32, device=x.device), 0
    if logit is True:
        logit = torch.empty(B, dtype=torch.float32, device=x.device)
    y_stride = 0 if y is None else _rows2d("fieldwise", "y", y, B, dim, y_offset)
    if logit is not None:
        _vec("fieldwise", "logit", logit, B)
        if head_w is None:
            raise ValueError("fieldwise: a logit needs head_w [dim]")
        head_w = _f32c(head_w, "head_w")
        if head_w.numel() != dim:
            raise ValueError("fieldwise: head_w must hold dim = %d elements" % dim)
    if add is not None:
        if logit is None:
            raise ValueError("fieldwise: add needs a logit output")
        add = _f32c(add, "add")
        if add.numel() != B:
            raise ValueError("fieldwise: add must hold %d elements" % B)
    _dev_check(x, kernel_mf, kernel_fm, bias_mf, bias_fm, y, head_w, add, logit)
    a, _keep = _fieldwise_args(x, groups, dim, x_offset, route, x.device, x_stride)
    a.kernel_mf, a.kernel_fm = kernel_mf.data_ptr(), kernel_fm.data_ptr()
    if bias_mf is not None:
        a.bias_mf, a.bias_fm = bias_mf.data_ptr(), bias_fm.data_ptr()
    if y is not None:
        a.y, a.y_stride, a.y_offset = y.data_ptr(), y_stride, int(y_offset)
    if logit is not None:
        a.logit, a.head_w = logit.data_ptr(), head_w.data_ptr()
    if add is not None:
        a.add = add.data_ptr()
    _C.check(_C.lib().dctr_fieldwise_fwd(ctypes.byref(a), _C.stream_ptr()), "dctr_fieldwise_fwd")
    return y, logit


def fieldwise_bwd(x, groups, dim, kernel_mf, kernel_fm, bias_mf=None, bias_fm=None, x_offset=0, dy=None, dlogit=None, head_w=None,
                  dx=None, dx_offset=0, accumulate=False, d_kernel_mf=None, d_kernel_fm=None, d_bias_mf=None, d_bias_fm=None,
                  d_head_w=None, max_blocks=0):
    """Backward of fieldwise() (include/dctr.h: dctr_fieldwise_bwd).  Upstream gradient: ``dy`` [B, >= dim], or ``dlogit`` [B] with
    ``head_w`` [dim].  ``dx`` [B, stride]: the groups' columns from ``dx_offset`` are written, or added to with ``accumulate``.  The
    weight gradients (shapes of the weights; ``d_head_w`` with dlogit only) are ACCUMULATED; any may be None."""
    dim = int(dim)
    groups = [(int(a), int(n)) for a, n in groups]
    x_stride, span, kernel_mf, kernel_fm, bias_mf, bias_fm = _fieldwise_operands("fieldwise_bwd", x, x_offset, groups, dim, kernel_mf,
                                                                                 kernel_fm, bias_mf, bias_fm)
    B = x.shape[0]
    if (dy is None) == (dlogit is None):
        raise ValueError("fieldwise_bwd: exactly one of dy / dlogit")
    if dy is not None:
        dy_stride = _rows2d("fieldwise_bwd", "dy", dy, B, dim)
        if d_head_w is not None:
            raise ValueError("fieldwise_bwd: d_head_w needs the dlogit form")
    else:
        _vec("fieldwise_bwd", "dlogit", dlogit, B)
        if head_w is None:
            raise ValueError("fieldwise_bwd: dlogit needs head_w [dim]")
        _vec("fieldwise_bwd", "head_w", head_w, dim)
    dx_stride = 0 if dx is None else _rows2d("fieldwise_bwd", "dx", dx, B, span, dx_offset)
    G = len(groups)
    for t, n, name in ((d_kernel_mf, G * (G - 1) // 2, "d_kernel_mf"), (d_kernel_fm, G, "d_kernel_fm"), (d_bias_mf, dim, "d_bias_mf"),
                       (d_bias_fm, dim, "d_bias_fm"), (d_head_w, dim, "d_head_w")):
        if t is not None:
            _vec("fieldwise_bwd", name, t, n)
    _dev_check(x, kernel_mf, kernel_fm, bias_mf, bias_fm, dy, dlogit, head_w, dx, d_kernel_mf, d_kernel_fm, d_bias_mf, d_bias_fm, d_head_w)
    b = _C.fieldwise.BwdArgs()
    b.fwd, _keep = _fieldwise_args(x, groups, dim, x_offset, None, x.device, x_stride)
    f = b.fwd
    f.kernel_mf, f.kernel_fm, f.max_blocks = kernel_mf.data_ptr(), kernel_fm.data_ptr(), int(max_blocks)
    if bias_mf is not None:
        f.bias_mf, f.bias_fm = bias_mf.data_ptr(), bias_fm.data_ptr()
    if dy is not None:
        b.dy, b.dy_stride = dy.data_ptr(), dy_stride
    else:
        b.dlogit, f.head_w = dlogit.data_ptr(), head_w.data_ptr()
    if dx is not None:
        b.dx, b.dx_stride, b.dx_offset, b.accumulate = dx.data_ptr(), dx_stride, int(dx_offset), int(bool(accumulate))
    for name, t in (("d_kernel_mf", d_kernel_mf), ("d_kernel_fm", d_kernel_fm), ("d_bias_mf", d_bias_mf), ("d_bias_fm", d_bias_fm),
                    ("d_head_w", d_head_w)):
        if t is not None:
            setattr(b, name, t.data_ptr())
    _C.check(_C.lib().dctr_fieldwise_bwd(ctypes.byref(b), _C.stream_ptr()), "dctr_fieldwise_bwd")


_EDCN_ROUTES = {None: _C.edcn.ROUTE_AUTO, "auto": _C.edcn.ROUTE_AUTO, "layered": _C.edcn.ROUTE_LAYERED}
_EDCN_ROUTE_NAMES = {_C.edcn.ROUTE_FUSED: "fused", _C.edcn.ROUTE_LAYERED: "layered"}
_EDCN_GEMM_K = 768              # reduction length of one dctr_sgemm call of the layered route's wide matrix cross (_edcn_cross)


def _edcn_args(batch, fields, dim, cross_num, bridge_type, parameterization, tau, activation, bridge_activation, route, x_stride=None,
               x_offset=0):
    if bridge_type not in _C.edcn.BRIDGES:
        raise ValueError("edcn: bridge_type %r: expected one of %s" % (bridge_type, sorted(_C.edcn.BRIDGES)))
    if parameterization not in ("vector", "matrix"):
        raise ValueError("parameterization should be 'vector' or 'matrix'")
    if route not in _EDCN_ROUTES:
        raise ValueError("edcn: route %r: expected None, 'auto' or 'layered'" % (route,))
    if tau == 0:
        raise ValueError("RegulationModule tau can not be zero.")
    if cross_num < 1:
        raise ValueError("Cross layer num must > 0")
    if activation not in _C.ACT_CODES or bridge_activation not in _C.ACT_CODES:
        raise ValueError("edcn: unknown activation %r / %r" % (activation, bridge_activation))
    D = int(fields) * int(dim)
    return _C.edcn.Args(batch=int(batch), x_stride=int(x_offset) + D if x_stride is None else int(x_stride), x_offset=int(x_offset),
                        fields=int(fields), dim=int(dim), cross_num=int(cross_num),
                        mode=_C.CROSS_VECTOR if parameterization == "vector" else _C.CROSS_MATRIX, bridge=_C.edcn.BRIDGES[bridge_type],
                        activation=_C.ACT_CODES[activation], bridge_activation=_C.ACT_CODES[bridge_activation], inv_tau=1.0 / tau,
                        route=_EDCN_ROUTES[route])


def edcn_route(fields, dim, cross_num=1, bridge_type="hadamard_product", parameterization="vector", activation="relu",
               bridge_activation="relu", route=None):
    """The route ops.edcn takes for these shapes and options: 'fused' (one dctr_edcn_fwd launch, the tiles in LDS) or 'layered' (read
    from the library: it knows what its LDS holds)."""
    a = _edcn_args(0, fields, dim, cross_num, bridge_type, parameterization, 1.0, activation, bridge_activation, route)
    return _route_name("dctr_edcn_route", _C.lib().dctr_edcn_route(ctypes.byref(a)), _EDCN_ROUTE_NAMES)


def edcn_regulate(x, g_deep, g_cross=None, tau=1.0, fields=None, dim=None, x_offset=0, deep=None, cross=None):
    """RegulationModule.call (reference core.py:304-312) over one read of x, for one or two gates: x [B,F,E], or with ``fields`` /
    ``dim`` the F*E columns from ``x_offset`` of a 2-D buffer; g_* hold F live weights.  ``deep`` / ``cross``: float32 2-D views to write
    [B, F*E] into (default: new tensors).  Returns (deep, cross); cross is None without g_cross."""
    if tau == 0:
        raise ValueError("RegulationModule tau can not be zero.")
    x, B, F, E, x_stride, x_offset = _x_in_place("edcn_regulate", x, fields, dim, x_offset)
    D = F * E
    _vec("edcn_regulate", "g_deep", g_deep, F)
    if g_cross is not None:
        _vec("edcn_regulate", "g_cross", g_cross, F)
    elif cross is not None:
        raise ValueError("edcn_regulate: a cross output needs g_cross")
    if deep is None:
        deep = torch.empty(B, D, dtype=torch.float32, device=x.device)
    if cross is None and g_cross is not None:
        cross = torch.empty(B, D, dtype=torch.float32, device=x.device)
    deep_stride = _rows2d("edcn_regulate", "deep", deep, B, D)
    cross_stride = 0 if cross is None else _rows2d("edcn_regulate", "cross", cross, B, D)
    _dev_check(x, g_deep, g_cross, deep, cross)
    _C.check(_C.lib().dctr_edcn_regulate(x.data_ptr() + 4 * x_offset, x_stride, B, F, E, _ptr(g_deep), _ptr(g_cross), 1.0 / tau, _ptr(deep),
                                         deep_stride, _ptr(cross), cross_stride, _C.stream_ptr()), "dctr_edcn_regulate")
    return deep, cross


def edcn_bridge(c, h, bridge_type, ax=None, ah=None, out=None):
    """BridgeModule.call's elementwise forms (reference interaction.py:1542-1553) on float32 2-D views [B, D]: 'pointwise_addition',
    'hadamard_product', or 'attention_pooling' = softmax(ax) * c + softmax(ah) * h with ``ax`` / ``ah`` the scores before the softmax
    over the row.  ('concatenation' is a Dense: ops.mlp.)"""
    if bridge_type not in ("pointwise_addition", "hadamard_product", "attention_pooling"):
        raise ValueError("edcn_bridge: bridge_type %r is no elementwise bridge" % (bridge_type,))
    if c.dim() != 2:
        raise ValueError("edcn_bridge: c must be a float32 [B, D] view with unit column stride")
    B, D = c.shape
    if out is None:
        out = torch.empty(B, D, dtype=torch.float32, device=c.device)
    strides = [_rows2d("edcn_bridge", n, t, B, D) for n, t in (("c", c), ("h", h), ("out", out))]
    att = [0, 0]
    if bridge_type == "attention_pooling":
        if ax is None or ah is None:
            raise ValueError("edcn_bridge: attention_pooling needs the scores ax and ah")
        att = [_rows2d("edcn_bridge", n, t, B, D) for n, t in (("ax", ax), ("ah", ah))]
    else:
        ax = ah = None
    _dev_check(c, h, ax, ah, out)
    _C.check(_C.lib().dctr_edcn_bridge(_C.edcn.BRIDGES[bridge_type], _ptr(c), strides[0], _ptr(h), strides[1], _ptr(ax), att[0], _ptr(ah),
                                       att[1], B, D, _ptr(out), strides[2], _C.stream_ptr()), "dctr_edcn_bridge")
    return out


def _edcn_cross(xc, w, b, mode, y):
    """One CrossNet layer whose x_0 is its input: dctr_crossnet_head_fwd with layers = 1, or — a matrix wider than its tiles hold —
    dctr_sgemm + dctr_crossnet_matrix_step.  xc [B, D] contiguous; y: a [B, D] view."""
    B, D = xc.shape
    st = _C.stream_ptr()
    need = int(_C.lib().dctr_crossnet_workspace_bytes(D, 1, mode, _ptr(w)))
    ws = _scratch(xc.device, need) if need else None
    a = _C.CrossnetArgs(x=xc.data_ptr(), batch=B, x_stride=D, dim=D, layers=1, mode=mode, workspace_ready=0, kernels=w.data_ptr(),
                        bias=b.data_ptr(), y=y.data_ptr(), y_stride=row_stride(y), workspace=_ptr(ws), workspace_bytes=need)
    rc = _C.lib().dctr_crossnet_head_fwd(ctypes.byref(a), st)
    if rc == _C.E_UNSUPPORTED and mode == _C.CROSS_MATRIX:
        u = torch.empty(B, D, dtype=torch.float32, device=xc.device)
        # column-major BLAS view: u^T (D x B) = W^T-view (k x n)^T . xc^T (k x B).  dctr_sgemm cuts a reduction of >= 1024 over
        # workgroups that add with float atomics when the output has few tiles: slices of k below that, accumulated call after call
        # (beta = 1), keep the forward free of atomics — the same bits on every call
        for k0 in range(0, D, _EDCN_GEMM_K):
            _C.check(_C.lib().dctr_sgemm(1, 0, D, B, min(_EDCN_GEMM_K, D - k0), w.data_ptr() + 4 * k0, D, 0, xc.data_ptr() + 4 * k0, D, 0,
                                         0.0 if k0 == 0 else 1.0, u.data_ptr(), D, 0, 1, st), "dctr_sgemm")
        rc = _C.lib().dctr_crossnet_matrix_step(xc.data_ptr(), D, xc.data_ptr(), D, u.data_ptr(), b.data_ptr(), B, D, y.data_ptr(),
                                                row_stride(y), st)
        _C.check(rc, "dctr_crossnet_matrix_step")
        return
    _C.check(rc, "dctr_crossnet_head_fwd")


def _edcn_layered(x, B, F, E, x_offset, gates, cross_kernels, cross_biases, dnn_kernels, dnn_biases, bridge_type, mode, tau, activation,
                  bn, dice, bridge_weights, bridge_activation, head_w, add, global_bias, sigmoid_out, logit, out, out_offset):
    """The tower layer by layer on the existing entry points: per round one regulate launch, the CrossNet layer, the DNN, the bridge."""
    D, L, dev = F * E, len(dnn_kernels), x.device
    stack = torch.empty(B, 3 * D, dtype=torch.float32, device=dev) if out is None else out[:, out_offset:out_offset + 3 * D]
    c, h, br = stack[:, :D], stack[:, D:2 * D], stack[:, 2 * D:]
    deep = torch.empty(B, D, dtype=torch.float32, device=dev)
    cross = torch.empty(B, D, dtype=torch.float32, device=dev)
    att = bridge_type == "attention_pooling"
    if att:
        ax, ah = (torch.empty(B, D, dtype=torch.float32, device=dev) for _ in range(2))
    src, src_off = x, x_offset
    for i in range(L):
        edcn_regulate(src, gates[2 * i], gates[2 * i + 1], tau, fields=F, dim=E, x_offset=src_off, deep=deep, cross=cross)
        _edcn_cross(cross, cross_kernels[i], cross_biases[i], mode, c)
        mlp(deep, [dnn_kernels[i]], [dnn_biases[i]], activation, dice=None if dice is None else [dice[i]],
            bn=None if bn is None else [bn[i]], in_dim=D, out=h)
        if bridge_type == "concatenation":
            wb, bb = bridge_weights[i]
            mlp(stack, [wb], [bb], bridge_activation, in_dim=2 * D, out=br)
        elif att:
            for src_t, (k0, b0, k1, b1), dst in ((c, bridge_weights[i][0], ax), (h, bridge_weights[i][1], ah)):
                hid = mlp(src_t, [k0], [b0], bridge_activation, in_dim=D)
                mlp(hid, [k1], [b1], "linear", in_dim=D, out=dst)
            edcn_bridge(c, h, bridge_type, ax=ax, ah=ah, out=br)
        else:
            edcn_bridge(c, h, bridge_type, out=br)
        src, src_off = br, 0
    if logit is not None:
        mlp(stack, [], [], "linear", head_w=head_w, add=add, global_bias=global_bias, sigmoid_out=sigmoid_out, in_dim=3 * D, out=logit)


def edcn(x, fields, dim, gates, cross_kernels, cross_biases, dnn_kernels, dnn_biases, bridge_type="hadamard_product",
         parameterization="vector", tau=1.0, activation="relu", bn=None, dice=None, bridge_weights=None, bridge_activation="relu",
         x_offset=0, head_w=None, add=(), global_bias=None, sigmoid_out=False, logit=None, out=None, out_offset=0, route=None,
         workspace=None):
    """EDCN's tower (reference models/edcn.py:66-87; include/dctr.h: dctr_edcn_fwd).  x: a float32 [B, stride] buffer whose ``fields``
    * ``dim`` columns from ``x_offset`` are read in place.  Per round i (cross_num = len(dnn_kernels)): ``gates[2i]`` / ``gates[2i+1]``
    the F field weights of the deep / cross RegulationModule, ``cross_kernels[i]`` [D, 1] or [D, D] with ``cross_biases[i]`` [D, 1],
    ``dnn_kernels[i]`` [D, D] with ``dnn_biases[i]`` [D], ``bn[i]`` None or (scale, shift), ``dice[i]`` (alpha, mean, variance) with
    activation 'dice', ``bridge_weights[i]``: (kernel [2D, D], bias [D]) for 'concatenation', ((k0, b0, k1, b1) of the DNN over c,
    the same over h) for 'attention_pooling'.  All weights are the live tensors.
    Outputs: ``logit`` (True or a float32 [B] tensor) = [c, h, br] . head_w + sum(add) + global_bias (sigmoid with sigmoid_out);
    ``out`` (True or a float32 2-D view) receives c, h, br of the last round in columns [out_offset, out_offset + 3D).  Default: the
    logit with head_w, else out.  One launch where ops.edcn_route says 'fused', else layer by layer.  Returns (logit, out)."""
    x, B, F, E, x_stride, x_offset = _x_in_place("edcn", x, int(fields), int(dim), x_offset)
    D, L = F * E, len(dnn_kernels)
    a = _edcn_args(B, F, E, L, bridge_type, parameterization, tau, activation, bridge_activation, route, x_stride, x_offset)
    if not (len(gates) == 2 * L and len(cross_kernels) == len(cross_biases) == len(dnn_biases) == L):
        raise ValueError("edcn: %d rounds take %d gates and %d of every other weight" % (L, 2 * L, L))
    for k, g in enumerate(gates):
        _vec("edcn", "gates[%d]" % k, g, F)
    for i in range(L):
        _vec("edcn", "cross_kernels[%d]" % i, cross_kernels[i], D if parameterization == "vector" else D * D)
        _vec("edcn", "cross_biases[%d]" % i, cross_biases[i], D)
        _vec("edcn", "dnn_kernels[%d]" % i, dnn_kernels[i], D * D)
        _vec("edcn", "dnn_biases[%d]" % i, dnn_biases[i], D)
    flat = list(gates) + list(cross_kernels) + list(cross_biases) + list(dnn_kernels) + list(dnn_biases)
    if bn is not None:
        if len(bn) != L:
            raise ValueError("edcn: bn holds one entry (None or (scale, shift)) per round")
        for i, sb in enumerate(bn):
            if sb is not None:
                _vec("edcn", "bn[%d] scale" % i, sb[0], D)
                _vec("edcn", "bn[%d] shift" % i, sb[1], D)
                flat += list(sb)
        if all(sb is None for sb in bn):
            bn = None
    if activation in ("dice", "Dice"):
        if dice is None or len(dice) != L:
            raise ValueError("edcn: activation 'dice' takes dice = [(alpha, moving_mean, moving_variance)] per round")
        for i, dp in enumerate(dice):
            for t in dp:
                _vec("edcn", "dice[%d]" % i, t, D)
            flat += list(dp)
    else:
        dice = None
    if bridge_type in ("concatenation", "attention_pooling"):
        if bridge_weights is None or len(bridge_weights) != L:
            raise ValueError("edcn: bridge_type %r takes bridge_weights per round" % bridge_type)
        for i, bw in enumerate(bridge_weights):
            if bridge_type == "concatenation":
                _vec("edcn", "bridge_weights[%d] kernel" % i, bw[0], 2 * D * D)
                _vec("edcn", "bridge_weights[%d] bias" % i, bw[1], D)
                flat += list(bw)
            else:
                for half in bw:
                    for j, t in enumerate(half):
                        _vec("edcn", "bridge_weights[%d]" % i, t, D if j % 2 else D * D)
                    flat += list(half)
    if logit is None and out is None:
        logit, out = (True, None) if head_w is not None else (None, True)
    if logit is True:
        logit = torch.empty(B, dtype=torch.float32, device=x.device)
    if out is True:
        out, out_offset = torch.empty(B, 3 * D, dtype=torch.float32, device=x.device), 0
    add = [t for t in add if t is not None]
    if logit is not None:
        _vec("edcn", "logit", logit, B)
        if head_w is None:
            raise ValueError("edcn: a logit needs head_w [3 * fields * dim]")
        _vec("edcn", "head_w", head_w, 3 * D)
        if len(add) > 4:
            raise ValueError("edcn: at most four logits to add")
        for t in add:
            _vec("edcn", "add", t, B)
        if global_bias is not None:
            _vec("edcn", "global_bias", global_bias, 1)
    elif add or global_bias is not None or sigmoid_out:
        raise ValueError("edcn: add / global_bias / sigmoid_out need a logit output")
    out_stride = 0 if out is None else _rows2d("edcn", "out", out, B, 3 * D, out_offset)
    _dev_check(x, head_w, global_bias, logit, out, *(flat + add))
    lib = _C.lib()
    if _route_name("dctr_edcn_route", lib.dctr_edcn_route(ctypes.byref(a)), _EDCN_ROUTE_NAMES) == "layered":
        _edcn_layered(x, B, F, E, x_offset, gates, cross_kernels, cross_biases, dnn_kernels, dnn_biases, bridge_type, a.mode, tau, activation,
                      bn, dice, bridge_weights, bridge_activation, head_w, add, global_bias, sigmoid_out, logit, out, out_offset)
        return logit, out
    keep = [_ptr_array(ts) for ts in (gates, cross_kernels, cross_biases, dnn_kernels, dnn_biases)]
    a.x = x.data_ptr()
    a.gates, a.cross_w, a.cross_b, a.dnn_w, a.dnn_b = (ctypes.cast(p, ctypes.c_void_p) for p in keep)
    if bn is not None:
        keep += [_ptr_array([None if sb is None else sb[j] for sb in bn]) for j in range(2)]
        a.bn_scale, a.bn_shift = (ctypes.cast(p, ctypes.c_void_p) for p in keep[-2:])
    if bridge_type == "concatenation":
        keep += [_ptr_array([bw[j] for bw in bridge_weights]) for j in range(2)]
        a.bridge_w, a.bridge_b = (ctypes.cast(p, ctypes.c_void_p) for p in keep[-2:])
    if logit is not None:
        a.logit, a.head_w, a.sigmoid_out = logit.data_ptr(), head_w.data_ptr(), int(bool(sigmoid_out))
        for i, t in enumerate(add):
            a.add[i] = t.data_ptr()
        if global_bias is not None:
            a.global_bias = global_bias.data_ptr()
    if out is not None:
        a.out, a.out_stride, a.out_offset = out.data_ptr(), out_stride, int(out_offset)
    _keep_ws = _workspace("edcn", a, int(lib.dctr_edcn_workspace_bytes(ctypes.byref(a))), workspace, x.device)
    _C.check(lib.dctr_edcn_fwd(ctypes.byref(a), _C.stream_ptr()), "dctr_edcn_fwd")
    return logit, out


def _edcn_train_shape(batch, fields, dim, cross_num, bridge_type, parameterization, activation, bridge_activation, bn=False, weights=True,
                      slices=0):
    """dctr_edcn_train_args_t with the fields the host-only queries read (shapes, options, which gradients are wanted)."""
    t = _C.edcn.TrainArgs(slices=int(slices))
    t.fwd = _edcn_args(batch, fields, dim, cross_num, bridge_type, parameterization, 1.0, activation, bridge_activation, None)
    if bn:
        t.fwd.bn_scale = t.fwd.bn_shift = 16          # (compared with NULL only)
    if weights:
        t.d_dnn_w = t.d_cross_w = t.d_bridge_w = 16
    return t


def edcn_bwd_supported(fields, dim, cross_num=1, bridge_type="hadamard_product", parameterization="vector", activation="relu",
                       bridge_activation="relu", bn=False):
    """Do dctr_edcn_train_fwd / dctr_edcn_bwd take these shapes and options (read from the library: it knows its LDS plan)?  ``bn``: the
    DNNs carry a BatchNormalization affine."""
    if int(fields) < 1 or int(dim) < 1 or int(cross_num) < 1 or bridge_type not in _C.edcn.BRIDGES \
            or parameterization not in ("vector", "matrix") or activation not in _C.ACT_CODES or bridge_activation not in _C.ACT_CODES:
        return False
    t = _edcn_train_shape(0, fields, dim, cross_num, bridge_type, parameterization, activation, bridge_activation, bn)
    return bool(_C.lib().dctr_edcn_bwd_supported(ctypes.byref(t)))


def edcn_tape_bytes(batch, fields, dim, cross_num):
    """Bytes of the tape edcn_train writes: [cross_num, batch, 3 * fields * dim] float32 (read from the library)."""
    t = _edcn_train_shape(batch, fields, dim, cross_num, "hadamard_product", "vector", "relu", "relu")
    return int(_C.lib().dctr_edcn_tape_bytes(ctypes.byref(t)))


def edcn_bwd_workspace_bytes(batch, fields, dim, cross_num=1, bridge_type="hadamard_product", parameterization="vector", activation="relu",
                             bridge_activation="relu", weights=True, slices=0):
    """Bytes of workspace dctr_edcn_bwd needs (read from the library; 0 for what it refuses).  ``weights``: are the [D, D] weight
    gradients wanted (their operands and the partials of ``slices`` batch slices wait in the workspace; 0 = the library's choice)."""
    t = _edcn_train_shape(batch, fields, dim, cross_num, bridge_type, parameterization, activation, bridge_activation, False, weights, slices)
    return int(_C.lib().dctr_edcn_bwd_workspace_bytes(ctypes.byref(t)))


def _edcn_train_operands(op, x, fields, dim, gates, cross_kernels, cross_biases, dnn_kernels, dnn_biases, bridge_type, parameterization, tau,
                         activation, bridge_weights, bridge_activation, x_offset, head_w):
    """What edcn_train() and edcn_bwd() read alike: x (_x_in_place) and the live weights of every round, checked as edcn() checks them.
    Returns (t, x, B, F, E, L, keep, tensors): ``t`` the dctr_edcn_train_args_t with t.fwd filled, ``keep`` the host pointer arrays."""
    x, B, F, E, x_stride, x_offset = _x_in_place(op, x, int(fields), int(dim), x_offset)
    D, L = F * E, len(dnn_kernels)
    t = _C.edcn.TrainArgs()
    t.fwd = _edcn_args(B, F, E, L, bridge_type, parameterization, tau, activation, bridge_activation, None, x_stride, x_offset)
    if not (len(gates) == 2 * L and len(cross_kernels) == len(cross_biases) == len(dnn_biases) == L):
        raise ValueError("%s: %d rounds take %d gates and %d of every other weight" % (op, L, 2 * L, L))
    for k, g in enumerate(gates):
        _vec(op, "gates[%d]" % k, g, F)
    for i in range(L):
        _vec(op, "cross_kernels[%d]" % i, cross_kernels[i], D if parameterization == "vector" else D * D)
        _vec(op, "cross_biases[%d]" % i, cross_biases[i], D)
        _vec(op, "dnn_kernels[%d]" % i, dnn_kernels[i], D * D)
        _vec(op, "dnn_biases[%d]" % i, dnn_biases[i], D)
    tensors = [x] + list(gates) + list(cross_kernels) + list(cross_biases) + list(dnn_kernels) + list(dnn_biases)
    keep = [_ptr_array(ts) for ts in (gates, cross_kernels, cross_biases, dnn_kernels, dnn_biases)]
    a = t.fwd
    a.x = x.data_ptr()
    a.gates, a.cross_w, a.cross_b, a.dnn_w, a.dnn_b = (ctypes.cast(p, ctypes.c_void_p) for p in keep)
    if bridge_type == "concatenation":
        if bridge_weights is None or len(bridge_weights) != L:
            raise ValueError("%s: bridge_type %r takes bridge_weights per round" % (op, bridge_type))
        for i, bw in enumerate(bridge_weights):
            _vec(op, "bridge_weights[%d] kernel" % i, bw[0], 2 * D * D)
            _vec(op, "bridge_weights[%d] bias" % i, bw[1], D)
            tensors += list(bw)
        keep += [_ptr_array([bw[j] for bw in bridge_weights]) for j in range(2)]
        a.bridge_w, a.bridge_b = (ctypes.cast(p, ctypes.c_void_p) for p in keep[-2:])
    if head_w is not None:
        _vec(op, "head_w", head_w, 3 * D)
        a.head_w = head_w.data_ptr()
        tensors.append(head_w)
    if not _C.lib().dctr_edcn_bwd_supported(ctypes.byref(t)):
        raise ValueError("%s: %d fields of dim %d, %d rounds, bridge %r, activations %r / %r: not what dctr_edcn_bwd takes "
                         "(ops.edcn_bwd_supported)" % (op, F, E, L, bridge_type, activation, bridge_activation))
    return t, x, B, F, E, L, keep, tensors


def edcn_train(x, fields, dim, gates, cross_kernels, cross_biases, dnn_kernels, dnn_biases, bridge_type="hadamard_product",
               parameterization="vector", tau=1.0, activation="relu", bridge_weights=None, bridge_activation="relu", x_offset=0, head_w=None,
               logit=None, out=None, out_offset=0, tape=None):
    """edcn() for training (include/dctr.h: dctr_edcn_train_fwd): the same launch under one more flag, which also writes ``tape``
    [cross_num, B, 3D] = c, h, br of every round (a contiguous float32 tensor, default: a new one).  Operands as edcn(), without bn /
    dice / add / global_bias / sigmoid: what ops.edcn_bwd_supported accepts.  ``logit`` / ``out`` as edcn() (default: the logit with
    head_w, else out); their bits are edcn()'s.  Returns (logit, out, tape)."""
    t, x, B, F, E, L, keep, tensors = _edcn_train_operands("edcn_train", x, fields, dim, gates, cross_kernels, cross_biases, dnn_kernels,
                                                           dnn_biases, bridge_type, parameterization, tau, activation, bridge_weights,
                                                           bridge_activation, x_offset, head_w)
    D = F * E
    if logit is None and out is None:
        logit, out = (True, None) if head_w is not None else (None, True)
    if logit is True:
        logit = torch.empty(B, dtype=torch.float32, device=x.device)
    if out is True:
        out, out_offset = torch.empty(B, 3 * D, dtype=torch.float32, device=x.device), 0
    if logit is not None:
        _vec("edcn_train", "logit", logit, B)
        if head_w is None:
            raise ValueError("edcn_train: a logit needs head_w [3 * fields * dim]")
        t.fwd.logit = logit.data_ptr()
    if out is not None:
        t.fwd.out, t.fwd.out_stride, t.fwd.out_offset = out.data_ptr(), _rows2d("edcn_train", "out", out, B, 3 * D, out_offset), int(out_offset)
    if tape is None:
        tape = torch.empty(L, B, 3 * D, dtype=torch.float32, device=x.device)
    _vec("edcn_train", "tape", tape, L * B * 3 * D)
    t.tape = tape.data_ptr()
    _dev_check(logit, out, tape, *tensors)
    _C.check(_C.lib().dctr_edcn_train_fwd(ctypes.byref(t), _C.stream_ptr()), "dctr_edcn_train_fwd")
    del keep
    return logit, out, tape


def _edcn_grad_list(op, name, want, like, sizes, device):
    """A per-round gradient output of edcn_bwd: None / False (not wanted), True (allocated here in the shapes of ``like``) or a list
    with a contiguous float32 tensor of ``sizes[i]`` elements, or None, per entry -> (list or None, host pointer array or None)."""
    if want is None or want is False:
        return None, None
    if want is True:
        want = [torch.empty(w.shape, dtype=torch.float32, device=device) for w in like]
    want = list(want)
    if len(want) != len(sizes):
        raise ValueError("%s: %s takes %d entries" % (op, name, len(sizes)))
    for i, g in enumerate(want):
        if g is not None:
            _vec(op, "%s[%d]" % (name, i), g, sizes[i])
    return want, _ptr_array(want)


def edcn_bwd(x, fields, dim, gates, cross_kernels, cross_biases, dnn_kernels, dnn_biases, tape, d_logit=None, d_out=None,
             bridge_type="hadamard_product", parameterization="vector", tau=1.0, activation="relu", bridge_weights=None,
             bridge_activation="relu", x_offset=0, head_w=None, dx=None, dx_offset=0, accumulate=False, d_gates=None, d_cross_w=None,
             d_cross_b=None, d_dnn_w=None, d_dnn_b=None, d_bridge_w=None, d_bridge_b=None, d_head_w=None, slices=0, workspace=None):
    """Backward of edcn_train() (include/dctr.h: dctr_edcn_bwd): x and the live weights as the forward read them, ``tape`` as it wrote
    it; ``d_logit`` [B] (needs head_w) and / or ``d_out`` [B, >= 3D] (unit column stride): the seed of the last round is
    d_out + d_logit * head_w.  Outputs — each None / False (not wanted, skipped) or True (allocated here): ``dx`` a float32 view that
    holds the F*E columns from ``dx_offset`` (_dx_operand; added to with ``accumulate``); ``d_gates`` [2L], ``d_cross_w`` / ``d_cross_b``
    / ``d_dnn_w`` / ``d_dnn_b`` / ``d_bridge_w`` / ``d_bridge_b`` [L]: lists of contiguous float32 tensors (an entry may be None);
    ``d_head_w`` [3D] (True: head_w's shape).  All are OVERWRITTEN.  ``slices``: the batch slices of the weight-gradient pass (0: the library's choice,
    1 .. 256 forces it).  No atomics: bit-identical from call to call.  Returns (dx, d_gates, d_cross_w, d_cross_b, d_dnn_w, d_dnn_b,
    d_bridge_w, d_bridge_b, d_head_w)."""
    t, x, B, F, E, L, keep, tensors = _edcn_train_operands("edcn_bwd", x, fields, dim, gates, cross_kernels, cross_biases, dnn_kernels,
                                                           dnn_biases, bridge_type, parameterization, tau, activation, bridge_weights,
                                                           bridge_activation, x_offset, head_w)
    D, dev = F * E, x.device
    if not 0 <= int(slices) <= 256:
        raise ValueError("edcn_bwd: slices = %d: 0 or 1 .. 256" % int(slices))
    t.slices, t.accumulate = int(slices), int(bool(accumulate))
    if tape is None or tape.dtype != torch.float32 or not tape.is_contiguous() or tape.numel() != L * B * 3 * D:
        raise ValueError("edcn_bwd: tape must be the contiguous float32 [%d, %d, %d] tensor edcn_train wrote" % (L, B, 3 * D))
    t.tape = tape.data_ptr()
    if d_logit is None and d_out is None:
        raise ValueError("edcn_bwd: give d_logit, d_out or both")
    if d_logit is not None:
        if head_w is None:
            raise ValueError("edcn_bwd: d_logit needs head_w [3 * fields * dim]")
        _vec("edcn_bwd", "d_logit", d_logit, B)
        t.d_logit = d_logit.data_ptr()
    if d_out is not None:
        t.d_out, t.d_out_stride = d_out.data_ptr(), _rows2d("edcn_bwd", "d_out", d_out, B, 3 * D)
    if dx is True:
        dx, dx_offset = torch.empty(B, D, dtype=torch.float32, device=dev), 0
        if accumulate:
            dx.zero_()
    elif dx is False:
        dx = None
    if dx is not None:
        t.dx, t.dx_stride, t.dx_offset = dx.data_ptr(), _dx_operand("edcn_bwd", dx, B, F, E, dx_offset), int(dx_offset)
    matrix, concat = parameterization == "matrix", bridge_type == "concatenation"
    if not concat and (d_bridge_w or d_bridge_b):
        raise ValueError("edcn_bwd: d_bridge_w / d_bridge_b exist with the concatenation bridge only")
    bw = [b[0] for b in bridge_weights] if concat else []
    bb = [b[1] for b in bridge_weights] if concat else []
    outs = []
    for name, want, like, size in (("d_gates", d_gates, gates, F), ("d_cross_w", d_cross_w, cross_kernels, D * D if matrix else D),
                                   ("d_cross_b", d_cross_b, cross_biases, D), ("d_dnn_w", d_dnn_w, dnn_kernels, D * D),
                                   ("d_dnn_b", d_dnn_b, dnn_biases, D), ("d_bridge_w", d_bridge_w, bw, 2 * D * D),
                                   ("d_bridge_b", d_bridge_b, bb, D)):
        lst, arr = _edcn_grad_list("edcn_bwd", name, want, like, [size] * len(like), dev)
        outs.append(lst)
        if arr is not None:
            keep.append(arr)
            setattr(t, name, ctypes.cast(arr, ctypes.c_void_p))
            tensors += [g for g in lst if g is not None]
    if d_head_w is True:
        d_head_w = torch.empty(3 * D if head_w is None else tuple(head_w.shape), dtype=torch.float32, device=dev)
    elif d_head_w is False:
        d_head_w = None
    if d_head_w is not None:
        if d_logit is None:
            raise ValueError("edcn_bwd: d_head_w needs d_logit")
        _vec("edcn_bwd", "d_head_w", d_head_w, 3 * D)
        t.d_head_w = d_head_w.data_ptr()
    _dev_check(tape, d_logit, d_out, dx, d_head_w, workspace, *tensors)
    _keep_ws = _workspace("edcn_bwd", t, int(_C.lib().dctr_edcn_bwd_workspace_bytes(ctypes.byref(t))), workspace, dev)
    _C.check(_C.lib().dctr_edcn_bwd(ctypes.byref(t), _C.stream_ptr()), "dctr_edcn_bwd")
    del keep
    return (dx,) + tuple(outs) + (d_head_w,)


class EDCNTowerFunction(torch.autograd.Function):
    """EDCN's tower with its head as one differentiable op (once differentiable): edcn_train() forward with the tape kept, ONE edcn_bwd()
    call backward.  ``apply(x, opts, head_w, *weights)``: x [B,F,d]; ``opts`` = (bridge_type, parameterization, tau, activation,
    bridge_activation); head_w: Dense(1)'s kernel [3D, 1]; ``weights`` = the 2L gates, then L each of the cross kernels, cross biases,
    DNN kernels, DNN biases (, bridge kernels, bridge biases with 'concatenation'), the live tensors in their own shapes.  Returns the
    tower's logit [B] = [c, h, br] . head_w.  Gradients are formed only for the inputs that need them; none leaves through atomics."""

    @staticmethod
    def _split(weights, concat):
        n = len(weights) // (8 if concat else 6)
        if n < 1 or len(weights) != n * (8 if concat else 6):
            raise ValueError("EDCNTowerFunction: %d weights: 2L gates and L of each other kind" % len(weights))
        parts = [list(weights[:2 * n])] + [list(weights[(2 + j) * n:(3 + j) * n]) for j in range(6 if concat else 4)]
        return n, parts

    @staticmethod
    def forward(ctx, x, opts, head_w, *weights):
        ctx.set_materialize_grads(False)
        bridge_type, parameterization, tau, activation, bridge_activation = opts
        if x.dim() != 3:
            raise ValueError("EDCNTowerFunction: x must be [B,F,d]")
        B, F, d = x.shape
        x2 = _f32c(x.detach(), "x").view(B, F * d)
        ws = [_f32c(w.detach(), "weight") for w in weights]
        hw = _f32c(head_w.detach(), "head_w")
        concat = bridge_type == "concatenation"
        L, parts = EDCNTowerFunction._split(ws, concat)
        bw = list(zip(parts[5], parts[6])) if concat else None
        logit, _, tape = edcn_train(x2, F, d, parts[0], parts[1], parts[2], parts[3], parts[4], bridge_type, parameterization, tau,
                                    activation, bw, bridge_activation, head_w=hw, logit=True)
        ctx.opts, ctx.shape, ctx.n_w = opts, (B, F, d), len(ws)
        ctx.save_for_backward(x2, tape, hw, *ws)
        return logit

    @staticmethod
    def backward(ctx, d_logit):
        n = 3 + ctx.n_w
        if d_logit is None:
            return (None,) * n
        bridge_type, parameterization, tau, activation, bridge_activation = ctx.opts
        B, F, d = ctx.shape
        saved = list(ctx.saved_tensors)
        x2, tape, hw, ws = saved[0], saved[1], saved[2], saved[3:]
        concat = bridge_type == "concatenation"
        L, parts = EDCNTowerFunction._split(ws, concat)
        need = ctx.needs_input_grad
        _, views = _zeroed_grads(ws, [bool(v) for v in need[3:]], x2.device)
        _, gparts = EDCNTowerFunction._split(views, concat)
        wanted = [g if any(v is not None for v in g) else None for g in gparts]
        bw = list(zip(parts[5], parts[6])) if concat else None
        res = edcn_bwd(x2, F, d, parts[0], parts[1], parts[2], parts[3], parts[4], tape, d_logit=_grad_operand(d_logit, False),
                       bridge_type=bridge_type, parameterization=parameterization, tau=tau, activation=activation, bridge_weights=bw,
                       bridge_activation=bridge_activation, head_w=hw, dx=bool(need[0]), d_gates=wanted[0], d_cross_w=wanted[1],
                       d_cross_b=wanted[2], d_dnn_w=wanted[3], d_dnn_b=wanted[4], d_bridge_w=wanted[5] if concat else None,
                       d_bridge_b=wanted[6] if concat else None, d_head_w=bool(need[2]))
        dx, d_head = res[0], res[8]
        return (None if dx is None else dx.view(B, F, d), None, None if d_head is None else d_head.view(hw.shape)) + tuple(views)


_MTL_ROUTES = {None: _C.mtl.ROUTE_AUTO, "auto": _C.mtl.ROUTE_AUTO, "layered": _C.mtl.ROUTE_LAYERED}
_MTL_ROUTE_NAMES = {_C.mtl.ROUTE_FUSED: "fused", _C.mtl.ROUTE_LAYERED: "layered"}
_MTL_MEMBERS = {}               # (device, members) -> int32 device copy of a gate-member list (dctr_mtl_mix reads it on the device)


def _i64_array(vals):
    arr = (ctypes.c_int64 * max(1, len(vals)))()
    for i, v in enumerate(vals):
        arr[i] = int(v)
    return arr


def _mtl_options(op, activation, route):
    if route not in _MTL_ROUTES:
        raise ValueError("%s: route %r: expected None, 'auto' or 'layered'" % (op, route))
    if activation not in _C.ACT_CODES:
        raise ValueError("%s: unknown activation %r" % (op, activation))


def _mtl_args(op, kind, batch, x_stride, x_offsets, in_dim, units, expert_src, activation, route, gate_units=(), gate_src=(), members=(),
              esmm=False, tile_rows=0):
    """The host side of dctr_mtl_args_t (sizes, slots, member lists): what dctr_mtl_route reads.  Returns (args, keep-alive)."""
    _mtl_options(op, activation, route)
    members = [[int(m) for m in ms] for ms in members]
    keep = [_i64_array(x_offsets), _i32_array(units), _i32_array(expert_src), _i32_array(gate_units), _i32_array(gate_src),
            _i32_array([len(ms) for ms in members]), _i32_array([m for ms in members for m in ms])]
    cast = lambda p: ctypes.cast(p, ctypes.c_void_p)       # noqa: E731
    a = _C.mtl.Args(batch=int(batch), x_stride=int(x_stride), x_offsets=cast(keep[0]), n_slots=len(x_offsets), in_dim=int(in_dim),
                    n_experts=len(expert_src), n_layers=len(units), units=cast(keep[1]), expert_src=cast(keep[2]),
                    activation=_C.ACT_CODES[activation], route=_MTL_ROUTES[route], n_gates=len(members), n_gate_layers=len(gate_units),
                    gate_units=cast(keep[3]), gate_src=cast(keep[4]), gate_n=cast(keep[5]), members=cast(keep[6]), esmm=int(bool(esmm)),
                    tile_rows=int(tile_rows))
    return a, keep


def mtl_route(in_dim, units, n_experts, members=None, gate_units=(), n_slots=1, expert_src=None, gate_src=None, activation="relu",
              towers=False, esmm=False, route=None):
    """The route ops.mtl_level (``towers=False``: ``members`` = the gates' expert lists) or ops.mtl_towers (``towers=True``: n_experts
    towers) takes for these shapes: 'fused' (one launch, everything in LDS) or 'layered' — the library's answer (dctr_mtl_route)."""
    expert_src = [0] * int(n_experts) if expert_src is None else list(expert_src)
    members = [] if towers else list(members)
    gate_src = [0] * len(members) if gate_src is None else list(gate_src)
    a, _keep = _mtl_args("mtl_route", _C.mtl.TOWERS if towers else _C.mtl.LEVEL, 0, int(in_dim), [0] * int(n_slots), in_dim, list(units),
                         expert_src, activation, route, list(gate_units), gate_src, members, esmm)
    return _route_name("dctr_mtl_route", _C.lib().dctr_mtl_route(ctypes.byref(a), _C.mtl.TOWERS if towers else _C.mtl.LEVEL),
                       _MTL_ROUTE_NAMES)


def _mtl_dnns(op, what, kernels, biases, bn, dice, activation, in_dim, units, flat):
    """Checks n DNNs of the same ``units`` over ``in_dim`` columns; returns (bn, dice) with None for 'absent everywhere'."""
    n, L = len(kernels), len(units)
    if len(biases) != n or (bn is not None and len(bn) != n):
        raise ValueError("%s: %s: one list of kernels, biases (and bn) per DNN" % (op, what))
    for i in range(n):
        if len(kernels[i]) != L or len(biases[i]) != L:
            raise ValueError("%s: %s %d: %d layers expected" % (op, what, i, L))
        k = in_dim
        for l in range(L):
            _vec(op, "%s %d kernel%d" % (what, i, l), kernels[i][l], k * units[l])
            _vec(op, "%s %d bias%d" % (what, i, l), biases[i][l], units[l])
            k = units[l]
        flat += list(kernels[i]) + list(biases[i])
        if bn is not None and bn[i] is not None:
            if len(bn[i]) != L:
                raise ValueError("%s: %s %d: bn holds one entry (None or (scale, shift)) per layer" % (op, what, i))
            for l, sb in enumerate(bn[i]):
                if sb is not None:
                    _vec(op, "%s %d bn scale%d" % (what, i, l), sb[0], units[l])
                    _vec(op, "%s %d bn shift%d" % (what, i, l), sb[1], units[l])
                    flat += list(sb)
    if bn is not None and all(b is None or all(sb is None for sb in b) for b in bn):
        bn = None
    if activation in ("dice", "Dice") and L:
        if dice is None or len(dice) != n or any(len(d) != L for d in dice):
            raise ValueError("%s: %s: activation 'dice' takes [(alpha, moving_mean, moving_variance)] per layer and DNN" % (op, what))
        for d in dice:
            for dp in d:
                flat += list(dp)
    else:
        dice = None
    return bn, dice


def _mtl_dnn_ptrs(kernels, biases, bn):
    """HOST arrays [n * L] of the device pointers (w, b, bn_scale, bn_shift; the last two None without bn)."""
    w = _ptr_array([k for ks in kernels for k in ks])
    b = _ptr_array([t for bs in biases for t in bs])
    if bn is None:
        return w, b, None, None
    per_layer = [None if bl is None else bl[l] for ks, bl in zip(kernels, bn) for l in range(len(ks))]
    return (w, b, _ptr_array([None if sb is None else sb[0] for sb in per_layer]),
            _ptr_array([None if sb is None else sb[1] for sb in per_layer]))


def mtl_mix(h, n_experts, width, z, gate_kernels, members, out=None, out_offset=0):
    """The gated mixtures of the layered route (dctr_mtl_mix).  h: float32 [B, >= n_experts * width] view, expert e in columns
    [e * width, + width); z: per gate a float32 [B, >= dz] view (the gate's input rows); gate_kernels[g] [dz, n_g]; members[g]: the n_g
    expert indices the gate mixes.  out: float32 2-D view, columns [out_offset + g * width, + width) written (default: new [B, G * width]).
    One launch for up to eight gates; any shape."""
    op = "mtl_mix"
    E, H, G = int(n_experts), int(width), len(gate_kernels)
    if h.dim() != 2:
        raise ValueError("mtl_mix: h must be a float32 [B, >= n_experts * width] view with unit column stride")
    B = h.shape[0]
    h_stride = _rows2d(op, "h", h, B, E * H)
    if not (G >= 1 and len(z) == G and len(members) == G):
        raise ValueError("mtl_mix: one input, kernel and member list per gate")
    dz = int(gate_kernels[0].shape[0])
    members = [[int(m) for m in ms] for ms in members]
    z_strides = []
    for g in range(G):
        if not members[g]:
            raise ValueError("mtl_mix: gate %d mixes no expert" % g)
        if any(m < 0 or m >= E for m in members[g]):
            raise ValueError("mtl_mix: gate %d: members %s with %d experts" % (g, members[g], E))
        if gate_kernels[g].dim() != 2 or gate_kernels[g].shape[0] != dz:
            raise ValueError("mtl_mix: gate_kernels[%d] must be [%d, n_g]" % (g, dz))
        _vec(op, "gate_kernels[%d]" % g, gate_kernels[g], dz * len(members[g]))
        z_strides.append(_rows2d(op, "z[%d]" % g, z[g], B, dz))
    if out is None:
        out, out_offset = torch.empty(B, G * H, dtype=torch.float32, device=h.device), 0
    out_stride = _rows2d(op, "out", out, B, G * H, out_offset)
    _dev_check(h, out, *(list(z) + list(gate_kernels)))
    mdev = _mtl_members_dev(h.device, members)
    keep = [_ptr_array(list(z)), _i64_array(z_strides), _ptr_array(list(gate_kernels)), _i32_array([len(ms) for ms in members]),
            _i32_array([m for ms in members for m in ms])]
    cast = lambda p: ctypes.cast(p, ctypes.c_void_p)       # noqa: E731
    a = _C.mtl.MixArgs(batch=B, h=h.data_ptr(), h_stride=h_stride, n_experts=E, width=H, n_gates=G, z_dim=dz, z=cast(keep[0]),
                       z_stride=cast(keep[1]), gate_kernel=cast(keep[2]), gate_n=cast(keep[3]), members=cast(keep[4]),
                       members_dev=mdev.data_ptr(), out=out.data_ptr(), out_stride=out_stride, out_offset=int(out_offset))
    _C.check(_C.lib().dctr_mtl_mix(ctypes.byref(a), _C.stream_ptr()), "dctr_mtl_mix")
    return out


def _mtl_members_dev(device, members):
    key = (device, tuple(tuple(ms) for ms in members))
    mdev = _MTL_MEMBERS.get(key)
    if mdev is None:
        if len(_MTL_MEMBERS) >= 64:
            _MTL_MEMBERS.clear()
        mdev = _MTL_MEMBERS[key] = torch.tensor([m for ms in members for m in ms], dtype=torch.int32).to(device)
    return mdev


def mtl_mix_bwd(h, n_experts, width, z, gate_kernels, members, d_out, dh, ds, d_out_offset=0, logits=None):
    """Backward of mtl_mix (dctr_mtl_mix_bwd); h, z, gate_kernels, members as the forward took them, nothing saved by it.  d_out: float32
    2-D view, gate g's gradient in columns [d_out_offset + g * width, + width).  Written: dh [B, >= n_experts * width] (expert e's
    gradient in columns [e * width, + width), summed over the gates in order; zeros for an expert no gate mixes), ds [B, >= sum n_g]
    (d loss / d gate logits, gate g from column sum_{g' < g} n_g') and, when given, logits [B, >= sum n_g] (the gate logits themselves).
    The gates' weight gradient and dz are a bias-free linear layer's: ops.mlp_bwd(z_g, dz, [Wg_g], [logits_g], "linear", ...,
    d_out=ds_g)."""
    op = "mtl_mix_bwd"
    E, H, G = int(n_experts), int(width), len(gate_kernels)
    if h.dim() != 2:
        raise ValueError("mtl_mix_bwd: h must be a float32 [B, >= n_experts * width] view with unit column stride")
    B = h.shape[0]
    h_stride = _rows2d(op, "h", h, B, E * H)
    if not (G >= 1 and len(z) == G and len(members) == G):
        raise ValueError("mtl_mix_bwd: one input, kernel and member list per gate")
    dz = int(gate_kernels[0].shape[0])
    members = [[int(m) for m in ms] for ms in members]
    z_strides = []
    for g in range(G):
        if not members[g]:
            raise ValueError("mtl_mix_bwd: gate %d mixes no expert" % g)
        if any(m < 0 or m >= E for m in members[g]):
            raise ValueError("mtl_mix_bwd: gate %d: members %s with %d experts" % (g, members[g], E))
        if gate_kernels[g].dim() != 2 or gate_kernels[g].shape[0] != dz:
            raise ValueError("mtl_mix_bwd: gate_kernels[%d] must be [%d, n_g]" % (g, dz))
        _vec(op, "gate_kernels[%d]" % g, gate_kernels[g], dz * len(members[g]))
        z_strides.append(_rows2d(op, "z[%d]" % g, z[g], B, dz))
    n_all = sum(len(ms) for ms in members)
    d_out_stride = _rows2d(op, "d_out", d_out, B, G * H, int(d_out_offset))
    dh_stride = _rows2d(op, "dh", dh, B, E * H)
    ds_stride = _rows2d(op, "ds", ds, B, n_all)
    lg_stride = 0 if logits is None else _rows2d(op, "logits", logits, B, n_all)
    _dev_check(h, d_out, dh, ds, logits, *(list(z) + list(gate_kernels)))
    mdev = _mtl_members_dev(h.device, members)
    keep = [_ptr_array(list(z)), _i64_array(z_strides), _ptr_array(list(gate_kernels)), _i32_array([len(ms) for ms in members]),
            _i32_array([m for ms in members for m in ms])]
    cast = lambda p: ctypes.cast(p, ctypes.c_void_p)       # noqa: E731
    a = _C.mtl.MixBwdArgs(batch=B, h=h.data_ptr(), h_stride=h_stride, n_experts=E, width=H, n_gates=G, z_dim=dz, z=cast(keep[0]),
                          z_stride=cast(keep[1]), gate_kernel=cast(keep[2]), gate_n=cast(keep[3]), members=cast(keep[4]),
                          members_dev=mdev.data_ptr(), d_out=d_out.data_ptr(), d_out_stride=d_out_stride, d_out_offset=int(d_out_offset),
                          dh=dh.data_ptr(), dh_stride=dh_stride, ds=ds.data_ptr(), ds_stride=ds_stride,
                          logits=None if logits is None else logits.data_ptr(), logits_stride=lg_stride)
    _C.check(_C.lib().dctr_mtl_mix_bwd(ctypes.byref(a), _C.stream_ptr()), "dctr_mtl_mix_bwd")
    return dh, ds


_MTL_LOSS_KINDS = {"binary_crossentropy": _C.mtl.LOSS_BCE, "logloss": _C.mtl.LOSS_BCE, "bce": _C.mtl.LOSS_BCE, "mse": _C.mtl.LOSS_MSE,
                   "mean_squared_error": _C.mtl.LOSS_MSE}


def _f32_array(vals):
    arr = (ctypes.c_float * max(1, len(vals)))()
    for i, v in enumerate(vals):
        arr[i] = float(v)
    return arr


def mtl_loss_grad(pred, y, dlogit, loss_sum, losses, binary, loss_weights=None, esmm=False, dbias=None):
    """The multi-task loss gradient (dctr_mtl_loss_grad).  pred, y, dlogit: float32 [T, B] with unit column stride; pred[t] = the tower's
    output (sigmoid applied where binary[t]; with ``esmm`` row 1 is sigmoid(l_cvr), not the product).  losses[t]: 'binary_crossentropy' |
    'mse' (binary + BCE and regression + MSE only).  dlogit = d(sum_t w_t mean_b loss_t) / d logit_t is written; loss_sum (float32 [T],
    contiguous) and the device scalars dbias[t] (None to skip one) are ADDED to: the tasks' summed reported losses and sum_b dlogit[t]."""
    op = "mtl_loss_grad"
    T = len(losses)
    if T < 1 or pred.dim() != 2 or pred.shape[0] != T:
        raise ValueError("mtl_loss_grad: pred must be a float32 [T, B] view with one row per loss")
    B = pred.shape[1]
    binary = [bool(b) for b in binary]
    weights = [1.0] * T if loss_weights is None else [float(w) for w in loss_weights]
    if len(binary) != T or len(weights) != T or (dbias is not None and len(dbias) != T):
        raise ValueError("mtl_loss_grad: one task type, loss weight (and bias gradient) per task")
    kinds = []
    for t, name in enumerate(losses):
        if not isinstance(name, str) or name.lower() not in _MTL_LOSS_KINDS:
            raise ValueError("mtl_loss_grad: unknown loss %r (binary_crossentropy, mse)" % (name,))
        kinds.append(_MTL_LOSS_KINDS[name.lower()])
        if binary[t] != (kinds[t] == _C.mtl.LOSS_BCE):
            raise ValueError("mtl_loss_grad: task %d: %s on a %s output (binary + binary_crossentropy or regression + mse)"
                             % (t, name, "binary" if binary[t] else "regression"))
    if esmm and not (T == 2 and all(binary)):
        raise ValueError("mtl_loss_grad: esmm takes two binary tasks")
    strides = [_rows2d(op, name, t_, T, B) if T > 1 else max(_rows2d(op, name, t_, T, B), B)
               for name, t_ in (("pred", pred), ("y", y), ("dlogit", dlogit))]
    _vec(op, "loss_sum", loss_sum, T)
    for b_ in dbias or []:
        if b_ is not None:
            _vec(op, "dbias entry", b_, 1)
    _dev_check(pred, y, dlogit, loss_sum, *(dbias or []))
    keep = [_i32_array(kinds), _i32_array([int(b) for b in binary]), _f32_array(weights), None if dbias is None else _ptr_array(list(dbias))]
    cast = lambda p: None if p is None else ctypes.cast(p, ctypes.c_void_p)       # noqa: E731
    a = _C.mtl.LossArgs(batch=B, n_tasks=T, esmm=int(bool(esmm)), pred=pred.data_ptr(), pred_stride=strides[0], y=y.data_ptr(),
                        y_stride=strides[1], loss_kind=cast(keep[0]), binary=cast(keep[1]), loss_weight=cast(keep[2]),
                        dlogit=dlogit.data_ptr(), dlogit_stride=strides[2], loss_sum=loss_sum.data_ptr(), dbias=cast(keep[3]))
    _C.check(_C.lib().dctr_mtl_loss_grad(ctypes.byref(a), _C.stream_ptr()), "dctr_mtl_loss_grad")
    return dlogit


def mtl_sum_slots(srcs, n, dst, dst_offset=0, accumulate=False):
    """dst[:, dst_offset : dst_offset + n] = (``accumulate``: +=) srcs[0][:, :n] + srcs[1][:, :n] + ..., summed in that order
    (dctr_mtl_sum_slots).  srcs: 1 .. 16 float32 [B, >= n] views with unit column stride, each with its own row stride.  The gradient of
    a slot that several DNNs read: ops.mlp_bwd writes its dx, so each reader writes to scratch and this launch forms the sum."""
    op = "mtl_sum_slots"
    srcs, n = list(srcs), int(n)
    if not 1 <= len(srcs) <= 16:
        raise ValueError("mtl_sum_slots: 1 .. 16 sources (%d given)" % len(srcs))
    if dst.dim() != 2 or n < 1:
        raise ValueError("mtl_sum_slots: dst must be a float32 2-D view with unit column stride, n >= 1")
    B = dst.shape[0]
    dst_stride = _rows2d(op, "dst", dst, B, n, int(dst_offset))
    strides = [_rows2d(op, "srcs[%d]" % k, s, B, n) for k, s in enumerate(srcs)]
    _dev_check(dst, *srcs)
    keep = [_ptr_array(srcs), _i64_array(strides)]
    _C.check(_C.lib().dctr_mtl_sum_slots(ctypes.cast(keep[0], ctypes.c_void_p), ctypes.cast(keep[1], ctypes.c_void_p), len(srcs), B, n,
                                         dst.data_ptr(), dst_stride, int(dst_offset), int(bool(accumulate)), _C.stream_ptr()),
             "dctr_mtl_sum_slots")
    return dst


def mtl_level(x, in_dim, x_offsets, expert_kernels, expert_biases, gate_kernels, members, expert_src=None, gate_src=None,
              activation="relu", expert_bn=None, expert_dice=None, gate_dnn_kernels=None, gate_dnn_biases=None, gate_bn=None, gate_dice=None,
              out=None, out_offset=0, route=None, tile_rows=0):
    """One expert / gate level of MMOE or PLE (reference mmoe.py:63-84, ple.py:65-133; include/dctr.h: dctr_mtl_level_fwd).
    x: a float32 [B, stride] buffer; slot s = the ``in_dim`` columns from ``x_offsets[s]``, read in place.  ``expert_kernels[e]`` /
    ``expert_biases[e]``: the L layers of expert e (the same units for every expert) over slot ``expert_src[e]`` (default 0);
    ``gate_kernels[g]`` [dz, n_g] over the gate's input — slot ``gate_src[g]``, or the output of the gate's DNN
    (``gate_dnn_kernels[g]`` / ``gate_dnn_biases[g]``, the same units for every gate); ``members[g]``: the n_g experts gate g mixes.
    ``*_bn[i][l]``: None or (scale, shift); ``*_dice[i][l]``: (alpha, moving_mean, moving_variance) with activation 'dice'.  All weights
    are the live tensors.  Returns out: columns [out_offset + g * H, + H) of a float32 2-D view (default: a new [B, G * H]) hold
    sum_j softmax(z_g Wg_g)[j] * h_{members[g][j]}.  One launch where ops.mtl_route says 'fused', else layer by layer."""
    op = "mtl_level"
    _mtl_options(op, activation, route)
    in_dim, x_offsets = int(in_dim), [int(o) for o in x_offsets]
    E, G = len(expert_kernels), len(gate_kernels)
    if E < 1 or G < 1 or not x_offsets or not expert_kernels[0]:
        raise ValueError("mtl_level: at least one slot, one expert of one layer and one gate")
    if x.dim() != 2:
        raise ValueError("mtl_level: x must be a float32 [B, stride] view with unit column stride")
    B = x.shape[0]
    if min(x_offsets) < 0:
        raise ValueError("mtl_level: negative slot offset")
    x_stride = _rows2d(op, "x", x, B, max(x_offsets) + in_dim)
    units = [int(k.shape[1]) for k in expert_kernels[0]]
    expert_src = [0] * E if expert_src is None else [int(s) for s in expert_src]
    gate_src = [0] * G if gate_src is None else [int(s) for s in gate_src]
    if len(expert_src) != E or len(gate_src) != G or len(members) != G:
        raise ValueError("mtl_level: one source slot per expert and gate, one member list per gate")
    if any(s < 0 or s >= len(x_offsets) for s in expert_src + gate_src):
        raise ValueError("mtl_level: source slots %s / %s with %d slots" % (expert_src, gate_src, len(x_offsets)))
    members = [[int(m) for m in ms] for ms in members]
    for g, ms in enumerate(members):
        if not ms:
            raise ValueError("mtl_level: gate %d mixes no expert" % g)
        if any(m < 0 or m >= E for m in ms):
            raise ValueError("mtl_level: gate %d: members %s with %d experts" % (g, ms, E))
    flat = []
    expert_bn, expert_dice = _mtl_dnns(op, "expert", expert_kernels, expert_biases, expert_bn, expert_dice, activation, in_dim, units, flat)
    gate_units = []
    if gate_dnn_kernels is not None and len(gate_dnn_kernels) and len(gate_dnn_kernels[0]):
        if len(gate_dnn_kernels) != G:
            raise ValueError("mtl_level: one gate DNN per gate")
        gate_units = [int(k.shape[1]) for k in gate_dnn_kernels[0]]
        gate_bn, gate_dice = _mtl_dnns(op, "gate DNN", gate_dnn_kernels, gate_dnn_biases, gate_bn, gate_dice, activation, in_dim, gate_units,
                                       flat)
    else:
        gate_dnn_kernels = gate_dnn_biases = gate_bn = gate_dice = None
    dz, H = (gate_units[-1] if gate_units else in_dim), units[-1]
    for g in range(G):
        _vec(op, "gate_kernels[%d]" % g, gate_kernels[g], dz * len(members[g]))
    if out is None:
        out, out_offset = torch.empty(B, G * H, dtype=torch.float32, device=x.device), 0
    out_stride = _rows2d(op, "out", out, B, G * H, out_offset)
    _dev_check(x, out, *(flat + list(gate_kernels)))
    a, keep = _mtl_args(op, _C.mtl.LEVEL, B, x_stride, x_offsets, in_dim, units, expert_src, activation, route, gate_units, gate_src, members,
                        tile_rows=tile_rows)
    lib = _C.lib()
    if _route_name("dctr_mtl_route", lib.dctr_mtl_route(ctypes.byref(a), _C.mtl.LEVEL), _MTL_ROUTE_NAMES) == "layered":
        slot = lambda s: x[:, x_offsets[s]:x_offsets[s] + in_dim]      # noqa: E731
        hbuf = torch.empty(B, E * H, dtype=torch.float32, device=x.device)
        for e in range(E):
            mlp(slot(expert_src[e]), list(expert_kernels[e]), list(expert_biases[e]), activation, dice=None if expert_dice is None else expert_dice[e],
                bn=None if expert_bn is None else expert_bn[e], in_dim=in_dim, out=hbuf[:, e * H:(e + 1) * H])
        zs = []
        for g in range(G):
            if gate_units:
                zs.append(mlp(slot(gate_src[g]), list(gate_dnn_kernels[g]), list(gate_dnn_biases[g]), activation,
                              dice=None if gate_dice is None else gate_dice[g], bn=None if gate_bn is None else gate_bn[g], in_dim=in_dim))
            else:
                zs.append(slot(gate_src[g]))
        return mtl_mix(hbuf, E, H, zs, gate_kernels, members, out=out, out_offset=out_offset)
    cast = lambda p: None if p is None else ctypes.cast(p, ctypes.c_void_p)       # noqa: E731
    ptrs = list(_mtl_dnn_ptrs(expert_kernels, expert_biases, expert_bn))
    a.x = x.data_ptr()
    a.expert_w, a.expert_b, a.expert_bn_scale, a.expert_bn_shift = (cast(p) for p in ptrs)
    if gate_units:
        gp = list(_mtl_dnn_ptrs(gate_dnn_kernels, gate_dnn_biases, gate_bn))
        a.gate_w, a.gate_b, a.gate_bn_scale, a.gate_bn_shift = (cast(p) for p in gp)
        ptrs += gp
    gk = _ptr_array(list(gate_kernels))
    a.gate_kernel = cast(gk)
    a.out, a.out_stride, a.out_offset = out.data_ptr(), out_stride, int(out_offset)
    _C.check(lib.dctr_mtl_level_fwd(ctypes.byref(a), _C.stream_ptr()), "dctr_mtl_level_fwd")
    del keep, ptrs, gk
    return out


def mtl_towers(x, in_dim, x_offsets, kernels, biases, head_ws, global_biases=None, binary=None, activation="relu", bn=None, dice=None,
               esmm=False, out=None, route=None, tile_rows=0):
    """All task towers (reference mmoe.py:86-94, esmm.py:52-63; include/dctr.h: dctr_mtl_towers_fwd).  Tower t reads the ``in_dim``
    columns from ``x_offsets[t]`` of the float32 [B, stride] buffer x in place: DNN ``kernels[t]`` / ``biases[t]`` (possibly no layer,
    the same units for every tower), . ``head_ws[t]``, + ``global_biases[t]``, the sigmoid where ``binary[t]``.  ``esmm``: two binary
    towers, out[1] = sigmoid(l_0) * sigmoid(l_1).  Returns out, float32 [T, B] (contiguous rows).  One launch where ops.mtl_route says
    'fused', else one ops.mlp call per tower."""
    op = "mtl_towers"
    _mtl_options(op, activation, route)
    in_dim, x_offsets = int(in_dim), [int(o) for o in x_offsets]
    T = len(head_ws)
    if T < 1 or len(x_offsets) != T or len(kernels) != T:
        raise ValueError("mtl_towers: one slot offset, DNN and head per tower")
    if x.dim() != 2:
        raise ValueError("mtl_towers: x must be a float32 [B, stride] view with unit column stride")
    B = x.shape[0]
    if min(x_offsets) < 0:
        raise ValueError("mtl_towers: negative slot offset")
    x_stride = _rows2d(op, "x", x, B, max(x_offsets) + in_dim)
    units = [int(k.shape[1]) for k in kernels[0]]
    binary = [True] * T if binary is None else [bool(b) for b in binary]
    if len(binary) != T or (global_biases is not None and len(global_biases) != T):
        raise ValueError("mtl_towers: one task type (and bias) per tower")
    if esmm and not (T == 2 and all(binary)):
        raise ValueError("mtl_towers: esmm takes two binary towers")
    flat = []
    bn, dice = _mtl_dnns(op, "tower", kernels, biases, bn, dice, activation, in_dim, units, flat)
    last = units[-1] if units else in_dim
    for t in range(T):
        _vec(op, "head_ws[%d]" % t, head_ws[t], last)
        if global_biases is not None and global_biases[t] is not None:
            _vec(op, "global_biases[%d]" % t, global_biases[t], 1)
    if out is None:
        out = torch.empty(T, B, dtype=torch.float32, device=x.device)
    if out.dim() != 2 or out.shape[0] != T or out.shape[1] != B or out.dtype != torch.float32 or (B > 1 and out.stride(1) != 1):
        raise ValueError("mtl_towers: out must be a float32 [%d, %d] tensor with unit column stride" % (T, B))
    _dev_check(x, out, *(flat + list(head_ws) + [g for g in (global_biases or []) if g is not None]))
    a, keep = _mtl_args(op, _C.mtl.TOWERS, B, x_stride, x_offsets, in_dim, units, list(range(T)), activation, route, esmm=esmm,
                        tile_rows=tile_rows)
    lib = _C.lib()
    gb = [None] * T if global_biases is None else list(global_biases)
    if _route_name("dctr_mtl_route", lib.dctr_mtl_route(ctypes.byref(a), _C.mtl.TOWERS), _MTL_ROUTE_NAMES) == "layered":
        cvr = torch.empty(B, dtype=torch.float32, device=x.device) if esmm else None
        for t in range(T):
            mlp(x[:, x_offsets[t]:x_offsets[t] + in_dim], list(kernels[t]), list(biases[t]), activation if units else "linear",
                dice=None if dice is None else dice[t], bn=None if bn is None else bn[t], head_w=head_ws[t], global_bias=gb[t],
                sigmoid_out=binary[t], in_dim=in_dim, out=cvr if (esmm and t == 1) else out[t])
        if esmm:
            edcn_bridge(out[0].reshape(B, 1), cvr.reshape(B, 1), "hadamard_product", out=out[1].reshape(B, 1))
        return out
    cast = lambda p: None if p is None else ctypes.cast(p, ctypes.c_void_p)       # noqa: E731
    ptrs = list(_mtl_dnn_ptrs(kernels, biases, bn))
    a.x = x.data_ptr()
    a.expert_w, a.expert_b, a.expert_bn_scale, a.expert_bn_shift = (cast(p) for p in ptrs)
    ptrs += [_ptr_array(list(head_ws)), _ptr_array(gb), _i32_array([int(b) for b in binary])]
    a.head_w, a.global_bias, a.binary = (cast(p) for p in ptrs[-3:])
    a.probs, a.probs_stride = out.data_ptr(), (int(out.stride(0)) if T > 1 else max(int(out.stride(0)), B))
    _C.check(lib.dctr_mtl_towers_fwd(ctypes.byref(a), _C.stream_ptr()), "dctr_mtl_towers_fwd")
    del keep, ptrs
    return out


_TRANSFORMER_ROUTES = {None: _C.transformer.ROUTE_AUTO, "auto": _C.transformer.ROUTE_AUTO, "fused": _C.transformer.ROUTE_FUSED,
                       "general": _C.transformer.ROUTE_GENERAL}
TRANSFORMER_WEIGHTS = ("query", "key", "value", "fw1", "fw2", "ln_gamma", "ln_beta", "pe_q", "pe_k")


def transformer_flops(T, E, n_layers=1, use_feed_forward=True):
    """FLOP per sample of the Transformer stack: 6 T E^2 projections + 4 T^2 E attention + 16 T E^2 feed-forward per layer."""
    return int(n_layers) * (6 * T * E * E + 4 * T * T * E + (16 * T * E * E if use_feed_forward else 0))


def _seq3d(op, name, t, B, T, E):
    """``t`` is a float32 [B, T, E] view with unit stride on the last axis; returns its (sample, position) strides in elements (the
    stride torch reports for a size-1 axis is arbitrary: such an axis gets the extent of what it holds)."""
    if t.dim() != 3 or t.dtype != torch.float32 or tuple(t.shape) != (B, T, E) or (E > 1 and t.stride(2) != 1):
        raise ValueError("%s: %s must be a float32 [%d, %d, %d] view with unit stride on the last axis" % (op, name, B, T, E))
    row = int(t.stride(1)) if T != 1 else max(int(t.stride(1)), E)
    sample = int(t.stride(0)) if B > 1 else max(int(t.stride(0)), (T - 1) * row + E)
    return sample, row


def _transformer_args(B, T, E, head_num, n_layers, use_positional_encoding, use_res, use_feed_forward, use_layer_norm, blinding,
                      output_type, route, ln_eps=1e-9):
    if output_type not in _C.transformer.OUTPUTS:
        raise ValueError("transformer: output_type must be None, 'mean' or 'sum', got %r" % (output_type,))
    if route not in _TRANSFORMER_ROUTES:
        raise ValueError("transformer: route must be None, 'fused' or 'general', got %r" % (route,))
    H = int(head_num)
    if H <= 0:
        raise ValueError("head_num must be a int > 0")
    if E % H:
        raise ValueError("att_embedding_size * head_num must equal the last dimension size of inputs,got %d * %d != %d" % (E // H, H, E))
    return _C.transformer.Args(batch=int(B), q_stride=int(T) * int(E), q_row_stride=int(E), k_stride=int(T) * int(E), k_row_stride=int(E),
                               seq_len=int(T), dim=int(E), att_embedding_size=E // H, head_num=H, n_layers=int(n_layers),
                               use_positional_encoding=int(bool(use_positional_encoding)), use_res=int(bool(use_res)),
                               use_feed_forward=int(bool(use_feed_forward)), use_layer_norm=int(bool(use_layer_norm)),
                               blinding=int(bool(blinding)), output_type=_C.transformer.OUTPUTS[output_type],
                               route=_TRANSFORMER_ROUTES[route], ln_eps=float(ln_eps), out_stride=int(T) * int(E), out_row_stride=int(E))


def transformer_workspace_bytes(batch, seq_len, dim, head_num, n_layers=1, use_positional_encoding=True, use_res=True,
                                use_feed_forward=True, use_layer_norm=False, blinding=True, output_type=None, route=None):
    """Bytes of the workspace dctr_transformer_fwd needs for these shapes (0 on the fused route; read from the library)."""
    a = _transformer_args(batch, seq_len, dim, head_num, n_layers, use_positional_encoding, use_res, use_feed_forward, use_layer_norm,
                          blinding, output_type, route)
    return int(_C.lib().dctr_transformer_workspace_bytes(ctypes.byref(a)))


def transformer_route(seq_len, dim, head_num, n_layers=1, use_positional_encoding=True, use_res=True, use_feed_forward=True,
                      use_layer_norm=False, blinding=True, output_type=None, route=None):
    """'fused' or 'general': the route dctr_transformer_fwd takes for these shapes (dctr_transformer_route)."""
    a = _transformer_args(1, seq_len, dim, head_num, n_layers, use_positional_encoding, use_res, use_feed_forward, use_layer_norm,
                          blinding, output_type, route)
    return _route_name("dctr_transformer_route", _C.lib().dctr_transformer_route(ctypes.byref(a)), (None, "fused", "general"))


def _transformer_mask(op, name, lengths, mask, B, T):
    """One side's mask operands: int32 lengths [B] or a uint8 / bool [B, T] mask, at most one of them."""
    if lengths is not None and mask is not None:
        raise ValueError("%s: give %s_lengths or %s_mask, not both" % (op, name, name))
    if lengths is not None:
        if lengths.dtype != torch.int32 or lengths.numel() != B or not lengths.is_contiguous():
            raise ValueError("%s: %s_lengths must be a contiguous int32 tensor of %d elements" % (op, name, B))
    if mask is not None:
        if mask.dtype == torch.bool:
            mask = mask.view(torch.uint8) if mask.is_contiguous() else mask.to(torch.uint8)
        if mask.dtype != torch.uint8 or tuple(mask.shape) != (B, T) or not mask.is_contiguous():
            raise ValueError("%s: %s_mask must be a contiguous uint8 or bool [%d, %d] tensor" % (op, name, B, T))
    return lengths, mask


def _transformer_operands(op, queries, layers, head_num, keys, query_lengths, key_lengths, query_mask, key_mask,
                          use_positional_encoding, use_res, use_feed_forward, use_layer_norm, blinding, output_type, route, ln_eps):
    """The checked operands transformer(), transformer_train() and transformer_bwd() share: the args struct with sizes, flags and
    the queries' / keys' strides, the flat weight list (None where a flag switches a weight off) and the four mask operands."""
    if queries.dim() != 3:
        raise ValueError("Unexpected inputs dimensions %d, expect to be 3 dimensions" % queries.dim())
    B, T, E = (int(v) for v in queries.shape)
    a = _transformer_args(B, T, E, head_num, len(layers), use_positional_encoding, use_res, use_feed_forward, use_layer_norm, blinding,
                          output_type, route, ln_eps)
    a.q_stride, a.q_row_stride = _seq3d(op, "queries", queries, B, T, E)
    if keys is not None:
        a.k_stride, a.k_row_stride = _seq3d(op, "keys", keys, B, T, E)
    if not layers:
        raise ValueError("%s: at least one layer" % op)
    shapes = {"query": (E, E), "key": (E, E), "value": (E, E), "fw1": (E, 4 * E), "fw2": (4 * E, E), "ln_gamma": (1, E), "ln_beta": (1, E),
              "pe_q": (T, E), "pe_k": (T, E)}
    needed = {"query": True, "key": True, "value": True, "fw1": bool(use_feed_forward and use_res), "fw2": bool(use_feed_forward and use_res),
              "ln_gamma": bool(use_layer_norm), "ln_beta": bool(use_layer_norm), "pe_q": bool(use_positional_encoding),
              "pe_k": bool(use_positional_encoding)}
    flat = []
    for li, layer in enumerate(layers):
        if not isinstance(layer, dict):
            layer = dict(zip(TRANSFORMER_WEIGHTS, layer))
        for name in TRANSFORMER_WEIGHTS:
            w = layer.get(name)
            if w is None or not needed[name]:
                if needed[name]:
                    raise ValueError("%s: layer %d: %s is missing" % (op, li, name))
                flat.append(None)
                continue
            rows, cols = shapes[name]
            if name.startswith("ln_"):
                _vec(op, "layer %d %s" % (li, name), w, cols)
            elif _rows2d(op, "layer %d %s" % (li, name), w, rows, cols) != cols and rows > 1:
                raise ValueError("%s: layer %d: %s must be contiguous" % (op, li, name))
            flat.append(w)
    query_lengths, query_mask = _transformer_mask(op, "query", query_lengths, query_mask, B, T)
    key_lengths, key_mask = _transformer_mask(op, "key", key_lengths, key_mask, B, T)
    return a, flat, (query_lengths, key_lengths, query_mask, key_mask)


def transformer(queries, layers, head_num, keys=None, query_lengths=None, key_lengths=None, query_mask=None, key_mask=None,
                use_positional_encoding=True, use_res=True, use_feed_forward=True, use_layer_norm=False, blinding=True,
                output_type=None, out=None, key_mask_out=None, route=None, workspace=None, ln_eps=1e-9):
    """Transformer.call (reference sequence.py:523-635) stacked over len(layers) layers (bst.py:84-92), one launch.

    ``queries`` [B, T, E] float32 view (any sample / position strides, unit stride on the last axis); ``keys`` the same shape or None
    (the queries).  ``layers``: per layer a dict (or a sequence in this order) of query, key, value [E, E], fw1 [E, 4E], fw2 [4E, E],
    ln_gamma, ln_beta [E], pe_q, pe_k [T, E] — the positional tables ALREADY multiplied by float32(sqrt(E)); weights a flag switches
    off may be None.  Masks: int32 lengths [B] or a uint8 / bool [B, T] mask per side, None = every position counts.
    ``out``: a [B, T, E] view (``output_type`` None; may be ``queries`` itself: in place) or [B, E] ('mean' / 'sum'), allocated when
    None.  ``key_mask_out``: a uint8 [B, T] tensor that receives the key mask.  Returns ``out``."""
    op = "transformer"
    a, flat, (query_lengths, key_lengths, query_mask, key_mask) = _transformer_operands(
        op, queries, layers, head_num, keys, query_lengths, key_lengths, query_mask, key_mask, use_positional_encoding, use_res,
        use_feed_forward, use_layer_norm, blinding, output_type, route, ln_eps)
    B, T, E = int(a.batch), int(a.seq_len), int(a.dim)
    if out is None:
        out = torch.empty((B, T, E) if output_type is None else (B, E), dtype=torch.float32, device=queries.device)
    if output_type is None:
        a.out_stride, a.out_row_stride = _seq3d(op, "out", out, B, T, E)
    else:
        a.out_stride = _rows2d(op, "out", out, B, E)
    if key_mask_out is not None and (key_mask_out.dtype != torch.uint8 or tuple(key_mask_out.shape) != (B, T) or not key_mask_out.is_contiguous()):
        raise ValueError("transformer: key_mask_out must be a contiguous uint8 [%d, %d] tensor" % (B, T))
    _dev_check(queries, keys, out, query_lengths, key_lengths, query_mask, key_mask, key_mask_out, *flat)
    lp = _ptr_array(flat)
    a.layers = ctypes.cast(lp, ctypes.c_void_p)
    a.queries = queries.data_ptr()
    a.keys = None if keys is None else keys.data_ptr()
    a.query_lengths, a.key_lengths = _ptr(query_lengths), _ptr(key_lengths)
    a.query_mask, a.key_mask = _ptr(query_mask), _ptr(key_mask)
    a.out = out.data_ptr()
    a.key_mask_out = _ptr(key_mask_out)
    _workspace(op, a, int(_C.lib().dctr_transformer_workspace_bytes(ctypes.byref(a))), workspace, queries.device)
    _C.check(_C.lib().dctr_transformer_fwd(ctypes.byref(a), _C.stream_ptr()), "dctr_transformer_fwd")
    del lp
    return out


def transformer_bwd_flops(T, E, n_layers=1, use_feed_forward=True):
    """FLOP per sample of dctr_transformer_bwd without its recompute of the forward: Y W^T and X^T dY for every projection (twice the
    forward's matrix FLOP) and the two attention walks, 12 T^2 E (csrc/transformer_bwd_kernels.hip has the model)."""
    return int(n_layers) * (12 * T * E * E + 12 * T * T * E + (32 * T * E * E if use_feed_forward else 0))


def _transformer_train_shape(B, T, E, head_num, n_layers, use_positional_encoding, use_res, use_feed_forward, use_layer_norm, blinding,
                             output_type, route, max_blocks=0):
    t = _C.transformer.TrainArgs()
    t.fwd = _transformer_args(B, T, E, head_num, n_layers, use_positional_encoding, use_res, use_feed_forward, use_layer_norm, blinding,
                              output_type, route)
    t.d_out_stride, t.d_out_row_stride = (int(T) * int(E), int(E)) if output_type is None else (int(E), 0)
    t.dx_stride, t.dx_row_stride = int(T) * int(E), int(E)
    t.max_blocks = int(max_blocks)
    return t


def transformer_tape_bytes(batch, seq_len, dim, head_num, n_layers=1):
    """Bytes of the tape dctr_transformer_train_fwd writes: the inputs of the layers past the first (read from the library)."""
    a = _transformer_args(batch, seq_len, dim, head_num, n_layers, True, True, True, False, True, None, None)
    return int(_C.lib().dctr_transformer_tape_bytes(ctypes.byref(a)))


def transformer_bwd_supported(seq_len, dim, head_num, n_layers=1, use_positional_encoding=True, use_res=True, use_feed_forward=True,
                              use_layer_norm=False, blinding=True, output_type=None, route=None):
    """Does dctr_transformer_bwd (and the training forward whose tape it reads) take these shapes and options (read from the
    library)?  Self-attention is understood: separate keys are never supported."""
    t = _transformer_train_shape(1, seq_len, dim, head_num, n_layers, use_positional_encoding, use_res, use_feed_forward, use_layer_norm,
                                 blinding, output_type, route)
    return bool(_C.lib().dctr_transformer_bwd_supported(ctypes.byref(t)))


def transformer_bwd_workspace_bytes(batch, seq_len, dim, head_num, n_layers=1, use_positional_encoding=True, use_res=True,
                                    use_feed_forward=True, use_layer_norm=False, blinding=True, output_type=None, route=None,
                                    max_blocks=0):
    """Bytes of the workspace dctr_transformer_bwd needs for these shapes (read from the library; 0 for a shape it refuses)."""
    t = _transformer_train_shape(batch, seq_len, dim, head_num, n_layers, use_positional_encoding, use_res, use_feed_forward,
                                 use_layer_norm, blinding, output_type, route, max_blocks)
    return int(_C.lib().dctr_transformer_bwd_workspace_bytes(ctypes.byref(t)))


def _transformer_train_operands(op, x, layers, head_num, keys, tape, query_lengths, key_lengths, query_mask, key_mask,
                                use_positional_encoding, use_res, use_feed_forward, use_layer_norm, blinding, output_type, route, ln_eps):
    """x, the weights, the masks and the tape of transformer_train() / transformer_bwd().  Returns (train args, weights, masks,
    keep-alive)."""
    a, flat, masks = _transformer_operands(op, x, layers, head_num, keys, query_lengths, key_lengths, query_mask, key_mask,
                                           use_positional_encoding, use_res, use_feed_forward, use_layer_norm, blinding, output_type,
                                           route, ln_eps)
    t = _C.transformer.TrainArgs()
    t.fwd = a
    need = (len(layers) - 1) * int(a.batch) * int(a.seq_len) * int(a.dim) * 4
    if need and (tape is None or tape.dtype != torch.float32 or not tape.is_contiguous() or tape.numel() * 4 < need):
        raise ValueError("%s: tape must be a contiguous float32 tensor of >= %d bytes (transformer_train allocates it)" % (op, need))
    lp = _ptr_array(flat)
    t.fwd.layers = ctypes.cast(lp, ctypes.c_void_p)
    t.fwd.queries = x.data_ptr()
    t.fwd.keys = None if keys is None else keys.data_ptr()
    t.fwd.query_lengths, t.fwd.key_lengths, t.fwd.query_mask, t.fwd.key_mask = (_ptr(m) for m in masks)
    if tape is not None:
        t.tape, t.tape_bytes = tape.data_ptr(), tape.numel() * 4
    return t, flat, masks, lp


def transformer_train(x, layers, head_num, query_lengths=None, key_lengths=None, query_mask=None, key_mask=None,
                      use_positional_encoding=True, use_res=True, use_feed_forward=True, use_layer_norm=False, blinding=True,
                      output_type=None, out=None, tape=None, route=None, workspace=None, ln_eps=1e-9):
    """transformer() over self-attention as the forward of a training step (dctr_transformer_train_fwd): the same kernel, so the
    same bits in ``out``, plus a tape.  Returns (out, tape): ``tape`` float32 [len(layers) - 1, B, T, E], the input of every layer
    past the first for transformer_bwd(), allocated when None."""
    op = "transformer_train"
    if tape is None:
        tape = torch.empty((max(0, len(layers) - 1),) + tuple(x.shape), dtype=torch.float32, device=x.device)
    t, flat, masks, keep = _transformer_train_operands(op, x, layers, head_num, None, tape, query_lengths, key_lengths, query_mask,
                                                       key_mask, use_positional_encoding, use_res, use_feed_forward, use_layer_norm,
                                                       blinding, output_type, route, ln_eps)
    a = t.fwd
    B, T, E = int(a.batch), int(a.seq_len), int(a.dim)
    if out is None:
        out = torch.empty((B, T, E) if output_type is None else (B, E), dtype=torch.float32, device=x.device)
    if output_type is None:
        t.fwd.out_stride, t.fwd.out_row_stride = _seq3d(op, "out", out, B, T, E)
    else:
        t.fwd.out_stride = _rows2d(op, "out", out, B, E)
    _dev_check(x, out, tape, *(list(masks) + flat))
    t.fwd.out = out.data_ptr()
    _workspace(op, t.fwd, int(_C.lib().dctr_transformer_workspace_bytes(ctypes.byref(t.fwd))), workspace, x.device)
    _C.check(_C.lib().dctr_transformer_train_fwd(ctypes.byref(t), _C.stream_ptr()), "dctr_transformer_train_fwd")
    del keep
    return out, tape


def transformer_bwd(x, layers, head_num, tape, d_out, query_lengths=None, key_lengths=None, query_mask=None, key_mask=None,
                    use_positional_encoding=True, use_res=True, use_feed_forward=True, use_layer_norm=False, blinding=True,
                    output_type=None, dx=None, accumulate=False, d_weights=None, max_blocks=0, route=None, workspace=None, ln_eps=1e-9,
                    keys=None):
    """Backward of transformer_train(): the whole stack in one call (include/dctr.h: dctr_transformer_bwd).  ``x``, ``layers``, the
    masks and the options as transformer_train(), ``tape`` what it returned.  ``d_out``: the gradient of its output, a float32
    [B, T, E] view (``output_type`` None) or [B, E] ('mean' / 'sum').  ``dx`` [B, T, E] view: written, or added to with
    ``accumulate``; ``d_weights``: 9 x len(layers) contiguous tensors of the weights' shapes in the layers' order (None where not
    wanted), ACCUMULATED into; the gradients of pe_q / pe_k are those of the pre-scaled tables.  ``keys``: only to hear the library
    refuse separate keys.  No atomics: the same bits on every call."""
    op = "transformer_bwd"
    t, flat, masks, keep = _transformer_train_operands(op, x, layers, head_num, keys, tape, query_lengths, key_lengths, query_mask,
                                                       key_mask, use_positional_encoding, use_res, use_feed_forward, use_layer_norm,
                                                       blinding, output_type, route, ln_eps)
    a = t.fwd
    B, T, E = int(a.batch), int(a.seq_len), int(a.dim)
    if output_type is None:
        t.d_out_stride, t.d_out_row_stride = _seq3d(op, "d_out", d_out, B, T, E)
    else:
        t.d_out_stride = _rows2d(op, "d_out", d_out, B, E)
    if dx is not None:
        t.dx_stride, t.dx_row_stride = _seq3d(op, "dx", dx, B, T, E)
    d_weights = [None] * len(flat) if d_weights is None else list(d_weights)
    if len(d_weights) != len(flat):
        raise ValueError("transformer_bwd: d_weights must hold %d entries (%s per layer)" % (len(flat), ", ".join(TRANSFORMER_WEIGHTS)))
    for i, (w, g) in enumerate(zip(flat, d_weights)):
        if g is not None:
            if w is None:
                raise ValueError("transformer_bwd: d_weights layer %d %s: the flags switch this weight off" % (i // 9, TRANSFORMER_WEIGHTS[i % 9]))
            _vec(op, "d_weights layer %d %s" % (i // 9, TRANSFORMER_WEIGHTS[i % 9]), g, w.numel())
    _dev_check(x, keys, tape, d_out, dx, *(list(masks) + flat + d_weights))
    dp = _ptr_array(d_weights)
    if any(g is not None for g in d_weights):
        t.d_layers = ctypes.cast(dp, ctypes.c_void_p)
    t.d_out, t.dx = d_out.data_ptr(), _ptr(dx)
    t.accumulate, t.max_blocks = int(bool(accumulate)), int(max_blocks)
    _workspace(op, t, int(_C.lib().dctr_transformer_bwd_workspace_bytes(ctypes.byref(t))), workspace, x.device)
    _C.check(_C.lib().dctr_transformer_bwd(ctypes.byref(t), _C.stream_ptr()), "dctr_transformer_bwd")
    del keep, dp


class TransformerFunction(torch.autograd.Function):
    """A stack of Transformer layers over self-attention as one differentiable op: transformer_train() forward (tape kept) and
    transformer_bwd() backward.  ``apply(x, query_lengths, key_lengths, query_mask, key_mask, head_num, flags, output_type,
    *weights)``: x [B,T,E]; the masks as transformer() takes them (no gradient); ``flags`` the dict of Transformer.flags();
    ``weights`` the 9 x n_layers tensors layer by layer in TRANSFORMER_WEIGHTS' order, None where a flag switches one off, the
    positional tables pre-scaled.  Returns [B,T,E], or [B,E] for 'mean' / 'sum'.  Gradients for x and the weights."""

    @staticmethod
    def forward(ctx, x, query_lengths, key_lengths, query_mask, key_mask, head_num, flags, output_type, *weights):
        x = x.detach()
        x = x if x.stride(2) == 1 or x.shape[2] == 1 else x.contiguous()
        ws = [None if w is None else w.detach().contiguous() for w in weights]
        layers = [ws[i:i + 9] for i in range(0, len(ws), 9)]
        masks = dict(query_lengths=query_lengths, key_lengths=key_lengths, query_mask=query_mask, key_mask=key_mask)
        out, tape = transformer_train(x, layers, head_num, output_type=output_type, **masks, **flags)
        ctx.cfg = (int(head_num), dict(flags), output_type, masks, [w is not None for w in ws])
        ctx.save_for_backward(x, tape, *[w for w in ws if w is not None])
        return out

    @staticmethod
    def backward(ctx, d_out):
        head_num, flags, output_type, masks, present = ctx.cfg
        saved = list(ctx.saved_tensors)
        x, tape, rest = saved[0], saved[1], saved[2:]
        ws = [rest.pop(0) if here else None for here in present]
        d = _grad_operand(d_out, output_type is not None)
        dx = torch.empty_like(x, memory_format=torch.contiguous_format) if ctx.needs_input_grad[0] else None
        wanted = [w is not None and ctx.needs_input_grad[8 + i] for i, w in enumerate(ws)]
        _, grads = _zeroed_grads(ws, wanted, x.device)      # one fill for all
        layers = [ws[i:i + 9] for i in range(0, len(ws), 9)]
        transformer_bwd(x, layers, head_num, tape, d, output_type=output_type, dx=dx, d_weights=grads, **masks, **flags)
        return (dx,) + (None,) * 7 + tuple(grads)


def layer_norm(x, gamma=None, beta=None, eps=1e-9, out=None):
    """LayerNormalization.call (reference layers/normalization.py:34-43) over the last axis of a contiguous float32 tensor; gamma / beta
    None = scale / center off."""
    x = _f32c(x, "x")
    dim = int(x.shape[-1])
    for name, t in (("gamma", gamma), ("beta", beta)):
        if t is not None:
            _vec("layer_norm", name, t, dim)
    if out is None:
        out = torch.empty_like(x)
    elif out.dtype != torch.float32 or not out.is_contiguous() or out.shape != x.shape:
        raise ValueError("layer_norm: out must be a contiguous float32 tensor of x's shape")
    _dev_check(x, gamma, beta, out)
    _C.check(_C.lib().dctr_layer_norm_fwd(_ptr(x), x.numel() // dim, dim, dim, _ptr(gamma), _ptr(beta), float(eps), _ptr(out), dim,
                                          _C.stream_ptr()), "dctr_layer_norm_fwd")
    return out


GRU_WEIGHTS = ("gate_kernel", "gate_bias", "candidate_kernel", "candidate_bias")


def gru_macs(T, E, n_layers=1):
    """Multiply-adds per sample of the recurrence: T x 6 E^2 per layer (4 E^2 gates + 2 E^2 candidate)."""
    return int(n_layers) * int(T) * 6 * int(E) * int(E)


def _gru_args(B, T, E, n_layers, cell, scale_input, return_sequence, route):
    if cell not in _C.gru.CELLS:
        raise ValueError("dynamic_gru: cell must be 'GRU', 'AGRU' or 'AUGRU', got %r" % (cell,))
    if route not in _C.gru.ROUTES:
        raise ValueError("dynamic_gru: route must be None, 'resident' or 'streamed', got %r" % (route,))
    return _C.gru.Args(batch=int(B), x_stride=int(T) * int(E), x_row_stride=int(E), att_stride=int(T), seq_len=int(T), dim=int(E),
                       n_layers=int(n_layers), cell=_C.gru.CELLS[cell], scale_input=int(bool(scale_input)),
                       return_sequence=int(bool(return_sequence)), route=_C.gru.ROUTES[route],
                       out_stride=int(T) * int(E) if return_sequence else int(E), out_row_stride=int(E))


def gru_workspace_bytes(batch, seq_len, dim, n_layers=1, cell="GRU", scale_input=False, return_sequence=True, route=None):
    """Bytes of the workspace dctr_gru_fwd needs for these shapes (0 while a workgroup's tiles fit the LDS; read from the library)."""
    a = _gru_args(batch, seq_len, dim, n_layers, cell, scale_input, return_sequence, route)
    return int(_C.lib().dctr_gru_workspace_bytes(ctypes.byref(a)))


def gru_route(seq_len, dim, n_layers=1, cell="GRU", scale_input=False, return_sequence=True, route=None):
    """'resident' or 'streamed': the route dctr_gru_fwd takes for these shapes (dctr_gru_route)."""
    a = _gru_args(1, seq_len, dim, n_layers, cell, scale_input, return_sequence, route)
    return _route_name("dctr_gru_route", _C.lib().dctr_gru_route(ctypes.byref(a)), (None, "resident", "streamed"))


def dynamic_gru(x, lengths, layers, cell="GRU", att_scores=None, scale_input=False, return_sequence=True, out=None, out_stride=None,
                route=None, workspace=None):
    """DynamicGRU.call (reference sequence.py:786-803) over one or two stacked layers, the whole time loop in one launch.

    ``x`` [B, T, E] float32 view (any sample / step strides, unit stride on the last axis); ``lengths`` int32 [B] (dynamic_rnn's
    sequence_length: state copied through and zero rows at t >= length).  ``layers``: per layer (gate kernel [2E, 2E], gate bias [2E],
    candidate kernel [2E, E], candidate bias [E]), or a dict of GRU_WEIGHTS.  ``cell``: 'GRU', 'AGRU' or 'AUGRU' (the attention-gated
    cells take one layer); ``att_scores`` [B, T] (or [B, T, 1] / [B, 1, T] contiguous) for them and for ``scale_input`` (x_t times its
    score: AIGRU).  ``out``: ``return_sequence`` a [B, T, E] view, else a [B, >= E] view with ``out_stride`` elements between samples
    (the final state, written in place into a wider buffer); allocated when None.  Returns ``out``."""
    op = "dynamic_gru"
    if x.dim() != 3:
        raise ValueError("Unexpected inputs dimensions %d, expect to be 3 dimensions" % x.dim())
    B, T, E = (int(v) for v in x.shape)
    if not layers:
        raise ValueError("dynamic_gru: at least one layer")
    a = _gru_args(B, T, E, len(layers), cell, scale_input, return_sequence, route)
    a.x_stride, a.x_row_stride = _seq3d(op, "x", x, B, T, E)
    if lengths.dtype != torch.int32 or lengths.numel() != B or not lengths.is_contiguous():
        raise ValueError("dynamic_gru: lengths must be a contiguous int32 tensor of %d elements" % B)
    need_att = cell != "GRU" or bool(scale_input)
    if need_att:
        if att_scores is None:
            raise ValueError("dynamic_gru: cell %r%s needs att_scores" % (cell, " with scale_input" if scale_input else ""))
        _vec(op, "att_scores", att_scores, B * T)
    else:
        att_scores = None
    shapes = {"gate_kernel": (2 * E, 2 * E), "gate_bias": (1, 2 * E), "candidate_kernel": (2 * E, E), "candidate_bias": (1, E)}
    flat = []
    for li, layer in enumerate(layers):
        if isinstance(layer, dict):
            layer = [layer.get(name) for name in GRU_WEIGHTS]
        if len(layer) != len(GRU_WEIGHTS) or any(w is None for w in layer):
            raise ValueError("dynamic_gru: layer %d: needs %s" % (li, ", ".join(GRU_WEIGHTS)))
        for name, w in zip(GRU_WEIGHTS, layer):
            rows, cols = shapes[name]
            if name.endswith("bias"):
                _vec(op, "layer %d %s" % (li, name), w, cols)
            elif _rows2d(op, "layer %d %s" % (li, name), w, rows, cols) != cols and rows > 1:
                raise ValueError("dynamic_gru: layer %d: %s must be contiguous" % (li, name))
            flat.append(w)
    if out is None:
        out = torch.empty((B, T, E) if return_sequence else (B, E), dtype=torch.float32, device=x.device)
    if return_sequence:
        a.out_stride, a.out_row_stride = _seq3d(op, "out", out, B, T, E)
    else:
        pitch = _rows2d(op, "out", out, B, E, at_least_rows=False)
        a.out_stride = int(out_stride) if out_stride is not None else pitch
        if a.out_stride < E:
            raise ValueError("dynamic_gru: out_stride %d < dim %d" % (a.out_stride, E))
    _dev_check(x, lengths, att_scores, out, *flat)
    lp = _ptr_array(flat)
    a.layers = ctypes.cast(lp, ctypes.c_void_p)
    a.x, a.lengths, a.att_scores, a.out = x.data_ptr(), lengths.data_ptr(), _ptr(att_scores), out.data_ptr()
    _workspace(op, a, int(_C.lib().dctr_gru_workspace_bytes(ctypes.byref(a))), workspace, x.device)
    _C.check(_C.lib().dctr_gru_fwd(ctypes.byref(a), _C.stream_ptr()), "dctr_gru_fwd")
    del lp
    return out


def gru_bwd_macs(T, E):
    """Multiply-adds per sample of one layer's backward: per step the forward's 6 E^2 recomputed + 12 E^2 for the four gradient
    products (dz W^T and A^T dz through the gate and the candidate kernel)."""
    return int(T) * 18 * int(E) * int(E)


def _gru_bwd_shape(batch, seq_len, dim, cell, scale_input, return_sequence, route=None, n_layers=1):
    T, E = int(seq_len), int(dim)
    b = _C.gru.BwdArgs(h_stride=T * E, h_row_stride=E, d_out_stride=T * E if return_sequence else E, d_out_row_stride=E,
                       dx_stride=T * E, dx_row_stride=E, d_att_stride=T)
    b.fwd = _gru_args(batch, T, E, n_layers, cell, scale_input, return_sequence, route)
    return b


def gru_bwd_supported(seq_len, dim, cell="GRU", scale_input=False, return_sequence=True, route=None, n_layers=1):
    """Does dctr_gru_bwd take these shapes and options (read from the library)?"""
    b = _gru_bwd_shape(1, seq_len, dim, cell, scale_input, return_sequence, route, n_layers)
    return bool(_C.lib().dctr_gru_bwd_supported(ctypes.byref(b)))


def gru_bwd_workspace_bytes(batch, seq_len, dim, cell="GRU", scale_input=False, return_sequence=True, route=None):
    """Bytes of the workspace dctr_gru_bwd needs for these shapes (read from the library; every supported shape runs out of the LDS)."""
    b = _gru_bwd_shape(batch, seq_len, dim, cell, scale_input, return_sequence, route)
    return int(_C.lib().dctr_gru_bwd_workspace_bytes(ctypes.byref(b)))


def gru_bwd(x, lengths, layer, h_seq, d_out, cell="GRU", att_scores=None, scale_input=False, return_sequence=True, dx=None,
            accumulate=False, d_att=None, d_weights=None, max_blocks=0, route=None, workspace=None):
    """Backward of dynamic_gru() over ONE layer, all T steps in one launch (include/dctr.h: dctr_gru_bwd).  ``x``, ``lengths``,
    ``att_scores``, ``cell``, ``scale_input`` as dynamic_gru(); ``layer``: its four weights (or a dict of GRU_WEIGHTS); ``h_seq``: the
    forward's return_sequence=True output of the layer, a [B, T, E] view; ``d_out``: the gradient of the forward's output, a [B, T, E]
    view with ``return_sequence``, else a [B, >= E] view (the final state's).  ``dx`` [B, T, E] view: written, or added to with
    ``accumulate``; ``d_att`` [B, >= T] view: written; ``d_weights``: four contiguous tensors of the weights' shapes, ACCUMULATED
    into.  Each output, and any entry of ``d_weights``, may be None."""
    op = "gru_bwd"
    if x.dim() != 3:
        raise ValueError("Unexpected inputs dimensions %d, expect to be 3 dimensions" % x.dim())
    B, T, E = (int(v) for v in x.shape)
    b = _gru_bwd_shape(B, T, E, cell, scale_input, return_sequence, route)
    a = b.fwd
    a.x_stride, a.x_row_stride = _seq3d(op, "x", x, B, T, E)
    b.h_stride, b.h_row_stride = _seq3d(op, "h_seq", h_seq, B, T, E)
    if lengths.dtype != torch.int32 or lengths.numel() != B or not lengths.is_contiguous():
        raise ValueError("gru_bwd: lengths must be a contiguous int32 tensor of %d elements" % B)
    need_att = cell != "GRU" or bool(scale_input)
    if need_att:
        if att_scores is None:
            raise ValueError("gru_bwd: cell %r%s needs att_scores" % (cell, " with scale_input" if scale_input else ""))
        _vec(op, "att_scores", att_scores, B * T)
        if d_att is not None:
            b.d_att_stride = _rows2d(op, "d_att", d_att, B, T)
    else:
        att_scores = d_att = None
    if isinstance(layer, dict):
        layer = [layer.get(name) for name in GRU_WEIGHTS]
    if len(layer) != len(GRU_WEIGHTS) or any(w is None for w in layer):
        raise ValueError("gru_bwd: the layer needs %s" % ", ".join(GRU_WEIGHTS))
    sizes = (4 * E * E, 2 * E, 2 * E * E, E)
    for name, w, n in zip(GRU_WEIGHTS, layer, sizes):
        _vec(op, name, w, n)
    d_weights = [None] * 4 if d_weights is None else list(d_weights)
    if len(d_weights) != 4:
        raise ValueError("gru_bwd: d_weights must hold four entries (%s)" % ", ".join(GRU_WEIGHTS))
    for name, g, n in zip(GRU_WEIGHTS, d_weights, sizes):
        if g is not None:
            _vec(op, "d_weights %s" % name, g, n)
    if return_sequence:
        b.d_out_stride, b.d_out_row_stride = _seq3d(op, "d_out", d_out, B, T, E)
    else:
        b.d_out_stride = _rows2d(op, "d_out", d_out, B, E)
    if dx is not None:
        b.dx_stride, b.dx_row_stride = _seq3d(op, "dx", dx, B, T, E)
    _dev_check(x, lengths, att_scores, h_seq, d_out, dx, d_att, *(list(layer) + d_weights))
    lp, dp = _ptr_array(list(layer)), _ptr_array(d_weights)
    a.layers = ctypes.cast(lp, ctypes.c_void_p)
    a.x, a.lengths, a.att_scores = x.data_ptr(), lengths.data_ptr(), _ptr(att_scores)
    b.h_seq, b.d_out, b.dx, b.d_att = h_seq.data_ptr(), d_out.data_ptr(), _ptr(dx), _ptr(d_att)
    if any(g is not None for g in d_weights):
        b.d_layers = ctypes.cast(dp, ctypes.c_void_p)
    b.accumulate, b.max_blocks = int(bool(accumulate)), int(max_blocks)
    _workspace(op, a, int(_C.lib().dctr_gru_bwd_workspace_bytes(ctypes.byref(b))), workspace, x.device)
    _C.check(_C.lib().dctr_gru_bwd(ctypes.byref(b), _C.stream_ptr()), "dctr_gru_bwd")
    del lp, dp


class DynamicGRUFunction(torch.autograd.Function):
    """One DynamicGRU layer as a differentiable op: dynamic_gru() forward (always with return_sequence: the backward reads h_{t-1}
    from it) and gru_bwd() backward, one launch each.  ``apply(x, lengths, att_scores, cell, scale_input, return_sequence, gate_kernel,
    gate_bias, candidate_kernel, candidate_bias)``: x [B,T,E], lengths int32 [B], att_scores [B,T] or None.  Returns [B,T,E], or the
    final state [B,E]: the row at length - 1 of the sequence, zeros for length <= 0."""

    @staticmethod
    def forward(ctx, x, lengths, att_scores, cell, scale_input, return_sequence, *weights):
        ctx.cfg = (cell, bool(scale_input), bool(return_sequence))
        x = x.detach()
        x = x if x.stride(2) == 1 or x.shape[2] == 1 else x.contiguous()
        B, T, E = x.shape
        lengths = lengths.reshape(-1).to(torch.int32).contiguous()
        need_att = cell != "GRU" or bool(scale_input)
        att = att_scores.detach().reshape(B, T).contiguous() if need_att else None
        ws = [w.detach().contiguous() for w in weights]
        seq = dynamic_gru(x, lengths, [ws], cell=cell, att_scores=att, scale_input=scale_input, return_sequence=True)
        ctx.has_att = att is not None
        ctx.save_for_backward(x, lengths, seq, *(ws + ([att] if att is not None else [])))
        if return_sequence:
            return seq
        last = (lengths.clamp(1, T) - 1).to(torch.int64)
        final = seq[torch.arange(B, device=x.device), last]
        return final * (lengths > 0).to(final.dtype).unsqueeze(1)

    @staticmethod
    def backward(ctx, d_out):
        cell, scale_input, return_sequence = ctx.cfg
        saved = list(ctx.saved_tensors)
        x, lengths, seq, ws = saved[0], saved[1], saved[2], saved[3:7]
        att = saved[7] if ctx.has_att else None
        d_out = _grad_operand(d_out, not return_sequence)
        dx = torch.empty_like(x, memory_format=torch.contiguous_format) if ctx.needs_input_grad[0] else None
        d_att = torch.empty_like(att) if att is not None and ctx.needs_input_grad[2] else None
        _, grads = _zeroed_grads(ws, [ctx.needs_input_grad[6 + i] for i in range(4)], x.device)     # one fill for the four
        gru_bwd(x, lengths, ws, seq, d_out, cell=cell, att_scores=att, scale_input=scale_input, return_sequence=return_sequence, dx=dx,
                d_att=d_att, d_weights=grads)
        return (dx, None, d_att, None, None, None) + tuple(grads)


LSTM_WEIGHTS =("fw_kernel", "fw_recurrent_kernel", "fw_bias", "bw_kernel", "bw_recurrent_kernel", "bw_bias")


def bilstm_macs(T, Din, u, n_layers=1):
    """Multiply-adds per sample of both stacks: T x 2 x 4u (D + u) per layer, D = Din for layer 0 and u after it."""
    T, Din, u = int(T), int(Din), int(u)
    return T * 2 * 4 * u * ((Din + u) + (int(n_layers) - 1) * 2 * u)


def _bilstm_args(B, T, Din, u, n_layers, res_layers, merge_mode, recurrent_activation, route):
    if merge_mode not in _C.lstm.MERGES:
        raise ValueError('Invalid merge mode. Merge mode should be one of {"fw","bw","sum", "mul", "ave", "concat", None}')
    if recurrent_activation not in _C.lstm.ACTIVATIONS:
        raise ValueError("bilstm: recurrent_activation must be 'sigmoid' or 'hard_sigmoid', got %r" % (recurrent_activation,))
    if route not in _C.lstm.ROUTES:
        raise ValueError("bilstm: route must be None, 'resident', 'streamed' or 'workspace', got %r" % (route,))
    n_layers, res_layers = int(n_layers), int(res_layers)
    if not 1 <= n_layers <= _C.lstm.MAX_LAYERS:
        raise ValueError("bilstm: 1 to %d layers, got %d" % (_C.lstm.MAX_LAYERS, n_layers))
    if res_layers >= n_layers and int(Din) != int(u):
        raise ValueError("bilstm: a residual over layer 0 needs inputs of the units' width, got %d and %d" % (Din, u))
    w = (2 if merge_mode == "concat" else 1) * int(u)
    return _C.lstm.Args(batch=int(B), x_stride=int(T) * int(Din), x_row_stride=int(Din), seq_len=int(T), in_dim=int(Din), units=int(u),
                        n_layers=n_layers, res_layers=max(res_layers, 0), merge_mode=_C.lstm.MERGES[merge_mode],
                        recurrent_activation=_C.lstm.ACTIVATIONS[recurrent_activation], route=_C.lstm.ROUTES[route],
                        out_stride=int(T) * w, out_row_stride=w, out_bw_stride=int(T) * int(u), out_bw_row_stride=int(u))


def bilstm_workspace_bytes(batch, T, Din, u, n_layers, res_layers=0, merge_mode="ave", route=None):
    """Bytes of the workspace dctr_bilstm_fwd needs for these shapes (0 while a workgroup's tiles fit the LDS; read from the library)."""
    a = _bilstm_args(batch, T, Din, u, n_layers, res_layers, merge_mode, "sigmoid", route)
    return int(_C.lib().dctr_bilstm_workspace_bytes(ctypes.byref(a)))


def bilstm_route(T, Din, u, n_layers, res_layers=0, merge_mode="ave", route=None):
    """'resident' or 'streamed': the route dctr_bilstm_fwd takes for these shapes (dctr_bilstm_route)."""
    a = _bilstm_args(1, T, Din, u, n_layers, res_layers, merge_mode, "sigmoid", route)
    return _route_name("dctr_bilstm_route", _C.lib().dctr_bilstm_route(ctypes.byref(a)), (None, "resident", "streamed"))


def _bilstm_operands(op, x, layers, res_layers, merge_mode, recurrent_activation, route):
    """The checks of x and the layers' weights that bilstm(), bilstm_train() and bilstm_bwd() share.  Returns (args struct with the
    sizes and x's strides, the 6 * n_layers weights in the library's order)."""
    if x.dim() != 3:
        raise ValueError("Unexpected inputs dimensions %d, expect to be 3 dimensions" % x.dim())
    B, T, Din = (int(v) for v in x.shape)
    if not layers:
        raise ValueError("%s: at least one layer" % op)
    rows = []
    for li, layer in enumerate(layers):
        if isinstance(layer, dict):
            layer = [layer.get(name) for name in LSTM_WEIGHTS]
        if len(layer) != len(LSTM_WEIGHTS) or any(w is None for w in layer):
            raise ValueError("%s: layer %d: needs %s" % (op, li, ", ".join(LSTM_WEIGHTS)))
        rows.append(layer)
    u = int(rows[0][1].shape[0])
    a = _bilstm_args(B, T, Din, u, len(rows), res_layers, merge_mode, recurrent_activation, route)
    a.x_stride, a.x_row_stride = _seq3d(op, "x", x, B, T, Din)
    flat = []
    for li, layer in enumerate(rows):
        D = Din if li == 0 else u
        shapes = {"kernel": (D, 4 * u), "recurrent_kernel": (u, 4 * u)}
        for name, w in zip(LSTM_WEIGHTS, layer):
            what = "layer %d %s" % (li, name)
            if name.endswith("bias"):
                _vec(op, what, w, 4 * u)
            else:
                r, c = shapes[name[3:]]
                if _rows2d(op, what, w, r, c) != c and r > 1:
                    raise ValueError("%s: %s must be contiguous" % (op, what))
            flat.append(w)
    return a, flat


def _bilstm_out(op, a, out, merge_mode, device):
    """``out`` of bilstm() / bilstm_train(): the given views, or new tensors; their strides go into ``a``.  Returns (out_fw, out_bw)."""
    B, T, u = int(a.batch), int(a.seq_len), int(a.units)
    wout = 2 * u if merge_mode == "concat" else u
    if merge_mode is None:
        out_fw, out_bw = out if out is not None else (None, None)
    else:
        out_fw, out_bw = out, None
    if out_fw is None:
        out_fw = torch.empty((B, T, wout), dtype=torch.float32, device=device)
    a.out_stride, a.out_row_stride = _seq3d(op, "out", out_fw, B, T, wout)
    if merge_mode is None:
        if out_bw is None:
            out_bw = torch.empty((B, T, u), dtype=torch.float32, device=device)
        a.out_bw_stride, a.out_bw_row_stride = _seq3d(op, "out (backward)", out_bw, B, T, u)
    return out_fw, out_bw


def bilstm(x, layers, res_layers=0, merge_mode="ave", recurrent_activation="sigmoid", out=None, route=None, workspace=None):
    """BiLSTM.call (reference sequence.py:375-409) over keras' LSTM: both stacks of len(layers) layers in one launch.

    ``x`` [B, T, Din] float32 view (any sample / step strides, unit stride on the last axis).  ``layers``: per layer (fw kernel [D, 4u],
    fw recurrent kernel [u, 4u], fw bias [4u], then the same three of the backward stack), or a dict of LSTM_WEIGHTS; D = Din for
    layer 0 and u after it, gate order i | f | c~ | o.  The last ``res_layers`` layers add their input to their output.  ``merge_mode``:
    'fw', 'bw', 'sum', 'mul', 'ave' -> [B, T, u], 'concat' -> [B, T, 2u], None -> the pair (fw, bw).  ``out``: a view of that shape (a
    pair for None), allocated when None.  Returns ``out``."""
    op = "bilstm"
    a, flat = _bilstm_operands(op, x, layers, res_layers, merge_mode, recurrent_activation, route)
    out_fw, out_bw = _bilstm_out(op, a, out, merge_mode, x.device)
    _dev_check(x, out_fw, out_bw, *flat)
    lp = _ptr_array(flat)
    a.layers = ctypes.cast(lp, ctypes.c_void_p)
    a.x, a.out, a.out_bw = x.data_ptr(), out_fw.data_ptr(), _ptr(out_bw)
    _workspace(op, a, int(_C.lib().dctr_bilstm_workspace_bytes(ctypes.byref(a))), workspace, x.device)
    _C.check(_C.lib().dctr_bilstm_fwd(ctypes.byref(a), _C.stream_ptr()), "dctr_bilstm_fwd")
    del lp
    return (out_fw, out_bw) if merge_mode is None else out_fw


def bilstm_bwd_macs(T, Din, u, n_layers=1):
    """Multiply-adds per sample of dctr_bilstm_bwd: the forward's products recomputed, as many for dz [W; U]^T and as many for the
    weight gradients [in | h_prev]^T dz — three times bilstm_macs()."""
    return 3 * bilstm_macs(T, Din, u, n_layers)


def _bilstm_train_shape(B, T, Din, u, n_layers, res_layers, merge_mode, recurrent_activation, route):
    t = _C.lstm.TrainArgs()
    t.fwd = _bilstm_args(B, T, Din, u, n_layers, res_layers, merge_mode, recurrent_activation, route)
    t.d_out_stride, t.d_out_row_stride = t.fwd.out_stride, t.fwd.out_row_stride
    t.d_out_bw_stride, t.d_out_bw_row_stride = t.fwd.out_bw_stride, t.fwd.out_bw_row_stride
    t.dx_stride, t.dx_row_stride = int(T) * int(Din), int(Din)
    return t


def bilstm_bwd_supported(T, Din, u, n_layers, res_layers=0, merge_mode="ave", recurrent_activation="sigmoid", route=None):
    """Does dctr_bilstm_bwd (and the training forward whose tape it reads) take these shapes and options (read from the library)?"""
    if int(n_layers) > _C.lstm.MAX_LAYERS:
        return False
    t = _bilstm_train_shape(1, T, Din, u, n_layers, res_layers, merge_mode, recurrent_activation, route)
    return bool(_C.lib().dctr_bilstm_bwd_supported(ctypes.byref(t)))


def bilstm_bwd_workspace_bytes(batch, T, Din, u, n_layers, res_layers=0, merge_mode="ave", route=None):
    """Bytes of the workspace dctr_bilstm_bwd needs for these shapes (read from the library; 0 for a shape it refuses)."""
    t = _bilstm_train_shape(batch, T, Din, u, n_layers, res_layers, merge_mode, "sigmoid", route)
    return int(_C.lib().dctr_bilstm_bwd_workspace_bytes(ctypes.byref(t)))


def _bilstm_train_operands(op, x, layers, masks, tape, res_layers, merge_mode, recurrent_activation, route):
    """x, the weights, the masks and the tape of bilstm_train() / bilstm_bwd().  Returns (train args, weights, masks, keep-alive)."""
    a, flat = _bilstm_operands(op, x, layers, res_layers, merge_mode, recurrent_activation, route)
    B, Din, u, L = int(a.batch), int(a.in_dim), int(a.units), int(a.n_layers)
    t = _C.lstm.TrainArgs()
    t.fwd = a
    masks = [None] * (2 * L) if masks is None else list(masks)
    if len(masks) != 2 * L:
        raise ValueError("%s: masks must hold 2 x %d entries (fw, bw per layer), got %d" % (op, L, len(masks)))
    for i, m in enumerate(masks):
        if m is not None:
            _vec(op, "mask %d" % i, m, B * (Din if i < 2 else u))
    need = int(_C.lib().dctr_bilstm_tape_bytes(ctypes.byref(a)))
    if tape is None or tape.dtype != torch.float32 or not tape.is_contiguous() or tape.numel() * 4 < need:
        raise ValueError("%s: tape must be a contiguous float32 tensor of >= %d bytes (bilstm_train allocates it)" % (op, need))
    lp, mp = _ptr_array(flat), _ptr_array(masks)
    t.fwd.layers = ctypes.cast(lp, ctypes.c_void_p)
    if any(m is not None for m in masks):
        t.masks = ctypes.cast(mp, ctypes.c_void_p)
    t.fwd.x, t.tape, t.tape_bytes = x.data_ptr(), tape.data_ptr(), tape.numel() * 4
    return t, flat, masks, (lp, mp)


def bilstm_train(x, layers, masks=None, res_layers=0, merge_mode="ave", recurrent_activation="sigmoid", out=None, tape=None,
                 route=None):
    """bilstm() as the forward of a training step (dctr_bilstm_train_fwd): the same kernel, so the same bits without masks.
    ``masks``: None, or 2 x len(layers) entries in the order fw layer 0, bw layer 0, fw layer 1, ...; each None or a contiguous
    float32 [B, D_l] (or [B, 1, D_l]) tensor that holds 0 or 1 / (1 - rate): the input dropout of that LSTM, the same for every step.
    Returns (out, tape): ``out`` as bilstm(), ``tape`` the h_t and c_t of every (layer, direction, step, sample) for bilstm_bwd()
    (include/dctr.h has the layout), allocated when None."""
    op = "bilstm_train"
    if tape is None:
        L = len(layers)
        u = int((layers[0]["fw_recurrent_kernel"] if isinstance(layers[0], dict) else layers[0][1]).shape[0]) if L else 0
        tape = torch.empty(max(1, L * 2 * int(x.shape[1]) * 2 * int(x.shape[0]) * u), dtype=torch.float32, device=x.device)
    t, flat, masks, keep = _bilstm_train_operands(op, x, layers, masks, tape, res_layers, merge_mode, recurrent_activation, route)
    out_fw, out_bw = _bilstm_out(op, t.fwd, out, merge_mode, x.device)
    _dev_check(x, out_fw, out_bw, tape, *(flat + masks))
    t.fwd.out, t.fwd.out_bw = out_fw.data_ptr(), _ptr(out_bw)
    _C.check(_C.lib().dctr_bilstm_train_fwd(ctypes.byref(t), _C.stream_ptr()), "dctr_bilstm_train_fwd")
    del keep
    return ((out_fw, out_bw) if merge_mode is None else out_fw), tape


def bilstm_bwd(x, layers, tape, d_out, masks=None, res_layers=0, merge_mode="ave", recurrent_activation="sigmoid", dx=None,
               accumulate=False, d_weights=None, max_blocks=0, route=None, workspace=None):
    """Backward of bilstm_train(): both stacks, all layers and all steps (include/dctr.h: dctr_bilstm_bwd).  ``x``, ``layers``,
    ``masks`` and the options as bilstm_train(), ``tape`` what it returned.  ``d_out``: the gradient of its output, a float32 view
    of the output's shape (the pair (d_fw, d_bw) for merge_mode None).  ``dx`` [B, T, Din] view: written, or added to with
    ``accumulate``; ``d_weights``: 6 x len(layers) contiguous tensors of the weights' shapes in the layers' order, ACCUMULATED into.
    ``dx`` and any entry of ``d_weights`` may be None.  No atomics: the same bits on every call."""
    op = "bilstm_bwd"
    t, flat, masks, keep = _bilstm_train_operands(op, x, layers, masks, tape, res_layers, merge_mode, recurrent_activation, route)
    a = t.fwd
    B, T, Din, u = int(a.batch), int(a.seq_len), int(a.in_dim), int(a.units)
    d_fw, d_bw = d_out if merge_mode is None else (d_out, None)
    t.d_out_stride, t.d_out_row_stride = _seq3d(op, "d_out", d_fw, B, T, 2 * u if merge_mode == "concat" else u)
    if merge_mode is None:
        t.d_out_bw_stride, t.d_out_bw_row_stride = _seq3d(op, "d_out (backward)", d_bw, B, T, u)
    if dx is not None:
        t.dx_stride, t.dx_row_stride = _seq3d(op, "dx", dx, B, T, Din)
    d_weights = [None] * len(flat) if d_weights is None else list(d_weights)
    if len(d_weights) != len(flat):
        raise ValueError("bilstm_bwd: d_weights must hold %d entries (%s per layer)" % (len(flat), ", ".join(LSTM_WEIGHTS)))
    for i, (w, g) in enumerate(zip(flat, d_weights)):
        if g is not None:
            _vec(op, "d_weights layer %d %s" % (i // 6, LSTM_WEIGHTS[i % 6]), g, w.numel())
    _dev_check(x, tape, d_fw, d_bw, dx, *(flat + masks + d_weights))
    dp = _ptr_array(d_weights)
    if any(g is not None for g in d_weights):
        t.d_layers = ctypes.cast(dp, ctypes.c_void_p)
    t.d_out, t.d_out_bw, t.dx = d_fw.data_ptr(), _ptr(d_bw), _ptr(dx)
    t.accumulate, t.max_blocks = int(bool(accumulate)), int(max_blocks)
    _workspace(op, t, int(_C.lib().dctr_bilstm_bwd_workspace_bytes(ctypes.byref(t))), workspace, x.device)
    _C.check(_C.lib().dctr_bilstm_bwd(ctypes.byref(t), _C.stream_ptr()), "dctr_bilstm_bwd")
    del keep, dp


class BiLSTMFunction(torch.autograd.Function):
    """BiLSTM as one differentiable op: bilstm_train() forward (masks applied, tape kept) and bilstm_bwd() backward.
    ``apply(x, masks, res_layers, merge_mode, recurrent_activation, *weights)``: x [B,T,Din]; ``masks`` None or the 2 x n_layers
    dropout masks of bilstm_train() (no gradient); ``weights`` the 6 x n_layers tensors layer by layer in LSTM_WEIGHTS' order.
    Returns what bilstm() returns, a pair for merge_mode None.  Gradients for x and the weights."""

    @staticmethod
    def forward(ctx, x, masks, res_layers, merge_mode, recurrent_activation, *weights):
        ctx.set_materialize_grads(False)
        x = x.detach()
        x = x if x.stride(2) == 1 or x.shape[2] == 1 else x.contiguous()
        B = x.shape[0]
        ws = [w.detach().contiguous() for w in weights]
        layers = [ws[i:i + 6] for i in range(0, len(ws), 6)]
        masks = None if masks is None else [None if m is None else m.detach().reshape(B, -1).contiguous() for m in masks]
        out, tape = bilstm_train(x, layers, masks, res_layers, merge_mode, recurrent_activation)
        ctx.cfg = (int(res_layers), merge_mode, recurrent_activation, masks)
        ctx.save_for_backward(x, tape, *ws)
        return out

    @staticmethod
    def backward(ctx, *d_out):
        res_layers, merge_mode, recurrent_activation, masks = ctx.cfg
        saved = list(ctx.saved_tensors)
        x, tape, ws = saved[0], saved[1], saved[2:]
        B, T, _ = x.shape
        u = ws[1].shape[0]
        if merge_mode is None:      # a branch nothing consumed has no gradient
            d = tuple(torch.zeros((B, T, u), dtype=torch.float32, device=x.device) if g is None else _grad_operand(g, False) for g in d_out)
        else:
            d = _grad_operand(d_out[0], False)
        dx = torch.empty_like(x, memory_format=torch.contiguous_format) if ctx.needs_input_grad[0] else None
        _, grads = _zeroed_grads(ws, [ctx.needs_input_grad[5 + i] for i in range(len(ws))], x.device)       # one fill for all
        layers = [ws[i:i + 6] for i in range(0, len(ws), 6)]
        bilstm_bwd(x, layers, tape, d, masks, res_layers, merge_mode, recurrent_activation, dx=dx, d_weights=grads)
        return (dx, None, None, None, None) + tuple(grads)


def bias_encoding(x, sess_bias, seq_bias, item_bias):
    """BiasEncoding.call (reference sequence.py:735-744) in place: ``x`` a float32 [B, S, T, E] view with unit stride on the last axis,
    x[b, s, t, e] += item_bias[e] + seq_bias[t] + sess_bias[s].  Returns ``x``."""
    op = "bias_encoding"
    if x.dim() != 4 or x.dtype != torch.float32 or (x.shape[3] > 1 and x.stride(3) != 1):
        raise ValueError("bias_encoding: x must be a float32 [B, S, T, E] view with unit stride on the last axis")
    B, S, T, E = (int(v) for v in x.shape)
    _vec(op, "sess_bias", sess_bias, S)
    _vec(op, "seq_bias", seq_bias, T)
    _vec(op, "item_bias", item_bias, E)
    row = int(x.stride(2)) if T != 1 else max(int(x.stride(2)), E)
    sess = int(x.stride(1)) if S != 1 else max(int(x.stride(1)), (T - 1) * row + E)
    sample = int(x.stride(0)) if B > 1 else max(int(x.stride(0)), (S - 1) * sess + (T - 1) * row + E)
    _dev_check(x, sess_bias, seq_bias, item_bias)
    _C.check(_C.lib().dctr_bias_encoding_fwd(_ptr(x), B, S, T, E, sample, sess, row, _ptr(sess_bias), _ptr(seq_bias), _ptr(item_bias),
                                             _C.stream_ptr()), "dctr_bias_encoding_fwd")
    return x


def _field_conv_stages(op, kernels, pools, fields, in_channels=None):
    """The stages' geometry from the kernels' shapes [w, C_in, C_out] and ``pools`` = per stage ('kmax', k) or ('max', p).  Returns
    (widths, channels, kinds, args, rows per stage's pooled map, C_0)."""
    if len(kernels) == 0 or len(kernels) != len(pools):
        raise ValueError("%s: one pooling per conv kernel and at least one stage, got %d and %d" % (op, len(kernels), len(pools)))
    if len(kernels) > _C.fieldconv.MAX_STAGES:
        raise ValueError("%s: at most %d stages, got %d" % (op, _C.fieldconv.MAX_STAGES, len(kernels)))
    widths, channels, kinds, args, rows_out = [], [], [], [], []
    rows, cin = int(fields), None
    for s, (kern, pool) in enumerate(zip(kernels, pools)):
        shape = tuple(int(v) for v in (kern.shape if hasattr(kern, "shape") else kern))
        if len(shape) == 4 and shape[1] == 1:           # keras' Conv2D kernel [w, 1, C_in, C_out]
            shape = (shape[0],) + shape[2:]
        if len(shape) != 3 or min(shape) < 1:
            raise ValueError("%s: stage %d: the kernel must be [w, C_in, C_out], got %s" % (op, s, shape))
        if cin is None:
            cin = shape[1] if in_channels is None else int(in_channels)
            c0 = cin
        if shape[1] != cin:
            raise ValueError("%s: stage %d: the kernel takes %d channels, its input has %d" % (op, s, shape[1], cin))
        kind, arg = pool
        if kind not in _C.fieldconv.POOLS:
            raise ValueError("%s: stage %d: pooling must be ('kmax', k) or ('max', p), got %r" % (op, s, pool))
        arg = int(arg)
        if not 1 <= arg <= rows:
            raise ValueError("%s: stage %d: %s %d outside 1..%d rows" % (op, s, "k" if kind == "kmax" else "pooling width", arg, rows))
        widths.append(shape[0])
        channels.append(shape[2])
        kinds.append(_C.fieldconv.POOLS[kind])
        args.append(arg)
        rows = arg if kind == "kmax" else rows // arg
        rows_out.append(rows)
        cin = shape[2]
    return widths, channels, kinds, args, rows_out, c0


def _field_conv_args(op, batch, fields, dim, kernels, pools, route, in_channels=None):
    if route not in _C.fieldconv.ROUTES:
        raise ValueError("%s: route must be None, 'resident', 'streamed' or 'workspace', got %r" % (op, route))
    widths, channels, kinds, pargs, rows_out, c0 = _field_conv_stages(op, kernels, pools, fields, in_channels)
    if int(fields) < 1 or int(dim) < 1:
        raise ValueError("%s: fields and dim must be >= 1, got %d and %d" % (op, fields, dim))
    arrs = [_i32_array(v) for v in (widths, channels, kinds, pargs)]
    a = _C.fieldconv.Args(batch=int(batch), x_stride=int(fields) * int(dim) * c0, x_offset=0, fields=int(fields), dim=int(dim), in_channels=c0,
                          n_stages=len(widths), route=_C.fieldconv.ROUTES[route], out_stride=rows_out[-1] * int(dim) * channels[-1], out_offset=0)
    a.widths, a.channels, a.pool_kinds, a.pool_args = (ctypes.cast(v, ctypes.c_void_p) for v in arrs)
    return a, arrs, channels, rows_out


def field_conv_macs(fields, dim, kernels, pools):
    """Multiply-adds per sample of the conv stack: E x sum over the stages of rows w C_in C_out (``kernels``: tensors or shapes)."""
    widths, channels, _, _, rows_out, c0 = _field_conv_stages("field_conv_macs", kernels, pools, fields)
    total, rows, cin = 0, int(fields), c0
    for w, c, ro in zip(widths, channels, rows_out):
        total += rows * w * cin * c
        rows, cin = ro, c
    return total * int(dim)


def field_conv_workspace_bytes(batch, fields, dim, kernels, pools, route=None):
    """Bytes of the workspace dctr_fieldconv_fwd needs for these shapes (0 while a workgroup's maps fit the LDS; read from the library).
    ``kernels``: tensors or shapes [w, C_in, C_out]."""
    a, arrs, _, _ = _field_conv_args("field_conv", batch, fields, dim, kernels, pools, route)
    return int(_C.lib().dctr_fieldconv_workspace_bytes(ctypes.byref(a)))


def field_conv_route(fields, dim, kernels, pools, route=None):
    """'resident' or 'streamed': the route dctr_fieldconv_fwd takes for these shapes (dctr_fieldconv_route)."""
    a, arrs, _, _ = _field_conv_args("field_conv", 1, fields, dim, kernels, pools, route)
    return _route_name("dctr_fieldconv_route", _C.lib().dctr_fieldconv_route(ctypes.byref(a)), (None, "resident", "streamed"))


def field_conv(x, kernels, biases, pools, fields=None, dim=None, x_offset=0, out=None, out_offset=0, stage_outs=None, route=None,
               workspace=None):
    """The conv / pool stack of CCPM and FGCNNLayer along the field axis (dctr_fieldconv_fwd), one launch.

    ``x`` [B, F, E] (or [B, F, E, C_0] channel-last); with ``fields`` / ``dim`` the F E C_0 columns from ``x_offset`` of a float32
    [B, stride] buffer read in place.  ``kernels``: per stage [w, C_in, C_out] (or keras' [w, 1, C_in, C_out]), ``biases`` [C_out],
    ``pools`` ('kmax', k) or ('max', p).  ``out``: a float32 [B, >= out_offset + rows E C] buffer that receives the last pooled map
    channel-last from column ``out_offset`` (allocated [B, rows, E, C] when None).  ``stage_outs``: True for every stage's pooled map in
    new [B, rows_s, E, C_s] tensors, or a list with per stage None or a float32 [B, >= rows_s E C_s] buffer.  Returns ``out``, or
    (out, stage_outs) with ``stage_outs``."""
    op = "field_conv"
    if len(kernels) != len(biases):
        raise ValueError("field_conv: one bias per kernel, got %d and %d" % (len(biases), len(kernels)))
    if fields is None:
        if x.dim() not in (3, 4):
            raise ValueError("Unexpected inputs dimensions %d, expect to be 3 or 4 dimensions" % x.dim())
        x = _f32c(x, "x")
        B, F, E = (int(v) for v in x.shape[:3])
        c_in = int(x.shape[3]) if x.dim() == 4 else 1
        a, arrs, channels, rows_out = _field_conv_args(op, B, F, E, kernels, pools, route, c_in)
    else:
        B, F, E = int(x.shape[0]), int(fields), int(dim)
        a, arrs, channels, rows_out = _field_conv_args(op, B, F, E, kernels, pools, route)
        a.x_stride, a.x_offset = _rows2d(op, "x (with fields / dim)", x, B, F * E * a.in_channels, x_offset), int(x_offset)
    flat = []
    for s, (kern, bias) in enumerate(zip(kernels, biases)):
        if kern.dtype != torch.float32 or not kern.is_contiguous():
            raise ValueError("field_conv: stage %d kernel must be a contiguous float32 tensor" % s)
        _vec(op, "stage %d bias" % s, bias, channels[s])
        flat += [kern, bias]
    widths_out = [r * E * c for r, c in zip(rows_out, channels)]
    ret = out
    if out is None:
        ret = torch.empty((B, rows_out[-1], E, channels[-1]), dtype=torch.float32, device=x.device)
        out = ret.view(B, -1)
    a.out_stride, a.out_offset = _rows2d(op, "out", out, B, widths_out[-1], out_offset), int(out_offset)
    souts = None
    if stage_outs is not None and stage_outs is not False:
        if stage_outs is True:
            souts = [torch.empty((B, r, E, c), dtype=torch.float32, device=x.device) for r, c in zip(rows_out, channels)]
        else:
            souts = list(stage_outs)
            if len(souts) != len(kernels):
                raise ValueError("field_conv: stage_outs needs one entry per stage, got %d for %d" % (len(souts), len(kernels)))
        strides = []
        for s, t in enumerate(souts):
            if t is None:
                strides.append(0)
            elif t.dim() == 4 and t.is_contiguous() and t.dtype == torch.float32 and tuple(t.shape) == (B, rows_out[s], E, channels[s]):
                strides.append(widths_out[s])
            else:
                strides.append(_rows2d(op, "stage_outs[%d]" % s, t, B, widths_out[s]))
        sp, ss = _ptr_array(souts), _i64_array(strides)
        a.stage_outs, a.stage_out_strides = ctypes.cast(sp, ctypes.c_void_p), ctypes.cast(ss, ctypes.c_void_p)
    _dev_check(x, out, *flat, *(souts or ()))
    kp, bp = _ptr_array(flat[0::2]), _ptr_array(flat[1::2])
    a.kernels, a.biases = ctypes.cast(kp, ctypes.c_void_p), ctypes.cast(bp, ctypes.c_void_p)
    a.x, a.out = x.data_ptr(), out.data_ptr()
    _workspace(op, a, int(_C.lib().dctr_fieldconv_workspace_bytes(ctypes.byref(a))), workspace, x.device)
    _C.check(_C.lib().dctr_fieldconv_fwd(ctypes.byref(a), _C.stream_ptr()), "dctr_fieldconv_fwd")
    del kp, bp, arrs
    return ret if souts is None else (ret, souts)


def kmax_pool(x, k, axis=-1):
    """KMaxPooling.call (reference sequence.py:853-864): the ``k`` largest values along ``axis`` of a tensor of any rank, in descending
    order of value (tf.nn.top_k(sorted=True)); the other axes keep their place."""
    nd = x.dim()
    if nd < 1 or not -nd <= int(axis) < nd:
        raise ValueError("kmax_pool: axis %d outside a tensor of %d dimensions" % (axis, nd))
    axis = int(axis) % nd
    n, k = int(x.shape[axis]), int(k)
    if not 1 <= k <= n:
        raise ValueError("k must be in 1 ~ %d,now k is %d" % (n, k))
    _dev_check(x)
    x = _f32c(x, "x")
    outer = int(np.prod(x.shape[:axis], dtype=np.int64))
    inner = int(np.prod(x.shape[axis + 1:], dtype=np.int64))
    y = torch.empty(tuple(x.shape[:axis]) + (k,) + tuple(x.shape[axis + 1:]), dtype=torch.float32, device=x.device)
    _C.check(_C.lib().dctr_kmax_pool_fwd(_ptr(x), outer, n, inner, k, _ptr(y), _C.stream_ptr()), "dctr_kmax_pool_fwd")
    return y


def afm(x, attention_W, attention_b, projection_h, projection_p, fields=None, dim=None, out=None):
    """AFMLayer.call (reference interaction.py:116-146), inference: x [B,F,E] -> [B,1].
    With ``fields``/``dim`` x is a 2-D buffer [B, stride >= fields*dim] read in place (a slice of dnn_in)."""
    _dev_check(x, attention_W, attention_b, projection_h, projection_p)
    x, B, F, E, stride, _ = _x_in_place("afm", x, fields, dim)
    A = attention_W.shape[1]
    y = torch.empty(B, 1, dtype=torch.float32, device=x.device) if out is None else out
    _C.check(_C.lib().dctr_afm_fwd(_ptr(x), B, stride, F, E, _ptr(_f32c(attention_W, "W")), _ptr(_f32c(attention_b, "b")),
                                   _ptr(_f32c(projection_h, "h").reshape(-1)), _ptr(_f32c(projection_p, "p").reshape(-1)),
                                   A, _ptr(y), _C.stream_ptr()), "dctr_afm_fwd")
    return y


_SCRATCH = {}


def _scratch(device, nbytes):
    """Per-device scratch buffer (grown on demand) for kernels whose workspace is rewritten by every call; stream order
    keeps successive calls on one stream from overlapping."""
    key = (device.type, device.index, torch.cuda.current_stream(device).cuda_stream)
    buf = _SCRATCH.get(key)
    if buf is None or buf.numel() * 4 < nbytes:
        buf = _SCRATCH[key] = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=device)
    return buf


def crossnet_mix(x, U, V, C, gating, bias, dim=None, out=None):
    """CrossNetMix.call (reference interaction.py:511-549): x [B, >= d]; U, V [L,experts,d,r]; C [L,experts,r,r];
    gating [experts,d]; bias [L,d].  ``out``: a 2-D (strided) view to write [B,d] into."""
    _dev_check(x, U, V, C, gating, bias)
    if x.dim() != 2:
        raise ValueError("Unexpected inputs dimensions %d, expect to be 2 dimensions" % x.dim())
    if x.dtype != torch.float32 or x.stride(1) != 1:
        x = _f32c(x, "x")
    d = x.shape[1] if dim is None else int(dim)
    L = 0 if U is None else U.shape[0]
    ne, r = (1, 1) if U is None else (U.shape[1], U.shape[3])
    if L:
        U, V, C, gating, bias = (_f32c(t, n) for t, n in ((U, "U"), (V, "V"), (C, "C"), (gating, "gating"), (bias, "bias")))
        if tuple(U.shape) != (L, ne, d, r) or tuple(V.shape) != (L, ne, d, r) or tuple(C.shape) != (L, ne, r, r) \
                or gating.numel() != ne * d or bias.numel() != L * d:
            raise ValueError("crossnet_mix: weight shapes do not match [L,experts,d,r] / [L,experts,r,r] / [experts,d] / [L,d]")
    y = torch.empty(x.shape[0], d, dtype=torch.float32, device=x.device) if out is None else out
    need = int(_C.lib().dctr_crossnet_mix_workspace_bytes(d, L, ne, r))
    ws = _scratch(x.device, need) if need else None
    _C.check(_C.lib().dctr_crossnet_mix_fwd(_ptr(x), x.shape[0], d, x.stride(0), _ptr(U), _ptr(V), _ptr(C), _ptr(gating),
                                            _ptr(bias), L, ne, r, _ptr(y), y.stride(0), _ptr(ws), need, _C.stream_ptr()),
             "dctr_crossnet_mix_fwd")
    return y


def bi_interaction(x, fields=None, dim=None, out=None):
    """BiInteractionPooling.call (reference interaction.py:190-203): x [B,F,E] -> [B,1,E]; with ``fields``/``dim`` x is a
    2-D buffer read in place and ``out`` a 2-D (strided) view to write [B,E] into."""
    _dev_check(x)
    x, B, F, E, xs, _ = _x_in_place("bi_interaction", x, fields, dim)
    if out is None:
        y = torch.empty(B, 1, E, dtype=torch.float32, device=x.device)
        ys = E
    else:
        y, ys = out, out.stride(0)
    _C.check(_C.lib().dctr_bi_interaction_fwd(_ptr(x), B, xs, F, E, _ptr(y), ys, _C.stream_ptr()), "dctr_bi_interaction_fwd")
    return y


def inner_product(x, reduce_sum=True, fields=None, dim=None, out=None):
    """InnerProductLayer.call (reference interaction.py:655-678): x [B,F,E] -> [B,P,1] or [B,P,E].
    With ``fields``/``dim`` x is a 2-D buffer read in place; ``out`` may be a 2-D (strided) view to write into."""
    _dev_check(x)
    x, B, F, E, xs, _ = _x_in_place("inner_product", x, fields, dim)
    P = F * (F - 1) // 2
    if out is None:
        y = torch.empty(B, P, 1 if reduce_sum else E, dtype=torch.float32, device=x.device)
        ys = P * (1 if reduce_sum else E)
    else:
        y, ys = out, out.stride(0)
    _C.check(_C.lib().dctr_inner_product_fwd(_ptr(x), B, xs, F, E, int(bool(reduce_sum)), _ptr(y), ys, _C.stream_ptr()),
             "dctr_inner_product_fwd")
    return y


def crossnet_fold_consts(kernels, bias, head, out=None):
    """The row-independent constants of the folded vector CrossNet (dctr_crossnet_fold_consts): float[4] for ``mlp(cross=(.., consts))``."""
    _dev_check(kernels, bias, head)
    kernels, bias, head = _f32c(kernels, "kernels"), _f32c(bias, "bias"), _f32c(head, "head")
    if out is None:
        out = torch.zeros(4, dtype=torch.float32, device=kernels.device)
    _C.check(_C.lib().dctr_crossnet_fold_consts(_ptr(kernels), _ptr(bias), _ptr(head), int(kernels.shape[0]), int(kernels.shape[1]), _ptr(out),
                                                _C.stream_ptr()), "dctr_crossnet_fold_consts")
    return out


# ---------------------------------------------------------------------------------------------
# adjacent: DNN (+ head), DIN attention
# ---------------------------------------------------------------------------------------------
_ONES = {}
_MLP_SCRATCH = {}
_MLP_SCRATCH_MAX = 1 << 29      # 512 MiB: the layer-by-layer DNN walks the rows in chunks of what its scratch holds


def _mlp_scratch(device, nbytes):
    """Per-device scratch of the layer-by-layer DNN route (grown on demand; launches on one stream are ordered, so one buffer serves)."""
    t = _MLP_SCRATCH.get(device)
    if t is None or t.numel() * 4 < nbytes:
        t = _MLP_SCRATCH[device] = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=device)
    return t


def mlp_fwd_supported(gather, m, add_fm_logit=False, add_lin_logit=False):
    """dctr_mlp_fwd_supported: would the library take this (fused, when ``gather`` is given) DNN launch?  The host asks; it does not
    re-derive the library's LDS / instantiation limits."""
    return bool(_C.lib().dctr_mlp_fwd_supported(None if gather is None else ctypes.byref(gather), ctypes.byref(m), int(bool(add_fm_logit)),
                                                int(bool(add_lin_logit))))


def _dnn_act_code(op, activation):
    """DCTR_ACT_* of a DNN activation name: relu / sigmoid / tanh / linear / dice and the tf.keras 2.x names elu, selu, softplus, softsign,
    exponential, hard_sigmoid, swish (= silu), gelu (the DNN entry points take them: include/dctr.h)."""
    try:
        return _C.DNN_ACT_CODES[activation]
    except (KeyError, TypeError):
        raise ValueError("%s: unknown activation %r" % (op, activation))


def mlp(x, kernels, biases, activation="relu", dice=None, dice_eps=1e-9, head_w=None, add=(), global_bias=None,
        sigmoid_out=False, in_dim=None, out=None, gather=None, add_fm_logit=False, add_lin_logit=False, batch=None,
        tile_rows=0, save_acts=None, probe=None, launch=True, bn=None, precision=0, workspace=None, cross=None):
    """DNN.call (reference core.py:189-208) for x [B, >=in_dim]; optional fused head:
    logit = h . head_w + sum(add) + global_bias, sigmoid (Dense(1) + add_func + PredictionLayer).
    ``activation``: relu / sigmoid / tanh / linear / dice, or a tf.keras 2.x name (elu, selu, softplus, softsign, exponential,
    hard_sigmoid, swish = silu, gelu: every route but the row-chained and streaming kernels, which decline them).
    ``dice`` = list of (alpha, moving_mean, moving_variance) per layer when activation == 'dice'.
    ``bn`` = list of (scale, shift) per layer (or None) for DNN(use_bn=True): inference BatchNormalization between bias_add
    and the activation, see dctr_mlp_args_t.bn_scale.
    ``tile_rows`` (0 = auto, 16, 32, 64; with a fused gather also 128 / 256 = the row-chained kernel) is the batch rows per
    workgroup — a throughput/latency knob.
    ``cross`` = (kernels [L, in_dim], bias [L, in_dim], head [in_dim]): CrossNet in its vector parameterization over the row the
    DNN reads (reference interaction.py:405-424) folded into the launch; the head adds x_L . head (dctr_mlp_args_t.cross_*)."""
    _dev_check(x, *kernels, *biases)
    if gather is None:
        if x.dim() != 2:
            raise ValueError("mlp expects a 2-D input")
        if x.dtype != torch.float32 or x.stride(1) != 1:
            x = _f32c(x, "x")
        B = x.shape[0]
        in_dim = x.shape[1] if in_dim is None else in_dim
    else:       # fused path: the input tile is gathered inside the kernel (dctr_embed_mlp_fwd)
        B = int(batch)
    n = len(kernels)
    units = [k.shape[1] for k in kernels]
    kernels = [_f32c(k, "kernel") for k in kernels]
    biases = [None if b is None else _f32c(b, "bias") for b in biases]
    act = _dnn_act_code("mlp", activation)
    has_head = head_w is not None
    last = units[-1] if n else in_dim
    if out is None:
        dev_t = x if x is not None else (kernels[0] if kernels else head_w)
        out = torch.empty((B,) if has_head else (B, last), dtype=torch.float32, device=dev_t.device)
    add = [a_ for a_ in add if a_ is not None]
    while len(add) > 4:
        # the fused head adds up to four extra logit vectors (DeepFM(fm_group=...) over many groups has more: linear + one FM logit per
        # group, models/deepfm.py:53-57): the surplus is summed by the head itself — its no-hidden-layer form, x . 1 + sum(add) — five
        # vectors into one per launch
        v = add[-5:]
        one = _ONES.get(v[0].device)
        if one is None:
            one = _ONES[v[0].device] = torch.ones(1, 1, dtype=torch.float32, device=v[0].device)
        folded = mlp(_f32c(v[0], "add").reshape(-1, 1), [], [], "linear", head_w=one, add=v[1:], in_dim=1)
        add = add[:-5] + [folded]
    add_arr = (ctypes.c_void_p * 4)()
    for i_, t_ in enumerate(add):
        add_arr[i_] = t_.data_ptr()
    keep = [kernels, biases]
    da = dm = dv = None
    if act == _C.ACT_DICE and n > 0:
        da = _ptr_array([_f32c(d[0], "alpha") for d in dice])
        dm = _ptr_array([_f32c(d[1], "mean") for d in dice])
        dv = _ptr_array([_f32c(d[2], "var") for d in dice])
    ua, kp, bp = _i32_array(units), _ptr_array(kernels), _ptr_array(biases)
    a = _C.MlpArgs(x=None if gather is not None else x.data_ptr(), batch=B,
                   x_stride=0 if gather is not None else x.stride(0), in_dim=in_dim, n_layers=n,
                   units=ctypes.cast(ua, ctypes.c_void_p), kernels=ctypes.cast(kp, ctypes.c_void_p),
                   biases=ctypes.cast(bp, ctypes.c_void_p), activation=act, has_head=int(has_head),
                   dice_alpha=None if da is None else ctypes.cast(da, ctypes.c_void_p),
                   dice_mean=None if dm is None else ctypes.cast(dm, ctypes.c_void_p),
                   dice_var=None if dv is None else ctypes.cast(dv, ctypes.c_void_p), dice_eps=float(dice_eps),
                   sigmoid_out=int(bool(sigmoid_out)),
                   head_w=None if head_w is None else _f32c(head_w, "head_w").data_ptr(),
                   add=add_arr,
                   global_bias=None if global_bias is None else global_bias.data_ptr(), y=out.data_ptr(),
                   y_stride=0 if has_head else out.stride(0), workspace=None, workspace_bytes=0,
                   tile_rows=int(tile_rows), precision=int(precision))
    if workspace is not None:           # caller-provided scratch of the layer-by-layer route (dctr_mlp_workspace_bytes)
        a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
        keep.append(workspace)
    if probe is not None:               # measurement aid: uint64[2] {min start, max end} wall-clock stamps (dctr.h)
        a.probe = probe.data_ptr()
    if bn is not None and n > 0 and any(b_ is not None for b_ in bn):
        bsc = _ptr_array([None if b_ is None else _f32c(b_[0], "bn_scale") for b_ in bn])
        bsh = _ptr_array([None if b_ is None else _f32c(b_[1], "bn_shift") for b_ in bn])
        keep.append((bsc, bsh, bn))
        a.bn_scale, a.bn_shift = ctypes.cast(bsc, ctypes.c_void_p), ctypes.cast(bsh, ctypes.c_void_p)
    if cross is not None:
        cw, cb, ch = (_f32c(t_, "cross") for t_ in cross[:3])
        if cw.dim() != 2 or cw.shape != cb.shape or cw.shape[1] != in_dim or ch.numel() != in_dim:
            raise ValueError("cross = (kernels [L, in_dim], bias [L, in_dim], head [in_dim][, consts [4] from crossnet_fold_consts])")
        keep.append((cw, cb, ch))
        a.cross_w, a.cross_b, a.cross_head, a.cross_layers = cw.data_ptr(), cb.data_ptr(), ch.data_ptr(), int(cw.shape[0])
        if len(cross) > 3 and cross[3] is not None:
            keep.append(cross[3])
            a.cross_const = cross[3].data_ptr()
    if save_acts is not None:           # training: layer outputs [B, units[l]] also go to HBM (dctr_mlp_bwd reads them)
        sa = _ptr_array(list(save_acts))
        keep.append(sa)
        a.save_acts = ctypes.cast(sa, ctypes.c_void_p)
    if not launch:                      # caller keeps the marshalled arguments and launches itself (per-batch fast path)
        return a, (keep, ua, kp, bp, da, dm, dv, add_arr, add, head_w, global_bias, out)
    if gather is None and workspace is None and precision == 0 and n > 0:
        # a layer wider than any LDS tile: the library runs the DNN layer by layer through two activation buffers it asks for (0 otherwise)
        need = int(_C.lib().dctr_mlp_workspace_bytes(ctypes.byref(a)))
        if need > 0:
            ws_t = _mlp_scratch(out.device, min(need, _MLP_SCRATCH_MAX))
            a.workspace, a.workspace_bytes = ws_t.data_ptr(), ws_t.numel() * 4
            keep.append(ws_t)
    if gather is not None:
        _C.check(_C.lib().dctr_embed_mlp_fwd(ctypes.byref(gather), ctypes.byref(a), int(bool(add_fm_logit)),
                                             int(bool(add_lin_logit)), _C.stream_ptr()), "dctr_embed_mlp_fwd")
    else:
        _C.check(_C.lib().dctr_mlp_fwd(ctypes.byref(a), _C.stream_ptr()), "dctr_mlp_fwd")
    del keep
    return out


def din_attention(query, keys, key_mask, kernels, biases, out_kernel, out_bias, activation="sigmoid", dice=None,
                  dice_eps=1e-9, weight_normalization=False, return_score=False, out=None, out_stride=None,
                  workspace=True, compact=True):
    """AttentionSequencePoolingLayer.call (reference sequence.py:261-298): query [B,1,E] / [B,E], keys [B,T,E],
    key_mask [B,T] (bool/uint8) -> [B,1,E] (or the scores [B,1,T]).  ``workspace=False`` withholds the [B*T]
    scratch and thereby selects the one-workgroup-per-sample kernel (see include/dctr.h); ``compact=False`` hands over the [B*T]
    floats only, without the row-list area: every position is scored, masked or not (A/B of the compaction)."""
    _dev_check(query, keys, key_mask, out_kernel, out_bias)
    keys = _f32c(keys, "keys")
    B, T, E = keys.shape
    query = _f32c(query, "query").reshape(B, E)
    mask = key_mask.to(torch.uint8).reshape(B, T).contiguous()
    n = len(kernels)
    units = [k.shape[1] for k in kernels]
    kernels = [_f32c(k, "kernel") for k in kernels]
    biases = [None if b is None else _f32c(b, "bias") for b in biases]
    act = _C.ACT_CODES[activation]
    own_out = out is None
    if own_out:
        out = torch.empty(B, E, dtype=torch.float32, device=keys.device)
        out_stride = E
    scores = torch.empty(B, T, dtype=torch.float32, device=keys.device) if return_score else None
    da = dm = dv = None
    if act == _C.ACT_DICE and n > 0:
        da = _ptr_array([_f32c(d[0], "alpha") for d in dice])
        dm = _ptr_array([_f32c(d[1], "mean") for d in dice])
        dv = _ptr_array([_f32c(d[2], "var") for d in dice])
    ua, kp, bp = _i32_array(units), _ptr_array(kernels), _ptr_array(biases)
    a = _C.DinAttnArgs(query=query.data_ptr(), keys=keys.data_ptr(), key_mask=mask.data_ptr(), batch=B, maxlen=T, dim=E,
                       n_layers=n, activation=act, units=ctypes.cast(ua, ctypes.c_void_p),
                       kernels=ctypes.cast(kp, ctypes.c_void_p), biases=ctypes.cast(bp, ctypes.c_void_p),
                       dice_alpha=None if da is None else ctypes.cast(da, ctypes.c_void_p),
                       dice_mean=None if dm is None else ctypes.cast(dm, ctypes.c_void_p),
                       dice_var=None if dv is None else ctypes.cast(dv, ctypes.c_void_p), dice_eps=float(dice_eps),
                       weight_normalization=int(bool(weight_normalization)),
                       out_kernel=_f32c(out_kernel, "out_kernel").reshape(-1).data_ptr(),
                       out_bias=_f32c(out_bias, "out_bias").data_ptr(), out=out.data_ptr(), out_stride=out_stride,
                       scores=None if scores is None else scores.data_ptr())
    if workspace:                      # [B*T] raw scores: enables the weights-in-LDS row kernel (include/dctr.h)
        need = int(_C.lib().dctr_din_attn_workspace_bytes(ctypes.byref(a))) if compact else B * T * 4
        ws = torch.empty(max(1, (need + 3) // 4), dtype=torch.float32, device=keys.device)
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    rc = _C.lib().dctr_din_attn_pool_fwd(ctypes.byref(a), _C.stream_ptr())
    if rc == _C.E_UNSUPPORTED:
        # a key width / attention MLP the on-chip kernels do not hold (e.g. three 32-wide history features: [q, k, q - k, q * k] is 384
        # wide, two 64-position tiles of it exceed the LDS): the materialised route of the training forward — [B*T, 4E] in HBM,
        # dctr_mlp_fwd (any width), masked (softmax-ed) weighted sum — samples in chunks of <= 256 MB of attention input
        step = max(1, (1 << 26) // max(1, T * 4 * E))
        for lo in range(0, B, step):
            hi = min(B, lo + step)
            att_in = torch.empty((hi - lo) * T, 4 * E, dtype=torch.float32, device=keys.device)
            din_att_in(query[lo:hi], keys[lo:hi], att_in)
            score = mlp(att_in, kernels, biases, activation, dice=dice, dice_eps=dice_eps, head_w=_f32c(out_kernel, "out_kernel").reshape(-1, 1),
                        global_bias=out_bias, in_dim=4 * E)
            m_ = mask[lo:hi]
            o_ = out[lo:hi] if out.dim() == 2 else out[lo:hi].reshape(hi - lo, -1)
            if weight_normalization:
                prob = din_softmax(score, m_, torch.empty_like(score))
                din_wsum(prob, torch.ones_like(m_), keys[lo:hi], o_)
                if scores is not None:
                    scores[lo:hi].copy_(prob.view(hi - lo, T))
            else:
                din_wsum(score, m_, keys[lo:hi], o_)
                if scores is not None:           # (the eager layer API only: the masked raw scores)
                    scores[lo:hi].copy_(torch.where(m_ != 0, score.view(hi - lo, T), torch.zeros((), device=score.device)))
    else:
        _C.check(rc, "dctr_din_attn_pool_fwd")
    if return_score:
        return scores.reshape(B, 1, T)
    return out.reshape(B, 1, E) if own_out else out


def din_attention_gather(hist_ids, query_ids, hist_tables, query_tables, mask_zero, kernels, biases, out_kernel, out_bias, activation="sigmoid",
                         dice=None, dice_eps=1e-9, weight_normalization=False, out=None, out_stride=None, status=None, compact=True):
    """AttentionSequencePoolingLayer.call with the query / key lookups folded in (dctr_din_attn_gather_fwd): ``hist_ids`` = list of
    [B, T] id tensors (one per history feature, int32 or int64 alike), ``query_ids`` = list of [B] id tensors (strided views
    allowed), ``*_tables`` = the features' [vocab, E_h] embedding tables, ``mask_zero`` = per feature whether id 0 masks the
    position.  Returns out [B, sum E_h], or None when the shape is outside the fused kernels (caller falls back to the lookups)."""
    nf = len(hist_ids)
    if nf < 1 or nf > 2 or len(query_ids) != nf:
        return None
    EH = hist_tables[0].shape[1]
    E = EH * nf
    if any(t.shape[1] != EH for t in list(hist_tables) + list(query_tables)) or EH % 16 != 0 or E not in (16, 32, 64) or len(kernels) != 2:
        return None
    B, T = hist_ids[0].shape
    i64 = hist_ids[0].dtype == torch.int64
    if any(t.dtype != hist_ids[0].dtype or t.stride(1) != 1 or t.stride(0) != hist_ids[0].stride(0) for t in hist_ids):
        return None
    if any(t.dtype != hist_ids[0].dtype or t.stride(0) != query_ids[0].stride(0) for t in query_ids):
        return None
    units = [k.shape[1] for k in kernels]
    kernels = [_f32c(k, "kernel") for k in kernels]
    biases = [None if b is None else _f32c(b, "bias") for b in biases]
    act = _C.ACT_CODES[activation]
    if out is None:
        out = torch.empty(B, E, dtype=torch.float32, device=hist_tables[0].device)
        out_stride = E
    da = dm = dv = None
    if act == _C.ACT_DICE:
        da = _ptr_array([_f32c(d[0], "alpha") for d in dice])
        dm = _ptr_array([_f32c(d[1], "mean") for d in dice])
        dv = _ptr_array([_f32c(d[2], "var") for d in dice])
    ua, kp, bp = _i32_array(units), _ptr_array(kernels), _ptr_array(biases)
    a = _C.DinAttnArgs(query=None, keys=None, key_mask=None, batch=B, maxlen=T, dim=E, n_layers=2, activation=act,
                       units=ctypes.cast(ua, ctypes.c_void_p), kernels=ctypes.cast(kp, ctypes.c_void_p),
                       biases=ctypes.cast(bp, ctypes.c_void_p),
                       dice_alpha=None if da is None else ctypes.cast(da, ctypes.c_void_p),
                       dice_mean=None if dm is None else ctypes.cast(dm, ctypes.c_void_p),
                       dice_var=None if dv is None else ctypes.cast(dv, ctypes.c_void_p), dice_eps=float(dice_eps),
                       weight_normalization=int(bool(weight_normalization)),
                       out_kernel=_f32c(out_kernel, "out_kernel").reshape(-1).data_ptr(),
                       out_bias=_f32c(out_bias, "out_bias").data_ptr(), out=out.data_ptr(), out_stride=out_stride, scores=None)
    # [B*T] raw scores + the list of the positions that count (compact=False: the scores only, every position is scored)
    need = int(_C.lib().dctr_din_attn_workspace_bytes(ctypes.byref(a))) if compact else B * T * 4
    ws = torch.empty(max(1, (need + 3) // 4), dtype=torch.float32, device=out.device)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    g = _C.DinGatherArgs(n_feats=nf, ids_is_i64=int(i64), hist_stride=hist_ids[0].stride(0), query_stride=query_ids[0].stride(0),
                         status=None if status is None else status.data_ptr())
    for h in range(nf):
        g.hist_ids[h] = hist_ids[h].data_ptr()
        g.query_ids[h] = query_ids[h].data_ptr()
        g.hist_table[h] = _f32c(hist_tables[h], "table").data_ptr()
        g.query_table[h] = _f32c(query_tables[h], "table").data_ptr()
        g.hist_vocab[h] = hist_tables[h].shape[0]
        g.query_vocab[h] = query_tables[h].shape[0]
        g.mask_zero[h] = int(bool(mask_zero[h]))
    rc = _C.lib().dctr_din_attn_gather_fwd(ctypes.byref(a), ctypes.byref(g), _C.stream_ptr())
    if rc == _C.E_UNSUPPORTED:
        return None
    _C.check(rc, "dctr_din_attn_gather_fwd")
    return out


# ---------------------------------------------------------------------------------------------
# backward + optimizer (include/dctr.h, last section)
# ---------------------------------------------------------------------------------------------
def bce_grad(pred, y, dlogit, loss_sum=None, dlogit_sum=None, task="binary", weight=None):
    """d(mean loss)/d(logit) for PredictionLayer + binary_crossentropy (or mse); the optional device floats accumulate
    the summed loss and the summed dlogit (= gradient of the global bias).  ``weight`` [B] float32: tf.keras' per-sample
    weights (loss = sum w_b l_b / B)."""
    _dev_check(pred, y, dlogit)
    if weight is not None:
        _dev_check(weight)
        if weight.dtype != torch.float32 or weight.numel() != pred.numel() or not weight.is_contiguous():
            raise ValueError("bce_grad: weight must be a contiguous float32 tensor of the batch's length")
    _C.check(_C.lib().dctr_bce_grad_w(_ptr(pred), _ptr(y), _ptr(weight), pred.numel(), 0 if task == "binary" else 1, _ptr(dlogit),
                                      _ptr(loss_sum), _ptr(dlogit_sum), _C.stream_ptr()), "dctr_bce_grad_w")


def make_field_grads(entries, device):
    """DEVICE array of dctr_field_grad_t from [(g_table or None, g_lin_table or None[, touched bytes or None]), ...]."""
    arr = (_C.FieldGrad * max(1, len(entries)))()
    for i, e in enumerate(entries):
        gt, gl = e[0], e[1]
        tch = e[2] if len(e) > 2 else None
        arr[i].g_table = None if gt is None else gt.data_ptr()
        arr[i].g_lin_table = None if gl is None else gl.data_ptr()
        arr[i].touched = None if (tch is None or gt is None) else tch.data_ptr()
    host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
    return host.to(device)


def embed_gather_fm_bwd(fwd_args, grads_dev, d_dnn_in=None, d_fm=None, d_lin=None, g_dense_lin_w=None, dense_lin_rows=None):
    """Backward of dctr_embed_gather_fm: row gradients are atomically added into the dense gradient tables."""
    a = _C.GatherFmBwdArgs(fwd=ctypes.pointer(fwd_args), grads=grads_dev.data_ptr(),
                           d_dnn_in=None if d_dnn_in is None else d_dnn_in.data_ptr(),
                           d_stride=0 if d_dnn_in is None else d_dnn_in.stride(0),
                           d_fm=None if d_fm is None else d_fm.data_ptr(), d_lin=None if d_lin is None else d_lin.data_ptr(),
                           g_dense_lin_w=None if g_dense_lin_w is None else g_dense_lin_w.data_ptr(),
                           dense_lin_rows=None if dense_lin_rows is None else dense_lin_rows.data_ptr())
    _C.check(_C.lib().dctr_embed_gather_fm_bwd(ctypes.byref(a), _C.stream_ptr()), "dctr_embed_gather_fm_bwd")


def _bwd_workspace(workspace, need, device):
    """The float32 workspace of a backward op: a fresh tensor per call, or with ``workspace`` (a dict the caller keeps alive, as
    ``mlp_bwd`` and ``cin_bwd`` take it) the tensor cached under "ws", replaced only when it is missing, on another device or smaller
    than ``need`` bytes."""
    if workspace is not None:
        ws = workspace.get("ws")
        if ws is None or ws.dtype != torch.float32 or not ws.is_contiguous() or ws.numel() * 4 < need or ws.device != device:
            ws = workspace["ws"] = torch.empty(max(1, need // 4), dtype=torch.float32, device=device)
        return ws
    return torch.empty(max(1, need // 4), dtype=torch.float32, device=device)


def crossnet_mix_bwd_supported(dim, layers, experts, low_rank):
    """Does dctr_crossnet_mix_bwd take these sizes (at most 16 experts; the forward takes any number)?"""
    return bool(_C.lib().dctr_crossnet_mix_bwd_supported(int(dim), int(layers), int(experts), int(low_rank)))


def crossnet_mix_bwd(x, dim, packed, dy, grads, dx, accumulate=False, workspace=None):
    """Backward of crossnet_mix: ``packed`` = (U, V, C, gating, bias) as the forward takes them, ``grads`` the same five shapes
    (accumulated into), dy [B, >= dim] gradient w.r.t. the output, dx [B, >= dim] written (or added to).  ``workspace``: a dict the
    caller keeps alive, as ``cin_bwd`` takes it (default: a fresh tensor per call)."""
    U, V, C, gating, bias = packed
    dU, dV, dC, dG, dB = grads
    _dev_check(x, dy, dx, U, V, C, gating, bias, dU, dV, dC, dG, dB)
    L, ne, r = (U.shape[0], U.shape[1], U.shape[3]) if U.dim() == 4 and U.shape[0] else (0, max(int(gating.shape[0]), 1), 1)
    a = _C.CrossMixBwdArgs(x=x.data_ptr(), x_stride=x.stride(0), batch=x.shape[0], dim=dim, layers=L, experts=ne, low_rank=r,
                           U=_ptr(U), V=_ptr(V), C=_ptr(C), gating=_ptr(gating), bias=_ptr(bias), dy=dy.data_ptr(),
                           dy_stride=dy.stride(0), dU=_ptr(dU), dV=_ptr(dV), dC=_ptr(dC), dgating=_ptr(dG), dbias=_ptr(dB),
                           dx=dx.data_ptr(), dx_stride=dx.stride(0), dx_accumulate=int(bool(accumulate)))
    need = int(_C.lib().dctr_crossnet_mix_bwd_workspace_bytes(ctypes.byref(a))) if L else x.shape[0] * dim * 4
    ws = _bwd_workspace(workspace, need, x.device)
    a.workspace, a.workspace_bytes = ws.data_ptr(), need
    _C.check(_C.lib().dctr_crossnet_mix_bwd(ctypes.byref(a), _C.stream_ptr()), "dctr_crossnet_mix_bwd")


def dice_train_fwd(z, alpha, moving_mean, moving_var, out, eps=1e-9, momentum=0.99, bias=None):
    """Dice under training=True on pre-activations z [R, n] (2-D, possibly strided): batch statistics (returned as
    (batch_mean, batch_var)), stored statistics moved in place, activations written to ``out`` (dctr_dice_train_fwd)."""
    _dev_check(z, alpha, moving_mean, moving_var, out, bias)
    R, n = z.shape
    bm = torch.empty(n, dtype=torch.float32, device=z.device)
    bv = torch.empty(n, dtype=torch.float32, device=z.device)
    _C.check(_C.lib().dctr_dice_train_fwd(_ptr(z), z.stride(0), _ptr(bias), R, n, _ptr(_f32c(alpha, "alpha")), float(eps), float(momentum),
                                          _ptr(moving_mean), _ptr(moving_var), _ptr(bm), _ptr(bv), _ptr(out), out.stride(0),
                                          _C.stream_ptr()), "dctr_dice_train_fwd")
    return bm, bv


def dnn_train_layer(z, activation, h=None, bn=None, dropout_rate=0.0, dropout_seed=0, dh=None, dz=None, d_gamma=None, d_beta=None):
    """One DNN layer under training=True behind its dense part (dctr_dnn_train_layer_fwd / _bwd; reference layers/core.py:196-208):
    z [R, n] = x W + b -> BatchNormalization(training) -> activation -> Dropout(training).
    Forward (``h`` given, a 2-D possibly strided [R, n] view): writes h; with ``bn`` = dict(gamma, beta, moving_mean, moving_var,
    eps, momentum, batch_mean, batch_var) the batch statistics are written to batch_mean / batch_var and the stored ones moved.
    Backward (``dh`` given): dz [R, n] contiguous (may be dh itself) from dh, the same ``bn`` dict (batch statistics as the forward left
    them) and the same dropout_rate / dropout_seed; d_gamma / d_beta are accumulated."""
    R, n = z.shape
    act = _dnn_act_code("dnn_train_layer", activation)
    if act == _C.ACT_DICE:
        raise ValueError("dnn_train_layer: activation 'dice' has its own training form (dice_train_fwd)")
    a = _C.DnnTrainLayer(z=z.data_ptr(), z_stride=z.stride(0), rows=R, n=n, activation=act,
                         dropout_rate=float(dropout_rate), dropout_seed=int(dropout_seed) & 0xFFFFFFFFFFFFFFFF)
    keep = [z]
    if bn is not None:
        a.use_bn, a.bn_eps, a.bn_momentum = 1, float(bn["eps"]), float(bn["momentum"])
        a.bn_gamma, a.bn_beta = _ptr(bn.get("gamma")), _ptr(bn.get("beta"))
        a.bn_moving_mean, a.bn_moving_var = _ptr(bn.get("moving_mean")), _ptr(bn.get("moving_var"))
        a.bn_batch_mean, a.bn_batch_var = _ptr(bn["batch_mean"]), _ptr(bn["batch_var"])
    if dh is None:
        _dev_check(z, h)
        a.h, a.h_stride = h.data_ptr(), h.stride(0)
        _C.check(_C.lib().dctr_dnn_train_layer_fwd(ctypes.byref(a), _C.stream_ptr()), "dctr_dnn_train_layer_fwd")
        return h
    _dev_check(z, dh, dz)
    if not dz.is_contiguous() or tuple(dz.shape) != (R, n):
        raise ValueError("dnn_train_layer: dz must be a contiguous [%d, %d] tensor" % (R, n))
    a.dh, a.dh_stride, a.dz = dh.data_ptr(), dh.stride(0), dz.data_ptr()
    a.d_gamma, a.d_beta = _ptr(d_gamma), _ptr(d_beta)
    if bn is not None:
        ws = _scratch(z.device, 2 * n * 4)
        a.workspace = ws.data_ptr()
        keep.append(ws)
    _C.check(_C.lib().dctr_dnn_train_layer_bwd(ctypes.byref(a), _C.stream_ptr()), "dctr_dnn_train_layer_bwd")
    return dz


def mlp_bwd(x, in_dim, kernels, acts, activation, head_w, dlogit, d_kernels, d_biases, d_head_w, dx=None, d_out=None, biases=None,
            dice=None, d_dice_alpha=None, dice_eps=1e-9, dice_batch=None, dw_stream=None, workspace=None, saved_z=None):
    """Backward of dctr_mlp_fwd (+ head).  Gradients are ACCUMULATED into d_kernels / d_biases / d_head_w; dx is written.
    Headless form: head_w = dlogit = d_head_w = None and ``d_out`` [B, >= units[-1]] = gradient w.r.t. the last layer.
    activation "dice": ``biases`` and ``dice`` = [(alpha, mean, var)] per layer as in the forward; ``d_dice_alpha`` (list,
    accumulated) optional; activation "swish" / "gelu": ``biases`` (act' is taken from the pre-activations); ``dice_batch`` = [(batch_mean, batch_var)] per layer (dice_train_fwd) switches to training-mode Dice:
    the gradient flows through the batch statistics; ``saved_z`` = the layers' pre-activations (bias included) when a forward kept them.
    ``dw_stream`` (a torch.cuda.Stream) sends the weight-gradient launches of the chained form there (include/dctr.h); it needs a
    ``workspace`` the caller keeps alive (a dict: the tensor is cached under "ws") and a join by the caller."""
    _dev_check(x, *kernels)
    n = len(kernels)
    units = [k.shape[1] for k in kernels]
    ua, kp, ap = _i32_array(units), _ptr_array(kernels), _ptr_array(acts)
    dkp, dbp = _ptr_array(d_kernels), _ptr_array(d_biases)
    extra = {}
    act = _dnn_act_code("mlp_bwd", activation)
    if act in (_C.ACT_SWISH, _C.ACT_GELU):
        # act' needs the pre-activations, as Dice: saved_z when a forward kept them, else recomputed from the layer inputs and `biases`
        if biases is None and (saved_z is None or any(z is None for z in saved_z)):
            raise ValueError("mlp_bwd: activation %r needs the forward's biases (or saved_z of every layer)" % (activation,))
        if biases is not None:
            bp = _ptr_array([None if t is None else _f32c(t, "bias") for t in biases])
            extra = dict(biases=ctypes.cast(bp, ctypes.c_void_p))
    if activation in ("dice", "Dice"):
        if dice is None or biases is None:
            raise ValueError("mlp_bwd: activation 'dice' needs the forward's biases and dice parameters")
        bp = _ptr_array([None if t is None else _f32c(t, "bias") for t in biases])
        da, dm, dv = (_ptr_array([_f32c(d[i], "dice") for d in dice]) for i in range(3))
        gp = _ptr_array(list(d_dice_alpha)) if d_dice_alpha is not None else None
        extra = dict(biases=ctypes.cast(bp, ctypes.c_void_p), dice_alpha=ctypes.cast(da, ctypes.c_void_p),
                     dice_mean=ctypes.cast(dm, ctypes.c_void_p), dice_var=ctypes.cast(dv, ctypes.c_void_p),
                     d_dice_alpha=None if gp is None else ctypes.cast(gp, ctypes.c_void_p), dice_eps=float(dice_eps))
        if dice_batch is not None:
            bmp, bvp = (_ptr_array([_f32c(d[i], "dice batch statistics") for d in dice_batch]) for i in range(2))
            extra.update(dice_batch_mean=ctypes.cast(bmp, ctypes.c_void_p), dice_batch_var=ctypes.cast(bvp, ctypes.c_void_p))
    if act in _C.ACT_FROM_Z:
        if saved_z is not None:       # the forward's pre-activations (bias included), dense [B, units[l]]: no recompute GEMM
            for z, u in zip(saved_z, units):
                if z is not None and (z.dtype != torch.float32 or not z.is_contiguous() or z.shape[-1] != u or z.numel() != x.shape[0] * u):
                    raise ValueError("mlp_bwd: saved_z entries must be dense float32 [B, units[l]]")
            szp = _ptr_array(list(saved_z))
            extra.update(saved_z=ctypes.cast(szp, ctypes.c_void_p))
    a = _C.MlpBwdArgs(x=x.data_ptr(), batch=x.shape[0], x_stride=x.stride(0), in_dim=in_dim, n_layers=n,
                      units=ctypes.cast(ua, ctypes.c_void_p), kernels=ctypes.cast(kp, ctypes.c_void_p),
                      acts=ctypes.cast(ap, ctypes.c_void_p), activation=act,
                      head_w=None if head_w is None else head_w.data_ptr(),
                      dlogit=None if dlogit is None else dlogit.data_ptr(), d_kernels=ctypes.cast(dkp, ctypes.c_void_p),
                      d_biases=ctypes.cast(dbp, ctypes.c_void_p), d_head_w=None if d_head_w is None else d_head_w.data_ptr(),
                      dx=None if dx is None else dx.data_ptr(), dx_stride=0 if dx is None else dx.stride(0),
                      d_out=None if d_out is None else d_out.data_ptr(), d_out_stride=0 if d_out is None else d_out.stride(0),
                      **extra)
    need = int(_C.lib().dctr_mlp_bwd_workspace_bytes(ctypes.byref(a)))
    if workspace is not None:
        ws = workspace.get("ws")
        if ws is None or ws.numel() * 4 < need or ws.device != x.device:
            ws = workspace["ws"] = torch.empty(max(1, need // 4), dtype=torch.float32, device=x.device)
        if dw_stream is not None:
            a.dw_stream = dw_stream.cuda_stream
    else:
        if dw_stream is not None:
            raise ValueError("mlp_bwd: dw_stream needs a caller-owned workspace")
        ws = torch.empty(max(1, need // 4), dtype=torch.float32, device=x.device)
    a.workspace, a.workspace_bytes = ws.data_ptr(), need
    _C.check(_C.lib().dctr_mlp_bwd(ctypes.byref(a), _C.stream_ptr()), "dctr_mlp_bwd")


def din_att_in(q, k, out):
    """[q, k, q - k, q * k] per (sample, position): q [B,E], k [B,T,E] -> out [B*T, 4E] (include/dctr.h)."""
    _dev_check(q, k, out)
    B, T, E = k.shape
    _C.check(_C.lib().dctr_din_att_in_fwd(_ptr(_f32c(q, "q")), _ptr(_f32c(k, "k")), B, T, E, _ptr(out), _C.stream_ptr()),
             "dctr_din_att_in_fwd")
    return out


def din_wsum(score, mask, k, out):
    """out[b, :E] = sum_t (mask ? score : 0) k[b,t,:]; ``out`` a 2-D (strided) view."""
    _dev_check(score, mask, k, out)
    B, T, E = k.shape
    _C.check(_C.lib().dctr_din_wsum_fwd(_ptr(score), _ptr(mask), _ptr(k), B, T, E, _ptr(out), out.stride(0), _C.stream_ptr()),
             "dctr_din_wsum_fwd")
    return out


def fm_bwd(x, fields, dim, dlogit, dx, accumulate=True):
    """Backward of FM.call on a strided [B, >= F*E] slice of the DNN input: dx[b,f,:] (+)= dlogit[b] (sum_f' x[b,f',:] - x[b,f,:])."""
    _dev_check(x, dlogit, dx)
    _C.check(_C.lib().dctr_fm_bwd(_ptr(x), x.shape[0], x.stride(0), int(fields), int(dim), _ptr(dlogit), _ptr(dx), dx.stride(0),
                                  int(bool(accumulate)), _C.stream_ptr()), "dctr_fm_bwd")


def din_softmax(score, mask, out):
    """softmax over all T positions of where(mask, score, -2^32 + 1) (att_weight_normalization=True): score / out [B*T] or [B, T]."""
    _dev_check(score, mask, out)
    B, T = mask.shape
    _C.check(_C.lib().dctr_din_softmax_fwd(_ptr(score), _ptr(mask), B, T, _ptr(out), _C.stream_ptr()), "dctr_din_softmax_fwd")
    return out


def din_softmax_bwd(p, mask, dp, d_score, d_bias=None):
    _dev_check(p, mask, dp, d_score, d_bias)
    B, T = mask.shape
    _C.check(_C.lib().dctr_din_softmax_bwd(_ptr(p), _ptr(mask), _ptr(dp), B, T, _ptr(d_score), _ptr(d_bias), _C.stream_ptr()),
             "dctr_din_softmax_bwd")


def din_wsum_bwd(d_out, score, mask, k, d_score, dk, d_bias=None):
    _dev_check(d_out, score, mask, k, d_score, dk, d_bias)
    B, T, E = k.shape
    _C.check(_C.lib().dctr_din_wsum_bwd(_ptr(d_out), d_out.stride(0), _ptr(score), _ptr(mask), _ptr(k), B, T, E, _ptr(d_score),
                                        _ptr(dk), _ptr(d_bias), _C.stream_ptr()), "dctr_din_wsum_bwd")


def din_att_in_bwd(da, q, k, dk, dx, qcol):
    _dev_check(da, q, k, dk, dx, qcol)
    B, T, E = k.shape
    _C.check(_C.lib().dctr_din_att_in_bwd(_ptr(da), _ptr(q), _ptr(k), B, T, E, _ptr(dk), _ptr(dx), dx.stride(0), _ptr(qcol),
                                          _C.stream_ptr()), "dctr_din_att_in_bwd")


def embed_lookup_bwd(idx, table_shape, hash_mode, d_out, g_table, touched=None):
    """g_table[row(idx[i])] += d_out[i]: idx any shape with n ids, d_out a view whose second-to-last stride is the row stride;
    touched: the table's touched bytes (include/dctr.h, dctr_field_grad_t) or None."""
    _dev_check(idx, d_out, g_table)
    ic, is64 = _ids(idx, "idx")
    vocab, dim = table_shape
    a = _C.LookupArgs(idx=ic.data_ptr(), table=None, vocab=int(vocab), n=ic.numel(), idx_is_i64=is64, dim=int(dim),
                      hash_mode=int(hash_mode), out=None, out_stride=0, mask=None, status=None)
    _C.check(_C.lib().dctr_embed_lookup_bwd(ctypes.byref(a), _ptr(d_out), d_out.stride(-2), _ptr(g_table), _ptr(touched), _C.stream_ptr()),
             "dctr_embed_lookup_bwd")


def adam_step(w, m, v, g, alpha, beta1=0.9, beta2=0.999, eps=1e-7, l2=0.0, zero_grad=True):
    """Keras Adam over a whole contiguous parameter (non-lazy), see include/dctr.h."""
    _dev_check(w, m, v, g)
    _C.check(_C.lib().dctr_adam_step(_ptr(w), _ptr(m), _ptr(v), _ptr(g), w.numel(), float(alpha), float(beta1), float(beta2),
                                     float(eps), float(l2), int(bool(zero_grad)), _C.stream_ptr()), "dctr_adam_step")


def make_adam_segments(params, device):
    """DEVICE array of dctr_adam_seg_t from [(w, m, v, g, l2[, touched bytes or None]), ...]; returns (tensor, n_segs, max_n)."""
    arr = (_C.AdamSeg * max(1, len(params)))()
    mx = 0
    for i, e in enumerate(params):
        w, m, v, g, l2 = e[:5]
        tch = e[5] if len(e) > 5 else None
        arr[i].w, arr[i].m, arr[i].v, arr[i].g = w.data_ptr(), m.data_ptr(), v.data_ptr(), g.data_ptr()
        arr[i].n, arr[i].l2 = w.numel(), float(l2)
        if tch is not None:
            if tch.dtype != torch.uint8 or tch.numel() != w.numel() // 4 or w.numel() % 4:
                raise ValueError("touched: uint8 [n / 4] beside a parameter of n %% 4 == 0 elements")
            arr[i].touched = tch.data_ptr()
        mx = max(mx, w.numel())
    return _upload(arr, device), len(params), mx


def adam_multi(segs, n_segs, max_n, alpha, beta1=0.9, beta2=0.999, eps=1e-7, zero_grad=True):
    """dctr_adam_step for every parameter in one launch (segments from make_adam_segments)."""
    _C.check(_C.lib().dctr_adam_multi(_ptr(segs), int(n_segs), int(max_n), float(alpha), float(beta1), float(beta2),
                                      float(eps), int(bool(zero_grad)), _C.stream_ptr()), "dctr_adam_multi")


def opt_multi(kind, segs, n_segs, max_n, lr, beta1=0.9, beta2=0.999, eps=1e-7, zero_grad=True, penalty=None, penalty_scale=0.0):
    """One optimizer step (kind: adam | adagrad | rmsprop | sgd) over every parameter segment in one launch.  ``penalty`` (a device
    float64 tensor of one element): the launch also adds penalty_scale * sum_segments l2 * sum(w^2) of the weights BEFORE the update to
    it — the regularisation losses tf.keras adds to the batch's loss (dctr_opt_multi_l2)."""
    if penalty is not None:
        if penalty.dtype != torch.float64 or penalty.numel() != 1 or not penalty.is_cuda:
            raise ValueError("opt_multi: penalty must be a device float64 tensor of one element")
        _C.check(_C.lib().dctr_opt_multi_l2(_C.OPT_CODES[kind], _ptr(segs), int(n_segs), int(max_n), float(lr), float(beta1), float(beta2),
                                            float(eps), int(bool(zero_grad)), penalty.data_ptr(), float(penalty_scale), _C.stream_ptr()),
                 "dctr_opt_multi_l2")
        return
    _C.check(_C.lib().dctr_opt_multi(_C.OPT_CODES[kind], _ptr(segs), int(n_segs), int(max_n), float(lr), float(beta1),
                                     float(beta2), float(eps), int(bool(zero_grad)), _C.stream_ptr()), "dctr_opt_multi")


def make_opt_segments(params, device):
    """DEVICE array of dctr_opt_seg_t from [(w, g, [state slots ...], l2[, touched bytes or None]), ...] for opt_apply /
    grad_clip_scales; returns (tensor, n_segs, max_n)."""
    arr = (_C.opt.Seg * max(1, len(params)))()
    mx = 0
    for i, e in enumerate(params):
        w, g, slots, l2 = e[:4]
        tch = e[4] if len(e) > 4 else None
        if len(slots) > 3 or any(s.numel() != w.numel() or s.dtype != torch.float32 for s in list(slots) + [g]):
            raise ValueError("opt segments: at most three float32 state slots, each (and g) of w's size")
        arr[i].w, arr[i].g = w.data_ptr(), g.data_ptr()
        for name, s in zip(("s0", "s1", "s2"), slots):
            setattr(arr[i], name, s.data_ptr())
        arr[i].n, arr[i].l2 = w.numel(), float(l2)
        if tch is not None:
            if tch.dtype != torch.uint8 or tch.numel() != w.numel() // 4 or w.numel() % 4 or any(
                    t.data_ptr() % 16 for t in [w, g] + list(slots)):
                raise ValueError("touched: uint8 [n / 4] beside 16-byte aligned buffers of n %% 4 == 0 elements")
            arr[i].touched = tch.data_ptr()
        mx = max(mx, w.numel())
    return _upload(arr, device), len(params), mx


def opt_apply(rule, segs, n_segs, max_n, lr, zero_grad=True, clip_scale=None, penalty=None, penalty_scale=0.0):
    """One update of an optimizer object's rule over every segment in one launch (dctr_opt_apply).  ``rule``: kind (an _C.opt code)
    and the rule's scalars / flags, as optimizers.Optimizer._rule() names them (+ clipvalue); ``lr``: the step's rate (Adam / Adamax:
    bias correction folded in).  ``clip_scale``: device float32 [n_segs] from grad_clip_scales.  ``penalty``: as opt_multi."""
    if penalty is not None and (penalty.dtype != torch.float64 or penalty.numel() != 1 or not penalty.is_cuda):
        raise ValueError("opt_apply: penalty must be a device float64 tensor of one element")
    if clip_scale is not None and (clip_scale.dtype != torch.float32 or clip_scale.numel() != n_segs or not clip_scale.is_cuda):
        raise ValueError("opt_apply: clip_scale must be a device float32 tensor of n_segs elements")
    lr = float(lr)
    l2f = float(rule.get("l2_ftrl", 0.0))
    if rule.get("beta"):                     # Ftrl's beta enters as l2 + beta / (2 lr), as tf.keras adjusts it
        l2f += float(rule["beta"]) / (2.0 * lr)
    a = _C.opt.Args(kind=int(rule["kind"]), lr=lr, beta1=float(rule.get("beta1", 0.0)), beta2=float(rule.get("beta2", 0.0)),
                    eps=float(rule.get("eps", 0.0)), momentum=float(rule.get("momentum", 0.0)), lr_power=float(rule.get("lr_power", 0.0)),
                    l1=float(rule.get("l1", 0.0)), l2_ftrl=l2f, l2_shrinkage=float(rule.get("l2_shrinkage", 0.0)),
                    nesterov=int(bool(rule.get("nesterov"))), centered=int(bool(rule.get("centered"))), amsgrad=int(bool(rule.get("amsgrad"))),
                    clipvalue=float(rule.get("clipvalue") or 0.0), clip_scale=None if clip_scale is None else clip_scale.data_ptr(), zero_grad=int(bool(zero_grad)),
                    penalty_scale=float(penalty_scale) if penalty is not None else 0.0, l2_penalty=None if penalty is None else penalty.data_ptr())
    _C.check(_C.lib().dctr_opt_apply(ctypes.byref(a), _ptr(segs), int(n_segs), int(max_n), _C.stream_ptr()), "dctr_opt_apply")


def grad_clip_workspace(n_segs, max_n, device):
    """(workspace, clip_scale) device tensors for grad_clip_scales over such a segment list."""
    nbytes = int(_C.lib().dctr_grad_clip_scales_workspace_bytes(int(n_segs), int(max_n)))
    return (torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=device),
            torch.empty(max(int(n_segs), 1), dtype=torch.float32, device=device))


def grad_clip_scales(segs, n_segs, max_n, clip, workspace, clip_scale, global_norm=False):
    """Keras' clipnorm (per segment) / global_clipnorm scales of g + 2 l2 w into ``clip_scale`` [n_segs], on the device
    (dctr_grad_clip_scales: float64 partial sums added in a fixed order)."""
    _C.check(_C.lib().dctr_grad_clip_scales(_ptr(segs), int(n_segs), int(max_n), _C.opt.CLIP_GLOBAL if global_norm else _C.opt.CLIP_PER_SEGMENT,
                                            float(clip), _ptr(workspace), workspace.numel() * workspace.element_size(), _ptr(clip_scale),
                                            _C.stream_ptr()), "dctr_grad_clip_scales")


def dense1_bwd(x, n, w, dlogit, dx, d_w):
    """Backward of Dense(1, use_bias=False) on the first n columns of a strided [B, >= n] input (include/dctr.h)."""
    _dev_check(x, w, dlogit, dx, d_w)
    _C.check(_C.lib().dctr_dense1_bwd(_ptr(x), x.stride(0), x.shape[0], int(n), _ptr(w), _ptr(dlogit), _ptr(dx), dx.stride(0),
                                      _ptr(d_w), _C.stream_ptr()), "dctr_dense1_bwd")


def afm_bwd_supported(fields, dim, att_factor):
    """Does dctr_afm_bwd take these shapes (the weights and four samples' tiles fit 160 KiB of LDS; afm() itself streams any shape)?"""
    return bool(_C.lib().dctr_afm_bwd_supported(int(fields), int(dim), int(att_factor)))


def afm_bwd(x, fields, dim, attention_W, attention_b, projection_h, projection_p, dy, dx, d_W, d_b, d_h, d_p, accumulate=False):
    """Backward of afm() on a strided [B, >= F*E] buffer: dy [B]; dx [B, >= F*E] written (or added to); the four weight
    gradients (shapes of the weights) are ACCUMULATED (include/dctr.h)."""
    _dev_check(x, attention_W, attention_b, projection_h, projection_p, dy, dx, d_W, d_b, d_h, d_p)
    a = _C.AfmBwdArgs(x=x.data_ptr(), batch=x.shape[0], x_stride=x.stride(0), fields=int(fields), dim=int(dim),
                      att_factor=attention_W.shape[1], dx_accumulate=int(bool(accumulate)),
                      att_w=_f32c(attention_W, "W").data_ptr(), att_b=_f32c(attention_b, "b").data_ptr(),
                      proj_h=_f32c(projection_h, "h").data_ptr(), proj_p=_f32c(projection_p, "p").data_ptr(),
                      dy=_f32c(dy, "dy").data_ptr(), dx=dx.data_ptr(), dx_stride=dx.stride(0), d_att_w=d_W.data_ptr(),
                      d_att_b=d_b.data_ptr(), d_proj_h=d_h.data_ptr(), d_proj_p=d_p.data_ptr())
    _C.check(_C.lib().dctr_afm_bwd(ctypes.byref(a), _C.stream_ptr()), "dctr_afm_bwd")


def bi_interaction_bwd(x, fields, dim, dy, dx, accumulate=False):
    """Backward of bi_interaction on a strided [B, >= F*E] buffer: dy [B, >= E], dx [B, >= F*E] (include/dctr.h)."""
    _dev_check(x, dy, dx)
    _C.check(_C.lib().dctr_bi_interaction_bwd(_ptr(x), x.shape[0], x.stride(0), int(fields), int(dim), _ptr(dy), dy.stride(0),
                                              _ptr(dx), dx.stride(0), int(bool(accumulate)), _C.stream_ptr()),
             "dctr_bi_interaction_bwd")


def inner_product_bwd(x, fields, dim, dy, dx, accumulate=False):
    """Backward of inner_product(reduce_sum=True) on a strided buffer: dy [B, >= F(F-1)/2], dx [B, >= F*E]."""
    _dev_check(x, dy, dx)
    _C.check(_C.lib().dctr_inner_product_bwd(_ptr(x), x.shape[0], x.stride(0), int(fields), int(dim), _ptr(dy), dy.stride(0),
                                             _ptr(dx), dx.stride(0), int(bool(accumulate)), _C.stream_ptr()),
             "dctr_inner_product_bwd")


def crossnet_bwd(x, d, kernels, bias, parameterization, dy, d_kernels, d_bias, dx, accumulate=False, saved_u=None, saved_x=None,
                 workspace=None):
    """Backward of dctr_crossnet_fwd: x [B, >= d] the forward input, dy [B, >= d]; d_kernels / d_bias are ACCUMULATED,
    dx [B, >= d] is written (or added to with ``accumulate``).  saved_u [L, B, d] / saved_x [L - 1, B, d] (matrix form): what the
    forward wrote through dctr_crossnet_args_t.save_u / save_x — the backward then recomputes nothing.  ``workspace``: a dict the
    caller keeps alive, as ``cin_bwd`` takes it (default: a fresh tensor per call)."""
    _dev_check(x, dy, dx, kernels, bias)
    L = 0 if kernels is None else kernels.shape[0]
    mode = _C.CROSS_VECTOR if parameterization == "vector" else _C.CROSS_MATRIX
    a = _C.CrossBwdArgs(x=x.data_ptr(), x_stride=x.stride(0), batch=x.shape[0], dim=int(d), layers=L, mode=mode,
                        dx_accumulate=int(bool(accumulate)), kernels=_ptr(kernels), bias=_ptr(bias), dy=dy.data_ptr(),
                        dy_stride=dy.stride(0), d_kernels=_ptr(d_kernels), d_bias=_ptr(d_bias), dx=dx.data_ptr(),
                        dx_stride=dx.stride(0), saved_u=_ptr(saved_u), saved_x=_ptr(saved_x))
    need = int(_C.lib().dctr_crossnet_bwd_workspace_bytes(ctypes.byref(a)))
    ws = _bwd_workspace(workspace, need, x.device)
    a.workspace, a.workspace_bytes = ws.data_ptr(), need
    _C.check(_C.lib().dctr_crossnet_bwd(ctypes.byref(a), _C.stream_ptr()), "dctr_crossnet_bwd")


def cin_bwd(x, filters, biases, layer_size, split_half, activation, d_out, d_filters, d_biases, dx=None, accumulate=False,
            fields=None, dim=None, saved_y=None, workspace=None):
    """Backward of dctr_cin_fwd: x as in ``cin`` (3-D, or the leading F0*D columns of a 2-D buffer with fields/dim);
    d_out [B, featuremap_num]; d_filters / d_biases are ACCUMULATED; dx (2-D, same layout as x) written or added to.
    ``workspace``: a dict the caller keeps alive, as ``mlp_bwd`` takes it: the tensor is cached under "ws" and replaced only when it
    is missing, on another device or smaller than dctr_cin_bwd_workspace_bytes (default: a fresh tensor per call)."""
    _dev_check(x, d_out, *filters)
    x, B, F0, D, x_stride, _ = _x_in_place("cin_bwd", x, fields, dim)
    n = len(layer_size)
    filters = [_f32c(f, "filter").reshape(-1, h) for f, h in zip(filters, layer_size)]
    biases = [_f32c(b, "bias") for b in biases]
    ls = _i32_array(layer_size)
    fp, bp = _ptr_array(filters), _ptr_array(biases)
    dfp, dbp = _ptr_array(list(d_filters)), _ptr_array(list(d_biases))
    fwd = _C.CinArgs(x=x.data_ptr(), batch=B, x_stride=x_stride, fields=F0, dim=D, n_layers=n, split_half=int(bool(split_half)),
                     activation=_C.ACT_CODES[activation], layer_size=ctypes.cast(ls, ctypes.c_void_p),
                     filters=ctypes.cast(fp, ctypes.c_void_p), bias=ctypes.cast(bp, ctypes.c_void_p), out=None,
                     workspace=None, workspace_bytes=0)
    d_out = _f32c(d_out, "d_out")
    a = _C.CinBwdArgs(fwd=ctypes.pointer(fwd), d_out=d_out.data_ptr(), out_dim=d_out.shape[1], dx_accumulate=int(bool(accumulate)),
                      d_filters=ctypes.cast(dfp, ctypes.c_void_p), d_bias=ctypes.cast(dbp, ctypes.c_void_p),
                      dx=None if dx is None else dx.data_ptr(), dx_stride=0 if dx is None else dx.stride(0))
    if saved_y is not None:                 # the forward call's cin(save_y=...) tensors: no recompute GEMMs
        _check_saved_y(saved_y, B * D, layer_size, x)
        syp = _ptr_array(list(saved_y))
        a.saved_y = ctypes.cast(syp, ctypes.c_void_p)
    need = int(_C.lib().dctr_cin_bwd_workspace_bytes(ctypes.byref(a)))
    if workspace is not None:
        ws = workspace.get("ws")
        if ws is None or ws.dtype != torch.float32 or not ws.is_contiguous() or ws.numel() * 4 < need or ws.device != x.device:
            ws = workspace["ws"] = torch.empty(max(1, need // 4), dtype=torch.float32, device=x.device)
    else:
        ws = torch.empty(max(1, need // 4), dtype=torch.float32, device=x.device)
    a.workspace, a.workspace_bytes = ws.data_ptr(), need
    _C.check(_C.lib().dctr_cin_bwd(ctypes.byref(a), _C.stream_ptr()), "dctr_cin_bwd")
