"""MLR (Mixed Logistic Regression, the piece-wise linear model of Gai et al.) — same signature as ``deepctr.models.mlr.MLR``
(reference deepctr/models/mlr.py:17-74): with R = region_num, 2R (+1) independent linear logits over the same ids — R region logits over
``region_feature_columns`` (tables ``region_<r>0sparse_emb_<name>``), R learner logits over ``base_feature_columns`` (``learner_<r>0...``;
the region columns when None or empty) and one bias logit over ``bias_feature_columns`` (``bias_10...``) — mixed as

    out = sum_r softmax(z_region)[r] * act(z_learner[r])  (* sigmoid(z_bias))        act = sigmoid (task 'binary') | identity

``out`` IS the model's output: no PredictionLayer, no global_bias, no final sigmoid.

HBM layout: the logit columns are numbered region 0..R-1, learner R..2R-1, bias 2R.  Every ``embedding_name`` owns ONE fp32 master
[vocab, pitch] per maximal run of columns that read it (one master for the default region = base; two for region + bias without base),
pitch = the run rounded up to 4 floats.  The reference's per-name ``embeddings`` are the [vocab, 1] strided views ``master[:, c:c+1]`` —
what ``named_weights()`` returns — so every weight-facing API keeps the reference's names while the kernel reads one 32-48-byte row per
id in place of 2R (+1) scattered dwords, and always sees the live values.

Forward: staged ids (one [F, N] matrix, hashed once at staging) -> dctr_embed_pool over the whole fused row for every sequence feature
(the linear part's pooling: combiner, length_name / weight_name / weight_norm, mask_zero) -> ONE ``dctr_mlr_fwd`` launch writing the
prediction.  The shared EmbeddingStage has no table: it stages the dense matrix and the sequences."""
from collections import OrderedDict

import numpy as np
import torch

from .. import ops
from ..engine import EmbeddingStage, _column, _fit_int32, _ids_from_column, prehashed_on_host
from ..feature_column import DenseFeat, SparseFeat, VarLenSparseFeat
from ..initializers import Zeros
from ..inputs import _check_embedding_compatible
from ..layers.base import Layer, name_scope
from ..layers.utils import Linear
from .. import training as tops
from ._common import FeatureModel


class FusedLinearEmbedding(Layer):
    """keras ``Embedding`` ``<prefix>0sparse_emb_<name>`` of one linear logit: its ``embeddings`` [vocab, 1] is one column of the
    name's fused rows, a strided view."""

    def __init__(self, view, mask_zero=False, **kwargs):
        super(FusedLinearEmbedding, self).__init__(**kwargs)
        self.input_dim, self.output_dim = int(view.shape[0]), 1
        self.mask_zero = mask_zero
        with torch.no_grad():
            view.copy_(Zeros()(tuple(view.shape)).to(torch.float32))
        self._weights["embeddings"] = view
        self.built = True

    @property
    def embeddings(self):
        return self.w("embeddings")

    def to(self, device):
        raise NotImplementedError("a fused linear embedding is a view of its name's fused rows: build the model on the device")


class _Group(object):
    """One linear logit (reference feature_column.py:171-210 with units = 1): its column, its features, tables and Linear layer."""

    def __init__(self, column, prefix, seed, cols):
        self.column, self.prefix, self.seed = column, prefix, seed
        # input_from_feature_columns: all SparseFeat, then all VarLenSparseFeat
        self.features = [fc for fc in cols if isinstance(fc, SparseFeat)] + [fc for fc in cols if isinstance(fc, VarLenSparseFeat)]
        self.dense = [fc for fc in cols if isinstance(fc, DenseFeat)]
        self.tables = OrderedDict()         # embedding_name -> FusedLinearEmbedding
        self.linear = None
        self.dense_pos = None               # int64 [n_dense_g]: its dense values' columns of the staged dense matrix


def _runs(cols):
    """Sorted ints -> [(first, count)] of the maximal runs of consecutive values."""
    out = []
    for c in cols:
        if out and out[-1][0] + out[-1][1] == c:
            out[-1] = (out[-1][0], out[-1][1] + 1)
        else:
            out.append((c, 1))
    return out


class _MLR(FeatureModel):
    output_kind = "prediction"

    def __init__(self, region_cols, base_cols, bias_cols, region_num, seed, task, device):
        super(_MLR, self).__init__("MLR", region_cols + base_cols + bias_cols, device, task)
        R = self.region_num = int(region_num)
        self.has_bias = len(bias_cols) > 0
        self.learner_task = task            # fixed here: the learners' activation does not follow later writes to self.task
        self.n_columns = 2 * R + int(self.has_bias)
        self.groups = ([_Group(r, "region_%d" % (r + 1), seed + r, region_cols) for r in range(R)] +
                       [_Group(R + r, "learner_%d" % (r + 1), seed + r, base_cols) for r in range(R)] +
                       ([_Group(2 * R, "bias_1", seed, bias_cols)] if self.has_bias else []))
        # ---- which columns read which embedding_name, which feature -----------------------------------------------------------
        by_name, self.features, feat_cols = OrderedDict(), OrderedDict(), OrderedDict()
        for g in self.groups:
            for fc in g.features:
                first = by_name.setdefault(fc.embedding_name, (fc, []))
                _check_embedding_compatible(fc.embedding_name, first[0], fc)
                if g.column not in first[1]:
                    first[1].append(g.column)
                self.features.setdefault(fc.name, fc)
                cs = feat_cols.setdefault(fc.name, [])
                if g.column not in cs:
                    cs.append(g.column)
        dense_cols = OrderedDict()
        for g in self.groups:
            for fc in g.dense:
                dense_cols.setdefault(fc.name, fc)
        with name_scope():
            self.masters = OrderedDict()      # embedding_name -> [(first column, columns, master [vocab, pitch])]
            for name, (fc, cs) in by_name.items():
                self.masters[name] = [(c0, n, torch.zeros(int(fc.vocabulary_size), (n + 3) // 4 * 4, dtype=torch.float32,
                                                          device=self.device)) for c0, n in _runs(sorted(cs))]
            self.mlr_tables = OrderedDict()   # layer name -> FusedLinearEmbedding (training: frozen_weights / regularized_weights)
            self.mlr_linears = []
            for g in self.groups:
                # create_embedding_dict's order and names: the names SparseFeat use first, then the ones only sequences use
                seq_names = set(fc.embedding_name for fc in g.features if isinstance(fc, VarLenSparseFeat))
                sparse_names = [fc.embedding_name for fc in g.features if isinstance(fc, SparseFeat)]
                for fc in g.features:
                    name = fc.embedding_name
                    if name in g.tables:
                        continue
                    kind = "emb" if name in sparse_names else "seq_emb"
                    emb = FusedLinearEmbedding(self._view(name, g.column), mask_zero=name in seq_names,
                                               name="%s0sparse_%s_%s" % (g.prefix, kind, name), device=self.device)
                    emb.trainable = by_name[name][0].trainable
                    g.tables[name] = self.mlr_tables[emb.name] = self._add(emb)
                # one Linear per logit, with or without weights: keras' auto names (linear, linear_1, ...) count them all
                n_dense = sum(fc.dimension for fc in g.dense)
                g.linear = Linear(mode=(2 if g.features else 1) if n_dense else 0, seed=g.seed, device=self.device).build_for(n_dense)
                self.mlr_linears.append(self._add(g.linear))
            self.stage_plan = EmbeddingStage({}, {}, [], list(dense_cols.values()), device=self.device)
        # ---- the dense part: each logit's linear_kernel rows at its dense values' columns of the staged matrix --------------------
        sp = self.stage_plan
        self.n_dense = sp.n_dense
        offs, at = {}, 0
        for fc in sp.dense_cols:
            offs[fc.name] = at
            at += fc.dimension
        flat = []
        for g in self.groups:
            pos = [offs[fc.name] + p for fc in g.dense for p in range(fc.dimension)]
            if pos:
                g.dense_pos = torch.as_tensor(pos, dtype=torch.int64, device=self.device)
                flat += [p * self.n_columns + g.column for p in pos]
        self._dense_w = torch.zeros(self.n_dense, self.n_columns, dtype=torch.float32, device=self.device) if self.n_dense else None
        self._dense_flat = torch.as_tensor(flat, dtype=torch.int64, device=self.device)
        # ---- the kernel's fields: per feature one entry per run of its columns -----------------------------------------------------
        self.id_features = [fc for fc in self.features.values() if isinstance(fc, SparseFeat)]       # rows of the [F, N] id matrix
        self._id_row = {fc.name: j for j, fc in enumerate(self.id_features)}
        self.entries = []       # dict(fc, master, first, col0, width, id_row | None)
        for fname, fc in self.features.items():
            for c0, n in _runs(sorted(feat_cols[fname])):
                m0, _, master = next(m for m in self.masters[fc.embedding_name] if m[0] <= c0 < m[0] + m[1])
                self.entries.append(dict(fc=fc, master=master, first=c0 - m0, col0=c0, width=n,
                                         id_row=self._id_row[fc.name] if isinstance(fc, SparseFeat) else None))

    def _view(self, name, column):
        for c0, n, master in self.masters[name]:
            if c0 <= column < c0 + n:
                return master[:, column - c0:column - c0 + 1]
        raise KeyError((name, column))

    # -- weights: the reference builds a second, never-used set of tables per logit (get_linear_logit calls
    #    input_from_feature_columns once more with the bare prefix: region_1sparse_emb_<name>, ...); a weight file of the reference holds
    #    them and they are skipped here, as FeatureModel skips linearsparse_* --------------------------------------------------------
    def _dangling(self, key):
        lname = key.rsplit("/", 1)[0]
        return any(lname.startswith(g.prefix + "sparse_") for g in self.groups)

    def set_weights_by_name(self, mapping, strict=True):
        mine = set(n for n, _ in self.named_weights())
        return super(_MLR, self).set_weights_by_name(
            OrderedDict((k, v) for k, v in mapping.items() if k in mine or not self._dangling(k)), strict=strict)

    def predict_logits(self, x, batch_size=256):
        raise NotImplementedError("MLR's output is a mixture of the learners' outputs, not the sigmoid of a logit: there is no "
                                  "pre-sigmoid value to return; use predict()")

    # -- staging ---------------------------------------------------------------------------------------------------------------------
    def _hashes(self, fc):
        return bool(fc.use_hash and not prehashed_on_host(fc))

    def _stage_inputs(self, feed, staged):
        sp, dev = self.stage_plan, self.device
        sp.stage(feed, staged)
        for fc in self.features.values():
            if isinstance(fc, VarLenSparseFeat):
                sp.stage_varlen(feed, staged, fc)
        cols = []
        for fc in self.id_features:
            a = _column(feed, fc.name).reshape(-1)
            if a.shape[0] != staged.n:
                raise ValueError("feature %r has %d rows, expected %d" % (fc.name, a.shape[0], staged.n))
            cols.append(_ids_from_column(a, fc, False, dev))
        if not cols:
            return
        any_hash = any(self._hashes(fc) for fc in self.id_features)
        dt = torch.int32 if (_fit_int32(cols) and not any_hash) else torch.int64
        mat = torch.zeros(len(cols), staged.n, dtype=dt, device=dev)      # [F, N]: a wave's samples read one contiguous run per field
        for j, (fc, c) in enumerate(zip(self.id_features, cols)):
            t = c if isinstance(c, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(c)).to(dev)
            if self._hashes(fc):                                          # Hash(vocabulary_size), once, where the ids arrive
                t = ops.hash_bucket(t.contiguous() if t.dtype in (torch.int32, torch.int64) else t.to(torch.int64),
                                    fc.vocabulary_size, False)
            mat[j] = t.to(dt)
        staged.ids = mat                                                  # (permute_staged_ permutes it along axis 1)

    def sparse_rows(self, staged, fc, lo, hi):
        """torch ops: the table rows (hashed at staging) of SparseFeat ``fc`` for samples [lo, hi)."""
        return staged.ids[self._id_row[fc.name], lo:hi].to(torch.int64)

    def _pipeline(self, x, batch_size):
        return None

    def _begin(self):
        if self._dense_w is not None and len(self._dense_flat):
            # packed in place from the live linear_kernels (zeros stay where a logit does not use a dense column)
            with torch.no_grad():
                self._dense_w.view(-1).index_copy_(0, self._dense_flat, torch.cat(
                    [g.linear.w("linear_kernel").detach().reshape(-1) for g in self.groups if g.dense_pos is not None]))

    # -- the HIP forward ---------------------------------------------------------------------------------------------------------------
    def _pool_keys(self):
        """(feature name, master's first column) of every pooled buffer: one per sequence feature and master it reads."""
        return [(e["fc"].name, e["col0"] - e["first"]) for e in self.entries if e["id_row"] is None]

    def _buffers(self, B):
        return self._per_batch(B, lambda: {"pooled": {(e["fc"].name, e["col0"] - e["first"]):
                                                      torch.zeros(B, e["master"].shape[1], dtype=torch.float32, device=self.device)
                                                      for e in self.entries if e["id_row"] is None}})

    def _run_pools(self, staged, lo, hi, bufs):
        sp = self.stage_plan
        done = set()
        for e in self.entries:
            key = (e["fc"].name, e["col0"] - e["first"])
            if e["id_row"] is not None or key in done:
                continue
            done.add(key)
            buf = bufs["pooled"][key]
            sp._pool(e["fc"], staged, lo, hi, e["master"], None, buf, None, sp.status())

    def _descriptors(self, staged, lo, hi, bufs):
        """dctr_mlr_field_t array of rows [lo, hi): cached per (staged id matrix: address, dtype, row stride, rows; lo) beside the
        per-B buffers it points into."""
        # the id matrix is [F, N]: field j's pointer is base + (j * N + lo) elements, so the key carries N (the row stride) beside the
        # base address — a later feed of another length may be handed the same address by the allocator
        ids = staged.ids
        key = (ids.data_ptr(), ids.dtype, int(ids.stride(0)), int(ids.shape[1]), lo) if ids is not None else (0, None, 0, 0, lo)
        cache = bufs.setdefault("desc", OrderedDict())
        desc = cache.get(key)
        if desc is None:
            fields = []
            for e in self.entries:
                if e["id_row"] is None:
                    rows, ids = bufs["pooled"][(e["fc"].name, e["col0"] - e["first"])][:, e["first"]:], None
                else:
                    rows, ids = e["master"][:, e["first"]:], staged.ids[e["id_row"], lo:hi]
                fields.append(dict(rows=rows, ids=ids, col0=e["col0"], width=e["width"]))
            while len(cache) >= 64:
                cache.popitem(last=False)
            desc = cache[key] = ops.make_mlr_fields(fields, self.device) if fields else None
        return desc

    def _forward(self, staged, lo, hi, out):
        B = hi - lo
        if not ops.mlr_supported(self.region_num, self.has_bias):
            # more than 64 logit columns: the library declines before any launch; the torch ops answer
            with torch.no_grad():
                out.copy_(tops._mlr_output(self, staged, lo, hi))
            return
        bufs = self._buffers(B)
        self._run_pools(staged, lo, hi, bufs)
        desc = self._descriptors(staged, lo, hi, bufs)
        dense = staged.dense[lo:hi] if self.n_dense else None
        ops.mlr(None, self.region_num, self.has_bias, self.learner_task, dense=dense, dense_w=self._dense_w if self.n_dense else None,
                out=out, status=self.stage_plan.status(), desc=desc, batch=B, n_fields=len(self.entries), device=self.device)

    # -- the autograd step -------------------------------------------------------------------------------------------------------------
    def _group_of(self, column):
        return self.groups[column]          # (groups are in column order)

    def _pooled_rows(self, staged, lo, hi, e):
        """torch ops: a sequence entry's [B, width] pooled rows, its per-name views pooled one by one and laid side by side."""
        fc = e["fc"]
        rows = tops._rows_for(fc, staged.seq[fc.name][lo:hi], True)
        length = staged.length[fc.length_name][lo:hi] if fc.length_name is not None else None
        weight = staged.weight[fc.weight_name][lo:hi] if fc.weight_name is not None else None
        return torch.cat([tops._pool(self._group_of(c).tables[fc.embedding_name].embeddings[rows], fc, rows != 0, length, weight)
                          .reshape(hi - lo, 1) for c in range(e["col0"], e["col0"] + e["width"])], dim=-1)

    def _output_on_hip(self, staged, lo, hi):
        """The prediction [B] as ONE differentiable HIP op (ops.MLRFunction), or None: the torch ops."""
        plan, views = [], []
        for e in self.entries:
            cols = range(e["col0"], e["col0"] + e["width"])
            if e["id_row"] is None:
                plan.append(dict(master=None, ids=None, first=0, col0=e["col0"], width=e["width"]))
                views.append(lambda e=e: self._pooled_rows(staged, lo, hi, e))
            else:
                plan.append(dict(master=e["master"], ids=staged.ids[e["id_row"], lo:hi], first=e["first"], col0=e["col0"],
                                 width=e["width"]))
                views.append([self._group_of(c).tables[e["fc"].embedding_name].embeddings for c in cols])
        if not plan:
            return None
        inputs = tops._mlr_on_hip(plan, views, hi - lo, self.region_num, self.has_bias, tops.MLR_HIP_MIN_ROWS)
        if inputs is None:
            return None
        dense = dense_w = None
        if self.n_dense and len(self._dense_flat):
            kernels = torch.cat([g.linear.w("linear_kernel").reshape(-1) for g in self.groups if g.dense_pos is not None])
            dense_w = torch.zeros(self.n_dense * self.n_columns, dtype=torch.float32, device=self.device).index_copy(
                0, self._dense_flat, kernels).view(self.n_dense, self.n_columns)
            dense = staged.dense[lo:hi]
        if not (any(t.requires_grad for t in inputs) or (dense_w is not None and dense_w.requires_grad)):
            return None
        return ops.MLRFunction.apply(plan, self.region_num, self.has_bias, self.learner_task, self.stage_plan.status(), dense, dense_w,
                                     *inputs)

    def autograd_logits(self, staged, lo, hi, training=False):
        """MLR's PREDICTION [B] of rows [lo, hi) (output_kind = "prediction"), differentiable."""
        out = self._output_on_hip(staged, lo, hi) if self.device.type == "cuda" else None
        return tops._mlr_output(self, staged, lo, hi) if out is None else out


def MLR(region_feature_columns, base_feature_columns=None, region_num=4, l2_reg_linear=1e-5, seed=1024, task='binary',
        bias_feature_columns=None, device=None):
    """Instantiates the Mixed Logistic Regression / piece-wise linear model on the MI355X forward path."""
    if region_num <= 1:
        raise ValueError("region_num must > 1")
    region = list(region_feature_columns or [])
    if not region:
        raise ValueError("MLR: region_feature_columns is empty (the reference's region softmax degenerates to a constant there)")
    base = list(base_feature_columns or [])
    if not base:
        base = region
    bias = list(bias_feature_columns or [])
    m = _MLR(region, base, bias, region_num, seed, task, device)
    m.regularizers = {"linear": float(l2_reg_linear)}
    return m
