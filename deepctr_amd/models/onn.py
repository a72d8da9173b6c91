"""ONN (Operation-aware Neural Networks, a.k.a. NFFM) — same signature as ``deepctr.models.onn.ONN`` (reference
deepctr/models/onn.py:32-108): every sparse / sequence feature j of ``dnn_feature_columns`` owns one embedding per partner feature i
(``sparse_emb_<j>_<i>``); per pair (i < j) the two field-aware embeddings are multiplied elementwise (summed with ``reduce_sum``), the
products go through an optional BatchNormalization and, with the dense values, into the DNN; Dense(1) + the linear logit.

HBM layout: ONE fused table [V_j, F-1, d] per feature (slot k = partner i in field order, j skipped).  The per-name weights are
strided views ``master[:, k, :]`` of it — what ``named_weights()`` returns — so every weight-facing API keeps the reference's names
while the kernel reads one contiguous (F-1)*d*4-byte row per id, and always sees the live values.

Forward: staged ids (hashed once per feature when staged) -> dctr_embed_pool over the whole fused row for every sequence feature
(ONN's semantics: mask_zero on the post-hash id; length_name / weight_name are not used by the deep part) -> ONE ``dctr_ffm_fwd``
launch writing the DNN input -> the DNN kernel with dense/kernel as its head, adding the linear logit, the bias and the sigmoid.
The linear part runs on the shared EmbeddingStage, whose only "deep" columns are the DenseFeat."""
import ctypes
from collections import OrderedDict

import numpy as np
import torch

from .. import _C, ops
from ..engine import EmbeddingStage, _column, _fit_int32, _ids_from_column, prehashed_on_host
from ..feature_column import DenseFeat, SparseFeat, VarLenSparseFeat
from ..layers.base import Layer, name_scope
from ..layers.core import DNN, BatchNormalization, Dense, PredictionLayer
from .. import training as tops
from ._common import FeatureModel


class FieldAwareEmbedding(Layer):
    """keras ``Embedding`` ``sparse_emb_<j>_<i>``: its ``embeddings`` is slot k of feature j's fused table, a strided view."""

    def __init__(self, view, initializer, mask_zero=False, **kwargs):
        super(FieldAwareEmbedding, self).__init__(**kwargs)
        self.input_dim, self.output_dim = int(view.shape[0]), int(view.shape[1])
        self.mask_zero = mask_zero
        with torch.no_grad():
            view.copy_(initializer(tuple(view.shape)).to(torch.float32))
        self._weights["embeddings"] = view
        self.built = True

    @property
    def embeddings(self):
        return self.w("embeddings")

    def to(self, device):
        raise NotImplementedError("a field-aware embedding is a view of its feature's fused table: build the model on the device")


def field_aware_columns(dnn_feature_columns):
    """The reference's field order (onn.py:59-62): all SparseFeat of dnn_feature_columns, then all VarLenSparseFeat — checked for what
    the reference itself cannot run."""
    cols = list(dnn_feature_columns or [])
    deep = [fc for fc in cols if isinstance(fc, SparseFeat)] + [fc for fc in cols if isinstance(fc, VarLenSparseFeat)]
    if len(deep) < 2:
        raise ValueError("ONN: dnn_feature_columns holds %d sparse / sequence feature(s); the pair products need at least 2 "
                         "(the reference concatenates an empty list)" % len(deep))
    dims = sorted(set(int(fc.embedding_dim) for fc in deep))
    if len(dims) != 1:
        raise ValueError("ONN multiplies the embeddings of every feature pair elementwise: they need one embedding_dim, got %s" % dims)
    for fc in deep:
        if fc.embedding_name != fc.name:
            raise ValueError("ONN: feature %r has embedding_name %r; the reference keys its field-aware tables by embedding_name and "
                             "looks them up by name (a KeyError there): leave embedding_name unset" % (fc.name, fc.embedding_name))
    return deep, dims[0]


class _ONN(FeatureModel):
    def __init__(self, linear_feature_columns, dnn_feature_columns, dnn_hidden_units, dnn_dropout, seed, use_bn, reduce_sum, task, device):
        linear_feature_columns, dnn_feature_columns = list(linear_feature_columns or []), list(dnn_feature_columns or [])
        deep, d = field_aware_columns(dnn_feature_columns)
        super(_ONN, self).__init__("ONN", linear_feature_columns + dnn_feature_columns, device, task)
        self.deep_cols, self.emb_dim, self.reduce_sum = deep, d, bool(reduce_sum)
        F = self.n_fields = len(deep)
        self.n_pairs = F * (F - 1) // 2
        self.pair_width = self.n_pairs if self.reduce_sum else self.n_pairs * d
        with name_scope():
            self.build_linear(linear_feature_columns, seed)
            self.tables = OrderedDict()       # "<j>_<i>" -> FieldAwareEmbedding (training: frozen_weights / regularized_weights)
            self.masters = []                 # per field: [V_j, F-1, d]
            for j, fc_j in enumerate(deep):
                master = torch.zeros(int(fc_j.vocabulary_size), F - 1, d, dtype=torch.float32, device=self.device)
                self.masters.append(master)
                k = 0
                for i, fc_i in enumerate(deep):
                    if i == j:
                        continue
                    emb = FieldAwareEmbedding(master[:, k, :], fc_j.embeddings_initializer, mask_zero=isinstance(fc_j, VarLenSparseFeat),
                                              name="sparse_emb_%s_%s" % (fc_j.embedding_name, fc_i.embedding_name), device=self.device)
                    emb.trainable = fc_j.trainable
                    self.tables["%s_%s" % (fc_j.embedding_name, fc_i.embedding_name)] = self._add(emb)
                    k += 1
            # the shared stage sees the DenseFeat of the deep part only: it stages the dense matrix, the linear part's ids and
            # sequences, and computes the linear logit; every sparse feature of the linear part is "linear only" to it
            dense_cols = [fc for fc in dnn_feature_columns if isinstance(fc, DenseFeat)]
            self.stage_plan = EmbeddingStage({}, self.linear_tables, linear_feature_columns, dense_cols, device=self.device)
            sp = self.stage_plan
            self.n_dense = sp.n_dense_dnn
            self.dnn_in_dim = self.pair_width + self.n_dense
            self.in_stride = (self.dnn_in_dim + 3) // 4 * 4
            self.bn = None
            if use_bn:
                self.bn = BatchNormalization(device=self.device)
                self.bn.build((None, self.pair_width))
                self.bn.built = True
                self._add(self.bn)
            units = list(dnn_hidden_units or [])
            self.dnn = self._add(DNN(units, 'relu', 0, dnn_dropout, False, seed=seed, device=self.device).build_for(self.dnn_in_dim))
            self.dense = self._add(Dense(1, use_bias=False, seed=seed, device=self.device).build_for(units[-1] if units else self.dnn_in_dim))
            self.prediction = self._add(PredictionLayer(task, device=self.device).build_for())
        self._scale = self._shift = None

    # -- staging: the shared stage (dense, linear part) + the deep part's ids, hashed once per feature ------------------------------
    def _hashes(self, fc):
        return bool(fc.use_hash and not prehashed_on_host(fc))

    def _stage_inputs(self, feed, staged):
        sp, dev = self.stage_plan, self.device
        sp.stage(feed, staged)
        cols = []
        for fc in self.deep_cols:
            if isinstance(fc, VarLenSparseFeat):
                if fc.name not in staged.seq:
                    sp.stage_varlen(feed, staged, fc)
                cols.append(None)
                if self._hashes(fc):      # plain Hash(vocabulary_size): padding zeros land in a real bucket (onn.py:84-85)
                    staged.extra["ffm_seq:" + fc.name] = ops.hash_bucket(staged.seq[fc.name], fc.vocabulary_size, False)
                continue
            a = _column(feed, fc.name).reshape(-1)
            if a.shape[0] != staged.n:
                raise ValueError("feature %r has %d rows, expected %d" % (fc.name, a.shape[0], staged.n))
            cols.append(_ids_from_column(a, fc, False, dev))
        real = [c for c in cols if c is not None]
        any_hash = any(self._hashes(fc) for fc in self.deep_cols if isinstance(fc, SparseFeat))
        dt = torch.int32 if (_fit_int32(real) and not any_hash) else torch.int64
        mat = torch.zeros(staged.n, len(cols), dtype=dt, device=dev)          # [N, F]: a tile's ids are one contiguous run
        for j, (fc, c) in enumerate(zip(self.deep_cols, cols)):
            if c is None:
                continue
            t = c if isinstance(c, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(c)).to(dev)
            if self._hashes(fc):
                t = ops.hash_bucket(t.contiguous() if t.dtype in (torch.int32, torch.int64) else t.to(torch.int64),
                                    fc.vocabulary_size, False)
            mat[:, j] = t.to(dt)
        staged.extra["ffm_ids"] = mat

    def _pipeline(self, x, batch_size):
        return None

    def _begin(self):
        super(_ONN, self)._begin()
        if self.bn is not None and not getattr(self, "_trainer_step", False):
            self._scale, self._shift = self.bn.scale_shift()      # from the live tensors, in place

    def _buffers(self, B):
        R = (self.n_fields - 1) * self.emb_dim
        # (zeros: the row padding to a multiple of 4 floats is never written, and the DNN kernels may read it)
        return self._per_batch(B, lambda: {"dnn_in": torch.zeros(B, self.in_stride, dtype=torch.float32, device=self.device),
                                           "pooled": {fc.name: torch.zeros(B, (R + 3) // 4 * 4, dtype=torch.float32, device=self.device)
                                                      for fc in self.deep_cols if isinstance(fc, VarLenSparseFeat)}})

    def _linear_logits(self, staged, lo, hi):
        """The [B] vectors of the linear part: the stage's gather over no field (dense . linear_kernel) and its linear-only gather."""
        sp = self.stage_plan
        ws = sp.run_pools(staged, lo, hi)
        add = []
        if sp.n_dense and sp.has_linear:
            a = sp.gather_args(staged, lo, hi, ws)
            _C.check(_C.lib().dctr_embed_gather_fm(ctypes.byref(a), _C.stream_ptr()), "dctr_embed_gather_fm")
            add.append(ws["lin"])
        sp.run_lin_only(staged, lo, hi, ws)
        if "lin2" in ws:
            add.append(ws["lin2"])
        return add

    def _descriptors(self, staged, lo, hi, bufs):
        """dctr_ffm_field_t array of rows [lo, hi): cached per (staged id matrix, lo) beside the per-B buffers it points into."""
        ids = staged.extra["ffm_ids"]
        R = (self.n_fields - 1) * self.emb_dim
        key = (ids.data_ptr(), lo)
        cache = bufs.setdefault("desc", OrderedDict())
        desc = cache.get(key)
        if desc is None:
            fields = []
            for j, (fc, master) in enumerate(zip(self.deep_cols, self.masters)):
                if isinstance(fc, VarLenSparseFeat):
                    fields.append(dict(rows=bufs["pooled"][fc.name], ids=None))
                else:
                    fields.append(dict(rows=master.view(master.shape[0], R), ids=ids[lo:hi, j]))
            while len(cache) >= 64:
                cache.popitem(last=False)
            desc = cache[key] = ops.make_ffm_fields(fields, self.device)
        return desc

    def field_aware_rows(self, staged, lo, hi):
        """torch ops (autograd_logits): embs[j][i] = feature j's embedding towards partner i for rows [lo, hi), gathered from the
        per-name views; sequences pooled with ONN's semantics (mask_zero on the post-hash id, no length / weight)."""
        ids = staged.extra["ffm_ids"]
        embs = []
        for j, fc_j in enumerate(self.deep_cols):
            row = {}
            if isinstance(fc_j, VarLenSparseFeat):
                seq = staged.extra.get("ffm_seq:" + fc_j.name)
                rows = (staged.seq[fc_j.name] if seq is None else seq)[lo:hi].to(torch.int64)
                mask = rows != 0
            else:
                rows = ids[lo:hi, j].to(torch.int64)
            for i, fc_i in enumerate(self.deep_cols):
                if i == j:
                    continue
                w = self.tables["%s_%s" % (fc_j.embedding_name, fc_i.embedding_name)].embeddings
                row[i] = tops._pool(w[rows], fc_j, mask, None, None) if isinstance(fc_j, VarLenSparseFeat) else w[rows]
            embs.append(row)
        return embs

    def _pooled_rows(self, staged, lo, hi, j):
        """torch ops: sequence feature j's [B, (F-1)*d] fused row, its F-1 per-name views pooled as field_aware_rows pools them and
        laid side by side in slot order — what ops.FieldAwareFunction takes for a field that arrives pooled."""
        fc_j = self.deep_cols[j]
        seq = staged.extra.get("ffm_seq:" + fc_j.name)
        rows = (staged.seq[fc_j.name] if seq is None else seq)[lo:hi].to(torch.int64)
        mask = rows != 0
        return torch.cat([tops._pool(self.tables["%s_%s" % (fc_j.embedding_name, fc_i.embedding_name)].embeddings[rows], fc_j, mask,
                                     None, None).reshape(hi - lo, -1) for i, fc_i in enumerate(self.deep_cols) if i != j], dim=-1)

    def _pairs_on_hip(self, staged, lo, hi):
        """The pair columns [B, P*d] ([B, P]) as ONE differentiable HIP op (ops.FieldAwareFunction), or None: the torch ops."""
        masters, views = [], []
        for j, (fc_j, master) in enumerate(zip(self.deep_cols, self.masters)):
            if isinstance(fc_j, VarLenSparseFeat):
                masters.append(None)
                views.append(lambda j=j: self._pooled_rows(staged, lo, hi, j))
            else:
                masters.append(master)
                views.append([self.tables["%s_%s" % (fc_j.embedding_name, fc_i.embedding_name)].embeddings
                              for i, fc_i in enumerate(self.deep_cols) if i != j])
        inputs = tops._ffm_on_hip(masters, views, hi - lo, tops.ONN_HIP_MIN_ROWS)
        if inputs is None or not any(t.requires_grad for t in inputs):
            return None
        return ops.FieldAwareFunction.apply(staged.extra["ffm_ids"][lo:hi].t(), masters, self.emb_dim, self.reduce_sum,
                                            self.stage_plan.status(), *inputs)

    def _autograd_logit(self, staged, lo, hi, parts, extra, training):       # onn.py:59-105
        x = self._pairs_on_hip(staged, lo, hi)
        if x is None:
            embs = self.field_aware_rows(staged, lo, hi)
            prods = []
            for i, j in zip(*tops._pair_indices(self.n_fields)):
                pr = embs[i][j] * embs[j][i]
                prods.append(pr.sum(-1, keepdim=True) if self.reduce_sum else pr)
            x = torch.cat(prods, dim=-1)
        if self.bn is not None:
            x = tops._batch_norm(self.bn, x, training)
        return (tops.dnn_forward(self.dnn, torch.cat([x] + parts, dim=-1), training) @ self.dense.w("kernel")).reshape(-1)

    def _forward(self, staged, lo, hi, out):
        sp = self.stage_plan
        B = hi - lo
        add = self._linear_logits(staged, lo, hi)
        bufs = self._buffers(B)
        st = sp.status()
        R = (self.n_fields - 1) * self.emb_dim
        for j, (fc, master) in enumerate(zip(self.deep_cols, self.masters)):
            if isinstance(fc, VarLenSparseFeat):
                seq = staged.extra.get("ffm_seq:" + fc.name)
                seq = (staged.seq[fc.name] if seq is None else seq)[lo:hi]
                buf = bufs["pooled"][fc.name]
                ops.embed_pool(seq, master.view(master.shape[0], R), fc.combiner, out=buf, out_stride=buf.stride(0), status=st)
        desc = self._descriptors(staged, lo, hi, bufs)
        dense = staged.dense[lo:hi] if self.n_dense else None
        ops.ffm(None, self.masters, dim=self.emb_dim, scale=self._scale if self.bn is not None else None,
                shift=self._shift if self.bn is not None else None, dense=dense, n_dense=self.n_dense, reduce_sum=self.reduce_sum,
                out=bufs["dnn_in"], status=st, desc=desc, batch=B)
        ops.mlp(bufs["dnn_in"], self.dnn.kernels, self.dnn.biases, self.dnn.activation, head_w=self.dense.w('kernel'),
                add=add, global_bias=self.prediction.w('global_bias'), sigmoid_out=self.task == "binary",
                in_dim=self.dnn_in_dim, out=out)


def ONN(linear_feature_columns, dnn_feature_columns, dnn_hidden_units=(256, 128, 64), l2_reg_embedding=1e-5, l2_reg_linear=1e-5,
        l2_reg_dnn=0, dnn_dropout=0, seed=1024, use_bn=True, reduce_sum=False, task='binary', device=None):
    """Instantiates the Operation-aware Neural Networks architecture on the MI355X forward path."""
    m = _ONN(linear_feature_columns, dnn_feature_columns, dnn_hidden_units, dnn_dropout, seed, use_bn, reduce_sum, task, device)
    m.regularizers = {"embedding": float(l2_reg_embedding), "linear": float(l2_reg_linear), "dnn": float(l2_reg_dnn)}
    return m
