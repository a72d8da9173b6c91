"""IFM (Input-aware Factorization Machine) — same signature as ``deepctr.models.ifm.IFM`` (reference deepctr/models/ifm.py:21-74): a DNN
over the sparse / sequence embeddings gives one factor per field, m = F * softmax(DNN(x) . dense/kernel); every field's embedding and
every first-order weight is multiplied by its factor before the FM and the linear sum.

As in the reference:
  * the deep part sees the embeddings only (``combined_dnn_input(sparse_embedding_list, [])``): a DenseFeat of ``dnn_feature_columns``
    declares an input, is accepted in the feed, and feeds nothing unless ``linear_feature_columns`` names it too;
  * the factor meets the first-order terms BY POSITION, not by name: term k of ``linear_feature_columns`` (its SparseFeat, then its
    VarLenSparseFeat, per embedding group) is multiplied by m[k], the factor of field k of ``dnn_feature_columns`` in the same order —
    a linear list in another order pairs a feature's weight with another feature's factor.  The dense linear term is not refined.
Unlike the reference, a linear part whose number of sparse / sequence features is neither 0 nor the deep part's is refused when the
model is built (the reference fails in the first batch with a broadcast error, or broadcasts silently when one of the counts is 1).

Forward: fused gather -> dnn_in (= the F*d embedding columns; the dense linear term as its own [B] vector) -> the DNN kernel, last
hidden layer to HBM -> ONE ``dctr_ifm_fwd`` launch: factor projection, softmax, refined FM and linear terms, bias, sigmoid.

fit() runs the autograd step; in it the factor projection, the softmax, the refined FM and the refined first-order terms are one
differentiable HIP op (``training.input_aware_fm``: dctr_ifm_fwd forward, dctr_ifm_bwd backward) from ``training.IFM_HIP_MIN_ROWS`` rows
on (DIFM: ``DIFM_HIP_MIN_ROWS``), and the torch ops of ``_autograd_logit`` everywhere else (profiles/ifm_bwd.txt)."""
from collections import OrderedDict

import numpy as np
import torch

from .. import ops
from .. import training as tops
from ..engine import EmbeddingStage, _column, _fit_int32, _ids_from_column, prehashed_on_host
from ..feature_column import DenseFeat, SparseFeat, VarLenSparseFeat
from ..layers.base import name_scope
from ..layers.core import DNN, Dense, PredictionLayer
from ._common import FeatureModel


def position_order(feature_columns):
    """The sparse / sequence columns in the order ``input_from_feature_columns`` lists their embeddings (reference inputs.py:175-181,
    feature_column.py:213-233): per embedding group in first-appearance order, the group's SparseFeat, then its VarLenSparseFeat."""
    groups = OrderedDict()
    for kind in (SparseFeat, VarLenSparseFeat):
        for fc in feature_columns:
            if isinstance(fc, kind):
                groups.setdefault(fc.group_name, []).append(fc)
    return [fc for g in groups.values() for fc in g]


class InputAwareModel(FeatureModel):
    """What IFM and DIFM share: the stage over the embeddings, the DNN, the first-order terms by position, the ``dctr_ifm_fwd`` call."""

    def _build_common(self, what, linear_feature_columns, dnn_feature_columns, dnn_hidden_units, dnn_activation, dnn_use_bn, dnn_dropout,
                      seed):
        """Linear part, embeddings, stage and the per-position plan; returns nothing (the subclass adds its layers in the reference's
        creation order, which fixes the auto-numbered names)."""
        self.lin_positions = position_order(linear_feature_columns)
        deep = position_order(dnn_feature_columns)
        F, F_lin = len(deep), len(self.lin_positions)
        if F_lin and F_lin != F:
            raise ValueError("%s: linear_feature_columns holds %d sparse / sequence feature(s), dnn_feature_columns %d: the input-aware "
                             "factor refines the first-order terms by position and needs as many of them as fields, or none"
                             % (what, F_lin, F))
        self.build_linear(linear_feature_columns, seed)
        self.build_embeddings(dnn_feature_columns, seed)
        # the stage sees the embeddings as its deep columns (in_dim = F*d) and the DenseFeat of the linear part as its linear columns:
        # its `lin` vector is dense . linear_kernel, unrefined
        self.stage_plan = EmbeddingStage(self.tables, self.linear_tables, [fc for fc in linear_feature_columns if isinstance(fc, DenseFeat)],
                                         [fc for fc in dnn_feature_columns if not isinstance(fc, DenseFeat)], device=self.device)
        sp = self.stage_plan
        dims = sorted(set(f.dim for f in sp.fields))
        if len(dims) > 1:
            raise ValueError("%s concatenates the sparse / sequence embeddings on axis 1: they need one embedding_dim, got %s" % (what, dims))
        self.n_fields, self.emb_dim = F, dims[0]
        assert [f.fc.name for f in sp.fields] == [fc.name for fc in deep]
        self.dnn = self._add(DNN(dnn_hidden_units, dnn_activation, 0, dnn_dropout, dnn_use_bn, seed=seed,
                                 device=self.device).build_for(sp.in_dim))
        self.hidden_dim = int(dnn_hidden_units[-1])

    # -- staging: the shared stage + the ids of the first-order terms, hashed once per feature ---------------------------------------
    def _hashes(self, fc):
        return bool(fc.use_hash and not prehashed_on_host(fc))

    def _stage_inputs(self, feed, staged):
        sp, dev = self.stage_plan, self.device
        sp.stage(feed, staged)
        if not self.lin_positions:
            return
        cols = []
        for fc in self.lin_positions:
            if isinstance(fc, VarLenSparseFeat):
                sp.stage_varlen(feed, staged, fc)
                cols.append(None)
                continue
            a = _column(feed, fc.name).reshape(-1)
            if a.shape[0] != staged.n:
                raise ValueError("feature %r has %d rows, expected %d" % (fc.name, a.shape[0], staged.n))
            cols.append(_ids_from_column(a, fc, False, dev))
        real = [c for c in cols if c is not None]
        any_hash = any(self._hashes(fc) for fc in self.lin_positions if isinstance(fc, SparseFeat))
        dt = torch.int32 if (_fit_int32(real) and not any_hash) else torch.int64
        mat = torch.zeros(staged.n, len(cols), dtype=dt, device=dev)          # [N, F]: rows on axis 0 (fit() permutes staged.extra so)
        for k, (fc, c) in enumerate(zip(self.lin_positions, cols)):
            if c is None:
                continue
            t = c if isinstance(c, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(c)).to(dev)
            if self._hashes(fc):
                t = ops.hash_bucket(t.contiguous() if t.dtype in (torch.int32, torch.int64) else t.to(torch.int64),
                                    fc.vocabulary_size, False)
            mat[:, k] = t.to(dt)
        staged.extra["ifm_lin_ids"] = mat

    def _pipeline(self, x, batch_size):
        return None

    def _lin_table(self, fc):
        return self.linear_tables[fc.embedding_name].embeddings

    def _buffers(self, B):
        def alloc():
            bufs = {"hidden": torch.zeros(B, self.hidden_dim, dtype=torch.float32, device=self.device),
                    "pooled": {fc.name: torch.zeros(B, 1, dtype=torch.float32, device=self.device)
                               for fc in self.lin_positions if isinstance(fc, VarLenSparseFeat)}}
            self._more_buffers(B, bufs)
            return bufs
        return self._per_batch(B, alloc)

    def _more_buffers(self, B, bufs):
        pass

    def _lin_descriptors(self, staged, lo, hi, bufs):
        """dctr_ifm_lin_t array of rows [lo, hi): cached per (staged id matrix, lo) beside the per-B buffers it points into."""
        ids = staged.extra["ifm_lin_ids"]
        key = (ids.data_ptr(), lo)
        cache = bufs.setdefault("desc", OrderedDict())
        desc = cache.get(key)
        if desc is None:
            terms = []
            for k, fc in enumerate(self.lin_positions):
                if isinstance(fc, VarLenSparseFeat):
                    terms.append(bufs["pooled"][fc.name])
                else:
                    terms.append((self._lin_table(fc), ids[lo:hi, k]))
            while len(cache) >= 64:
                cache.popitem(last=False)
            desc = cache[key] = ops.make_ifm_lin(terms, hi - lo, self.device)
        return desc

    def linear_terms(self, staged, lo, hi):
        """torch ops (autograd_logits): the [B, F_lin] first-order terms of rows [lo, hi) in position order, or None."""
        if not self.lin_positions:
            return None
        ids = staged.extra["ifm_lin_ids"]
        out = []
        for k, fc in enumerate(self.lin_positions):
            lt = self._lin_table(fc).reshape(-1)
            if isinstance(fc, VarLenSparseFeat):
                rows = tops._rows_for(fc, staged.seq[fc.name][lo:hi], True)
                length = staged.length[fc.length_name][lo:hi] if fc.length_name is not None else None
                weight = staged.weight[fc.weight_name][lo:hi] if fc.weight_name is not None else None
                out.append(tops._pool(lt[rows].unsqueeze(-1), fc, rows != 0, length, weight).reshape(-1))
            else:
                out.append(lt[ids[lo:hi, k].to(torch.int64)])
        return torch.stack(out, dim=1)

    def _autograd_logit(self, staged, lo, hi, parts, extra, training):       # ifm.py:55-72, difm.py:59-80
        x = torch.stack(parts[:self.n_fields], dim=1)              # [B,F,d]
        h = tops.dnn_forward(self.dnn, x.reshape(x.shape[0], -1), training)
        if tops._ifm_on_hip(x, self._hip_min_rows()):              # one differentiable HIP op: dctr_ifm_fwd / dctr_ifm_bwd
            sources, softmax = self._factor_sources(x, h)
            return tops.input_aware_fm(x, sources, softmax, terms=self.linear_terms(staged, lo, hi))
        m = self._autograd_factor(x, h)
        r = x * m.unsqueeze(-1)
        logit = 0.5 * (r.sum(1).pow(2) - (r * r).sum(1)).sum(-1)
        terms = self.linear_terms(staged, lo, hi)                   # [B,F] in position order: paired with m by position
        if terms is not None:
            logit = logit + (terms * m).sum(-1)
        return logit                                                # (the stage's linear part holds the DenseFeat only: not refined)

    def _stage_run(self, staged, lo, hi):
        """The stage's launches and the pooled first-order terms: (workspace, per-B buffers, add vectors, descriptors or None)."""
        sp = self.stage_plan
        ws = sp.run(staged, lo, hi)
        bufs = self._buffers(hi - lo)
        desc = None
        if self.lin_positions:
            st = sp.status()
            for fc in self.lin_positions:
                if isinstance(fc, VarLenSparseFeat):
                    sp._pool(fc, staged, lo, hi, self._lin_table(fc), None, bufs["pooled"][fc.name], None, st)
            desc = self._lin_descriptors(staged, lo, hi, bufs)
        return ws, bufs, self._logits_to_add(ws), desc

    def _dnn_hidden(self, ws, bufs):
        sp = self.stage_plan
        return ops.mlp(ws["dnn_in"], self.dnn.kernels, self.dnn.biases, self.dnn.activation, dice=self.dnn.dice_params(),
                       bn=self.dnn.bn_params(), in_dim=sp.in_dim, out=bufs["hidden"])


class _IFM(InputAwareModel):
    def __init__(self, linear_feature_columns, dnn_feature_columns, dnn_hidden_units, seed, dnn_dropout, dnn_activation, dnn_use_bn, task,
                 device):
        linear_feature_columns, dnn_feature_columns = list(linear_feature_columns or []), list(dnn_feature_columns or [])
        if not len(dnn_hidden_units) > 0:
            raise ValueError("dnn_hidden_units is null!")
        if not position_order(dnn_feature_columns):
            raise ValueError("there are no sparse features")
        super(_IFM, self).__init__("IFM", linear_feature_columns + dnn_feature_columns, device, task)
        with name_scope():
            self._build_common("IFM", linear_feature_columns, dnn_feature_columns, dnn_hidden_units, dnn_activation, dnn_use_bn,
                               dnn_dropout, seed)
            self.dense = self._add(Dense(self.n_fields, use_bias=False, seed=seed, device=self.device).build_for(self.hidden_dim))
            self.prediction = self._add(PredictionLayer(task, device=self.device).build_for())

    def _autograd_factor(self, x, h):
        return x.shape[1] * torch.softmax(h @ self.dense.w("kernel"), dim=1)

    def _factor_sources(self, x, h):
        return [(h, self.dense.w("kernel"))], True

    def _hip_min_rows(self):
        return tops.IFM_HIP_MIN_ROWS

    def _forward(self, staged, lo, hi, out):
        ws, bufs, add, desc = self._stage_run(staged, lo, hi)
        hidden = self._dnn_hidden(ws, bufs)
        ops.ifm(ws["dnn_in"], self.n_fields, self.emb_dim, sources=[(hidden, self.dense.w('kernel'))], softmax=True,
                lin=self.lin_positions, lin_desc=desc, add=add, global_bias=self.prediction.w('global_bias'),
                sigmoid_out=self.task == "binary", out=out, status=self.stage_plan.status())


def IFM(linear_feature_columns, dnn_feature_columns, dnn_hidden_units=(256, 128, 64), l2_reg_linear=0.00001, l2_reg_embedding=0.00001,
        l2_reg_dnn=0, seed=1024, dnn_dropout=0, dnn_activation='relu', dnn_use_bn=False, task='binary', device=None):
    """Instantiates the IFM Network architecture on the MI355X forward path."""
    m = _IFM(linear_feature_columns, dnn_feature_columns, dnn_hidden_units, seed, dnn_dropout, dnn_activation, dnn_use_bn, task, device)
    m.regularizers = {"embedding": float(l2_reg_embedding), "linear": float(l2_reg_linear), "dnn": float(l2_reg_dnn)}
    return m
