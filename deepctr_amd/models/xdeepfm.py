"""xDeepFM — same signature as ``deepctr.models.xdeepfm.xDeepFM`` (reference deepctr/models/xdeepfm.py:18-70).
Fixed-length features (round 4): TWO launches per call and no DNN input in HBM — ``dctr_cin_gather_fwd`` (CIN kernel: all layers on
f32 MFMA, its [samples, F0, D] tile read from the embedding tables, the Dense(1) over the maps taken on chip -> one logit per row)
and ``dctr_embed_mlp_fwd`` (ids -> DNN -> head, + linear logit + the CIN logit).  Otherwise (pooled / hashed-in-kernel features,
``fuse_cin = False``): fused gather (+ linear logit) -> dnn_in -> CIN kernel -> Dense(1) on the CIN maps -> DNN kernel with the head."""
import torch

from .. import ops
from .. import training as tops
from ..engine import EmbeddingStage
from ..layers.base import name_scope
from ..layers.core import DNN, Dense, PredictionLayer
from ..layers.interaction import CIN
from ._common import FeatureModel, FusedForward


class _xDeepFM(FusedForward, FeatureModel):
    _records_capable = False     # (the CIN / matrix-CrossNet launches read the fused launch's gather arguments: plain tables)
    def __init__(self, linear_feature_columns, dnn_feature_columns, dnn_hidden_units, cin_layer_size, cin_split_half,
                 cin_activation, seed, dnn_dropout, dnn_activation, dnn_use_bn, task, device):
        super(_xDeepFM, self).__init__("xDeepFM", list(linear_feature_columns) + list(dnn_feature_columns), device, task)
        with name_scope():
            self.build_linear(linear_feature_columns, seed)
            self.build_embeddings(dnn_feature_columns, seed)
            self.stage_plan = EmbeddingStage(self.tables, self.linear_tables, linear_feature_columns,
                                             dnn_feature_columns, device=self.device)
            sp = self.stage_plan
            self.dnn = self._add(DNN(dnn_hidden_units, dnn_activation, 0, dnn_dropout, dnn_use_bn, seed=seed,
                                     device=self.device).build_for(sp.in_dim))
            last = dnn_hidden_units[-1] if len(dnn_hidden_units) else sp.in_dim
            self.dense = self._add(Dense(1, use_bias=False, seed=seed, device=self.device).build_for(last))
            self.cin = None
            if len(cin_layer_size) > 0:
                dims = set(f.dim for f in sp.fields)
                if len(dims) != 1:
                    raise ValueError("CIN needs one embedding_dim for every sparse / sequence feature, got %s" % sorted(dims))
                self.cin_dim = dims.pop()
                self.cin = self._add(CIN(cin_layer_size, cin_activation, cin_split_half, 0, seed,
                                         device=self.device).build_for(len(sp.fields)))
                self.cin_out_dim = ops.cin_output_dim(list(cin_layer_size), cin_split_half)
                self.dense_1 = self._add(Dense(1, use_bias=False, seed=seed, device=self.device).build_for(self.cin_out_dim))
            self.prediction = self._add(PredictionLayer(task, device=self.device).build_for())
        self._buf = {}
        self._cin_ws = None         # layer 0's folded filter rows (dctr_cin_args_t.workspace): written by the first CIN launch after _begin()
        self._cin_ws_ready = False
        self._cin_gather_ok = None  # dctr_cin_fwd_supported's answer for the two-launch form (asked once)
        self._fast_g = None         # the marshalled gather arguments of the fused launch being issued (FusedForward)
        self.fuse_cin = True        # False: the route through dnn_in (gather -> HBM -> CIN / DNN launches)
        if len(dnn_hidden_units) > 0:
            self._init_fused(dnn_hidden_units, dnn_activation)

    def _cin_fuse_ok(self):
        """The two-launch form needs dctr_cin_gather_fwd to take the CIN with its head: the library answers (dctr_cin_fwd_supported) —
        asked once, for the summary a fused launch's gather arguments carry (ids pre-hashed, plain tables)."""
        if not (self.fuse_cin and self.fused):
            return False
        if self.cin is None:
            return True
        if self._cin_gather_ok is None:
            sp = self.stage_plan
            self._cin_gather_ok = ops.cin_supported(
                len(sp.fields), self.cin_dim, list(self.cin.layer_size), self.cin.split_half, self.cin.activation, fused_head=True,
                gather=dict(n_fields=len(sp.fields), uniform_dim=sp.uniform_dim, all_dim4=sp.all_dim4, any_hash=0,
                            any_identity=bool(sp.pooled_fields), any_pitch=0))
        return self._cin_gather_ok

    def _prehash(self, B):
        # hashed SparseFeat: ALWAYS hashed by the dctr_hash_fields launch in front (the CIN launch takes plain rows only)
        sp = self.stage_plan
        return bool(sp.any_hash and sp.uniform_dim in (4, 8, 16, 32, 64))

    def _fast_path(self, staged):
        return self._cin_fuse_ok() and super(_xDeepFM, self)._fast_path(staged) and (not self.stage_plan.any_hash or self._prehash(0))

    def _rows_per_launch(self, staged, batch_size):
        # CIN's persistent-round efficiency peaks around 65,536 rows per launch; the one-launch DNN takes any span
        return FeatureModel._rows_per_launch(self, staged, batch_size)

    def _cin_workspace(self):
        if self._cin_ws is None:
            need = ops.cin_workspace_bytes(len(self.stage_plan.fields), self.cin_dim, list(self.cin.layer_size), self.cin.split_half)
            self._cin_ws = torch.empty(max(need // 4, 1), dtype=torch.float32, device=self.device)
        return self._cin_ws

    def _extra_logit_buffers(self, B):
        """The CIN logit vector the fused head adds."""
        if self.cin is None:
            return []
        bufs = self._buf.get(("logit", B))
        if bufs is None:
            if len(self._buf) >= 8:
                self._buf.clear()
            bufs = self._buf[("logit", B)] = torch.zeros(B, dtype=torch.float32, device=self.device)
        return [bufs]

    def _launch_extra(self, staged, lo, hi, bufs):
        """The CIN logit of rows [lo, hi): dctr_cin_gather_fwd on the gather arguments of the fused launch (issued in front of it)."""
        if self.cin is None:
            return
        ok = ops.cin_gather(self._fast_g, self.cin.filters, self.cin.biases, list(self.cin.layer_size), self.cin.split_half,
                            self.cin.activation, self.cin_dim, self.dense_1.w('kernel'), bufs[0], self._cin_workspace(), self._cin_ws_ready)
        if not ok:
            raise RuntimeError("dctr_cin_gather_fwd declined a shape _cin_fuse_ok() admitted")
        self._cin_ws_ready = True

    # CIN's persistent-round efficiency grows with the launch (C3: 300 us per 4096-row launch, 257 us per 4096 rows at 65,536)
    span_rows = 65536

    def _begin(self):
        super(_xDeepFM, self)._begin()
        self._cin_ws_ready = False  # the filters may have moved since the last call

    def _forward(self, staged, lo, hi, out):
        if self._fast_path(staged) and self._forward_fast(staged, lo, hi, out):
            return
        ws = self.stage_plan.run(staged, lo, hi)
        B = hi - lo
        add = self._logits_to_add(ws)
        if self.cin is not None:
            bufs = self._buf.get(B)
            if bufs is None:
                if len(self._buf) >= 4:            # ragged remainder sizes (N % span) must not pile up per-B buffers
                    self._buf.clear()
                bufs = self._buf[B] = (torch.zeros(B, self.cin_out_dim, dtype=torch.float32, device=self.device),
                                       torch.zeros(B, dtype=torch.float32, device=self.device))
            maps, logit = bufs
            self._cin_workspace()
            ops.cin(ws["dnn_in"], [f.reshape(-1, f.shape[-1]) for f in self.cin.filters], self.cin.biases,
                    list(self.cin.layer_size), self.cin.split_half, self.cin.activation, fields=len(self.stage_plan.fields),
                    dim=self.cin_dim, out=maps, workspace=self._cin_ws, workspace_ready=self._cin_ws_ready)
            self._cin_ws_ready = True
            ops.mlp(maps, [], [], "linear", head_w=self.dense_1.w('kernel'), in_dim=self.cin_out_dim, out=logit)
            add.append(logit)
        ops.mlp(ws["dnn_in"], self.dnn.kernels, self.dnn.biases, self.dnn.activation, dice=self.dnn.dice_params(), bn=self.dnn.bn_params(),
                head_w=self.dense.w('kernel'), add=add, global_bias=self.prediction.w('global_bias'),
                sigmoid_out=self.task == "binary", in_dim=self.stage_plan.in_dim, out=out)

    def _autograd_logit(self, staged, lo, hi, parts, extra, training):       # xdeepfm.py:53-66: the DNN logit + Dense(1) over the CIN maps
        logit = super(_xDeepFM, self)._autograd_logit(staged, lo, hi, parts, extra, training)
        if self.cin is None:
            return logit
        x0 = torch.stack(parts[:len(self.stage_plan.fields)], dim=1)             # [B,F,D]
        hidden, finals = x0, []
        n = len(self.cin.layer_size)
        for i, (w, b) in enumerate(zip(self.cin.filters, self.cin.biases)):
            z = torch.einsum("bid,bjd->bdij", x0, hidden).reshape(x0.shape[0], x0.shape[2], -1)
            cur = tops._act(self.cin.activation, z @ w[0] + b).transpose(1, 2)
            H = cur.shape[1]
            if self.cin.split_half:
                if i != n - 1:
                    hidden, direct = cur[:, :H // 2], cur[:, H // 2:]
                else:
                    hidden, direct = None, cur
            else:
                hidden, direct = cur, cur
            finals.append(direct)
        return logit + (torch.cat(finals, dim=1).sum(-1) @ self.dense_1.w("kernel")).reshape(-1)

    # ---- the HIP training step (training_hip.HipTrainer): the DNN step with the CIN in front and dctr_cin_bwd behind -------------------
    def _hip_supported(self):
        sp, cin = self.stage_plan, self.cin
        # (the library's answer — dctr_cin_fwd_supported: any embedding width, in slices of d past 128)
        if cin is not None and (not ops.cin_supported(len(sp.fields), self.cin_dim, list(cin.layer_size), cin.split_half, cin.activation)
                                or cin.activation not in ("relu", "linear", "sigmoid", "tanh")):
            return False
        return self._hip_family_ok()

    def _hip_params(self, tr):
        if self.cin is not None:
            tr.own.update(cin_f=[tr.param(f, getattr(self, "regularizers", {}).get("cin", 0.0)) for f in self.cin.filters],
                          cin_b=[tr.param(b) for b in self.cin.biases], head1=tr.param(self.dense_1.w("kernel")))

    def _hip_forward_backward(self, tr, staged, lo, hi, ws, buf, y, binary):
        sp, cin, own = self.stage_plan, self.cin, tr.own
        add = self._hip_add(ws)
        if cin is not None:             # xdeepfm.py:52-66: CIN over the embeddings -> Dense(1) -> extra logit
            B, nf, dim, dev = hi - lo, len(sp.fields), self.cin_dim, self.device
            if "maps" not in buf:
                buf.update(maps=torch.empty(B, self.cin_out_dim, dtype=torch.float32, device=dev),
                           dmaps=torch.empty(B, self.cin_out_dim, dtype=torch.float32, device=dev),
                           cin_logit=torch.empty(B, dtype=torch.float32, device=dev),
                           # layer activations written by the forward CIN kernel for dctr_cin_bwd; None beyond the 2-GiB buffer-descriptor
                           # range dctr_cin_fwd takes for save_y: dctr_cin_bwd then re-runs the forward into its own workspace
                           cin_y=[torch.empty(B * dim, h, dtype=torch.float32, device=dev) for h in cin.layer_size]
                           if B * dim * max(cin.layer_size) * 4 < 2 ** 31 else None)
            filt = [f.reshape(-1, f.shape[-1]) for f in cin.filters]
            ops.cin(ws["dnn_in"], filt, cin.biases, list(cin.layer_size), cin.split_half, cin.activation, fields=nf, dim=dim,
                    out=buf["maps"], save_y=buf["cin_y"])
            ops.mlp(buf["maps"], [], [], "linear", head_w=own["head1"].w, in_dim=self.cin_out_dim, out=buf["cin_logit"])
            add.append(buf["cin_logit"])
        tr._dnn_step(ws["dnn_in"], sp.in_dim, buf, y, binary, add=add)
        if cin is not None:
            ops.dense1_bwd(buf["maps"], self.cin_out_dim, own["head1"].w, buf["dlogit"], buf["dmaps"], own["head1"].g)
            ops.cin_bwd(ws["dnn_in"], filt, cin.biases, list(cin.layer_size), cin.split_half, cin.activation, buf["dmaps"],
                        [p.g.reshape(-1, p.g.shape[-1]) for p in own["cin_f"]], [p.g for p in own["cin_b"]], dx=buf["dx"],
                        accumulate=True, fields=nf, dim=dim, saved_y=buf["cin_y"])


def xDeepFM(linear_feature_columns, dnn_feature_columns, dnn_hidden_units=(256, 128, 64), cin_layer_size=(128, 128,),
            cin_split_half=True, cin_activation='relu', l2_reg_linear=0.00001, l2_reg_embedding=0.00001, l2_reg_dnn=0,
            l2_reg_cin=0, seed=1024, dnn_dropout=0, dnn_activation='relu', dnn_use_bn=False, task='binary', device=None):
    """Instantiates the xDeepFM architecture on the MI355X forward path."""
    m = _xDeepFM(linear_feature_columns, dnn_feature_columns, dnn_hidden_units, cin_layer_size, cin_split_half,
                 cin_activation, seed, dnn_dropout, dnn_activation, dnn_use_bn, task, device)
    m.regularizers = {"embedding": float(l2_reg_embedding), "linear": float(l2_reg_linear), "dnn": float(l2_reg_dnn),
                      "cin": float(l2_reg_cin)}
    return m
