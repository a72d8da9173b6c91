"""CPU: BST / Transformer / LayerNormalization — the NumPy oracle (tests/ref_bst.py) against the reference's own outputs
(tests/golden/model_bst_*.npz, transformer_layer.npz; scripts/make_golden_bst.py) and the conditions that script records, the torch
restatement the training path uses against the oracle in float64, the API contract, and the C ABI's argument checks (no launch)."""
import ctypes
import inspect
import json

import numpy as np
import pytest
import torch

from tests import ref_bst as RB
from tests.spec import columns_from_spec
from tests.test_autoint_cpu import att_rows
from tests.util import assert_close, golden_meta, load_golden, sigmoid_inv

BST_FIXTURES = ["model_bst_base", "model_bst_t2", "model_bst_h1", "model_bst_hash", "model_bst_bn", "model_bst_regression",
                "model_bst_one", "model_bst_extra"]
LAYER_TAGS = ["all", "nope", "nores", "noffn", "noln", "blind", "mean", "sum", "masking", "cross"]


def build_bst(meta, device):
    from deepctr_amd.models import BST
    return BST(columns_from_spec(meta["dnn"]), meta["extra_args"][0], device=device, **meta["kwargs"])


def fixture_feed(g):
    return {k[5:]: v for k, v in g.items() if k.startswith("feed/")}


def fixture_weights(g):
    return {k[2:]: v for k, v in g.items() if k.startswith("w/")}


def layer_case(g, tag):
    """(cfg, queries, keys, query mask, key mask, weights in ref_bst's names, y) of a transformer_layer.npz case."""
    cfg = json.loads(bytes(g[tag + "/cfg"]).decode())
    q, k = g[tag + "/queries"], g[tag + "/keys"]
    T = q.shape[1]
    if tag + "/query_mask" in g:
        qm, km = g[tag + "/query_mask"], g[tag + "/key_mask"]
    else:
        qm, km = RB.sequence_mask(g[tag + "/query_lengths"], T), RB.sequence_mask(g[tag + "/key_lengths"], T)
    named = {n[len(tag) + 3:]: v for n, v in g.items() if n.startswith(tag + "/w/")}
    w = {k2: named["transformer/" + k2] for k2 in ("query", "key", "value", "fw1", "fw2") if "transformer/" + k2 in named}
    if cfg["use_layer_norm"]:
        w["ln_gamma"], w["ln_beta"] = named["layer_normalization/gamma"], named["layer_normalization/beta"]
    if cfg["use_positional_encoding"]:
        w["pe_q"], w["pe_k"] = named["position_encoding/lookup_table"], named["position_encoding_1/lookup_table"]
    return cfg, q, k, qm, km, w, named, g[tag + "/y"]


def layer_flags(cfg):
    return {k: cfg[k] for k in ("use_positional_encoding", "use_res", "use_feed_forward", "use_layer_norm", "blinding", "output_type")}


@pytest.mark.parametrize("name", BST_FIXTURES)
def test_oracle_matches_reference_code_and_the_fixture_conditions_hold(name):
    g = load_golden(name)
    meta = golden_meta(g)
    ref = g["y"]
    stats = []
    y64 = RB.run_fixture(g, np.float64, stats=stats)
    assert y64.shape == ref.shape
    assert_close(y64, ref, rtol=1e-4, atol=1e-6, what=name + " float64")
    assert_close(RB.run_fixture(g, np.float32), ref, rtol=1e-4, atol=1e-6, what=name + " float32")
    if meta["kwargs"].get("task") != "regression":
        assert ref.min() > 1e-3 and ref.max() < 1 - 1e-3
        assert_close(sigmoid_inv(y64), sigmoid_inv(ref), rtol=1e-4, atol=2e-5, what=name + " logit")
    feed = fixture_feed(g)
    rows = att_rows(meta, feed, ref.shape[0])
    assert rows.sum() >= ref.shape[0] // 2
    # the comparison is no test of 1 / sqrt(1e-9): every row that enters a LayerNormalization has a real variance
    assert len(stats) == meta["kwargs"]["transformer_num"] * 2 * ref.shape[0] * 6 and min(stats) >= 1e-3
    lens = feed["seq_length"].reshape(-1)
    assert set([0, 1, 6, 9]) <= set(lens.tolist())


@pytest.mark.parametrize("tag", LAYER_TAGS)
def test_layer_oracle_matches_reference_code(tag):
    g = load_golden("transformer_layer")
    cfg, q, k, qm, km, w, _, y = layer_case(g, tag)
    for dt in (np.float32, np.float64):
        stats = []
        got = RB.transformer(q, k, w, cfg["head_num"], qm, km, dtype=dt, stats=stats, **layer_flags(cfg))
        assert got.shape == y.shape
        assert_close(got, y, rtol=1e-4, atol=2e-6, what="transformer " + tag)
    # every row that enters a LayerNormalization has a real variance here too (none does without use_layer_norm)
    n_ln = (2 if cfg["use_feed_forward"] else 1) * q.shape[0] * q.shape[1] if cfg["use_layer_norm"] else 0
    assert len(stats) == n_ln and (not stats or min(stats) >= 1e-3)
    if tag in ("all", "cross"):
        assert not np.array_equal(w["pe_q"], w["pe_k"]) and not np.allclose(w["ln_gamma"], 1) and np.abs(w["ln_beta"]).min() > 0
    if tag == "masking":
        assert not qm[0].any() and not km[1].any()
    else:
        assert set([0, 1, 5, 8]) <= set(g[tag + "/query_lengths"].tolist())


def _to_float64(layer):
    for k in list(layer._weights):
        layer._weights[k] = layer._weights[k].double()
    for sub in layer._sublayers:
        _to_float64(sub)


# (model_bst_hash is left to the GPU suite: the integer Hash runs inside the HIP kernels only)
@pytest.mark.parametrize("name", [n for n in BST_FIXTURES if n != "model_bst_hash"])
def test_torch_restatement_matches_oracle_in_float64(name):
    from deepctr_amd import engine, training
    g = load_golden(name)
    meta = golden_meta(g)
    model = build_bst(meta, torch.device("cpu"))
    model.set_weights_by_name(fixture_weights(g))
    for layer in model.layers:
        _to_float64(layer)
    n = g["y"].shape[0]
    staged = engine.Staged(n)
    model._stage_inputs(fixture_feed(g), staged)
    model._begin()
    with torch.no_grad():
        logit = training.model_logits(model, staged, 0, n)
    assert logit.dtype == torch.float64
    ref = RB.run_fixture(g, np.float64, task="regression").reshape(-1)
    assert_close(logit.numpy().reshape(-1), ref, rtol=1e-6, atol=1e-7, what=name + " model_logits")


@pytest.mark.parametrize("tag", LAYER_TAGS)
def test_torch_layer_restatement_matches_oracle_in_float64(tag):
    from deepctr_amd import training
    from deepctr_amd.layers import Transformer
    g = load_golden("transformer_layer")
    cfg, q, k, qm, km, w, named, _ = layer_case(g, tag)
    layer = Transformer(device="cpu", **cfg)
    layer.build([(None,) + q.shape[1:], (None,) + k.shape[1:]])
    # (the layer names count the layers built before in the process: match by weight name within the creation order)
    order = [n for n, _ in layer.named_weights()]
    assert [n.rsplit("/", 1)[1] for n in order] == [n.rsplit("/", 1)[1] for n in named]
    layer.set_weights(list(named.values()))
    _to_float64(layer)
    with torch.no_grad():
        got = training._transformer(layer, torch.from_numpy(q).double(), torch.from_numpy(k).double(), torch.from_numpy(qm),
                                    torch.from_numpy(km)).numpy()
    ref = RB.transformer(q, k, w, cfg["head_num"], qm, km, dtype=np.float64, **layer_flags(cfg))
    assert_close(got, ref, rtol=1e-6, atol=1e-7, what="torch transformer " + tag)


def test_signature_defaults_match_the_reference():
    from deepctr_amd.layers import LayerNormalization, PositionEncoding, Transformer
    from deepctr_amd.models import BST
    params = inspect.signature(BST).parameters
    want = dict(transformer_num=1, att_head_num=8, use_bn=False, dnn_hidden_units=(256, 128, 64), dnn_activation='relu', l2_reg_dnn=0,
                l2_reg_embedding=1e-6, dnn_dropout=0.0, seed=1024, task='binary')
    names = list(params)
    assert names[:2] == ["dnn_feature_columns", "history_feature_list"]
    assert names[2:2 + len(want)] == list(want) and names[2 + len(want):] == ["device"]
    for k, v in want.items():
        assert params[k].default == v, k
    lp = inspect.signature(Transformer.__init__).parameters
    want = [("att_embedding_size", 1), ("head_num", 8), ("dropout_rate", 0.0), ("use_positional_encoding", True), ("use_res", True),
            ("use_feed_forward", True), ("use_layer_norm", False), ("blinding", True), ("seed", 1024), ("supports_masking", False),
            ("attention_type", "scaled_dot_product"), ("output_type", "mean")]
    assert [(k, lp[k].default) for k in list(lp)[1:1 + len(want)]] == want
    pp = inspect.signature(PositionEncoding.__init__).parameters
    assert [(k, pp[k].default) for k in list(pp)[1:4]] == [("pos_embedding_trainable", True), ("zero_pad", False), ("scale", True)]
    np_ = inspect.signature(LayerNormalization.__init__).parameters
    assert [(k, np_[k].default) for k in list(np_)[1:5]] == [("axis", -1), ("eps", 1e-9), ("center", True), ("scale", True)]


def test_construction_errors():
    from deepctr_amd.feature_column import SparseFeat, VarLenSparseFeat
    from deepctr_amd.layers import Transformer
    from deepctr_amd.models import BST
    item, cate = SparseFeat("item_id", 10, 8), SparseFeat("cate_id", 5, 4)
    hist = lambda length_name: [VarLenSparseFeat(SparseFeat("hist_item_id", 10, 8, embedding_name="item_id"), 4, length_name=length_name),   # noqa: E731
                                VarLenSparseFeat(SparseFeat("hist_cate_id", 5, 4, embedding_name="cate_id"), 4, length_name=length_name)]
    with pytest.raises(ValueError, match="history_feature_list"):
        BST([item, cate], ["item_id", "cate_id"], device="cpu")
    with pytest.raises(ValueError, match="seq_length"):          # (the reference: KeyError from features["seq_length"])
        BST([item, cate] + hist("hist_len"), ["item_id", "cate_id"], att_head_num=2, device="cpu")
    with pytest.raises(ValueError, match="att_embedding_size \\* head_num must equal"):
        BST([item, cate] + hist("seq_length"), ["item_id", "cate_id"], att_head_num=8, device="cpu")        # 12 % 8
    BST([item, cate] + hist("seq_length"), ["item_id", "cate_id"], att_head_num=4, device="cpu")
    with pytest.raises(ValueError, match="head_num must be a int > 0"):
        Transformer(head_num=0)
    for kind in ("cos", "ln", "additive"):
        with pytest.raises(NotImplementedError, match=kind):
            Transformer(attention_type=kind)
    with pytest.raises(ValueError, match="attention_type must be"):
        Transformer(attention_type="dot")
    layer = Transformer(3, 2, device="cpu")
    with pytest.raises(ValueError, match="att_embedding_size \\* head_num must equal"):
        layer.build([(None, 4, 7), (None, 4, 7), (None, 1), (None, 1)])


@pytest.mark.parametrize("name", BST_FIXTURES)
def test_weight_names_and_shapes_match_the_fixture(name):
    g = load_golden(name)
    model = build_bst(golden_meta(g), torch.device("cpu"))
    mine = {k: tuple(v.shape) for k, v in model.get_weights_by_name().items()}
    ref = {k: tuple(v.shape) for k, v in fixture_weights(g).items()}
    assert mine == ref
    assert any(k.endswith("position_encoding_1/lookup_table") for k in mine) and "layer_normalization/gamma" in mine


def test_layer_contract():
    from deepctr_amd.layers import LayerNormalization, PositionEncoding, Transformer, custom_objects
    for cls in (Transformer, PositionEncoding, LayerNormalization):
        assert custom_objects[cls.__name__] is cls
    layer = Transformer(3, 2, dropout_rate=0.1, use_layer_norm=True, blinding=False, output_type=None, device="cpu")
    layer.build([(None, 5, 6), (None, 5, 6), (None, 1), (None, 1)])
    got = [(n.rsplit("/", 1)[1], tuple(t.shape)) for n, t in layer.named_weights()]
    assert got == [("query", (6, 6)), ("key", (6, 6)), ("value", (6, 6)), ("fw1", (6, 24)), ("fw2", (24, 6)), ("gamma", (6,)), ("beta", (6,)),
                   ("lookup_table", (5, 6)), ("lookup_table", (5, 6))]
    assert layer.seq_len_max == 5 and layer.num_units == 6
    assert layer.compute_output_shape([(None, 5, 6)] * 2) == (None, 1, 6)       # the reference's answer for every output_type
    assert layer.compute_mask(None, None) is None
    cfg = layer.get_config()
    want = dict(att_embedding_size=3, head_num=2, dropout_rate=0.1, use_res=True, use_positional_encoding=True, use_feed_forward=True,
                use_layer_norm=True, seed=1024, supports_masking=False, blinding=False, attention_type="scaled_dot_product",
                output_type=None)
    assert {k: cfg[k] for k in want} == want
    # the positional tables start equal, at the sinusoid of sequence.py:667-673
    pq, pk = layer.query_pe.w("lookup_table").numpy(), layer.key_pe.w("lookup_table").numpy()
    assert np.array_equal(pq, pk) and pq[0, 0] == 0 and pq[0, 1] == 1 and abs(pq[1, 0] - np.sin(1.0)) < 1e-6
    bare = Transformer(3, 2, use_feed_forward=False, use_positional_encoding=False, device="cpu")
    bare.build([(None, 5, 6)] * 2)
    assert [n.rsplit("/", 1)[1] for n, _ in bare.named_weights()] == ["query", "key", "value"]
    pe = PositionEncoding(zero_pad=True, device="cpu")
    pe.build((None, 4, 6))
    assert not pe.w("lookup_table")[0].any() and pe.compute_output_shape((None, 4, 6)) == (None, 4, 6)
    assert {k: pe.get_config()[k] for k in ("pos_embedding_trainable", "zero_pad", "scale")} == \
        dict(pos_embedding_trainable=True, zero_pad=True, scale=True)
    ln = LayerNormalization(device="cpu")
    ln.build((None, 4, 6))
    assert [(n.rsplit("/", 1)[1], tuple(t.shape)) for n, t in ln.named_weights()] == [("gamma", (6,)), ("beta", (6,))]
    assert {k: ln.get_config()[k] for k in ("axis", "eps", "center", "scale")} == dict(axis=-1, eps=1e-9, center=True, scale=True)
    assert float(ln.w("gamma").min()) == 1.0 and float(ln.w("beta").abs().max()) == 0.0


def test_reference_import_names():
    import deepctr
    import deepctr_amd.layers
    import deepctr_amd.models
    from deepctr.layers.normalization import LayerNormalization
    from deepctr.layers.sequence import PositionEncoding, Transformer
    from deepctr.models import BST
    from deepctr.models.sequence import BST as B3
    from deepctr.models.sequence.bst import BST as B2
    assert BST is deepctr_amd.models.BST is B2 is B3 is deepctr.models.BST
    assert Transformer is deepctr_amd.layers.Transformer and PositionEncoding is deepctr_amd.layers.PositionEncoding
    assert LayerNormalization is deepctr_amd.layers.LayerNormalization


def _args(**kw):
    from deepctr_amd import _C
    base = dict(batch=4, q_stride=5 * 8, q_row_stride=8, seq_len=5, dim=8, att_embedding_size=4, head_num=2, n_layers=1,
                use_positional_encoding=1, use_res=1, use_feed_forward=1, use_layer_norm=1, blinding=0, ln_eps=1e-9, out_stride=5 * 8,
                out_row_stride=8)
    base.update(kw)
    return _C.transformer.Args(**base)


def test_abi_argument_errors_without_a_gpu():
    from deepctr_amd import _C
    lib = _C.lib()
    assert lib.dctr_abi_version() == 13 == _C.ABI_VERSION
    f = lambda a: lib.dctr_transformer_fwd(ctypes.byref(a), None)   # noqa: E731
    r = lambda a: lib.dctr_transformer_route(ctypes.byref(a))       # noqa: E731
    assert lib.dctr_transformer_fwd(None, None) == -1 and lib.dctr_transformer_route(None) == -1
    assert f(_args()) == -1                                           # queries / layers / out missing
    assert b"transformer" in lib.dctr_last_error()
    for bad in (dict(seq_len=0), dict(dim=0), dict(head_num=0), dict(n_layers=0), dict(att_embedding_size=3), dict(head_num=3),
                dict(q_row_stride=7), dict(q_stride=39), dict(out=16, out_row_stride=7), dict(keys=16, k_stride=0, k_row_stride=0),
                dict(batch=-1)):
        assert f(_args(**bad)) == -2 and r(_args(**bad)) == -2, bad
    for bad in (dict(use_res=2), dict(blinding=-1), dict(output_type=3), dict(route=3), dict(query_lengths=16, query_mask=16),
                dict(key_lengths=16, key_mask=16)):
        assert f(_args(**bad)) == -4, bad
    # a null weight is reported before anything is launched
    ptrs = [16] * 9
    ptrs[6] = None                                                    # ln_beta with use_layer_norm
    arr = (ctypes.c_void_p * 9)(*ptrs)
    a = _args(queries=16, out=16, layers=ctypes.cast(arr, ctypes.c_void_p))
    assert f(a) == -1
    a.use_layer_norm = 0
    a.batch = 0
    assert f(a) == 0                                                  # complete arguments, empty batch: a no-op
    # the general route without its workspace
    big = _args(seq_len=200, dim=64, att_embedding_size=8, head_num=8, q_stride=200 * 64, q_row_stride=64, out_stride=200 * 64,
                out_row_stride=64, queries=16, out=16, layers=ctypes.cast((ctypes.c_void_p * 9)(*([16] * 9)), ctypes.c_void_p))
    assert r(big) == _C.transformer.ROUTE_GENERAL and f(big) == -1 and b"workspace" in lib.dctr_last_error()
    big.route = _C.transformer.ROUTE_FUSED
    assert r(big) == -5


def test_routes_and_workspace_sizes_without_a_gpu():
    from deepctr_amd import ops
    bst = dict(use_layer_norm=True, blinding=False)
    assert ops.transformer_route(50, 32, 8, 2, **bst) == "fused" and ops.transformer_workspace_bytes(4096, 50, 32, 8, 2, **bst) == 0
    assert ops.transformer_route(64, 64, 8, 1, **bst) == "fused"          # one sample alone within 160 KiB
    assert ops.transformer_route(1, 4, 2) == "fused"
    assert ops.transformer_route(200, 64, 8, 2, **bst) == "general"
    big = ops.transformer_workspace_bytes(3, 200, 64, 8, 2, **bst)
    assert big > 0 and big % 16 == 0 and big == ops.transformer_workspace_bytes(70000, 200, 64, 8, 2, **bst) and big <= 256 << 20
    assert ops.transformer_route(24, 16, 4, 2, route="general") == "general"
    assert ops.transformer_workspace_bytes(5, 24, 16, 4, 2, route="general") > 0
    # more than 16 layers with a pooled output: the activations between launches
    assert ops.transformer_workspace_bytes(10, 4, 4, 2, 17, output_type="mean") == 10 * 4 * 4 * 4
    assert ops.transformer_workspace_bytes(10, 4, 4, 2, 17, output_type=None) == 0
    with pytest.raises(ValueError, match="att_embedding_size \\* head_num"):
        ops.transformer_route(5, 12, 8)


def test_float32_restatement_against_float64_on_the_op_sweep():
    """The float32 NumPy restatement of the block, in the reference's operation order, against the float64 oracle on the GPU op
    sweep's own inputs, as a fraction of that sweep's bar (|err| <= 1e-4 |ref| + 2e-6 max|ref of the sample|): the figures
    DESIGN.md §4.16 quotes beside the kernel's.  Printed per case as BST's flags | the worst variant; the bar must be reachable in
    float32 at all, so every ratio is below 1."""
    from tests import test_gpu_bst as G
    for T, E, H, L, B in G.SWEEP:
        rng = np.random.RandomState(T * 1000 + E * 10 + L)
        ws = G.make_weights(rng, T, E, L)
        mask = RB.sequence_mask(G.draw_lengths(rng, B, T), T)
        x = rng.standard_normal((B, T, E + 3)).astype(np.float32)[:, :, :E]
        ratios = []
        for flags, ot in G.sweep_variants():
            ref = G.oracle(x, x, ws, H, mask, mask, flags, ot)
            got = G.oracle(x, x, ws, H, mask, mask, flags, ot, dtype=np.float32)
            ratios.append(G.within_bar(got.reshape(B, -1), ref.reshape(B, -1)))
        print("T %d E %d H %d L %d: float32 NumPy / bar %.3f | %.3f" % (T, E, H, L, ratios[0], max(ratios)))
        assert max(ratios) < 1.0


def test_cost_model():
    """The arithmetic the kernel's header and DESIGN.md §4.16 quote (T 50, E 32): 6 T E^2 + 4 T^2 E + 16 T E^2 per sample and layer."""
    from deepctr_amd.ops import transformer_flops
    assert transformer_flops(50, 32) == 307200 + 320000 + 819200 == 1446400
    assert transformer_flops(50, 32, 2) == 2 * 1446400
    assert transformer_flops(50, 32, 1, use_feed_forward=False) == 627200


def test_args_mirror_has_the_layout_the_c_compiler_gives_the_header(tmp_path):
    import os
    import shutil
    import subprocess
    from deepctr_amd import _C
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    cls = _C.transformer.Args
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dctr.h"', "int main(void) {",
             '    printf("sizeof %zu\\n", sizeof(dctr_transformer_args_t));',
             '    printf("ptrs %d\\n", DCTR_TRANSFORMER_LAYER_PTRS);', '    printf("abi %d\\n", DCTR_ABI_VERSION);']
    for fname, _ in cls._fields_:
        lines.append('    printf("%s %%zu\\n", offsetof(dctr_transformer_args_t, %s));' % (fname, fname))
    lines += ["    return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    for line in filter(None, out):
        field, val = line.split()
        if field == "ptrs":
            want = _C.transformer.LAYER_PTRS
        elif field == "abi":
            want = 13
        else:
            want = ctypes.sizeof(cls) if field == "sizeof" else getattr(cls, field).offset
        assert int(val) == want, "%s: C says %s, ctypes %d" % (field, val, want)
