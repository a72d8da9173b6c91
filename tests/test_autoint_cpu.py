"""CPU: AutoInt / InteractingLayer — the NumPy oracle (tests/ref_autoint.py) against the reference's own outputs
(tests/golden/model_autoint_*.npz, interacting_layer.npz; scripts/make_golden_autoint.py), the torch restatement the training path
uses (training.model_logits) against the oracle, the API contract, and the C ABI's argument checks (no launch)."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from tests import ref_autoint as RA
from tests.spec import columns_from_spec
from tests.util import assert_close, golden_meta, load_golden, sigmoid_inv

AUTOINT_FIXTURES = ["model_autoint_mixed", "model_autoint_hash", "model_autoint_attonly", "model_autoint_deeponly",
                    "model_autoint_nores", "model_autoint_h3", "model_autoint_fixed"]
LAYER_TAGS = ["t", "t_scale", "t_nores", "t_both", "c", "one", "wide"]


def att_rows(meta, feed, n):
    """Rows whose max-pooled sequences are not all padding: the reference's -1e9 (layers/sequence.py:96-98) enters Q K^T at 1e18,
    and the attention of such a row is rounding noise in any fp32 implementation."""
    ok = np.ones(n, dtype=bool)
    for d in meta["dnn"]:
        if d["type"] == "varlen" and d.get("combiner") == "max":
            if d.get("length_name"):
                ok &= np.asarray(feed[d["length_name"]]).reshape(-1) > 0
            else:
                ok &= (np.asarray(feed[d["sparsefeat"]["name"]]).reshape(n, -1) != 0).any(axis=1)
    return ok


def build_autoint(meta, device):
    from deepctr_amd.models import AutoInt
    return AutoInt(columns_from_spec(meta["linear"]), columns_from_spec(meta["dnn"]), device=device, **meta["kwargs"])


@pytest.mark.parametrize("name", AUTOINT_FIXTURES)
def test_oracle_matches_reference_code(name):
    g = load_golden(name)
    y, ref = RA.run_fixture(g), g["y"]
    assert y.shape == ref.shape
    assert_close(y, ref, rtol=1e-4, atol=1e-6, what=name + " prob")
    ok = (ref > 1e-6) & (ref < 1 - 1e-6)
    if ok.any():
        assert_close(sigmoid_inv(y[ok]), sigmoid_inv(ref[ok]), rtol=1e-4, atol=2e-5, what=name + " logit")
    y64 = RA.run_fixture(g, np.float64)
    assert_close(y64, ref, rtol=1e-4, atol=1e-6, what=name + " float64 prob")


@pytest.mark.parametrize("tag", LAYER_TAGS)
def test_layer_oracle_matches_reference_code(tag):
    g = load_golden("interacting_layer")
    d, H, res, scaling = (int(v) for v in g[tag + "_cfg"])
    for dt in (np.float32, np.float64):
        y = RA.interacting_layer(g[tag + "_x"], g[tag + "_query"], g[tag + "_key"], g[tag + "_value"], g.get(tag + "_res"), d, H,
                                 bool(res), bool(scaling), dtype=dt)
        assert y.shape == g[tag + "_y"].shape
        assert_close(y, g[tag + "_y"], rtol=1e-4, atol=1e-6, what="interacting_layer " + tag)


@pytest.mark.parametrize("name", AUTOINT_FIXTURES)
def test_torch_restatement_matches_oracle(name):
    from deepctr_amd import engine, training
    g = load_golden(name)
    meta = golden_meta(g)
    if any(d.get("use_hash") or d.get("sparsefeat", {}).get("use_hash") for d in meta["dnn"] + meta["linear"]):
        pytest.skip("integer Hash runs inside the HIP gather kernel; the GPU suite covers this fixture")
    model = build_autoint(meta, torch.device("cpu"))
    model.set_weights_by_name({k[2:]: v for k, v in g.items() if k.startswith("w/")})
    feed = {k[5:]: v for k, v in g.items() if k.startswith("feed/")}
    n = g["y"].shape[0]
    staged = engine.Staged(n)
    model._stage_inputs(feed, staged)
    model._begin()
    with torch.no_grad():
        logit = training.model_logits(model, staged, 0, n).numpy().astype(np.float64).reshape(-1)
    ref = RA.run_fixture(g, np.float64, task="regression").reshape(-1)
    rows = att_rows(meta, feed, n)
    assert rows.sum() >= n // 2
    assert_close(logit[rows], ref[rows], rtol=1e-4, atol=2e-5, what=name + " model_logits")


def test_signature_defaults_match_the_reference():
    from deepctr_amd.models import AutoInt
    params = inspect.signature(AutoInt).parameters
    want = dict(att_layer_num=3, att_embedding_size=8, att_head_num=2, att_res=True, dnn_hidden_units=(256, 128, 64),
                dnn_activation='relu', l2_reg_linear=1e-5, l2_reg_embedding=1e-5, l2_reg_dnn=0, dnn_use_bn=False, dnn_dropout=0,
                seed=1024, task='binary')
    names = list(params)
    assert names[:2] == ["linear_feature_columns", "dnn_feature_columns"]
    assert names[2:2 + len(want)] == list(want)
    for k, v in want.items():
        assert params[k].default == v, k
    from deepctr_amd.layers import InteractingLayer
    lp = inspect.signature(InteractingLayer.__init__).parameters
    assert [(k, lp[k].default) for k in ("att_embedding_size", "head_num", "use_res", "scaling", "seed")] == \
        [("att_embedding_size", 8), ("head_num", 2), ("use_res", True), ("scaling", False), ("seed", 1024)]


def test_construction_errors_match_the_reference():
    from deepctr_amd.feature_column import DenseFeat, SparseFeat, VarLenSparseFeat
    from deepctr_amd.layers import InteractingLayer
    from deepctr_amd.models import AutoInt
    cols = [SparseFeat("a", 5, 4), SparseFeat("b", 6, 4), DenseFeat("c", 1)]
    with pytest.raises(ValueError, match="Either hidden_layer or att_layer_num must > 0"):
        AutoInt(cols, cols, att_layer_num=0, dnn_hidden_units=(), device="cpu")
    mixed = [SparseFeat("a", 5, 4), VarLenSparseFeat(SparseFeat("s", 6, 8), maxlen=3)]
    for kw in (dict(), dict(att_layer_num=0)):          # concat_func(axis=1) runs whatever the branches
        with pytest.raises(ValueError):
            AutoInt(mixed, mixed, device="cpu", **kw)
    with pytest.raises(ValueError, match="head_num must be a int > 0"):
        InteractingLayer(head_num=0)


def test_layer_contract():
    from deepctr_amd.layers import InteractingLayer, custom_objects
    assert custom_objects["InteractingLayer"] is InteractingLayer
    layer = InteractingLayer(6, 3, use_res=True, scaling=True, device="cpu")
    layer.build((None, 5, 7))
    # (the layer name counts the layers built before in the process: interacting_layer, interacting_layer_1, ...)
    assert layer.name.startswith("interacting_layer")
    assert [(n.rsplit("/", 1)[1], tuple(t.shape)) for n, t in layer.named_weights()] == \
        [(w, (7, 18)) for w in ("query", "key", "value", "res")]
    assert layer.compute_output_shape((None, 5, 7)) == (None, 5, 18)
    cfg = layer.get_config()
    assert {k: cfg[k] for k in ("att_embedding_size", "head_num", "use_res", "seed")} == \
        dict(att_embedding_size=6, head_num=3, use_res=True, seed=1024)
    assert "scaling" not in cfg                         # the reference's get_config omits it
    nores = InteractingLayer(4, 2, use_res=False, device="cpu")
    nores.build((None, 3, 5))
    assert [n.rsplit("/", 1)[1] for n, _ in nores.named_weights()] == ["query", "key", "value"]
    w = layer.w("query")
    assert float(w.abs().max()) <= 2 * 0.05 + 1e-7 and 0.02 < float(w.std()) < 0.06      # TruncatedNormal(0, 0.05)


@pytest.mark.parametrize("name", AUTOINT_FIXTURES)
def test_weight_names_and_shapes_match_the_fixture(name):
    g = load_golden(name)
    model = build_autoint(golden_meta(g), torch.device("cpu"))
    mine = {k: tuple(v.shape) for k, v in model.get_weights_by_name().items()}
    ref = {k[2:]: tuple(v.shape) for k, v in g.items() if k.startswith("w/") and not k.startswith("w/linearsparse_")}
    assert mine == ref


def test_reference_import_names():
    import deepctr
    import deepctr_amd.models
    from deepctr.layers import InteractingLayer
    from deepctr.models import AutoInt
    from deepctr.models.autoint import AutoInt as A2
    assert AutoInt is deepctr_amd.models.AutoInt is A2
    assert InteractingLayer is deepctr_amd.layers.InteractingLayer
    assert deepctr.models.AutoInt is AutoInt


def _args(**kw):
    from deepctr_amd import _C
    base = dict(batch=4, x_stride=12, fields=4, dim=3, n_layers=1, att_embedding_size=8, head_num=2, use_res=1, scaling=0)
    base.update(kw)
    return _C.interacting.Args(**base)


def test_abi_argument_errors_without_a_gpu():
    from deepctr_amd import _C
    lib = _C.lib()
    f = lambda a: lib.dctr_interacting_fwd(ctypes.byref(a), None)   # noqa: E731
    assert lib.dctr_interacting_fwd(None, None) == -1
    assert f(_args()) == -1                                           # x / layers / out missing
    assert f(_args(fields=0)) == -2
    assert f(_args(head_num=0)) == -2
    assert f(_args(att_embedding_size=0)) == -2
    assert f(_args(n_layers=0)) == -2
    assert f(_args(x_stride=11)) == -2
    assert f(_args(out=16, out_stride=63)) == -2
    assert f(_args(use_res=2)) == -4
    assert f(_args(scaling=-1)) == -4
    assert f(_args(head_w=16)) == -1                                  # head_w without logit
    assert f(_args(batch=0)) == 0                                     # empty batch: a no-op
    assert b"interacting" in lib.dctr_last_error()
    # a null weight is reported before anything is launched
    arr = (ctypes.c_void_p * 4)(16, 16, None, 16)
    a = _args(x=16, out=16, out_stride=64, layers=ctypes.cast(arr, ctypes.c_void_p))
    assert f(a) == -1


def test_workspace_sizes_without_a_gpu():
    from deepctr_amd import ops
    # the LDS route needs none: Criteo defaults, the reference test's shape, F = 128 at d*H = 16
    assert ops.interacting_workspace_bytes(65536, 26, 16, 3, 8, 2) == 0
    assert ops.interacting_workspace_bytes(5, 4, 3, 1, 8, 2) == 0
    assert ops.interacting_workspace_bytes(5, 128, 16, 2, 8, 2) == 0
    # a sample too large for the LDS: the general route's slices, independent of the batch
    big = ops.interacting_workspace_bytes(7, 200, 32, 2, 16, 4)
    assert big > 0 and big % 16 == 0 and big == ops.interacting_workspace_bytes(70000, 200, 32, 2, 16, 4)
    assert big <= 256 << 20
    # more than 32 layers with the head only: the activations between launches
    assert ops.interacting_workspace_bytes(10, 4, 3, 33, 2, 2, with_out=False) == 10 * 4 * 4 * 4
    assert ops.interacting_workspace_bytes(10, 4, 3, 33, 2, 2, with_out=True) == 0
    from deepctr_amd import _C
    a = _args(fields=0)
    assert _C.lib().dctr_interacting_workspace_bytes(ctypes.byref(a)) == 0


def test_cost_model():
    """The arithmetic DESIGN.md quotes (defaults on Criteo-shaped input: F 26, E 16, d 8, H 2, 3 layers)."""
    from deepctr_amd.models.autoint import interacting_flops
    assert interacting_flops(26, 16, 8, 2, 3, True) == 3 * (53248 + 2 * 21632)


def test_args_mirror_has_the_layout_the_c_compiler_gives_the_header(tmp_path):
    import os
    import shutil
    import subprocess
    from deepctr_amd import _C
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    cls = _C.interacting.Args
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dctr.h"', "int main(void) {",
             '    printf("sizeof %zu\\n", sizeof(dctr_interacting_args_t));']
    for fname, _ in cls._fields_:
        lines.append('    printf("%s %%zu\\n", offsetof(dctr_interacting_args_t, %s));' % (fname, fname))
    lines += ["    return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    for line in filter(None, out):
        field, val = line.split()
        want = ctypes.sizeof(cls) if field == "sizeof" else getattr(cls, field).offset
        assert int(val) == want, "%s: C says %s, ctypes %d" % (field, val, want)
