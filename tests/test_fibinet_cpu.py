"""CPU: FiBiNET / SENETLayer / BilinearInteraction — the NumPy oracle (tests/ref_fibinet.py) against the reference's own outputs
(tests/golden/model_fibinet_*.npz, senet_bilinear_layer.npz; scripts/make_golden_fibinet.py), the torch restatement the training path
uses (training.model_logits) against the oracle, the API contract, and the C ABI's argument checks (no launch)."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from tests import ref_fibinet as RF
from tests.spec import columns_from_spec
from tests.test_autoint_cpu import att_rows
from tests.util import assert_close, golden_meta, load_golden, sigmoid_inv

FIBINET_FIXTURES = ["model_fibinet_interaction", "model_fibinet_all", "model_fibinet_each", "model_fibinet_hash", "model_fibinet_nodnn",
                    "model_fibinet_r1", "model_fibinet_rbig", "model_fibinet_regression", "model_fibinet_fixed"]
SENET_TAGS = ["s", "s_c", "s_r1", "s_big"]
BILINEAR_TAGS = ["b_all", "b_each", "b_int", "b_two", "b_wide"]


def build_fibinet(meta, device):
    from deepctr_amd.models import FiBiNET
    return FiBiNET(columns_from_spec(meta["linear"]), columns_from_spec(meta["dnn"]), device=device, **meta["kwargs"])


def _has_hash(meta):
    return any(d.get("use_hash") or d.get("sparsefeat", {}).get("use_hash") for d in meta["dnn"] + meta["linear"])


@pytest.mark.parametrize("name", FIBINET_FIXTURES)
def test_oracle_matches_reference_code(name):
    g = load_golden(name)
    y, ref = RF.run_fixture(g), g["y"]
    assert y.shape == ref.shape
    assert_close(y, ref, rtol=1e-4, atol=1e-6, what=name + " prob")
    if golden_meta(g)["kwargs"].get("task") != "regression":
        ok = (ref > 1e-6) & (ref < 1 - 1e-6)
        if ok.any():
            assert_close(sigmoid_inv(y[ok]), sigmoid_inv(ref[ok]), rtol=1e-4, atol=2e-5, what=name + " logit")
    y64 = RF.run_fixture(g, np.float64)
    assert_close(y64, ref, rtol=1e-4, atol=1e-6, what=name + " float64 prob")


def test_fixed_fixture_is_unsaturated():
    ref = load_golden("model_fibinet_fixed")["y"]
    assert ((ref > 1e-3) & (ref < 1 - 1e-3)).all()


@pytest.mark.parametrize("tag", SENET_TAGS)
def test_senet_oracle_matches_reference_code(tag):
    g = load_golden("senet_bilinear_layer")
    for dt in (np.float32, np.float64):
        y = RF.senet(g[tag + "_x"], g[tag + "_W_1"], g[tag + "_W_2"], dtype=dt)
        assert_close(y, g[tag + "_y"], rtol=1e-4, atol=1e-6, what="senet " + tag)
    F, ratio = g[tag + "_x"].shape[1], int(g[tag + "_cfg"][0])
    assert g[tag + "_W_1"].shape == (F, max(1, F // ratio))


@pytest.mark.parametrize("tag", BILINEAR_TAGS)
def test_bilinear_oracle_matches_reference_code(tag):
    g = load_golden("senet_bilinear_layer")
    btype = bytes(g[tag + "_type"]).decode()
    for dt in (np.float32, np.float64):
        y = RF.bilinear(g[tag + "_x"], list(g[tag + "_w"]), btype, dtype=dt)
        assert y.shape == g[tag + "_y"].shape
        assert_close(y, g[tag + "_y"], rtol=1e-4, atol=1e-6, what="bilinear " + tag)


@pytest.mark.parametrize("name", FIBINET_FIXTURES)
def test_torch_restatement_matches_oracle(name):
    from deepctr_amd import engine, training
    g = load_golden(name)
    meta = golden_meta(g)
    if _has_hash(meta):
        pytest.skip("integer Hash runs inside the HIP gather kernel; the GPU suite covers this fixture")
    model = build_fibinet(meta, torch.device("cpu"))
    model.set_weights_by_name({k[2:]: v for k, v in g.items() if k.startswith("w/")})
    feed = {k[5:]: v for k, v in g.items() if k.startswith("feed/")}
    n = g["y"].shape[0]
    staged = engine.Staged(n)
    model._stage_inputs(feed, staged)
    model._begin()
    with torch.no_grad():
        logit = training.model_logits(model, staged, 0, n).numpy().astype(np.float64).reshape(-1)
    ref = RF.run_fixture(g, np.float64, task="regression").reshape(-1)
    rows = att_rows(meta, feed, n)
    assert rows.sum() >= n // 2
    assert_close(logit[rows], ref[rows], rtol=1e-4, atol=2e-5, what=name + " model_logits")


def test_signature_defaults_match_the_reference():
    from deepctr_amd.models import FiBiNET
    params = inspect.signature(FiBiNET).parameters
    want = dict(bilinear_type='interaction', reduction_ratio=3, dnn_hidden_units=(256, 128, 64), l2_reg_linear=1e-5,
                l2_reg_embedding=1e-5, l2_reg_dnn=0, seed=1024, dnn_dropout=0, dnn_activation='relu', task='binary', device=None)
    names = list(params)
    assert names == ["linear_feature_columns", "dnn_feature_columns"] + list(want)
    for k, v in want.items():
        assert params[k].default == v, k
    from deepctr_amd.layers import BilinearInteraction, SENETLayer
    sp = inspect.signature(SENETLayer.__init__).parameters
    assert [(k, sp[k].default) for k in ("reduction_ratio", "seed")] == [("reduction_ratio", 3), ("seed", 1024)]
    bp = inspect.signature(BilinearInteraction.__init__).parameters
    assert [(k, bp[k].default) for k in ("bilinear_type", "seed")] == [("bilinear_type", "interaction"), ("seed", 1024)]


def test_construction_errors_match_the_reference():
    from deepctr_amd.feature_column import DenseFeat, SparseFeat, VarLenSparseFeat
    from deepctr_amd.layers import BilinearInteraction, SENETLayer
    from deepctr_amd.models import FiBiNET
    one = [SparseFeat("a", 5, 4), DenseFeat("c", 1)]
    with pytest.raises(ValueError, match="at least 2"):
        FiBiNET(one, one, device="cpu")
    mixed = [SparseFeat("a", 5, 4), VarLenSparseFeat(SparseFeat("s", 6, 8), maxlen=3)]
    with pytest.raises(ValueError, match="embedding_dim"):
        FiBiNET(mixed, mixed, device="cpu")
    cols = [SparseFeat("a", 5, 4), SparseFeat("b", 6, 4)]
    with pytest.raises(NotImplementedError):
        FiBiNET(cols, cols, bilinear_type="outer", device="cpu")
    for layer in (SENETLayer(device="cpu"), BilinearInteraction(device="cpu")):
        with pytest.raises(ValueError, match="at least 2 inputs"):
            layer.build([(None, 1, 4)])
    with pytest.raises(NotImplementedError):
        BilinearInteraction("outer", device="cpu").build([(None, 1, 4)] * 3)


def test_layer_contract():
    from deepctr_amd.layers import BilinearInteraction, SENETLayer, custom_objects
    assert custom_objects["SENETLayer"] is SENETLayer and custom_objects["BilinearInteraction"] is BilinearInteraction
    s = SENETLayer(2, device="cpu")
    s.build([(None, 1, 6)] * 5)
    # (the layer name counts the layers built before in the process: senet_layer, senet_layer_1, ...)
    assert s.name.startswith("senet_layer")
    assert [(n.rsplit("/", 1)[1], tuple(t.shape)) for n, t in s.named_weights()] == [("W_1", (5, 2)), ("W_2", (2, 5))]
    assert s.compute_output_shape([(None, 1, 6)] * 5) == [(None, 1, 6)] * 5
    assert s.compute_mask(None) == [None] * 5
    assert {k: s.get_config()[k] for k in ("reduction_ratio", "seed")} == dict(reduction_ratio=2, seed=1024)
    for btype, names in [("all", ["bilinear_weight"]), ("each", ["bilinear_weight%d" % i for i in range(3)]),
                         ("interaction", ["bilinear_weight%d_%d" % p for p in [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]])]:
        b = BilinearInteraction(btype, device="cpu")
        b.build([(None, 1, 7)] * 4)
        assert b.name.startswith("bilinear_interaction")
        assert [(n.rsplit("/", 1)[1], tuple(t.shape)) for n, t in b.named_weights()] == [(n, (7, 7)) for n in names]
        assert b.compute_output_shape([(None, 1, 7)] * 4) == (None, 6, 7)
        assert b.get_config()["bilinear_type"] == btype


@pytest.mark.parametrize("name", FIBINET_FIXTURES)
def test_weight_names_and_shapes_match_the_fixture(name):
    g = load_golden(name)
    model = build_fibinet(golden_meta(g), torch.device("cpu"))
    mine = {k: tuple(v.shape) for k, v in model.get_weights_by_name().items()}
    ref = {k[2:]: tuple(v.shape) for k, v in g.items() if k.startswith("w/") and not k.startswith("w/linearsparse_")}
    assert mine == ref


def test_fit_loss_carries_the_three_l2_penalties():
    """fit()'s reported loss adds l2 * sum(w^2) over the embeddings, the linear part and the DNN kernels, not over the SENET or
    bilinear weights (reference fibinet.py: the layers take no regulariser)."""
    from deepctr_amd import training
    g = load_golden("model_fibinet_fixed")
    meta = golden_meta(g)
    from deepctr_amd.models import FiBiNET
    model = FiBiNET(columns_from_spec(meta["linear"]), columns_from_spec(meta["dnn"]), l2_reg_linear=0.1, l2_reg_embedding=0.2,
                    l2_reg_dnn=0.3, device="cpu", **meta["kwargs"])
    regs = training.regularized_weights(model)
    names = {t.data_ptr(): n for n, t in model.named_weights()}
    got = sorted((names[t.data_ptr()], l2) for t, l2 in regs)
    want = sorted([(n, 0.2) for n, _ in model.named_weights() if n.startswith("sparse_emb_")] +
                  [(n, 0.1) for n, _ in model.named_weights() if n.startswith("linear")] +
                  [(n, 0.3) for n, _ in model.named_weights() if n.startswith("dnn/kernel")])
    assert got == want
    assert not any(n.startswith(("senet_layer", "bilinear_interaction")) for n, _ in got)


def test_reference_import_names():
    import deepctr
    import deepctr_amd.models
    from deepctr.layers import BilinearInteraction, SENETLayer
    from deepctr.layers.interaction import BilinearInteraction as B2, SENETLayer as S2
    from deepctr.models import FiBiNET
    from deepctr.models.fibinet import FiBiNET as F2
    assert FiBiNET is deepctr_amd.models.FiBiNET is F2 is deepctr.models.FiBiNET
    assert SENETLayer is S2 is deepctr_amd.layers.SENETLayer
    assert BilinearInteraction is B2 is deepctr_amd.layers.BilinearInteraction


def test_cost_model():
    """The arithmetic DESIGN.md §4.9 quotes (defaults on Criteo-shaped input: F 26, E 16, 13 dense)."""
    from deepctr_amd.models.fibinet import bilinear_flops
    assert bilinear_flops(26, 16, "interaction") == 332800
    assert bilinear_flops(26, 16, "all") == bilinear_flops(26, 16, "each") == 25600
    assert 2 * 325 * 16 + 13 == 10413


def _args(**kw):
    from deepctr_amd import _C
    base = dict(batch=4, x_stride=12, fields=4, dim=3, bilinear_type=2, mode=0, reduction_size=1, dense_cols=0, out_stride=36)
    base.update(kw)
    return _C.bilinear.Args(**base)


def test_abi_argument_errors_without_a_gpu():
    from deepctr_amd import _C
    lib = _C.lib()
    f = lambda a: lib.dctr_bilinear_fwd(ctypes.byref(a), None)   # noqa: E731
    full = dict(x=16, out=16, senet_w1=16, senet_w2=16, senet_bilinear_w=16, bilinear_w=16)
    assert lib.dctr_bilinear_fwd(None, None) == -1
    assert f(_args()) == -1                                          # x / out / weights missing
    assert f(_args(fields=1, x_stride=3, **full)) == -2              # F < 2
    assert f(_args(fields=0, **full)) == -2
    assert f(_args(bilinear_type=3, **full)) == -4                   # unknown type
    assert f(_args(bilinear_type=-1, **full)) == -4
    assert f(_args(mode=3, **full)) == -4
    assert f(_args(dim=0, **full)) == -2                             # E < 1
    assert f(_args(reduction_size=0, **full)) == -2
    assert f(_args(x_stride=11, **full)) == -2
    assert f(_args(out_stride=35, **full)) == -2                     # 2 * 6 pairs * 3
    assert f(_args(dense_cols=2, x_stride=13, out_stride=40, **full)) == -2
    assert f(_args(dense_cols=1, mode=2, out_stride=18, **full)) == -2   # dense columns: the model mode only
    assert b"bilinear" in lib.dctr_last_error()
    for k in full:                                                   # every pointer the model mode reads is checked
        a = dict(full)
        del a[k]
        assert f(_args(**a)) == -1, k
    assert f(_args(mode=1, out_stride=12, x=16, out=16, senet_w1=16)) == -1         # SENET only: W_2 missing
    assert f(_args(mode=2, out_stride=18, x=16, out=16, senet_bilinear_w=16)) == -1  # one layer: its table missing
    assert f(_args(batch=0, **full)) == 0                            # empty batch: a no-op


def test_workspace_sizes_without_a_gpu():
    from deepctr_amd import ops
    # the LDS route needs none: Criteo defaults (three types), the layer tests' shapes, F = 2
    for btype in ("interaction", "all", "each"):
        assert ops.senet_bilinear_workspace_bytes(65536, 26, 16, btype, 0, 8) == 0
    assert ops.senet_bilinear_workspace_bytes(5, 4, 3, "interaction", 2) == 0
    assert ops.senet_bilinear_workspace_bytes(5, 2, 1, "all", 1, 1) == 0
    # a tile too large for the LDS: the general route's slices, independent of the batch
    big = ops.senet_bilinear_workspace_bytes(3, 200, 256, "all", 0, 66)
    assert big > 0 and big % 16 == 0 and big == ops.senet_bilinear_workspace_bytes(70000, 200, 256, "all", 0, 66)
    assert big <= 256 << 20
    from deepctr_amd import _C
    a = _args(fields=1)
    assert _C.lib().dctr_bilinear_workspace_bytes(ctypes.byref(a)) == 0


def test_args_mirror_has_the_layout_the_c_compiler_gives_the_header(tmp_path):
    import os
    import shutil
    import subprocess
    from deepctr_amd import _C
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    cls = _C.bilinear.Args
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dctr.h"', "int main(void) {",
             '    printf("sizeof %zu\\n", sizeof(dctr_bilinear_args_t));',
             '    printf("enums %d %d %d %d %d %d\\n", DCTR_BILINEAR_ALL, DCTR_BILINEAR_EACH, DCTR_BILINEAR_INTERACTION,'
             ' DCTR_BILINEAR_MODE_MODEL, DCTR_BILINEAR_MODE_SENET, DCTR_BILINEAR_MODE_LAYER);']
    for fname, _ in cls._fields_:
        lines.append('    printf("%s %%zu\\n", offsetof(dctr_bilinear_args_t, %s));' % (fname, fname))
    lines += ["    return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    for line in filter(None, out):
        field, *vals = line.split()
        if field == "enums":
            B = _C.bilinear
            assert [int(v) for v in vals] == [B.ALL, B.EACH, B.INTERACTION, B.MODE_MODEL, B.MODE_SENET, B.MODE_LAYER]
            continue
        want = ctypes.sizeof(cls) if field == "sizeof" else getattr(cls, field).offset
        assert int(vals[0]) == want, "%s: C says %s, ctypes %d" % (field, vals[0], want)
