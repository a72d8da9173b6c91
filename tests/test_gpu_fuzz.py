"""GPU parity, randomised: seeded random model configurations (feature-column mixes the fixtures do not enumerate — many fields,
embedding widths that are not a multiple of 4, hashed / shared / grouped / weighted-sequence features, DNN shapes outside the
instantiated widths, every launch-size regime of dctr_embed_mlp_fwd) scored by ``predict`` and compared with the float64 NumPy
oracle (oracle/ref_models.py, pinned to the reference's own output by tests/test_oracle_golden.py).  The reference builds these
through deepctr/feature_column.py:15-122 + inputs.py:44-181 and the model constructors under deepctr/models/.

Bar: north_star's 1e-4 relative on probabilities (check_probs of tests/test_gpu_models.py)."""
import json
import os

import numpy as np
import pytest

from tests.test_gpu_models import _randomise, build_model, check_probs
from tests.test_oracle_golden import run_oracle_model
from tests.util import assert_close

FM_MODELS = ("DeepFM", "NFM", "AFM", "PNN", "xDeepFM")          # one embedding width for every field (the reference concatenates them)
ALL_MODELS = ("DeepFM", "WDL", "FNN", "DCN", "DCNM", "DCNMix") + FM_MODELS[1:]
DNN_SHAPES = [(8,), (32, 16), (256, 128, 64), (200, 80), (128, 128), (64,), (400, 400), (17, 9, 5), (256, 256, 256, 128)]
# hidden_units with a layer wider than any LDS tile holds (> 1,216 units: the layer-by-layer route of dctr_mlp_fwd; reference
# layers/core.py:160-175 takes any width).  Chosen by the seed alone — no generator draw — so every other configuration stays what it was
WIDE_DNN_SHAPES = [(1024, 512, 256), (2048,), (1300, 40), (2048, 1024)]
ROW_COUNTS = [1, 7, 300, 1000, 4099, 20011, 70001, 2, 65, 16384, 16383, 8192]


def random_config(seed, rows=None, dims4=False):
    """-> (meta dict in the golden fixtures' format, feed, n rows).  dims4: embedding widths that are multiples of 4 only (the HIP
    training step's family; the others train on the autograd step)."""
    rng = np.random.RandomState(1000 + seed)
    model = ALL_MODELS[seed % len(ALL_MODELS)]
    fm = model in FM_MODELS
    n = int(ROW_COUNTS[(seed // len(ALL_MODELS) + seed) % len(ROW_COUNTS)]) if rows is None else int(rows)
    if model in ("xDeepFM", "AFM", "PNN") and n > 20011:
        n = 20011
    exotic = seed >= 240                  # the second family: widths past 64 / "auto", up to 60 fields, FM groups, linear-only features
    uniform = int(rng.choice([4, 8, 16, 32, 12, 6] if fm else [4, 8, 16, 5, 10, 3, 64]))
    if exotic:
        uniform = int(rng.choice([20, 24, 48, 2, 1, 28, 80] if fm else [20, 48, 102, 1, 2, 80]))
    n_sparse = int(rng.randint(1, 31 if not fm else 27))
    if exotic and not fm and rng.rand() < 0.4:
        n_sparse = int(rng.randint(31, 61))
    if dims4:
        uniform = int(rng.choice([4, 8, 16, 32, 12, 20] if fm else [4, 8, 16, 64, 24]))
    if model in ("AFM", "PNN", "xDeepFM"):
        n_sparse = max(2, min(n_sparse, 12))
    mixed_dims = (not fm) and rng.rand() < 0.5
    dnn, feed = [], {}

    def dim():
        if mixed_dims:
            return int(rng.choice([4, 8, 16, 32, 12] if dims4 else [4, 8, 16, 5, 10, 3, 32] + ([102, 20, 1, 72] if exotic else [])))
        return uniform

    shared = None
    for i in range(n_sparse):
        v = int(rng.choice([3, 17, 100, 1000, 5003]))
        d = {"type": "sparse", "name": "s%d" % i, "vocabulary_size": v, "embedding_dim": dim()}
        if rng.rand() < 0.2:
            d["use_hash"] = True
            d["dtype"] = "int64" if rng.rand() < 0.5 else "int32"
            feed[d["name"]] = rng.randint(0, 10 ** 6, n).astype(d["dtype"])
        else:
            feed[d["name"]] = rng.randint(0, v, n).astype(np.int64 if rng.rand() < 0.3 else np.int32)
        if rng.rand() < 0.15 and (not fm or (exotic and model == "DeepFM")):
            d["group_name"] = "g%d" % rng.randint(2)
        if shared is not None and rng.rand() < 0.15 and not d.get("use_hash"):
            d["embedding_name"] = shared["name"]
            d["vocabulary_size"] = shared["vocabulary_size"]
            d["embedding_dim"] = shared["embedding_dim"]
            feed[d["name"]] = rng.randint(0, shared["vocabulary_size"], n).astype(np.int32)
        elif shared is None and not d.get("use_hash"):
            shared = d
        dnn.append(d)
    for i in range(int(rng.choice([0, 0, 1, 2, 3]))):
        T = int(rng.choice([1, 3, 8, 20]))
        v = int(rng.choice([6, 50, 700]))
        sf = {"type": "sparse", "name": "q%d" % i, "vocabulary_size": v, "embedding_dim": dim()}
        d = {"type": "varlen", "sparsefeat": sf, "maxlen": T, "combiner": str(rng.choice(["mean", "sum", "max"]))}
        lens = rng.randint(0 if d["combiner"] != "max" or not fm else 1, T + 1, n)
        ids = rng.randint(1, v, (n, T)).astype(np.int32)
        ids[np.arange(T)[None, :] >= lens[:, None]] = 0
        feed[sf["name"]] = ids
        if rng.rand() < 0.5:
            d["length_name"] = sf["name"] + "_len"
            feed[d["length_name"]] = lens.astype(np.int32).reshape(n, 1)
        if rng.rand() < 0.3:
            d["weight_name"] = sf["name"] + "_w"
            d["weight_norm"] = bool(rng.rand() < 0.5)
            feed[d["weight_name"]] = rng.rand(n, T, 1).astype(np.float32)
        dnn.append(d)
    dense = []
    for i in range(int(rng.choice([0, 1, 2, 13]))):
        k = int(rng.choice([1, 1, 1, 3]))
        dense.append({"type": "dense", "name": "d%d" % i, "dimension": k})
        feed["d%d" % i] = rng.rand(n, k).astype(np.float32)
    if model != "AFM":                  # AFM: DenseFeat only among the linear columns (inputs.py:201-202, support_dense=False)
        dnn += dense
    order = rng.permutation(len(dnn)) if rng.rand() < 0.5 else np.arange(len(dnn))
    dnn = [dnn[j] for j in order]
    r = rng.rand()
    linear = list(dnn) if r < 0.6 else ([d for d in dnn if rng.rand() < 0.5] if r < 0.85 else [])
    if model == "AFM":
        linear = linear + dense
    if exotic and rng.rand() < 0.4:       # features only the linear part sees (linear_feature_columns is its own list in every constructor)
        for i in range(int(rng.randint(1, 4))):
            v = int(rng.choice([5, 300]))
            linear.append({"type": "sparse", "name": "l%d" % i, "vocabulary_size": v, "embedding_dim": 4})
            feed["l%d" % i] = rng.randint(0, v, n).astype(np.int32)
        if rng.rand() < 0.5:
            linear.append({"type": "dense", "name": "ld", "dimension": 2})
            feed["ld"] = rng.rand(n, 2).astype(np.float32)
    units = DNN_SHAPES[int(rng.randint(len(DNN_SHAPES)))]
    if seed % 23 == 5:
        units = WIDE_DNN_SHAPES[(seed // 23) % len(WIDE_DNN_SHAPES)]
    act = str(rng.choice(["relu", "relu", "tanh", "sigmoid"]))
    kw = {"seed": 1024 + seed}
    name = model
    if model in ("DeepFM", "WDL", "FNN", "NFM"):
        kw.update(dnn_hidden_units=units, dnn_activation=act)
        if model == "DeepFM" and exotic:
            groups = sorted(set(d.get("group_name", "default_group") for d in dnn if d["type"] == "sparse"))
            kw["fm_group"] = [g for g in groups if rng.rand() < 0.7] or groups[:1]
    elif model in ("DCN", "DCNM"):
        name = "DCN"
        kw.update(dnn_hidden_units=units if rng.rand() < 0.85 else (), dnn_activation=act, cross_num=int(rng.randint(1, 4)),
                  cross_parameterization="vector" if model == "DCN" else "matrix")
    elif model == "DCNMix":
        kw.update(dnn_hidden_units=units, dnn_activation=act, cross_num=int(rng.randint(1, 3)), low_rank=int(rng.choice([4, 32])),
                  num_experts=int(rng.choice([1, 4])))
    elif model == "xDeepFM":
        kw.update(dnn_hidden_units=units, dnn_activation=act, cin_layer_size=[(16, 16), (32,), (128, 128), (10, 6, 4)][int(rng.randint(4))],
                  cin_split_half=bool(rng.rand() < 0.5), cin_activation=str(rng.choice(["relu", "linear"])))
    elif model == "AFM":
        kw.update(use_attention=bool(rng.rand() < 0.8), attention_factor=int(rng.choice([4, 8])))
    elif model == "PNN":
        kw.update(dnn_hidden_units=units, dnn_activation=act, use_inner=bool(rng.rand() < 0.8))
    if rng.rand() < 0.15:
        kw["task"] = "regression"
    if seed >= 60 and model in ("DeepFM", "DCN", "DCNM", "xDeepFM") and kw["dnn_hidden_units"] and rng.rand() < 0.25:
        kw["dnn_use_bn"] = True
    meta = {"model": name, "linear": linear, "dnn": dnn, "kwargs": kw}
    return json.loads(json.dumps(meta)), feed, n


def run_case(seed, device, config=None):
    meta, feed, n = (config or random_config)(seed)
    model = build_model(meta, device)
    rng = np.random.RandomState(seed)
    w = _randomise(model, rng)
    bn = {k: v for k, v in w.items() if "batch_normalization" in k}
    if bn:                              # inference-mode BatchNormalization: a positive moving variance, gamma around 1
        for k, v in bn.items():
            if k.endswith("moving_variance"):
                w[k] = (0.5 + rng.rand(*v.shape)).astype(np.float32)
            elif k.endswith("gamma"):
                w[k] = (1.0 + 0.1 * rng.standard_normal(v.shape)).astype(np.float32)
        model.set_weights_by_name(w)
    g = {"meta": np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)}
    g.update({"w/" + k: v for k, v in w.items()})
    g.update({"feed/" + k: v for k, v in feed.items()})
    ref = np.asarray(run_oracle_model(g, np.float64)).astype(np.float32).reshape(n, 1)
    return meta, model, feed, n, ref


# 400 seeds + what the one-off sweeps over further seeds found (round 6, seeds 400 .. 1199: DeepFM(fm_group=...) over so many groups that
# the head had more than four extra logit vectors to add — 690, 910, 930, 1050, 1170; scripts/gpu_call_r06g.sh)
# 789, 2399, 3199, 3619: xDeepFM configurations whose logits reach 9 - 16 — the CHECKER's finding: logit(p) recovered from fp32
# probabilities is ill-conditioned there, the float32 NumPy oracle misses the old bar too (tests/test_gpu_models.check_probs)
SEEDS = [int(t) for t in os.environ.get("DCTR_FUZZ_SEEDS", "").split(",") if t] or (
    list(range(400)) + [690, 910, 930, 1050, 1170, 789, 2399, 3199, 3619])


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_random_configuration_matches_the_oracle(device, seed):
    meta, model, feed, n, ref = run_case(seed, device)
    what = "fuzz %d %s n=%d" % (seed, meta["model"], n)
    ok = None
    if meta["model"] in FM_MODELS:
        # an all-padding max-pooled sequence is emb - 1e9 in the reference; its second-order terms are rounding noise (test_gpu_models)
        from tests.test_gpu_models import well_conditioned_rows
        ok = well_conditioned_rows(meta, feed, n)
    for bs in (4096, 333):
        y = model.predict(feed, batch_size=bs)
        if meta["kwargs"].get("task") == "regression":      # the raw logit: 1e-4 relative + the fp32 floor of its O(1..10) terms
            assert y.shape == ref.shape and y.dtype == np.float32
            sel = slice(None) if ok is None else ok
            assert_close(y[sel], ref[sel], rtol=1e-4, atol=2e-5, what="%s bs=%d" % (what, bs))
        else:
            check_probs(y, ref, "%s bs=%d" % (what, bs), ok)


DIN_ROWS = [1, 7, 300, 2048, 5000, 33000]


def random_din_config(seed, dims4=False):
    """DIN (deepctr/models/sequence/din.py:25-98): behaviour features with their history sequences on shared tables, further sparse /
    dense / pooled-sequence features, the attention unit's shape and activation, weight normalisation."""
    rng = np.random.RandomState(5000 + seed)
    n = int(DIN_ROWS[seed % len(DIN_ROWS)])
    T = int(rng.choice([1, 4, 10, 50]))
    if n > 5000:
        T = min(T, 10)
    use_hash = bool(rng.rand() < 0.25)
    with_len = bool(rng.rand() < 0.5)
    dnn, feed, hist = [], {}, []
    for i in range(int(rng.randint(0, 4))):
        v = int(rng.choice([3, 50, 1000]))
        dnn.append({"type": "sparse", "name": "u%d" % i, "vocabulary_size": v, "embedding_dim": int(rng.choice([4, 8, 12, 16] if dims4 else [4, 8, 10, 3, 16])), "use_hash": use_hash})
        feed["u%d" % i] = rng.randint(0, v, n).astype(np.int32)
    lens = rng.randint(0, T + 1, n)
    for i in range(int(rng.randint(1, 4))):
        v = int(rng.choice([5, 60, 2000]))
        e = int(rng.choice([4, 8, 16, 32] if dims4 else [4, 8, 16, 32, 6, 10]))
        dnn.append({"type": "sparse", "name": "b%d" % i, "vocabulary_size": v, "embedding_dim": e, "use_hash": use_hash})
        feed["b%d" % i] = rng.randint(1, v, n).astype(np.int32)
        hist.append("b%d" % i)
    for i in range(int(rng.choice([0, 0, 1, 2]))):
        dnn.append({"type": "dense", "name": "d%d" % i, "dimension": int(rng.choice([1, 3]))})
        feed["d%d" % i] = rng.rand(n, dnn[-1]["dimension"]).astype(np.float32)
    for name in hist:
        src = [d for d in dnn if d.get("name") == name][0]
        sf = {"type": "sparse", "name": "hist_" + name, "vocabulary_size": src["vocabulary_size"], "embedding_dim": src["embedding_dim"],
              "use_hash": use_hash, "embedding_name": name}
        d = {"type": "varlen", "sparsefeat": sf, "maxlen": T}
        if with_len:
            d["length_name"] = "seq_length"
        ids = rng.randint(1, src["vocabulary_size"], (n, T)).astype(np.int32)
        ids[np.arange(T)[None, :] >= lens[:, None]] = 0
        feed["hist_" + name] = ids
        dnn.append(d)
    if with_len:
        feed["seq_length"] = lens.astype(np.int32).reshape(n, 1)
    if rng.rand() < 0.3:                  # a pooled sequence beside the attended ones (din.py:73-78)
        v, T2 = 40, int(rng.choice([3, 8]))
        sf = {"type": "sparse", "name": "tags", "vocabulary_size": v, "embedding_dim": int(rng.choice([4, 8])), "use_hash": use_hash}
        dnn.append({"type": "varlen", "sparsefeat": sf, "maxlen": T2, "combiner": str(rng.choice(["mean", "sum"]))})
        l2 = rng.randint(1, T2 + 1, n)
        ids = rng.randint(1, v, (n, T2)).astype(np.int32)
        ids[np.arange(T2)[None, :] >= l2[:, None]] = 0
        feed["tags"] = ids
    kw = {"seed": 1024 + seed, "dnn_hidden_units": DNN_SHAPES[int(rng.randint(len(DNN_SHAPES)))],
          "dnn_activation": str(rng.choice(["relu", "relu", "tanh", "sigmoid"])),
          "att_hidden_size": [(80, 40), (8,), (64, 16), (36, 20, 4)][int(rng.randint(4))],
          "att_activation": str(rng.choice(["dice", "dice", "sigmoid", "relu"])),
          "att_weight_normalization": bool(rng.rand() < 0.5)}
    if seed % 11 == 3:
        kw["dnn_hidden_units"] = WIDE_DNN_SHAPES[(seed // 11) % len(WIDE_DNN_SHAPES)]
    if rng.rand() < 0.2:
        kw["dnn_use_bn"] = True
    if rng.rand() < 0.1:
        kw["task"] = "regression"
    meta = {"model": "DIN", "linear": [], "dnn": dnn, "kwargs": kw, "extra_args": [hist]}
    return json.loads(json.dumps(meta)), feed, n


@pytest.mark.gpu
# (+ 295, 323, 355, 365: round 6's sweep — three history features of widths 32 + 32 + 16 / 32: a key width no attention kernel held)
@pytest.mark.parametrize("seed", [int(t) for t in os.environ.get("DCTR_FUZZ_DIN_SEEDS", "").split(",") if t] or (list(range(90)) + [295, 323, 355, 365]))
def test_random_din_configuration_matches_the_oracle(device, seed):
    meta, model, feed, n, ref = run_case(seed, device, random_din_config)
    what = "fuzz DIN %d n=%d" % (seed, n)
    for bs in (2048, 333):
        y = model.predict(feed, batch_size=bs)
        if meta["kwargs"].get("task") == "regression":
            assert y.shape == ref.shape and y.dtype == np.float32
            assert_close(y, ref, rtol=1e-4, atol=2e-5, what="%s bs=%d" % (what, bs))
        else:
            check_probs(y, ref, "%s bs=%d" % (what, bs))


def _fit_once(meta, feed, y, weights, device, hip, optimizer, bs):
    model = build_model(meta, device)
    model.set_weights_by_name(weights)
    model.hip_training = hip
    model.compile(optimizer, "binary_crossentropy" if meta["kwargs"].get("task", "binary") == "binary" else "mse")
    h = model.fit(feed, y, batch_size=bs, epochs=1, verbose=0, shuffle=False)
    return model, h.history["loss"][-1]


@pytest.mark.gpu
# (+ 569, 581: round 6's sweep — Adam losses 1.2 - 1.5 x off their bar while the HIP step reported the l2 penalties of an epoch's two ends;
#  + 14, 28, 42 ... hold features of the linear part alone, on the HIP step since round 6)
@pytest.mark.parametrize("seed", [int(t) for t in os.environ.get("DCTR_FUZZ_FIT_SEEDS", "").split(",") if t] or (list(range(160)) + [569, 581, 306, 312, 329]))
def test_random_configuration_trains_alike_on_the_hip_and_the_autograd_step(device, seed):
    """fit() — three consecutive batches, the last one ragged — on the HIP training step against the torch-autograd step (the checker:
    autograd over the restatement of the forward that tests/test_training_checker_cpu.py pins to the fixtures) from the same weights:
    the same loss and the same updated weights.  SGD shows every gradient linearly (two of three seeds), Adam the optimizer's own path."""
    from deepctr_amd import training_hip
    bs = [64, 256, 1000][seed % 3]
    n = 2 * bs + max(1, bs // 3)
    dims4 = seed % 4 != 3                 # (three of four: widths the HIP step takes)
    if seed % 5:
        meta, feed, n = random_config(seed // 5 * 4 + seed % 5 - 1 + (240 if seed % 7 == 0 else 0), rows=n, dims4=dims4)   # every model kind in turn
    else:
        meta, feed, n = random_din_config(seed, dims4=dims4)
        n = min(n, 2 * bs + max(1, bs // 3), 700)
        feed = {k: v[:n] for k, v in feed.items()}
    _check_fit(meta, feed, n, seed, bs, device)


def _check_fit(meta, feed, n, seed, bs, device, must_be_supported=False):
    from deepctr_amd import training_hip
    rng = np.random.RandomState(seed)
    probe = build_model(meta, device)
    if not training_hip.supported(probe):
        assert not must_be_supported, "%s: fit() would take the autograd step" % meta["model"]
        pytest.skip("%s: outside the HIP training step's family (fit() takes the autograd step)" % meta["model"])
    w = _randomise(probe, rng)
    for k, v in w.items():
        if "batch_normalization" in k and k.endswith("moving_variance"):
            w[k] = (0.5 + rng.rand(*v.shape)).astype(np.float32)
    # (the probe scores with the STORED statistics: it must see the positive variances too — before this line every configuration with
    #  BatchNormalization / Dice probed NaN logits and was skipped as "saturated")
    probe.set_weights_by_name(w)
    y = (rng.rand(n) > 0.5).astype(np.float32)
    optimizer = "adam" if seed % 3 == 2 else "sgd"
    lg = probe.predict_logits(feed, batch_size=4096) if hasattr(probe, "predict_logits") else np.zeros(1)
    if not (np.isfinite(lg).all() and np.abs(lg).max() < 30.0):
        pytest.skip("fit fuzz %d %s: the random weights saturate the output (|logit| up to %.3g): gradients overflow fp32 in either step"
                    % (seed, meta["model"], float(np.abs(lg).max())))
    m_hip, loss_hip = _fit_once(meta, feed, y, w, device, True, optimizer, bs)
    assert getattr(m_hip, "_hip_trainer", None) is not None, "fit() did not take the HIP training step"
    m_ref, loss_ref = _fit_once(meta, feed, y, w, device, False, optimizer, bs)
    assert getattr(m_ref, "_hip_trainer", None) is None
    what = "fit fuzz %d %s %s bs=%d" % (seed, meta["model"], optimizer, bs)
    if not (np.isfinite(loss_ref) and loss_ref < 50.0):
        pytest.skip("%s: the random weights diverge under this optimizer (loss %.3g): nothing to compare" % (what, loss_ref))
    # (both steps add the l2 penalties at every batch's weights — the HIP step inside its optimizer launch: tests/test_gpu_l2.py)
    assert_close(np.array([loss_hip]), np.array([loss_ref]), rtol=1e-3, atol=1e-6, what=what + " loss")
    w_hip, w_ref = m_hip.get_weights_by_name(), m_ref.get_weights_by_name()
    for k in w_ref:
        d_hip, d_ref = (w_hip[k] - w[k]).astype(np.float64), (w_ref[k] - w[k]).astype(np.float64)
        moved = float(np.abs(d_ref).max())
        scale = max(moved, 1e-6)          # (updates below 1e-6: a saturated layer's gradient is rounding noise)
        err = np.abs(d_hip - d_ref) / scale
        if optimizer == "sgd":
            # three SGD steps: the update is the sum of three gradients — within 2 % of the tensor's largest update everywhere (a wrong
            # or missing term is O(1); cancelling sums of either step leave a few 1e-3)
            assert float(err.max()) < 2e-2, "%s: update of %s (largest %.3g): off by %.3g of it" % (what, k, moved, float(err.max()))
        else:
            # Adam's steps are ~ lr * sign(g): an element whose gradient is rounding noise may take either sign — all but 1 % agree to 10 %
            if moved < 3e-4:              # (a tensor whose largest step in three is a tenth of lr: gradients around epsilon, i.e. noise)
                continue
            bad = float((err > 0.1).mean())
            assert bad < 1e-2, "%s: update of %s (largest %.3g): %.2f %% of the elements differ by > 10 %% of it" % (what, k, moved, 100 * bad)


WIDE_CIN_WIDTHS = [132, 160, 192, 256, 131, 136]


def wide_xdeepfm_config(seed, rows=None):
    """An xDeepFM configuration of random_config with every embedding as wide as WIDE_CIN_WIDTHS says: past the 128 dimensions one
    workgroup of the CIN kernel holds (the reference's CIN takes any width, interaction.py:277-325; "auto" = 6 * vocab ** 0.25 passes 128
    from 2e5 ids on, feature_column.py:44-45) — dctr_cin_fwd walks such samples in slices of d."""
    meta, feed, n = random_config(9 + 10 * seed, rows=[300, 1000, 4099, 65][seed % 4] if rows is None else rows)
    assert meta["model"] == "xDeepFM"
    W = WIDE_CIN_WIDTHS[seed % len(WIDE_CIN_WIDTHS)]
    for lst in (meta["dnn"], meta["linear"]):
        for d in lst:
            if d["type"] == "sparse":
                d["embedding_dim"] = W
            elif d["type"] == "varlen":
                d["sparsefeat"]["embedding_dim"] = W
    return meta, feed, n


@pytest.mark.gpu
@pytest.mark.parametrize("seed", list(range(12)))
def test_xdeepfm_over_embeddings_wider_than_128_matches_the_oracle(device, seed):
    meta, model, feed, n, ref = run_case(seed, device, wide_xdeepfm_config)
    from tests.test_gpu_models import well_conditioned_rows
    ok = well_conditioned_rows(meta, feed, n)
    what = "wide xDeepFM %d (embedding_dim %d) n=%d" % (seed, WIDE_CIN_WIDTHS[seed % len(WIDE_CIN_WIDTHS)], n)
    for bs in (4096, 333):
        y = model.predict(feed, batch_size=bs)
        if meta["kwargs"].get("task") == "regression":
            assert_close(y[ok], ref[ok], rtol=1e-4, atol=2e-5, what="%s bs=%d" % (what, bs))
        else:
            check_probs(y, ref, "%s bs=%d" % (what, bs), ok)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", list(range(6)))
def test_xdeepfm_over_embeddings_wider_than_128_trains_on_the_hip_step(device, seed):
    """... and fit() keeps the HIP training step for them (the forward's saved activations are the sample's rows whatever the slicing;
    dctr_cin_bwd works on rows (b, d))."""
    bs = [64, 256][seed % 2]
    n = 2 * bs + max(1, bs // 3)
    meta, feed, n = wide_xdeepfm_config(seed, rows=n)
    if any(d["type"] == "sparse" and d not in meta["dnn"] for d in meta["linear"]):
        pytest.skip("linear-only features: the autograd step")
    _check_fit(meta, feed, n, 7000 + seed, bs, device, must_be_supported=True)


@pytest.mark.gpu
@pytest.mark.parametrize("par,emb,cross_num", [("matrix", 32, 2), ("vector", 64, 2), ("matrix", 64, 1), ("vector", 96, 3)])
def test_dcn_over_criteo_width_inputs_trains_on_the_hip_step(device, par, emb, cross_num):
    """DCN over Criteo's 26 + 13 columns at embedding_dim 32 / 64 / 96 — 845 / 1,677 / 2,509 DNN-input columns: past the one-kernel
    training forward of the matrix CrossNet (~832) and the one-kernel backward of the vector form (2048 columns, 48 L d bytes of LDS).
    Round 6: fit() keeps the HIP step (layer-by-layer forward into saved_u / saved_x; layer-by-layer vector backward) — same loss and
    updates as the autograd step; predict() against the float64 oracle."""
    seed = {"matrix": 11, "vector": 12}[par] + emb
    rng = np.random.RandomState(seed)
    bs = 64
    n = 2 * bs + 21
    cols, feed = [], {}
    for i in range(26):
        v = int(rng.choice([7, 100, 1000]))
        cols.append({"type": "sparse", "name": "C%d" % i, "vocabulary_size": v, "embedding_dim": emb})
        feed["C%d" % i] = rng.randint(0, v, n).astype(np.int32)
    for i in range(13):
        cols.append({"type": "dense", "name": "I%d" % i, "dimension": 1})
        feed["I%d" % i] = rng.rand(n, 1).astype(np.float32)
    meta = json.loads(json.dumps({"model": "DCN", "linear": cols, "dnn": cols, "kwargs": {
        "seed": 1024 + seed, "cross_num": cross_num, "cross_parameterization": par, "dnn_hidden_units": [64, 32], "dnn_activation": "relu"}}))
    _, model, _, _, ref = run_case(seed, device, lambda s: (meta, feed, n))
    check_probs(model.predict(feed, batch_size=4096), ref, "DCN %s emb %d" % (par, emb), None)
    _check_fit(meta, feed, n, seed, bs, device, must_be_supported=True)


DIN_KEY_WIDTHS = [128, 6, 10, 72, 3, 100]


def odd_width_din_config(seed, rows=None):
    """A DIN configuration of random_din_config whose behaviour features (and their histories) are DIN_KEY_WIDTHS wide: not a multiple of
    4, or past 64 — the widths the HIP training step left to the autograd step before round 6."""
    meta, feed, n = random_din_config(seed)
    if rows is not None and rows < n:
        n = rows
        feed = {k: v[:n] for k, v in feed.items()}
    W = DIN_KEY_WIDTHS[seed % len(DIN_KEY_WIDTHS)]
    hist = set(meta["extra_args"][0])
    for d in meta["dnn"]:
        if d["type"] == "sparse" and d["name"] in hist:
            d["embedding_dim"] = W
        elif d["type"] == "varlen" and d["sparsefeat"].get("embedding_name") in hist:
            d["sparsefeat"]["embedding_dim"] = W
    return meta, feed, n


@pytest.mark.gpu
@pytest.mark.parametrize("seed", list(range(12)))
def test_din_over_any_key_width_trains_on_the_hip_step(device, seed):
    bs = [64, 256][seed % 2]
    meta, feed, n = odd_width_din_config(seed, rows=2 * bs + max(1, bs // 3))
    _, model, _, _, ref = run_case(seed, device, lambda s: (meta, feed, n))
    what = "DIN key width %d (%d)" % (DIN_KEY_WIDTHS[seed % len(DIN_KEY_WIDTHS)], seed)
    y = model.predict(feed, batch_size=4096)
    if meta["kwargs"].get("task") == "regression":
        assert_close(y, ref, rtol=1e-4, atol=2e-5, what=what)
    else:
        check_probs(y, ref, what, None)
    _check_fit(meta, feed, n, 9000 + seed, bs, device, must_be_supported=True)


def test_random_configurations_are_valid_for_the_oracle():
    """CPU: the generator's configurations build (CPU-resident weights) and the oracle scores them — the GPU test's inputs are sound."""
    import torch
    for seed in range(0, 400, 7):
        meta, feed, n = random_config(seed)
        if n > 1000:
            continue
        _, _, _, n, ref = run_case(seed, torch.device("cpu"))
        assert ref.shape == (n, 1) and np.isfinite(ref).all()
    for seed in range(0, 90, 6):
        meta, feed, n = random_din_config(seed)
        if n > 1000:
            continue
        _, _, _, n, ref = run_case(seed, torch.device("cpu"), random_din_config)
        assert ref.shape == (n, 1) and np.isfinite(ref).all()
