"""GPU: BST's forward (dctr_transformer_fwd in place over the key buffer + the attention pooling and DNN kernels) against the reference's
own outputs and the float64 oracle (tests/ref_bst.py), the Transformer layer against its fixtures, the transformer kernel against the
oracle over a seeded sweep of shapes (both routes, every flag, both mask forms, in place and out of place), live weights, fit() on the
autograd step and a seeded fuzz over BST configurations."""
import numpy as np
import pytest
import torch

from tests import ref_bst as RB
from tests.test_autoint_cpu import att_rows
from tests.test_bst_cpu import BST_FIXTURES, LAYER_TAGS, build_bst, fixture_feed, fixture_weights, layer_case, layer_flags
from tests.test_gpu_models import check_probs
from tests.util import assert_close, golden_meta, load_golden

pytestmark = pytest.mark.gpu

FLAGS = dict(use_positional_encoding=True, use_res=True, use_feed_forward=True, use_layer_norm=True, blinding=False)


def make_weights(rng, T, E, L):
    out = []
    for _ in range(L):
        w = {k: rng.standard_normal((E, E)) * (0.6 / np.sqrt(E)) for k in ("query", "key", "value")}
        w["fw1"] = rng.standard_normal((E, 4 * E)) * (0.6 / np.sqrt(E))
        w["fw2"] = rng.standard_normal((4 * E, E)) * (0.6 / np.sqrt(4 * E))
        w["ln_gamma"] = 1.0 + 0.2 * rng.standard_normal(E)
        w["ln_beta"] = 0.1 * rng.standard_normal(E)
        w["pe_q"] = 0.3 * rng.standard_normal((T, E))
        w["pe_k"] = 0.3 * rng.standard_normal((T, E))           # pe_q != pe_k always
        out.append({k: v.astype(np.float32) for k, v in w.items()})
    return out


def device_weights(ws, E, device):
    """The op's operands: the positional tables folded with float32(sqrt(E)) as the layer does."""
    out = []
    for w in ws:
        t = {k: torch.from_numpy(v).to(device) for k, v in w.items()}
        s = np.float32(E ** 0.5)
        t["pe_q"], t["pe_k"] = t["pe_q"] * float(s), t["pe_k"] * float(s)
        out.append(t)
    return out


def oracle(x, keys, ws, H, qm, km, flags, output_type, dtype=np.float64):
    h, k = x.astype(dtype), keys.astype(dtype)
    for i, w in enumerate(ws):
        last = i == len(ws) - 1
        h = RB.transformer(h, k, w, H, qm, km, output_type=output_type if last else None, dtype=dtype, **flags)
        k = h
    return h


def draw_lengths(rng, B, T):
    base = np.array([0, 1, T - 1, T, T + 3])
    lens = rng.randint(0, T + 4, size=B)
    n = min(B, base.size)
    lens[:n] = base[:n]
    return lens.astype(np.int32)


def within_bar(got, ref):
    """The project's bar for the attention stack: |err| <= 1e-4 |ref| + 2e-6 max|ref of the sample|; returns max err / bar."""
    got, ref = got.reshape(got.shape[0], -1).astype(np.float64), ref.reshape(ref.shape[0], -1)
    scale = np.abs(ref).max(axis=1, keepdims=True) + 1e-30
    return float((np.abs(got - ref) / (1e-4 * np.abs(ref) + 2e-6 * scale)).max())


def sweep_variants():
    """(flags, output_type) of every run of a sweep case: BST's flags first, each flag off once, blinding on once, mean and sum."""
    variants = [(FLAGS, None)]
    variants += [(dict(FLAGS, **{k: False}), None) for k in ("use_positional_encoding", "use_res", "use_feed_forward", "use_layer_norm")]
    return variants + [(dict(FLAGS, blinding=True), None), (FLAGS, "mean"), (FLAGS, "sum")]


SWEEP = [  # T, E, H, layers, B
    (1, 4, 2, 1, 5),            # one position
    (5, 4, 1, 1, 33),           # E and T below a tile
    (17, 12, 3, 2, 9),          # nothing a multiple of 16, d = 4
    (16, 16, 16, 1, 7),         # d = 1
    (50, 32, 8, 2, 130),        # BST's own shape, a batch that is no multiple of S
    (64, 64, 8, 1, 6),
    (200, 64, 8, 2, 3),         # one sample exceeds the LDS: the general route
]


@pytest.mark.parametrize("T,E,H,L,B", SWEEP)
def test_transformer_op_vs_float64_oracle(device, T, E, H, L, B):
    from deepctr_amd import ops
    rng = np.random.RandomState(T * 1000 + E * 10 + L)
    ws = make_weights(rng, T, E, L)
    tw = device_weights(ws, E, device)
    lens = draw_lengths(rng, B, T)
    mask = RB.sequence_mask(lens, T)
    pad = 3
    xbuf = rng.standard_normal((B, T, E + pad)).astype(np.float32)        # padding columns after every position
    x = xbuf[:, :, :E]
    route = ops.transformer_route(T, E, H, L, **FLAGS)
    assert route == ("general" if T == 200 else "fused")
    assert (ops.transformer_workspace_bytes(B, T, E, H, L, **FLAGS) > 0) == (route == "general")
    lt = torch.from_numpy(lens).to(device)

    def run(flags, output_type, in_place=False, masks=False):
        xt = torch.from_numpy(xbuf).to(device)
        if in_place:
            obuf = xt
        else:
            obuf = torch.full((B, T, E + pad) if output_type is None else (B, E + pad), float("nan"), device=device)
        out = obuf[..., :E]
        kw = dict(query_lengths=lt, key_lengths=lt)
        if masks:
            m = torch.from_numpy(mask.astype(np.uint8)).to(device)
            kw = dict(query_mask=m, key_mask=m)
        ops.transformer(xt[:, :, :E], tw, H, output_type=output_type, out=out, **dict(flags, **kw))
        torch.cuda.synchronize()
        return obuf.cpu().numpy()

    base = run(FLAGS, None)
    assert np.isnan(base[:, :, E:]).all(), "the padding columns of out were written"
    got = base[:, :, :E]
    assert np.isfinite(got).all()
    ref = oracle(x, x, ws, H, mask, mask, FLAGS, None)
    worst = within_bar(got, ref)
    print("T %d E %d H %d L %d B %d (%s): max err / bar %.3g" % (T, E, H, L, B, route, worst))
    assert worst <= 1.0, "max err / bar %.3g" % worst
    inp = run(FLAGS, None, in_place=True)
    assert np.array_equal(inp[:, :, :E], got), "in place differs from out of place"
    assert np.array_equal(inp[:, :, E:], xbuf[:, :, E:]), "the padding columns of x were written"
    assert np.array_equal(run(FLAGS, None, masks=True)[:, :, :E], got), "the uint8-mask form differs from the lengths form"
    for flags, ot in sweep_variants()[1:]:
        o = run(flags, ot)
        g = o[..., :E]
        assert np.isnan(o[..., E:]).all() and np.isfinite(g).all()
        r = oracle(x, x, ws, H, mask, mask, flags, ot)
        worst = within_bar(g, r.reshape(g.shape))
        what = "%s output_type=%s" % ([k for k in FLAGS if flags[k] != FLAGS[k]], ot)
        print("   %s: max err / bar %.3g" % (what, worst))
        assert worst <= 1.0, "%s: max err / bar %.3g" % (what, worst)


def test_cross_form_with_separate_keys(device):
    from deepctr_amd import ops
    rng = np.random.RandomState(11)
    T, E, H, B = 7, 8, 2, 10
    ws = make_weights(rng, T, E, 1)
    q, k = (rng.standard_normal((B, T, E)).astype(np.float32) for _ in range(2))
    ql, kl = draw_lengths(rng, B, T), draw_lengths(rng, B, T)[::-1].copy()
    ref = oracle(q, k, ws, H, RB.sequence_mask(ql, T), RB.sequence_mask(kl, T), FLAGS, None)
    km_out = torch.zeros(B, T, dtype=torch.uint8, device=device)
    got = ops.transformer(torch.from_numpy(q).to(device), device_weights(ws, E, device), H, keys=torch.from_numpy(k).to(device),
                          query_lengths=torch.from_numpy(ql).to(device), key_lengths=torch.from_numpy(kl).to(device), key_mask_out=km_out,
                          **FLAGS)
    assert within_bar(got.cpu().numpy(), ref) <= 1.0
    assert np.array_equal(km_out.cpu().numpy().astype(bool), RB.sequence_mask(kl, T))


@pytest.mark.parametrize("output_type", [None, "mean", "sum"])
def test_more_layers_than_one_launch_takes_are_chained(device, output_type):
    """17 layers: two launches, chained through out (output_type None) or through the workspace (pooled outputs)."""
    from deepctr_amd import ops
    rng = np.random.RandomState(15)
    T, E, H, L, B = 4, 4, 2, 17, 11
    ws = make_weights(rng, T, E, L)
    x = rng.standard_normal((B, T, E)).astype(np.float32)
    lens = draw_lengths(rng, B, T)
    mask = RB.sequence_mask(lens, T)
    assert (ops.transformer_workspace_bytes(B, T, E, H, L, output_type=output_type, **FLAGS) > 0) == (output_type is not None)
    lt = torch.from_numpy(lens).to(device)
    xt = torch.from_numpy(x).to(device)
    got = ops.transformer(xt, device_weights(ws, E, device), H, query_lengths=lt, key_lengths=lt, output_type=output_type, **FLAGS)
    ref = oracle(x, x, ws, H, mask, mask, FLAGS, output_type)
    assert torch.equal(xt.cpu(), torch.from_numpy(x)), "the input was written"
    worst = within_bar(got.cpu().numpy(), ref.reshape(tuple(got.shape)))
    assert worst <= 1.0, "max err / bar %.3g" % worst


def test_routes_agree(device):
    from deepctr_amd import ops
    rng = np.random.RandomState(12)
    T, E, H, L, B = 24, 16, 4, 2, 21
    ws = make_weights(rng, T, E, L)
    tw = device_weights(ws, E, device)
    x = rng.standard_normal((B, T, E)).astype(np.float32)
    lens = draw_lengths(rng, B, T)
    mask = RB.sequence_mask(lens, T)
    ref = oracle(x, x, ws, H, mask, mask, FLAGS, None)
    lt = torch.from_numpy(lens).to(device)
    assert ops.transformer_route(T, E, H, L, route="general", **FLAGS) == "general"
    assert ops.transformer_route(T, E, H, L, route="fused", **FLAGS) == "fused"
    for route in ("fused", "general"):
        got = ops.transformer(torch.from_numpy(x).to(device), tw, H, query_lengths=lt, key_lengths=lt, route=route, **FLAGS)
        worst = within_bar(got.cpu().numpy(), ref)
        assert worst <= 1.0, "%s route: max err / bar %.3g" % (route, worst)


def test_live_weights(device):
    """A positional table or gamma changed in place between two calls changes the output: nothing is folded or cached across calls."""
    from deepctr_amd.layers import Transformer
    rng = np.random.RandomState(13)
    B, T, E, H = 9, 6, 8, 2
    layer = Transformer(E // H, H, use_layer_norm=True, blinding=False, output_type=None, device=device)
    x = torch.from_numpy(rng.standard_normal((B, T, E)).astype(np.float32)).to(device)
    lens = torch.from_numpy(draw_lengths(rng, B, T)).to(device)
    y0 = layer([x, x, lens.reshape(-1, 1), lens.reshape(-1, 1)]).clone()
    assert torch.equal(layer([x, x, lens.reshape(-1, 1), lens.reshape(-1, 1)]), y0)
    for t in (layer.query_pe.w("lookup_table"), layer.key_pe.w("lookup_table"), layer.ln.w("gamma"), layer.ln.w("beta")):
        with torch.no_grad():
            t.add_(0.25)
        y1 = layer([x, x, lens.reshape(-1, 1), lens.reshape(-1, 1)]).clone()
        assert not torch.equal(y1, y0)
        y0 = y1
    # and the result is the oracle's over the live weights
    w = {k: v.cpu().numpy() for k, v in (("query", layer.w("query")), ("key", layer.w("key")), ("value", layer.w("value")),
                                         ("fw1", layer.w("fw1")), ("fw2", layer.w("fw2")), ("ln_gamma", layer.ln.w("gamma")),
                                         ("ln_beta", layer.ln.w("beta")), ("pe_q", layer.query_pe.w("lookup_table")),
                                         ("pe_k", layer.key_pe.w("lookup_table")))}
    m = RB.sequence_mask(lens.cpu().numpy(), T)
    ref = oracle(x.cpu().numpy(), x.cpu().numpy(), [w], H, m, m, FLAGS, None)
    assert within_bar(y0.cpu().numpy(), ref) <= 1.0


@pytest.mark.parametrize("name", BST_FIXTURES)
def test_bst_matches_reference_code(device, name):
    g = load_golden(name)
    meta = golden_meta(g)
    model = build_bst(meta, device)
    model.set_weights_by_name(fixture_weights(g))
    feed = fixture_feed(g)
    assert (feed["seq_length"] == 0).any()                                  # length-0 rows are compared, not excluded
    rows = att_rows(meta, feed, g["y"].shape[0])
    assert rows.sum() >= 0.5 * rows.size
    for bs in (256, 5, 37):
        check_probs(model.predict(feed, batch_size=bs), g["y"], "%s bs=%d" % (name, bs), rows)
    y = model.predict([feed[n] for n in model.input_names], batch_size=64)
    check_probs(y, g["y"], name + " list feed", rows)
    assert_close(np.asarray(model.predict_logits(feed, batch_size=256)).reshape(-1),
                 RB.run_fixture(g, np.float64, task="regression").reshape(-1), rtol=1e-4, atol=2e-5, what=name + " logits vs float64")


@pytest.mark.parametrize("tag", LAYER_TAGS)
def test_transformer_layer_matches_reference_code(device, tag):
    from deepctr_amd.layers import Transformer
    g = load_golden("transformer_layer")
    cfg, q, k, qm, km, w, named, y = layer_case(g, tag)
    layer = Transformer(device=device, **cfg)
    layer.build([(None,) + q.shape[1:], (None,) + k.shape[1:]])
    layer.set_weights(list(named.values()))
    tq = torch.from_numpy(q).to(device)
    tk = tq if tag != "cross" else torch.from_numpy(k).to(device)
    if cfg["supports_masking"]:
        got = layer.call([tq, tk], mask=[torch.from_numpy(qm).to(device), torch.from_numpy(km).to(device)])
    else:
        ql, kl = (torch.from_numpy(g[tag + "/%s_lengths" % s].reshape(-1, 1)).to(device) for s in ("query", "key"))
        got = layer.call([tq, tk, ql, kl])
    assert tuple(got.shape) == y.shape
    ref = RB.transformer(q, k, w, cfg["head_num"], qm, km, dtype=np.float64, **layer_flags(cfg))
    assert within_bar(got.cpu().numpy(), ref) <= 1.0
    assert_close(got.cpu().numpy(), y, rtol=1e-4, atol=2e-6, what="transformer layer " + tag)


def test_layer_normalization_layer(device):
    from deepctr_amd.layers import LayerNormalization
    rng = np.random.RandomState(14)
    x = rng.standard_normal((7, 5, 12)).astype(np.float32)
    ln = LayerNormalization(device=device)
    ln.build((None, 5, 12))
    gamma, beta = (1 + 0.2 * rng.standard_normal(12)).astype(np.float32), (0.1 * rng.standard_normal(12)).astype(np.float32)
    ln.set_weights([gamma, beta])
    got = ln(torch.from_numpy(x).to(device)).cpu().numpy()
    ref = RB.layer_norm(x.astype(np.float64), gamma.astype(np.float64), beta.astype(np.float64))
    assert_close(got, ref, rtol=1e-5, atol=2e-6, what="LayerNormalization")


def _bst_problem(rng, n, n_hist=2, T=6, widths=(8, 4), hash_=False, extra_seq=False, dense=False, vocab=30):
    from deepctr_amd.feature_column import DenseFeat, SparseFeat, VarLenSparseFeat
    names = ["item_id", "cate_id", "shop_id"][:n_hist]
    cols = [SparseFeat("user", 7, 4, use_hash=hash_)]
    cols += [SparseFeat(nm, vocab, w, use_hash=hash_) for nm, w in zip(names, widths)]
    cols += [VarLenSparseFeat(SparseFeat("hist_" + nm, vocab, w, embedding_name=nm, use_hash=hash_), T, length_name="seq_length")
             for nm, w in zip(names, widths)]
    hi = 10 ** 6 if hash_ else vocab
    feed = {"user": rng.randint(0, 10 ** 6 if hash_ else 7, n).astype(np.int32)}
    lens = rng.randint(0, T + 4, n).astype(np.int32)
    lens[:min(n, 4)] = np.array([0, 1, T, T + 3])[:min(n, 4)]
    feed["seq_length"] = lens
    for nm in names:
        feed[nm] = rng.randint(1, hi, n).astype(np.int32)
        ids = rng.randint(1, hi, (n, T)).astype(np.int32)
        ids[np.arange(T)[None, :] >= lens[:, None]] = 0
        feed["hist_" + nm] = ids
    if extra_seq:
        cols.append(VarLenSparseFeat(SparseFeat("other_seq", 11, 6), 4, combiner="mean"))
        ids = rng.randint(1, 11, (n, 4)).astype(np.int32)
        ol = rng.randint(1, 5, n)
        ids[np.arange(4)[None, :] >= ol[:, None]] = 0
        feed["other_seq"] = ids
    if dense:
        cols.append(DenseFeat("pay_score", 1))
        feed["pay_score"] = rng.rand(n).astype(np.float32)
    return cols, names, feed


def _randomise(model, rng):
    """Trained-like weights: the LayerNorm affine away from (1, 0), the two positional tables of a layer apart."""
    new = {}
    for k, v in model.get_weights_by_name().items():
        draw = rng.standard_normal(v.shape)
        if k.endswith("embeddings"):
            a = 0.3 * draw
        elif k.endswith("gamma"):
            a = 1.0 + 0.2 * draw
        elif k.endswith("moving_variance"):
            a = rng.uniform(0.5, 1.5, v.shape)
        elif k.endswith("lookup_table"):
            a = v + 0.1 * draw
        elif "bias" in k or k.endswith("beta") or k.endswith("moving_mean"):
            a = 0.1 * draw
        else:
            a = draw * (v.std() if v.std() > 0 else 0.1)
        new[k] = a.astype(np.float32)
    model.set_weights_by_name(new)
    return new


def test_fit_takes_the_autograd_step_and_learns(device):
    from deepctr_amd import engine, training, training_hip
    from deepctr_amd.models import BST
    rng = np.random.RandomState(9)
    n = 4096
    cols, names, feed = _bst_problem(rng, n, T=6, vocab=20)
    y = ((feed["item_id"] % 2) ^ (feed["hist_item_id"][:, 0] % 2)).astype(np.float32)      # planted: the candidate against the history
    model = BST(cols, names, transformer_num=2, att_head_num=2, dnn_hidden_units=(32, 16), device=device)
    assert not training_hip.supported(model)
    before = {k: t.clone() for layer in model.transformers for k, t in layer.named_weights()}
    assert len(before) == 2 * 9
    model.compile("adam", "binary_crossentropy")
    hist = model.fit(feed, y, batch_size=256, epochs=3, verbose=0)
    assert getattr(model, "_hip_trainer", None) is None
    assert hist.history["loss"][-1] < hist.history["loss"][0]
    after = {k: t for layer in model.transformers for k, t in layer.named_weights()}
    unchanged = [k for k in before if torch.equal(before[k], after[k])]
    assert not unchanged, "weights the fit did not move: %s" % unchanged      # both positional tables and gamma / beta included
    sub = {k: v[:1024] for k, v in feed.items()}
    staged = engine.Staged(1024)
    model._stage_inputs(sub, staged)
    model._begin()
    with torch.no_grad():
        ref = training.model_logits(model, staged, 0, 1024).cpu().numpy()
    assert_close(np.asarray(model.predict_logits(sub, batch_size=1024)).reshape(-1), ref, rtol=1e-4, atol=2e-5,
                 what="predict after fit vs model_logits")


@pytest.mark.parametrize("seed", range(20))
def test_fuzz_predict_logits_vs_oracle(device, seed):
    """Seeded random BST configurations against the float64 oracle, at the model-level bar the EDCN fuzz applies where no magnitude
    mode exists (softmax and LayerNormalization are not sums of products): rtol 1e-4, atol 2e-5 on the logit."""
    from deepctr_amd.models import BST
    rng = np.random.RandomState(3000 + seed)
    n_hist = int(rng.randint(1, 4))
    T = int(rng.randint(1, 13))
    widths = [int(rng.choice([2, 4, 6, 8])) for _ in range(n_hist)]
    E = sum(widths)
    H = int(rng.choice([h for h in (1, 2, 3, 4, 6, 8) if E % h == 0]))
    L = int(rng.randint(1, 4))
    hash_, use_bn = bool(rng.rand() < 0.3), bool(rng.rand() < 0.3)
    task = "regression" if rng.rand() < 0.25 else "binary"
    n = int(rng.randint(3, 200))
    cols, names, feed = _bst_problem(rng, n, n_hist, T, widths, hash_, extra_seq=bool(rng.rand() < 0.5), dense=bool(rng.rand() < 0.5))
    model = BST(cols, names, transformer_num=L, att_head_num=H, use_bn=use_bn, dnn_hidden_units=(16, 8), task=task, device=device)
    w = _randomise(model, rng)
    what = "seed %d: hist=%d T=%d widths=%s H=%d L=%d hash=%d bn=%d %s n=%d" % (seed, n_hist, T, widths, H, L, hash_, use_bn, task, n)
    got = np.asarray(model.predict_logits(feed, batch_size=64)).reshape(-1)
    ref = RB.bst(cols, names, w, feed, transformer_num=L, att_head_num=H, use_bn=use_bn, task="regression", dtype=np.float64).reshape(-1)
    assert np.isfinite(got).all()
    assert_close(got, ref, rtol=1e-4, atol=2e-5, what=what)
