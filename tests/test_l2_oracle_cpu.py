"""CPU: tests/ref_l2.py before the GPU sees it — the rule "which weight carries which regulariser" on every model kind's weight names,
the closed form w_0 (1 - 2 lr l)^t and the epoch loss against torch float64 (autograd of sum l sum(w^2), a plain SGD step), and
training.regularized_weights (what the autograd step and evaluate() add to the loss) against the rule."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_l2 as RL  # noqa: E402


def _names(kind, frozen=False):
    model = RL.make_model(kind, "cpu", frozen=frozen)
    return model, list(model.get_weights_by_name())


@pytest.mark.parametrize("kind", RL.KINDS)
def test_the_rule_places_every_weight(kind):
    """Every weight name of every kind has a family or is known to have none, and the families a kind must have are there."""
    model, names = _names(kind)
    fams = {n: RL.family(kind, n) for n in names}
    have = {f for f in fams.values() if f}
    want = {"embedding", "dnn"}
    if kind in ("DeepFM", "WDL", "NFM", "AFM", "DCN", "DCNMatrix", "DCNMix", "xDeepFM", "FLEN"):
        want.add("linear")
    if kind == "AFM":
        want = {"embedding", "linear", "att"}
    if kind in ("DCN", "DCNMatrix", "DCNMix"):
        want.add("cross")
    if kind == "xDeepFM":
        want.add("cin")
    assert have == want, (kind, have)
    l2s = RL.l2_by_name(kind, names)
    assert len(set(RL.REGS.values())) == len(RL.REGS)                      # one value per family: a swapped regulariser shows
    assert all(l2s[n] == (RL.REGS[f] if f else 0.0) for n, f in fams.items())
    # the places a regulariser is most easily put by mistake
    zero = {"AFM": ["afm_layer/attention_b", "afm_layer/projection_h", "afm_layer/projection_p"],
            "DCNMix": ["dense/kernel", "dense_1/kernel", "dense_2/kernel", "cross_net_mix/bias0"],
            "DCN": ["cross_net/bias0", "dense/kernel"], "DCNMatrix": ["cross_net/bias1"],
            "DIN": ["dnn/kernel0", "dnn/kernel1", "local_activation_unit/kernel", "local_activation_unit/bias"],
            "FLEN": ["field_wise_bi_interaction/kernel_mf", "field_wise_bi_interaction/kernel_fm", "dense/kernel"],
            "MMOE": ["gate_softmax_ctr/kernel", "gate_softmax_ctcvr/kernel", "dense/kernel", "ctr/global_bias"],
            "PLE": ["level_0_gate_softmax_shared/kernel", "level_1_gate_softmax_specific_ctr/kernel"],
            "xDeepFM": ["cin/bias0", "dense_1/kernel"], "PNN": ["outter_product_layer/kernel"]}.get(kind, [])
    for n in zero + [n for n in names if "bias" in n]:
        assert l2s[n] == 0.0, n
    some = {"AFM": [("afm_layer/attention_W", "att")], "DCNMix": [("cross_net_mix/U_list0", "cross"), ("cross_net_mix/V_list1", "cross"),
                                                                   ("cross_net_mix/C_list0", "cross")],
            "DCNMatrix": [("cross_net/kernel1", "cross")], "DIN": [("dnn_1/kernel0", "dnn"), ("sparse_seq_emb_s/embeddings", "embedding")],
            "ESMM": [("dnn/kernel0", "dnn"), ("dnn_1/kernel1", "dnn")], "SharedBottom": [("tower_ctr/kernel0", "dnn"), ("dnn/kernel1", "dnn")],
            "PLE": [("level_1_expert_shared_0/kernel0", "dnn"), ("tower_ctcvr/kernel0", "dnn")],
            "MMOE": [("expert_2/kernel1", "dnn"), ("tower_ctr/kernel0", "dnn")], "xDeepFM": [("cin/filter1", "cin")],
            "DeepFM": [("linear0sparse_emb_z/embeddings", "linear"), ("linear/linear_kernel", "linear"), ("sparse_emb_c/embeddings", "embedding")],
            "FLEN": [("dnn/kernel0", "dnn"), ("linear0sparse_emb_e/embeddings", "linear")]}.get(kind, [])
    for n, f in some:
        assert l2s[n] == RL.REGS[f], n
    # the table SparseFeat c and the sequence s share exists once (inputs.py:19-41: one Embedding per embedding_name)
    if kind != "DIN":
        assert sum(n.endswith("emb_c/embeddings") and not n.startswith("linear") for n in names) == 1 and not any("emb_s/" in n for n in names)
    with pytest.raises(KeyError):
        RL.family(kind, "some_layer/some_new_weight")


@pytest.mark.parametrize("kind", RL.KINDS)
def test_regularized_weights_follow_the_rule(kind):
    """training.regularized_weights — the penalties of the autograd step, of evaluate() and of the check in front of the HIP fit — lists
    exactly the rule's weights with the rule's values, each storage once."""
    from deepctr_amd import training
    model, names = _names(kind)
    by_ptr = {t.data_ptr(): n for n, t in model.named_weights()}
    got = {}
    for t, l2 in training.regularized_weights(model):
        assert by_ptr[t.data_ptr()] not in got, "listed twice: %s" % by_ptr[t.data_ptr()]
        got[by_ptr[t.data_ptr()]] = l2
    want = {n: l for n, l in RL.l2_by_name(kind, names).items() if l}
    assert got == want, (sorted(set(got) ^ set(want)), {n: (got[n], want[n]) for n in set(got) & set(want) if got[n] != want[n]})


@pytest.mark.parametrize("kind", list(RL.FROZEN))
def test_a_frozen_table_is_out_of_the_rule(kind):
    model, names = _names(kind, frozen=True)
    e = RL.FROZEN[kind]
    l2s = RL.l2_by_name(kind, names, frozen=[e])
    frozen = [n for n in names if n.endswith("emb_%s/embeddings" % e)]
    assert len(frozen) == (2 if kind == "DeepFM" else 1) and all(l2s[n] == 0.0 for n in frozen)
    assert sum(1 for n in names if l2s[n] == RL.REGS["embedding"]) >= 2


@pytest.mark.parametrize("kind", ["DeepFM", "DCNMix", "AFM", "MMOE"])
@pytest.mark.parametrize("lr", [0.01, 0.1])
def test_closed_form_against_float64_autograd_sgd(kind, lr):
    """Three plain SGD steps on sum_weights l sum(w^2) alone, torch float64 autograd over copies of the model's weights: the weights
    equal decayed(), the rows-weighted mean of the steps' penalties equals epoch_loss(), both to float64 rounding; an unregularised
    weight does not move at all; and float32 SGD stays inside sgd_bar()."""
    model, names = _names(kind)
    rng = np.random.RandomState(5)
    w0 = RL.random_weights(model, rng)
    l2s = RL.l2_by_name(kind, names)
    p64 = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in w0.items()}
    p32 = {k: torch.tensor(v, dtype=torch.float32) for k, v in w0.items()}
    losses = []
    for _ in RL.BATCH_ROWS:
        pen = sum(l2s[k] * (p ** 2).sum() for k, p in p64.items())
        losses.append(float(pen.detach()))
        grads = torch.autograd.grad(pen, list(p64.values()), allow_unused=True)
        with torch.no_grad():
            for (k, p), g in zip(p64.items(), grads):
                if g is not None:
                    p -= lr * g
            for k, p in p32.items():                                        # float32, as the optimizer kernel evaluates it
                p -= np.float32(lr) * (np.float32(2.0 * l2s[k]) * p)
    t = len(RL.BATCH_ROWS)
    moved = 0
    for k in names:
        want = RL.decayed(w0[k], l2s[k], lr, t)
        got = p64[k].detach().numpy()
        if l2s[k] == 0.0:
            assert np.array_equal(got, w0[k].astype(np.float64)) and np.array_equal(p32[k].numpy(), w0[k]), k
            continue
        moved += 1
        assert np.all(np.abs(got - want) <= 8 * np.finfo(np.float64).eps * np.abs(want)), k
        assert np.all(np.abs(want - w0[k]) > 100 * np.spacing(np.abs(w0[k]))), "%s: the decay is meant to be far above float32's resolution" % k
        err = np.abs(p32[k].numpy().astype(np.float64) - want)
        assert np.all(err <= RL.sgd_bar(w0[k], l2s[k], lr, t)), (k, float((err / RL.sgd_bar(w0[k], l2s[k], lr, t)).max()))
    assert moved >= 3
    mean = sum(r * l for r, l in zip(RL.BATCH_ROWS, losses)) / sum(RL.BATCH_ROWS)
    assert abs(RL.epoch_loss(w0, l2s, lr, RL.BATCH_ROWS) - mean) <= 1e-13 * mean and mean > 0
    assert abs(RL.penalty(w0, l2s) - losses[0]) <= 1e-13 * losses[0]


def test_the_feed_touches_few_rows():
    rng = np.random.RandomState(0)
    for kind in ("DeepFM", "DIN", "FLEN", "MMOE"):
        feed = RL.make_feed(kind, rng)
        assert all(v.shape[0] == RL.N_ROWS and (v.dtype.kind == "f" or int(v.max()) < 8) for v in feed.values())
    assert sum(RL.BATCH_ROWS) == RL.N_ROWS and RL.BATCH_ROWS[-1] == RL.N_ROWS % RL.BATCH and len(RL.BATCH_ROWS) == 3
