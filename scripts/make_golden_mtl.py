"""Generates the multi-task fixtures tests/golden/model_{mmoe,ple,sb,esmm}_*.npz, mtl_layer.npz and model_mmoe_census.npz by running
the reference's own SharedBottom, ESMM, MMOE and PLE (deepctr/models/multitask/) on the oracle's TensorFlow shim, with the oracle's
deterministic weights (oracle/make_golden.py).  CPU only; needs the reference checkout, so it is not part of the suite:

    python scripts/make_golden_mtl.py [--out DIR]

Run it into a scratch directory and compare with the committed files to check that the recipe has not rotted (a second run gives the
same bytes).

ESMM needs one symbol the shim does not restate, ``tf.keras.layers.Multiply``.  Installed here, after the shim, RESTATED FROM THE KERAS
DOCUMENTATION and not taken from its code (the precedent of ``Add`` in scripts/make_golden_edcn.py): the elementwise
product of a list of inputs of one shape.

Every file holds ``y`` stacked [T, B, 1] (the reference's list of outputs in task_names order), the feeds, the weights and the meta
(constructor, spec, kwargs).  Model fixtures, all on oracle.make_golden.mixed_spec(4) with B = 32 and RandomState(61), feeds drawn in the
order plain / hashed:

    mmoe_base      3 experts (16, 8), tower (8,), no gate DNN, ('binary', 'regression')
    mmoe_gate      4 experts (16, 8), empty tower, gate DNN (6,), three binary tasks
    mmoe_bn        BatchNormalization in every DNN (experts, gate DNN (6,), towers)
    mmoe_hash      the hashed spec
    mmoe_nodense   the spec without its DenseFeats
    ple_22         shared 2, specific 2, 2 levels, gate DNN (5,)
    ple_11         shared 1, specific 1, 1 level
    ple_01         shared 0, specific 1, 2 levels: every task gate has one member
    ple_3x3        3 levels, 3 tasks, ('binary', 'regression', 'binary')
    sb_base        bottom (16, 8), tower (8,)
    sb_nobottom    empty bottom
    sb_regbin      ('regression', 'binary')
    esmm_base      tower (16, 8)
    esmm_notower   empty tower

mtl_layer.npz: the reference's MMOE (3 experts (16, 8), gate DNN (6,)) and a two-level PLE (specific 2, shared 2, experts (16,)) over
ONE DenseFeat of 12 standard-normal columns, so the DNN input is the feed itself; the gate kernels are drawn N(0, 1) (the oracle's hook
draws Glorot-sized ones: softmaxes too close to uniform to be seen).  The outputs of the reference's ``gate_mul_expert_*`` Lambda layers
are recorded while its constructor runs: ``mmoe/out`` [B, T, H]; ``ple/out0`` [B, T + 1, H], the non-last level, and ``ple/out1``
[B, T, H], the last level, whose inputs are out0's slots.

model_mmoe_census.npz: examples/run_mtl.py's own preprocessing and model (tower_dnn_hidden_units=[], embedding 4) on
examples/census-income.sample, which is copied to tests/golden/ (200 rows); the file also holds the two label columns.

Rows whose max-pooled sequence is all padding are excluded by the tests (tests.test_autoint_cpu.att_rows).  Rows kept and the range of
the compared probabilities (binary outputs), as the tests assert them (>= half the rows, (1e-3, 1 - 1e-3)), as printed by this script:

    model_mmoe_base            19/32  0.506 .. 0.535
    model_mmoe_gate            19/32  0.454 .. 0.629
    model_mmoe_bn              19/32  0.434 .. 0.547
    model_mmoe_hash            20/32  0.445 .. 0.525
    model_mmoe_nodense         19/32  0.470 .. 0.529
    model_ple_22               19/32  0.480 .. 0.536
    model_ple_11               19/32  0.433 .. 0.518
    model_ple_01               19/32  0.402 .. 0.563
    model_ple_3x3              19/32  0.514 .. 0.534
    model_sb_base              19/32  0.423 .. 0.524
    model_sb_nobottom          19/32  0.313 .. 0.540
    model_sb_regbin            19/32  0.423 .. 0.488
    model_esmm_base            19/32  0.155 .. 0.530
    model_esmm_notower         19/32  0.133 .. 0.790
    model_mmoe_census          200/200  0.408 .. 0.537
"""
import json
import os
import shutil
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import make_golden as G  # noqa: E402
from oracle import tf_shim as S  # noqa: E402

SEED = 61
CENSUS_COLUMNS = ['age', 'class_worker', 'det_ind_code', 'det_occ_code', 'education', 'wage_per_hour', 'hs_college', 'marital_stat',
                  'major_ind_code', 'major_occ_code', 'race', 'hisp_origin', 'sex', 'union_member', 'unemp_reason', 'full_or_part_emp',
                  'capital_gains', 'capital_losses', 'stock_dividends', 'tax_filer_stat', 'region_prev_res', 'state_prev_res',
                  'det_hh_fam_stat', 'det_hh_summ', 'instance_weight', 'mig_chg_msa', 'mig_chg_reg', 'mig_move_reg', 'mig_same',
                  'mig_prev_sunbelt', 'num_emp', 'fam_under_18', 'country_father', 'country_mother', 'country_self', 'citizenship',
                  'own_or_self', 'vet_question', 'vet_benefits', 'weeks_worked', 'year', 'income_50k']
CENSUS_SPARSE = ['class_worker', 'det_ind_code', 'det_occ_code', 'education', 'hs_college', 'major_ind_code', 'major_occ_code', 'race',
                 'hisp_origin', 'sex', 'union_member', 'unemp_reason', 'full_or_part_emp', 'tax_filer_stat', 'region_prev_res',
                 'state_prev_res', 'det_hh_fam_stat', 'det_hh_summ', 'mig_chg_msa', 'mig_chg_reg', 'mig_move_reg', 'mig_same',
                 'mig_prev_sunbelt', 'fam_under_18', 'country_father', 'country_mother', 'country_self', 'citizenship', 'vet_question']


def install_restated_symbols():
    class Multiply(S.Layer):
        def call(self, inputs):
            out = np.asarray(S._arr(inputs[0]))
            for v in inputs[1:]:
                out = out * np.asarray(S._arr(v))
            return S.Tensor(out)

    sys.modules["tensorflow.keras.layers"].Multiply = Multiply


def run_model(name, ctor_name, spec, feed, kwargs, extra=None):
    S.reset()
    S.set_feed(feed)
    mod = __import__("deepctr.models.multitask", fromlist=[ctor_name])
    model = getattr(mod, ctor_name)(G.build_ref_columns(spec), **kwargs)
    y = np.stack([np.asarray(S._arr(o), dtype=np.float32).reshape(-1, 1) for o in model.outputs])
    arrays = {"y": y}
    for k, v in feed.items():
        arrays["feed/" + k] = v
    for k, v in G._weights_dict().items():
        arrays["w/" + k] = v
    arrays.update(extra or {})
    meta = {"model": ctor_name, "linear": [], "dnn": spec, "kwargs": kwargs, "extra_args": []}
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    G._save(name, **arrays)


def report(name):
    """Rows kept and probability range of a written fixture, by the rule the tests apply."""
    g = dict(np.load(os.path.join(G.OUT, name + ".npz")))
    meta = json.loads(bytes(g["meta"]).decode())
    n = g["y"].shape[1]
    keep = np.ones(n, dtype=bool)
    for d in meta["dnn"]:
        if d["type"] == "varlen" and d["combiner"] == "max":
            ids = g["feed/" + d["sparsefeat"]["name"]]
            if d.get("length_name"):
                keep &= g["feed/" + d["length_name"]].reshape(-1) > 0
            else:
                keep &= (ids != 0).any(axis=1)
    types = meta["kwargs"].get("task_types", ["binary", "binary"])
    y = np.concatenate([g["y"][t].reshape(-1)[keep] for t, tt in enumerate(types) if tt == "binary"])
    print("    %-26s %d/%d  %.3f .. %.3f" % (name, keep.sum(), keep.size, y.min(), y.max()))


def gen_models():
    rng = np.random.RandomState(SEED)
    B = 32
    spec = G.mixed_spec(4, False)
    feed = G._feed_for(spec, B, rng)
    spec_h = G.mixed_spec(4, True)
    feed_h = G._feed_for(spec_h, B, rng)
    spec_n = [d for d in json.loads(json.dumps(spec)) if d["type"] != "dense"]
    feed_n = {k: v for k, v in feed.items() if not k.startswith("dense_")}
    names = []

    def run(suffix, ctor, sp, fd, **kw):
        run_model("model_" + suffix, ctor, sp, fd, kw)
        names.append("model_" + suffix)

    mm = dict(num_experts=3, expert_dnn_hidden_units=[16, 8], tower_dnn_hidden_units=[8], gate_dnn_hidden_units=[])
    run("mmoe_base", "MMOE", spec, feed, task_types=["binary", "regression"], task_names=["ctr", "ctcvr"], **mm)
    run("mmoe_gate", "MMOE", spec, feed, num_experts=4, expert_dnn_hidden_units=[16, 8], tower_dnn_hidden_units=[], gate_dnn_hidden_units=[6],
        task_types=["binary", "binary", "binary"], task_names=["ctr", "ctcvr", "like"])
    run("mmoe_bn", "MMOE", spec, feed, dnn_use_bn=True, num_experts=3, expert_dnn_hidden_units=[16, 8], tower_dnn_hidden_units=[8],
        gate_dnn_hidden_units=[6], task_types=["binary", "binary"], task_names=["ctr", "ctcvr"])
    run("mmoe_hash", "MMOE", spec_h, feed_h, task_types=["binary", "binary"], task_names=["ctr", "ctcvr"], **mm)
    run("mmoe_nodense", "MMOE", spec_n, feed_n, task_types=["binary", "binary"], task_names=["ctr", "ctcvr"], **mm)
    pl = dict(expert_dnn_hidden_units=[16], tower_dnn_hidden_units=[8], task_types=["binary", "binary"], task_names=["ctr", "ctcvr"])
    run("ple_22", "PLE", spec, feed, shared_expert_num=2, specific_expert_num=2, num_levels=2, gate_dnn_hidden_units=[5], **pl)
    run("ple_11", "PLE", spec, feed, shared_expert_num=1, specific_expert_num=1, num_levels=1, gate_dnn_hidden_units=[], **pl)
    run("ple_01", "PLE", spec, feed, shared_expert_num=0, specific_expert_num=1, num_levels=2, gate_dnn_hidden_units=[], **pl)
    run("ple_3x3", "PLE", spec, feed, shared_expert_num=1, specific_expert_num=2, num_levels=3, gate_dnn_hidden_units=[],
        expert_dnn_hidden_units=[16], tower_dnn_hidden_units=[8], task_types=["binary", "regression", "binary"],
        task_names=["ctr", "ctcvr", "like"])
    sb = dict(bottom_dnn_hidden_units=[16, 8], tower_dnn_hidden_units=[8])
    run("sb_base", "SharedBottom", spec, feed, task_types=["binary", "binary"], task_names=["ctr", "ctcvr"], **sb)
    run("sb_nobottom", "SharedBottom", spec, feed, bottom_dnn_hidden_units=[], tower_dnn_hidden_units=[8], task_types=["binary", "binary"],
        task_names=["ctr", "ctcvr"])
    run("sb_regbin", "SharedBottom", spec, feed, task_types=["regression", "binary"], task_names=["ctr", "ctcvr"], **sb)
    run("esmm_base", "ESMM", spec, feed, tower_dnn_hidden_units=[16, 8], task_types=["binary", "binary"], task_names=["ctr", "ctcvr"])
    run("esmm_notower", "ESMM", spec, feed, tower_dnn_hidden_units=[], task_types=["binary", "binary"], task_names=["ctr", "ctcvr"])
    return names


def gen_layers():
    from deepctr.models.multitask import MMOE, PLE
    rng = np.random.RandomState(SEED + 1)
    hook, lam_call = S.WEIGHT_HOOK, S.Lambda.call
    recorded = {}

    def normal_gates(layer, wname, default):
        if "gate_softmax" in layer.name:
            return rng.standard_normal(default.shape)
        return hook(layer, wname, default)

    def recording_call(self, inputs, **kw):
        out = lam_call(self, inputs, **kw)
        if "gate_mul_expert" in self.name:
            recorded[self.name] = np.asarray(S._arr(out), dtype=np.float32)
        return out

    spec = [dict(type="dense", name="x", dimension=12)]
    names = ["ctr", "ctcvr"]
    arrays = {}
    S.WEIGHT_HOOK, S.Lambda.call = normal_gates, recording_call
    try:
        for tag, ctor, kw in (("mmoe", MMOE, dict(num_experts=3, expert_dnn_hidden_units=[16, 8], gate_dnn_hidden_units=[6])),
                              ("ple", PLE, dict(shared_expert_num=2, specific_expert_num=2, num_levels=2, expert_dnn_hidden_units=[16],
                                                gate_dnn_hidden_units=[]))):
            S.reset()
            recorded.clear()
            x = rng.standard_normal((9, 12)).astype(np.float32)
            S.set_feed({"x": x})
            ctor(G.build_ref_columns(spec), tower_dnn_hidden_units=[], task_names=names, **kw)
            arrays[tag + "/x"] = x
            arrays[tag + "/kwargs"] = np.frombuffer(json.dumps(kw).encode(), dtype=np.uint8)
            for k, v in G._weights_dict().items():
                arrays["%s/w/%s" % (tag, k)] = v
            if tag == "mmoe":
                arrays["mmoe/out"] = np.stack([recorded["gate_mul_expert_" + n] for n in names], axis=1)
            else:
                for lvl in (0, 1):
                    outs = [recorded["level_%d_gate_mul_expert_specific_%s" % (lvl, n)] for n in names]
                    if lvl == 0:
                        outs.append(recorded["level_0_gate_mul_expert_shared"])
                    arrays["ple/out%d" % lvl] = np.stack(outs, axis=1)
    finally:
        S.WEIGHT_HOOK, S.Lambda.call = hook, lam_call
    G._save("mtl_layer", **arrays)


def census_frame(path):
    """examples/run_mtl.py:10-40, its own preprocessing."""
    import pandas as pd
    from sklearn.preprocessing import LabelEncoder, MinMaxScaler
    data = pd.read_csv(path, header=None, names=CENSUS_COLUMNS)
    data['label_income'] = data['income_50k'].map({' - 50000.': 0, ' 50000+.': 1})
    data['label_marital'] = data['marital_stat'].apply(lambda x: 1 if x == ' Never married' else 0)
    data.drop(labels=['income_50k', 'marital_stat'], axis=1, inplace=True)
    dense = [c for c in data.columns.values.tolist() if c not in CENSUS_SPARSE and c not in ['label_income', 'label_marital']]
    data[CENSUS_SPARSE] = data[CENSUS_SPARSE].fillna('-1', )
    data[dense] = data[dense].fillna(0, )
    data[dense] = MinMaxScaler(feature_range=(0, 1)).fit_transform(data[dense])
    for feat in CENSUS_SPARSE:
        data[feat] = LabelEncoder().fit_transform(data[feat])
    return data, dense


def gen_census():
    src = os.path.join(G.REF, "examples", "census-income.sample")
    os.makedirs(G.OUT, exist_ok=True)
    shutil.copyfile(src, os.path.join(G.OUT, "census-income.sample"))
    data, dense = census_frame(src)
    spec = [dict(type="sparse", name=f, vocabulary_size=int(data[f].max()) + 1, embedding_dim=4) for f in CENSUS_SPARSE]
    spec += [dict(type="dense", name=f, dimension=1) for f in dense]
    feed = {f: data[f].values.astype(np.int32) for f in CENSUS_SPARSE}
    feed.update({f: data[f].values.astype(np.float32) for f in dense})
    labels = {"label/label_income": data['label_income'].values.astype(np.float32),
              "label/label_marital": data['label_marital'].values.astype(np.float32)}
    run_model("model_mmoe_census", "MMOE", spec, feed, dict(tower_dnn_hidden_units=[], task_types=['binary', 'binary'],
                                                             task_names=['label_income', 'label_marital']), extra=labels)
    return "model_mmoe_census"


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if "--out" in argv:
        i = argv.index("--out")
        G.OUT = os.path.abspath(argv[i + 1])
        del argv[i:i + 2]
    S.install(G.REF)
    S.WEIGHT_HOOK = G.weight_hook
    install_restated_symbols()
    names = gen_models()
    gen_layers()
    names.append(gen_census())
    for name in names:
        report(name)


if __name__ == "__main__":
    sys.exit(main())
