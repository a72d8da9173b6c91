"""ESMM — same signature as ``deepctr.models.multitask.esmm.ESMM`` (reference esmm.py:19-66): a ctr and a cvr tower over the DNN
input; outputs ctr = sigmoid(l_ctr) and ctcvr = ctr * sigmoid(l_cvr).

Forward: gather -> dnn_in -> ONE ``ops.mtl_towers`` launch with the ESMM head."""
from ...layers.base import name_scope
from ._base import MultiTaskModel


def ESMM(dnn_feature_columns, tower_dnn_hidden_units=(256, 128, 64), l2_reg_embedding=0.00001, l2_reg_dnn=0, seed=1024, dnn_dropout=0,
         dnn_activation='relu', dnn_use_bn=False, task_types=('binary', 'binary'), task_names=('ctr', 'ctcvr'), device=None):
    """Instantiates the Entire Space Multi-Task Model architecture on the MI355X forward path."""
    if len(task_names) != 2:
        raise ValueError("the length of task_names must be equal to 2")
    for task_type in task_types:
        if task_type != 'binary':
            raise ValueError("task must be binary in ESMM, {} is illegal".format(task_type))
    m = MultiTaskModel("ESMM", dnn_feature_columns, device, ['binary', 'binary'], task_names)
    m._dnn_cfg = dict(activation=dnn_activation, l2=l2_reg_dnn, dropout=dnn_dropout, bn=dnn_use_bn, seed=seed)
    m.esmm = True
    with name_scope():
        in_dim = m._build_inputs(dnn_feature_columns, seed)
        # (the cvr PredictionLayer is auto-named; the ctcvr output is a weightless Multiply named task_names[1])
        m._build_towers(tower_dnn_hidden_units, in_dim, prediction_names=[task_names[0], None])
    m.regularizers = {"embedding": float(l2_reg_embedding), "linear": 0.0, "dnn": float(l2_reg_dnn)}
    return m
