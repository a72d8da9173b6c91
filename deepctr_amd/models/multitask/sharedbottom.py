"""SharedBottom — same signature as ``deepctr.models.multitask.sharedbottom.SharedBottom`` (reference sharedbottom.py:19-68): one DNN
over the DNN input shared by every task, then per task a tower DNN, Dense(1, use_bias=False) and a PredictionLayer.

Forward: gather -> dnn_in -> ``ops.mlp`` for the bottom -> ONE ``ops.mtl_towers`` launch for all towers."""
from ...layers.base import name_scope
from ._base import MultiTaskModel, check_tasks


def SharedBottom(dnn_feature_columns, bottom_dnn_hidden_units=(256, 128), tower_dnn_hidden_units=(64,), l2_reg_embedding=0.00001,
                 l2_reg_dnn=0, seed=1024, dnn_dropout=0, dnn_activation='relu', dnn_use_bn=False, task_types=('binary', 'binary'),
                 task_names=('ctr', 'ctcvr'), device=None):
    """Instantiates the SharedBottom multi-task learning Network architecture on the MI355X forward path."""
    check_tasks(task_types, task_names)
    m = MultiTaskModel("SharedBottom", dnn_feature_columns, device, task_types, task_names)
    m._dnn_cfg = dict(activation=dnn_activation, l2=l2_reg_dnn, dropout=dnn_dropout, bn=dnn_use_bn, seed=seed)
    with name_scope():
        in_dim = m._build_inputs(dnn_feature_columns, seed)
        m.bottom = m._dnn(bottom_dnn_hidden_units, in_dim)
        width = bottom_dnn_hidden_units[-1] if len(bottom_dnn_hidden_units) else in_dim
        m._build_towers(tower_dnn_hidden_units, width, names=["tower_" + n for n in task_names])
    m.regularizers = {"embedding": float(l2_reg_embedding), "linear": 0.0, "dnn": float(l2_reg_dnn)}
    return m
