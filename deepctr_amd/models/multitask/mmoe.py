"""MMOE — same signature as ``deepctr.models.multitask.mmoe.MMOE`` (reference mmoe.py:20-97): num_experts expert DNNs over the DNN
input, per task a softmax gate (an optional gate DNN, then Dense(num_experts, use_bias=False)) that mixes the experts' outputs, then
the task's tower.

Forward: gather -> dnn_in -> ONE ``ops.mtl_level`` launch (experts, gates, mixtures) -> ONE ``ops.mtl_towers`` launch
(DESIGN.md §4.15)."""
from ...layers.base import name_scope
from ...layers.core import Dense
from ._base import Level, MultiTaskModel, check_tasks


def MMOE(dnn_feature_columns, num_experts=3, expert_dnn_hidden_units=(256, 128), tower_dnn_hidden_units=(64,), gate_dnn_hidden_units=(),
         l2_reg_embedding=0.00001, l2_reg_dnn=0, seed=1024, dnn_dropout=0, dnn_activation='relu', dnn_use_bn=False,
         task_types=('binary', 'binary'), task_names=('ctr', 'ctcvr'), device=None):
    """Instantiates the Multi-gate Mixture-of-Experts multi-task learning architecture on the MI355X forward path."""
    num_tasks = len(task_names)
    if num_tasks <= 1:
        raise ValueError("num_tasks must be greater than 1")
    if num_experts <= 1:
        raise ValueError("num_experts must be greater than 1")
    check_tasks(task_types, task_names)
    if not len(expert_dnn_hidden_units):
        raise ValueError("expert_dnn_hidden_units must hold at least one layer")
    m = MultiTaskModel("MMOE", dnn_feature_columns, device, task_types, task_names)
    m._dnn_cfg = dict(activation=dnn_activation, l2=l2_reg_dnn, dropout=dnn_dropout, bn=dnn_use_bn, seed=seed)
    with name_scope():
        in_dim = m._build_inputs(dnn_feature_columns, seed)
        experts = [m._dnn(expert_dnn_hidden_units, in_dim, 'expert_' + str(i)) for i in range(num_experts)]
        dz = gate_dnn_hidden_units[-1] if len(gate_dnn_hidden_units) else in_dim
        gate_dnns, gate_dense = [], []
        for name in task_names:
            gate_dnns.append(m._dnn(gate_dnn_hidden_units, in_dim, 'gate_' + name))
            gate_dense.append(m._add(Dense(num_experts, use_bias=False, name='gate_softmax_' + name, device=m.device).build_for(dz)))
        m.levels = [Level(experts, [0] * num_experts, gate_dnns, gate_dense, [0] * num_tasks,
                          [list(range(num_experts)) for _ in task_names], 1)]
        m._build_towers(tower_dnn_hidden_units, expert_dnn_hidden_units[-1], names=["tower_" + n for n in task_names])
    m.regularizers = {"embedding": float(l2_reg_embedding), "linear": 0.0, "dnn": float(l2_reg_dnn)}
    return m
