"""PLE — same signature as ``deepctr.models.multitask.ple.PLE`` (reference ple.py:20-155): num_levels Customized Gate Control levels.
A level holds specific_expert_num experts per task and shared_expert_num shared ones; task i's gate mixes its own experts and the
shared ones (ple.py:91-92), and every level but the last has one more gate over all experts (ple.py:114) that feeds the next level's
shared experts.

Forward: gather -> dnn_in -> ONE ``ops.mtl_level`` launch per level -> ONE ``ops.mtl_towers`` launch."""
from ...layers.base import name_scope
from ...layers.core import Dense
from ._base import Level, MultiTaskModel, check_tasks


def PLE(dnn_feature_columns, shared_expert_num=1, specific_expert_num=1, num_levels=2, expert_dnn_hidden_units=(256,),
        tower_dnn_hidden_units=(64,), gate_dnn_hidden_units=(), l2_reg_embedding=0.00001, l2_reg_dnn=0, seed=1024, dnn_dropout=0,
        dnn_activation='relu', dnn_use_bn=False, task_types=('binary', 'binary'), task_names=('ctr', 'ctcvr'), device=None):
    """Instantiates the multi level of Customized Gate Control of Progressive Layered Extraction architecture on the MI355X forward
    path."""
    check_tasks(task_types, task_names)
    T, ns, nh = len(task_names), int(specific_expert_num), int(shared_expert_num)
    if not len(expert_dnn_hidden_units) or num_levels < 1 or ns + nh < 1 or ns < 0 or nh < 0:
        raise ValueError("PLE needs at least one level, one expert per gate and one expert layer")
    # (shared_expert_num = 0 builds, as in the reference: the shared gate of a non-last level then mixes the specific experts only)
    m =MultiTaskModel("PLE", dnn_feature_columns, device, task_types, task_names)
    m._dnn_cfg = dict(activation=dnn_activation, l2=l2_reg_dnn, dropout=dnn_dropout, bn=dnn_use_bn, seed=seed)
    with name_scope():
        in_dim0 = m._build_inputs(dnn_feature_columns, seed)
        in_dim = in_dim0
        dz_of = lambda width: gate_dnn_hidden_units[-1] if len(gate_dnn_hidden_units) else width       # noqa: E731
        for lvl in range(num_levels):
            last, first = lvl == num_levels - 1, lvl == 0
            prefix = 'level_' + str(lvl) + '_'
            shared_slot = 0 if first else T             # level 0: every input is the DNN input (ple.py:136)
            experts, esrc = [], []
            for i in range(T):
                for j in range(ns):
                    experts.append(m._dnn(expert_dnn_hidden_units, in_dim, prefix + 'task_' + task_names[i] + '_expert_specific_' + str(j)))
                    esrc.append(0 if first else i)
            for k in range(nh):
                experts.append(m._dnn(expert_dnn_hidden_units, in_dim, prefix + 'expert_shared_' + str(k)))
                esrc.append(shared_slot)
            shared = list(range(T * ns, T * ns + nh))
            gate_dnns, gate_dense, gsrc, members = [], [], [], []
            for i in range(T):
                gate_dnns.append(m._dnn(gate_dnn_hidden_units, in_dim, prefix + 'gate_specific_' + task_names[i]))
                gate_dense.append(m._add(Dense(ns + nh, use_bias=False, name=prefix + 'gate_softmax_specific_' + task_names[i],
                                               device=m.device).build_for(dz_of(in_dim))))
                gsrc.append(0 if first else i)
                members.append(list(range(i * ns, (i + 1) * ns)) + shared)
            if not last:
                gate_dnns.append(m._dnn(gate_dnn_hidden_units, in_dim, prefix + 'gate_shared'))
                gate_dense.append(m._add(Dense(T * ns + nh, use_bias=False, name=prefix + 'gate_softmax_shared',
                                               device=m.device).build_for(dz_of(in_dim))))
                gsrc.append(shared_slot)
                members.append(list(range(T * ns + nh)))
            m.levels.append(Level(experts, esrc, gate_dnns, gate_dense, gsrc, members, 1 if first else T + 1))
            in_dim = expert_dnn_hidden_units[-1]
        m._build_towers(tower_dnn_hidden_units, in_dim, names=["tower_" + n for n in task_names])
    m.regularizers = {"embedding": float(l2_reg_embedding), "linear": 0.0, "dnn": float(l2_reg_dnn)}
    return m
