"""FirstFitAgent.act / BestFitAgent.act (firstfit.py:21-38, bestfit.py:21-40)
restated over one f32 observation, with numpy's scalar introsort argsort from
the oracle (oracle_argsort_f32, pinned by the BestFit goldens).

TEST INFRASTRUCTURE ONLY: shared by tests/test_gpu_act_obs.py and the trace
model of tests/seq_cases.py. numpy and the oracle only."""
import numpy as np

from oracle import oracle as O


def _argsort(v):
    v = np.ascontiguousarray(v, dtype=np.float32)
    out = np.zeros(v.size, np.int64)
    O.lib().oracle_argsort_f32(O._p(v), v.size, O._p(out))
    return out


def literal_act(obs, P, V, policy):
    """firstfit.py:21-38 / bestfit.py:21-40 over one f32 observation."""
    obs = np.asarray(obs, dtype=np.float32)
    placement = obs[:V].astype(np.int64)  # convert_obs_to_dict's astype(int), utils.py:41
    vm_cpu, vm_mem = obs[V:2 * V], obs[2 * V:3 * V]
    cpu, mem = obs[3 * V:3 * V + P].copy(), obs[3 * V + P:].copy()
    action = placement.copy()
    one = np.float32(1)
    for v in range(V):
        if placement[v] != P:
            continue
        order = range(P) if policy == "firstfit" else np.flip(_argsort(cpu + mem))
        for p in order:
            if cpu[p] + vm_cpu[v] <= one and mem[p] + vm_mem[v] <= one:
                action[v] = p
                cpu[p] += vm_cpu[v]
                if policy == "bestfit":
                    mem[p] += vm_mem[v]
                break
    return action
