"""vmp.agents.RolloutAgent on the GPU. On a trace its choices equal a brute
force that needs no branch: per step and candidate a twin handle is restored
from the env's snapshot, steps the candidate's action, runs K FirstFit steps
and adds the rewards in step order. On an RNG workload two agents with one
seed choose alike, and the futures are common random numbers."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
P, V, N, K, STEPS = 10, 30, 3, 5, 10
CANDS = ("firstfit", "bestfit", "wait")
CFG = dict(allow_null_action=True, training_steps=10000, eval_steps=100000, seed=0, sequence="uniform",
           cap_target_util=True, beta=0.3, service_length=8, pms=P, vms=V, arrival_rate=V / 4.0,
           reward_function="wr")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")


def _env(n=N, **over):
    from vmp.batched import BatchedVmEnv
    from vmp.config import Config
    return BatchedVmEnv(Config(**dict(CFG, **over)), n, seeds=np.arange(n, dtype=np.int64) * 4, device=DEV)


def _trace():
    """24 steps by hand: bursts of large VMs between quiet steps, so that ten
    PMs fill, VMs wait, and where a VM goes decides what fits later."""
    from vmp.trace import Trace
    arrivals = [6, 0, 5, 1, 0, 7, 2, 0, 4, 3, 0, 6, 1, 2, 0, 5, 0, 3, 4, 0, 2, 6, 0, 1]
    n = sum(arrivals)
    k = np.arange(n)
    cpu = 15 + (k * 37) % 60   # 15 .. 74 hundredths
    mem = 20 + (k * 53) % 55   # 20 .. 74
    runtime = 2 + (k * 7) % 9  # 2 .. 10 steps
    offs = np.concatenate([[0], np.cumsum(arrivals)])
    return Trace(offs, cpu, mem, runtime)


def _candidate_actions(b):
    wait = b.state()["vm_placement"].to(torch.int32)
    return [b.heuristic_act("firstfit"), b.heuristic_act("bestfit"), wait]


def test_choices_equal_the_snapshot_restore_brute_force():
    from vmp.agents import RolloutAgent
    tr = _trace()
    env, twin = _env(), _env()
    env.set_trace(tr)
    twin.set_trace(tr)
    # three different histories on the one trace: a FirstFit, a BestFit and a waiting env
    for _ in range(3):
        a = _candidate_actions(env)
        env.step(torch.stack([a[0][0], a[1][1], a[2][2]]))
    agent = RolloutAgent(env, candidates=CANDS, horizon=K, futures=4, base="firstfit")
    assert agent.M == 1 and agent.scratch.n_envs == N * 3  # a trace has one future
    chosen = []
    for t in range(STEPS):
        snap = env.snapshot()
        acts = _candidate_actions(env)
        ret = np.zeros((N, 3))
        for c, a in enumerate(acts):
            twin.restore(snap)
            _, total, _, _ = twin.step(a)
            rew, _ = twin.rollout("firstfit", K)
            total = total.cpu().numpy().copy()
            for k in range(K):
                total = total + rew[k].cpu().numpy()
            ret[:, c] = total
        want = [int(np.flatnonzero(r == r.max())[0]) for r in ret]
        got_ret = agent.returns(torch.stack(acts, dim=1)).cpu().numpy()
        assert np.array_equal(got_ret, ret), (t, got_ret, ret)
        before = env.counters()
        obs, reward, done, valid, choice = agent.step()
        assert choice.tolist() == want, (t, choice.tolist(), want, ret)
        # the env made exactly one step, with the chosen candidate's action
        twin.restore(snap)
        o2, r2, _, _ = twin.step(torch.stack([acts[c][i] for i, c in enumerate(want)]))
        assert torch.equal(obs, o2) and torch.equal(reward, r2), t
        assert torch.equal(env.counters()[:, 5], before[:, 5] + 1)
        chosen += want
    print("choices:", chosen)
    assert len(set(chosen)) >= 2, chosen  # the rollouts decided something
    assert agent.t == STEPS
    agent.close()
    env.close()
    twin.close()


def test_rng_futures_are_reproducible_and_paired():
    from vmp.agents import RolloutAgent
    M = 4
    envs = [_env(), _env()]
    agents = [RolloutAgent(e, candidates=CANDS, horizon=K, futures=M, seed=123) for e in envs]
    for e in envs:
        for _ in range(5):
            e.heuristic_step("bestfit")
    for t in range(STEPS):
        out = [a.step() for a in agents]
        assert torch.equal(out[0][4], out[1][4]), t
        assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]), t
        # futures differ from each other and are the same for every candidate
        tot = agents[0].scratch.counters()[:, 0].view(N, 3, M).cpu().numpy()
        assert np.all(tot == tot[:, :1, :]), t
        assert np.any(tot != tot[:, :, :1]), t
    assert torch.equal(envs[0].counters(), envs[1].counters())
    for k, v in envs[0].state().items():
        assert torch.equal(v, envs[1].state()[k]), k
    s0 = agents[0].future_seeds().cpu().numpy()
    assert s0.min() >= 0 and len(set(s0.tolist())) == N * M
    for a in agents:
        a.close()
    for e in envs:
        e.close()
