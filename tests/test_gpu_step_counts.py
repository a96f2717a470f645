"""The wave env kernels' event-derived VM counts against the C oracle.

The kernels take a step's existing / waiting VM counts and the "a NULL slot is
left" hint bit from the step's events and carry the waiting count through a
fused rollout ("Counts from events"). Every case of
tests/step_counts_cases.py (tests/test_step_counts_cpu.py shows that its walks
hold the steps that matter) runs with FirstFit and BestFit and the rewards wr,
ut and kl, and each is driven four ways from the oracle's two walks:

  bare     per-step heuristic launches, nothing but obs / reward / done
           returned (the benchmark's call), beside a twin handle stepped by
           fused one-step rollouts whose snapshot bytes must equal the
           handle's after every step (the header's hint word included)
  actions  the same with want_actions
  fused    fused rollouts of 1, 7 and 100 steps, repeated (the carried n_w)
  ext      external-action launches with the walk's random, mostly invalid
           actions, suspensions included

obs, reward and done are compared at every step, bit for bit (the reward
within tests.traj.kl_close under kl, as the other kl tests); counters, state
and the waiting ratio at the end. A trace-fed variant of two cases runs the
trace kernels through the bare, fused and ext drives."""
import functools

import numpy as np
import pytest
import torch

from tests import step_counts_cases as S
from tests import traj as T

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
STATE_KEYS = ("vm_placement", "vm_cpu", "vm_memory", "cpu", "memory", "vm_remaining_runtime")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")


def _handle(case, reward, traces=None):
    from vmp.batched import BatchedVmEnv
    from vmp.config import Config
    from vmp.trace import Trace
    b = BatchedVmEnv(Config(**case.cfg(reward)), S.N_ENV, seeds=np.asarray(S.SEEDS, dtype=np.int64),
                     device=DEV)
    if traces is not None:
        b.set_trace([Trace(*t) for t in traces], np.arange(S.N_ENV))
    return b


@functools.lru_cache(maxsize=None)
def _snapshot_mask(P, V):
    """True for every snapshot byte of the env state: all but the VM words of
    the padded slots v >= V, which no kernel writes (vmp_layout.h: blocks of 64
    slot words then 64 time words, the block count a power of two)."""
    N = S.N_ENV
    blocks = 1
    while blocks * 64 < V:
        blocks *= 2
    pitch = blocks * 128
    v = np.arange(V)
    slot = (v >> 6 << 7) | (v & 63)
    words = np.zeros(pitch, bool)
    words[slot] = words[slot + 64] = True
    keep = np.ones(256 + N * 256 + 16 * N * P + 4 * N * pitch, bool)
    keep[256 + N * 256 + 16 * N * P:] = np.tile(np.repeat(words, 4), N)
    return torch.from_numpy(keep).to(DEV)


def _rew(got, exp, kl, where):
    got = np.asarray(got)
    if not kl:
        assert np.array_equal(got, exp), ("reward",) + where + (got, exp)
    else:
        assert all(T.kl_close(g, e) for g, e in zip(got.ravel(), exp.ravel())), \
            ("reward",) + where + (got, exp)


def _step_outputs(w, t, obs, rew, done, where):
    assert np.array_equal(obs.cpu().numpy(), w.obs[t]), ("obs",) + where + (t,)
    assert np.array_equal(done.cpu().numpy(), w.done[t]), ("done",) + where + (t,)
    _rew(rew.cpu().numpy(), w.rew[t], w.reward == "kl", where + (t,))


def _end(w, b, where):
    st = {k: v.cpu().numpy() for k, v in b.state().items()}
    ctr, sts = b.counters().cpu().numpy(), b.stats().cpu().numpy()
    for i in range(S.N_ENV):
        assert np.array_equal(ctr[i], w.ctr[-1, i]), ("counters",) + where + (i, ctr[i], w.ctr[-1, i])
        for k, x in zip(STATE_KEYS, w.state[i]):
            assert st[k][i].dtype == x.dtype and np.array_equal(st[k][i], x), (k,) + where + (i,)
        # waiting_ratio, total_cpu_requested, total_memory_requested
        for j in (0, 3, 4):
            assert sts[i][j] == w.stats[i][j], ("stats", j) + where + (i, sts[i][j], w.stats[i][j])


def _drive_bare(w, traces=None):
    b, twin = _handle(w.case, w.reward, traces), _handle(w.case, w.reward, traces)
    try:
        keep = _snapshot_mask(w.case.P, w.case.V)
        assert keep.numel() == b.snapshot().numel()
        for t in range(w.case.steps):
            obs, rew, done, valid, act = b.heuristic_step(w.policy)
            assert valid is None and act is None
            _step_outputs(w, t, obs, rew, done, ("bare",))
            rs, _ = twin.rollout(w.policy, 1)
            _rew(rs.cpu().numpy()[0], w.rew[t], w.reward == "kl", ("twin", t))
            assert torch.equal(b.snapshot()[keep], twin.snapshot()[keep]), ("snapshot", t)
        _end(w, b, ("bare",))
        _end(w, twin, ("twin",))
    finally:
        b.close()
        twin.close()


def _drive_actions(w):
    b = _handle(w.case, w.reward)
    try:
        for t in range(w.case.steps):
            obs, rew, done, valid, act = b.heuristic_step(w.policy, want_actions=True)
            assert np.array_equal(act.cpu().numpy(), w.act[t]), ("actions", t)
            _step_outputs(w, t, obs, rew, done, ("actions",))
        _end(w, b, ("actions",))
    finally:
        b.close()


def _drive_fused(w, traces=None):
    b = _handle(w.case, w.reward, traces)
    try:
        t, j = 0, 0
        while t < w.case.steps:
            K = min(S.ROLLS[j % len(S.ROLLS)], w.case.steps - t)
            rs, dc = b.rollout(w.policy, K)
            _rew(rs.cpu().numpy(), w.rew[t:t + K], w.reward == "kl", ("fused", t, K))
            assert np.array_equal(dc.cpu().numpy(), w.done[t:t + K].sum(0)), ("done_count", t, K)
            t += K
            j += 1
        assert j >= 2 * len(S.ROLLS)
        assert np.array_equal(b.obs().cpu().numpy(), w.obs[-1]), ("obs", "fused")
        _end(w, b, ("fused",))
    finally:
        b.close()


def _drive_ext(w, traces=None):
    b = _handle(w.case, w.reward, traces)
    try:
        acts = torch.tensor(w.act, dtype=torch.int32, device=DEV)
        for t in range(w.case.steps):
            obs, rew, done, valid = b.step(acts[t])
            assert np.array_equal(valid.cpu().numpy(), w.valid[t]), ("valid", t)
            _step_outputs(w, t, obs, rew, done, ("ext",))
        _end(w, b, ("ext",))
    finally:
        b.close()


@pytest.mark.parametrize("reward", S.REWARDS)
@pytest.mark.parametrize("policy", S.POLICIES)
@pytest.mark.parametrize("case", S.CASES, ids=[c.name for c in S.CASES])
def test_counts_vs_oracle(case, policy, reward):
    wh = S.walk(case, policy, reward, "heur")
    _drive_bare(wh)
    _drive_actions(wh)
    _drive_fused(wh)
    _drive_ext(S.walk(case, policy, reward, "ext"))


@pytest.mark.parametrize("policy,reward", (("firstfit", "wr"), ("bestfit", "kl")))
@pytest.mark.parametrize("name", S.TRACE_CASES)
def test_counts_vs_oracle_trace(name, policy, reward):
    """The trace kernels: every env replays the requests its own oracle walk
    accepted (rejected proposals of the external walk included)."""
    case = S.BY_NAME[name]
    wh = S.walk(case, policy, reward, "heur", want_trace=True)
    _drive_bare(wh, wh.traces)
    _drive_fused(wh, wh.traces)
    we = S.walk(case, policy, reward, "ext", want_trace=True)
    _drive_ext(we, we.traces)
