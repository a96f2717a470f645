"""Every env step kernel instantiation against the C oracle at the slot borders.

One test per case of tests/env_cases.py (its docstring has the plan; the CPU
half, tests/test_env_cases_cpu.py, shows that the cases select all 45 wave and
24 block instantiations and go where the kernels can go wrong). A test builds
ONE handle and walks it through every launch kind in turn, so that the step
hints one launch kind leaves in the header are read by the next; every value
a launch returns is compared with the oracle's record of the same plan
(env_cases.run_oracle, which never sees a device value): obs, valid, done,
actions, mask bits, state and counters bit for bit, the reward bit for bit
under wr / ut and within tests.traj.kl_close under kl (device log / exp
against glibc, the bound of the kl cases of tests/test_gpu_env.py).

External actions, trace source: derive_trace takes the validity flags, so the
trace handle is fed the very actions of the oracle run its traces were derived
from, rejected proposals included (the first form the plan allows)."""
import numpy as np
import pytest
import torch

from tests import env_cases as C
from tests import traj as T

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
STATE_KEYS = ("vm_placement", "vm_cpu", "vm_memory", "cpu", "memory", "vm_remaining_runtime")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")


def _handle(case, ref, monkeypatch):
    from vmp.batched import BatchedVmEnv
    from vmp.config import Config
    from vmp.trace import Trace
    seeds = np.asarray(case.seeds, dtype=np.int64)
    kw = {}
    if case.source == "workload":
        kw = dict(arrival_rate=np.array([w[0] for w in case.wl]),
                  service_length=np.array([w[1] for w in case.wl]))
    if case.big:
        monkeypatch.setenv("VMP_BIG_KERNEL", "1")
    try:
        b = BatchedVmEnv(Config(**case.cfg()), C.N_ENV, seeds=seeds, device=DEV, **kw)
    finally:
        if case.big:
            monkeypatch.delenv("VMP_BIG_KERNEL")
    if case.source == "trace":
        # the config's own workload is never drawn from on a traced env
        b.set_trace([Trace(*t) for t in ref.traces], np.arange(C.N_ENV))
    return b


def _unpack(bits, A):
    """int32 [N, V, W] -> bool [N, V, A] (bit a of word a // 32 set = invalid)."""
    w = bits.cpu().numpy().view(np.uint32)
    a = np.arange(A)
    return ((w[:, :, a // 32] >> (a % 32).astype(np.uint32)) & 1).astype(bool)


def _rew(got, exp, kl, where):
    got = got.cpu().numpy()
    if not kl:
        assert np.array_equal(got, exp), ("reward",) + where + (got, exp)
    else:
        assert all(T.kl_close(g, e) for g, e in zip(got.ravel(), exp.ravel())), \
            ("reward",) + where + (got, exp)


def _walk(case, ref, b):
    kl = case.reward == "kl"
    t = 0
    # 1: per-step heuristic, everything requested
    for _ in range(case.n_full):
        obs, rew, done, valid, act = b.heuristic_step(case.policy, want_actions=True, want_valid=True)
        assert np.array_equal(act.cpu().numpy(), ref.act[t]), ("actions", 1, t)
        assert np.array_equal(valid.cpu().numpy(), ref.valid[t]), ("valid", 1, t)
        assert np.array_equal(obs.cpu().numpy(), ref.obs[t]), ("obs", 1, t)
        assert np.array_equal(done.cpu().numpy(), ref.done[t]), ("done", 1, t)
        _rew(rew, ref.rew[t], kl, (1, t))
        t += 1
    # 2: external actions, the post-step mask in the same launch
    for k in range(case.n_ext):
        a = torch.tensor(ref.act[t], dtype=torch.int32, device=DEV)
        mo = torch.full((C.N_ENV, case.V, b.W), -1, dtype=torch.int32, device=DEV)
        obs, rew, done, valid = b.step(a, mask_out=mo)
        assert np.array_equal(valid.cpu().numpy(), ref.valid[t]), ("valid", 2, t)
        assert np.array_equal(obs.cpu().numpy(), ref.obs[t]), ("obs", 2, t)
        assert np.array_equal(done.cpu().numpy(), ref.done[t]), ("done", 2, t)
        _rew(rew, ref.rew[t], kl, (2, t))
        assert np.array_equal(_unpack(mo, case.A), ref.ext_mask[k]), ("mask_out", 2, t)
        t += 1
    # 3: the readers and the act-only launch, no step
    assert np.array_equal(b.mask().cpu().numpy(), ref.mid["mask"]), ("mask", 3)
    assert np.array_equal(_unpack(b.mask_bits(), case.A), ref.mid["mask"]), ("mask_bits", 3)
    assert np.array_equal(b.obs().cpu().numpy(), ref.mid["obs"]), ("obs", 3)
    assert np.array_equal(b.heuristic_act(case.policy).cpu().numpy(), ref.mid["act"]), ("act", 3)
    # 4: fused rollouts, each continued from the last
    for K in case.rolls:
        rs, dc = b.rollout(case.policy, K)
        assert rs.shape == (K, C.N_ENV)
        _rew(rs, ref.rew[t:t + K], kl, (4, t, K))
        assert np.array_equal(dc.cpu().numpy(), ref.done[t:t + K].sum(0)), ("done_count", 4, t, K)
        t += K
    # 5: per-step heuristic with nothing requested (the headline variant)
    for _ in range(case.n_bare):
        obs, rew, done, valid, act = b.heuristic_step(case.policy, want_actions=False,
                                                      want_valid=False)
        assert valid is None and act is None
        assert np.array_equal(obs.cpu().numpy(), ref.obs[t]), ("obs", 5, t)
        assert np.array_equal(done.cpu().numpy(), ref.done[t]), ("done", 5, t)
        _rew(rew, ref.rew[t], kl, (5, t))
        t += 1
    assert t == case.steps
    # 6: the whole state and the counters
    st = {k: v.cpu().numpy() for k, v in b.state().items()}
    ctr = b.counters().cpu().numpy()
    for i in range(C.N_ENV):
        assert np.array_equal(ctr[i], ref.ctr[-1, i]), ("counters", i, ctr[i], ref.ctr[-1, i])
        for k, x in zip(STATE_KEYS, ref.state[i]):
            assert st[k][i].dtype == x.dtype and np.array_equal(st[k][i], x), (k, i)


@pytest.mark.parametrize("case", C.CASES, ids=[c.name for c in C.CASES])
def test_case_vs_oracle(case, monkeypatch):
    ref = C.run_oracle(case)
    b = _handle(case, ref, monkeypatch)
    try:
        _walk(case, ref, b)
    finally:
        b.close()
