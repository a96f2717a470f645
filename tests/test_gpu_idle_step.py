"""The idle step of the per-step heuristic launch (k_env<VPT, true>, DESIGN.md
§3.1): a launch whose header says that nothing can be placed, accepted or
finished leaves through a short path of its own. Small shapes in which both
paths and the hand-over between them occur hundreds of times, against the C
oracle and against a twin handle that is kept on the general path (a `valid`
buffer is returned, which the idle predicate refuses)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, STEPS = 16, 400
SEEDS = 4 * np.arange(N, dtype=np.int64)
KEYS = ("vm_placement", "vm_cpu", "vm_memory", "cpu", "memory", "vm_remaining_runtime")

# (P, V, lambda, L): VPT 1; VPT 2 with 63 padded lanes; VPT 4; 2P = 256, the
# most PM words the predicate admits; 2P > 256, where it must refuse
ROWS = [(4, 64, 1.0, 40), (4, 65, 1.0, 40), (4, 130, 1.0, 40), (128, 65, 4.0, 200),
        (130, 64, 4.0, 200)]
ROW_IDS = ["p4v64", "p4v65", "p4v130", "p128v65", "p130v64"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")


def _env(row):
    from tools.idle_step_stats import config
    from vmp.batched import BatchedVmEnv
    from vmp.config import Config
    b = BatchedVmEnv(Config(**config(*row)), N, seeds=SEEDS, device=DEV)
    b.eval(False)
    return b


@functools.lru_cache(maxsize=None)
def _oracle(row):
    """STEPS per-step FirstFit steps of the N envs on the C oracle, computed once
    per row (tools/idle_step_stats.py, the replay behind the table in DESIGN
    §3.1): every step's obs / reward / done, the final state and counters, and
    per env-step whether it met the idle predicate (recomputed from the
    oracle's state before the step: the previous step placed, finished and
    accepted nothing, no slot is NULL, no running VM has remaining <= 1) and
    whether it was the last such step before a finisher (smallest remaining 2)."""
    from tools.idle_step_stats import replay
    ref = replay(*row, N, 0, STEPS, record=True)
    for a in ref.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return ref


class _Stepper:
    """Per-step launches into the caller's own output buffers, filled before
    every launch with values no step writes (NaN obs and reward, done 0xFF):
    an element the launch leaves unwritten cannot pass for the previous step's,
    which an idle step's outputs equal by definition."""

    def __init__(self, env):
        self.env = env
        self.obs = torch.empty((env.n_envs, env.D), dtype=torch.float32, device=DEV)
        self.rew = torch.empty((env.n_envs,), dtype=torch.float64, device=DEV)
        self.done = torch.empty((env.n_envs,), dtype=torch.uint8, device=DEV)

    def __call__(self, **kw):
        self.obs.fill_(float("nan"))
        self.rew.fill_(float("nan"))
        self.done.fill_(0xFF)
        self.env.heuristic_step("firstfit", obs=self.obs, reward=self.rew, done=self.done, **kw)
        return self.obs, self.rew, self.done


def _snapshot_mask(row):
    """True for every snapshot byte that belongs to the env state: all of it but
    the VM words of the padded slots v >= V (vmp_layout.h: blocks of 64 slot
    words then 64 time words, the block count rounded up to a power of two).
    vmp_create does not clear those words and no kernel writes them, so they
    hold whatever the allocation held: two handles differ there before either
    has made a step, with or without the idle path."""
    P, V = row[0], row[1]
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


def _same_outputs(x, y, what):
    """obs / reward / done of two launches equal (torch.equal: a NaN left from
    the fill equals nothing), done a written 0 / 1."""
    for a, b, name in zip(x[:3], y[:3], ("obs", "reward", "done")):
        assert torch.equal(a, b), (name,) + what
    assert int(x[2].max()) <= 1, ("done",) + what


def _same_state(a, b, what):
    assert torch.equal(a.counters(), b.counters()), ("counters",) + what
    assert torch.equal(a.stats(), b.stats()), ("stats",) + what
    sa, sb = a.state(), b.state()
    for k in KEYS:
        assert torch.equal(sa[k], sb[k]), (k,) + what


@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_idle_step_vs_oracle(row):
    """Per-step FirstFit launches that return no actions and no validity flags
    (so idle steps take the idle path) equal the oracle at every step: obs bit
    for bit, reward and done; counters and the exported state at the end. The
    inputs must reach the path: >= 0.25 of the env-steps meet the predicate and
    >= 100 of them are the last idle step before a finisher."""
    ref = _oracle(row)
    assert ref["idle"].mean() >= 0.25, ref["idle"].mean()
    assert ref["edge"].sum() >= 100, ref["edge"].sum()
    b = _env(row)
    step = _Stepper(b)
    for t in range(STEPS):
        obs, rew, done = (x.cpu().numpy() for x in step())
        for i in range(N):
            assert rew[i] == ref["rew"][t, i], (t, i, rew[i], ref["rew"][t, i])
            assert done[i] == int(ref["done"][t, i]), (t, i, done[i])
            assert np.array_equal(obs[i], ref["obs"][t, i]), (t, i)
    ctr = b.counters().cpu().numpy()
    sd = {k: v.cpu().numpy() for k, v in b.state().items()}
    for i in range(N):
        assert np.array_equal(ctr[i], ref["ctr"][i]), i
        for j, k in enumerate(KEYS):
            assert np.array_equal(sd[k][i], ref["state"][i][j]), (k, i)
    b.close()


@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_idle_step_twin_handles_snapshot_equal(row):
    """Two handles with the same seeds, per-step launches only: A returns no
    validity flags, B does and so never leaves the general path. After every
    step obs, reward and done are equal and the snapshots are byte-identical:
    the whole header (the hint word and the four RNG streams included), the PM
    words and every VM slot's two words. Only the never-initialised words of
    the padded slots are left out (_snapshot_mask); before this change two
    handles' whole snapshots differed there too whenever V is no multiple of
    64 (P4 V65 after the first step)."""
    a, b = _env(row), _env(row)
    sa, sb = _Stepper(a), _Stepper(b)
    keep = _snapshot_mask(row)
    assert keep.numel() == a.snapshot().numel()
    for t in range(STEPS):
        _same_outputs(sa(), sb(want_valid=True), (t,))
        assert torch.equal(a.snapshot()[keep], b.snapshot()[keep]), ("snapshot", t)
    _same_state(a, b, ("end",))
    a.close()
    b.close()


def test_idle_step_after_fused_rollout_chunks():
    """Handle A alternates runs of per-step launches with fused 7-step rollouts,
    whose hint word the idle predicate must refuse until a per-step launch has
    written its own; handle B makes the same steps one general-path launch at a
    time. Outputs equal at every per-step launch and every fused step's reward;
    state, counters and stats equal at every chunk end."""
    row = ROWS[1]
    a, b = _env(row), _env(row)
    sa, sb = _Stepper(a), _Stepper(b)
    t = 0
    for chunk in range(36):
        for _ in range(1 + chunk % 5):  # 1..5 per-step launches, then a fused chunk
            _same_outputs(sa(), sb(want_valid=True), (t,))
            t += 1
        _same_state(a, b, ("per-step", chunk))
        rs = a.rollout("firstfit", 7)[0]
        for k in range(7):
            rb = sb(want_valid=True)[1]
            assert torch.equal(rs[k], rb), (t, k)
            t += 1
        _same_state(a, b, ("fused", chunk))
    assert t >= 300
    a.close()
    b.close()


def test_idle_step_per_env_workload_kernel():
    """The per-env-workload kernels take the same path: a handle given a
    workload equal to the config's in every env equals the untouched handle at
    every step."""
    row = ROWS[1]
    a, b = _env(row), _env(row)
    a.set_workload(arrival_rate=np.full(N, row[2]), service_length=np.full(N, float(row[3])))
    sa, sb = _Stepper(a), _Stepper(b)
    for t in range(STEPS):
        _same_outputs(sa(), sb(), (t,))
    _same_state(a, b, ("end",))
    a.close()
    b.close()
