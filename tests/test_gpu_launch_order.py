"""The launch order of the per-step wave launches ("Launch
order"; csrc/vmp_launch_order.h): which env a workgroup takes changes from
launch to launch, what every env computes does not. The idle-step rows of
tests/test_gpu_idle_step.py (both paths alternate hundreds of times there, so
the flags change all the time) at batch sizes with no tail ranks (5), one
chunk (64), three chunks (130) and a partial last rank (517); twin handles, one
of them kept in index order."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import launch_order_rule as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
STEPS = 300
KEYS = ("vm_placement", "vm_cpu", "vm_memory", "cpu", "memory", "vm_remaining_runtime")
ROWS = [(4, 64, 1.0, 40), (4, 130, 1.0, 40)]
ROW_IDS = ["p4v64", "p4v130"]
SIZES = [5, 64, 130, 517]
N_REF = 130  # the oracle replays this many envs once per row; smaller batches are its prefix


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")


def _env(row, n, mode=None):
    """A handle of n envs (seeds 4 i); mode None leaves the library's default order."""
    from tools.idle_step_stats import config
    from vmp import _lib
    from vmp.batched import BatchedVmEnv
    from vmp.config import Config
    b = BatchedVmEnv(Config(**config(*row)), n, seeds=4 * np.arange(n, dtype=np.int64), device=DEV)
    b.eval(False)
    if mode is not None:
        _lib.check(_lib.lib().vmp_debug_launch_order(b._bind(), mode))
    return b


@functools.lru_cache(maxsize=None)
def _oracle(row):
    """STEPS per-step FirstFit steps of N_REF envs on the C oracle, once per row,
    on the device: obs f32 [STEPS, N_REF, D], rew f64, done u8."""
    from tools.idle_step_stats import replay
    ref = replay(*row, N_REF, 0, STEPS, record=True)
    return (torch.from_numpy(ref["obs"]).to(DEV), torch.from_numpy(ref["rew"]).to(DEV),
            torch.from_numpy(ref["done"].astype(np.uint8)).to(DEV))


class _Stepper:
    """Per-step launches into the caller's own buffers, poisoned before every
    launch (NaN obs and reward, done 0xFF): an element a launch leaves
    unwritten, as a map that is no permutation would, equals nothing."""

    def __init__(self, env):
        self.env = env
        self.obs = torch.empty((env.n_envs, env.D), dtype=torch.float32, device=DEV)
        self.rew = torch.empty((env.n_envs,), dtype=torch.float64, device=DEV)
        self.done = torch.empty((env.n_envs,), dtype=torch.uint8, device=DEV)

    def poison(self):
        self.obs.fill_(float("nan"))
        self.rew.fill_(float("nan"))
        self.done.fill_(0xFF)

    def __call__(self):
        self.poison()
        self.env.heuristic_step("firstfit", obs=self.obs, reward=self.rew, done=self.done)
        return self.obs, self.rew, self.done


def _snapshot_mask(row, n):
    """True for the snapshot bytes that belong to the env state: all but the VM
    words of the padded slots v >= V, which nothing initialises or writes
    (tests/test_gpu_idle_step.py)."""
    P, V = row[0], row[1]
    blocks = 1
    while blocks * 64 < V:
        blocks *= 2
    pitch = blocks * 128
    v = np.arange(V)
    slot = (v >> 6 << 7) | (v & 63)
    words = np.zeros(pitch, bool)
    words[slot] = words[slot + 64] = True
    keep = np.ones(256 + n * 256 + 16 * n * P + 4 * n * pitch, bool)
    keep[256 + n * 256 + 16 * n * P:] = np.tile(np.repeat(words, 4), n)
    return torch.from_numpy(keep).to(DEV)


def _same_outputs(x, y, what):
    for a, b, name in zip(x[:3], y[:3], ("obs", "reward", "done")):
        assert torch.equal(a, b), (name,) + what
    assert int(x[2].max()) <= 1, ("done",) + what


def _same_state(a, b, keep, what):
    assert torch.equal(a.counters(), b.counters()), ("counters",) + what
    assert torch.equal(a.stats(), b.stats()), ("stats",) + what
    sa, sb = a.state(), b.state()
    for k in KEYS:
        assert torch.equal(sa[k], sb[k]), (k,) + what
    assert keep.numel() == a.snapshot().numel()
    assert torch.equal(a.snapshot()[keep], b.snapshot()[keep]), ("snapshot",) + what


def _launch_map(env):
    """(env_of_block int64 [n], flags u8 [64 C]) of the next heuristic per-step launch."""
    from vmp import _lib
    m = torch.full((env.n_envs,), -1, dtype=torch.int32, device=DEV)
    f = torch.full((64 * R.chunks(env.n_envs),), 0xEE, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.lib().vmp_debug_launch_map(env._bind(), ctypes.c_void_p(m.data_ptr()),
                                               ctypes.c_void_p(f.data_ptr())))
    return m.cpu().numpy().astype(np.int64), f.cpu().numpy()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_twin_handles_default_order_vs_index_order(row, n):
    """The library's default order against index order over 300 per-step
    FirstFit launches: obs, reward and done equal at every step (and equal to
    the oracle's for n <= 130); counters, stats, exported state and the
    snapshot's state bytes equal at the end."""
    a, b = _env(row, n), _env(row, n, 0)
    sa, sb = _Stepper(a), _Stepper(b)
    ref = _oracle(row) if n <= N_REF else None
    for t in range(STEPS):
        xa, xb = sa(), sb()
        _same_outputs(xa, xb, (t,))
        if ref is not None:
            assert torch.equal(xa[0], ref[0][t, :n]), ("obs vs oracle", t)
            assert torch.equal(xa[1], ref[1][t, :n]), ("reward vs oracle", t)
            assert torch.equal(xa[2], ref[2][t, :n]), ("done vs oracle", t)
    _same_state(a, b, _snapshot_mask(row, n), ("end",))
    a.close()
    b.close()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_launch_map_follows_the_rule(row, n):
    """Before every launch of a handle in mode 2 (all 300, not only the first
    100: the V = 130 row has no idle env, and so nothing to exchange, before
    its slots have filled at about step 130), the map the device computes is a
    permutation, equals the rule restated in tests/launch_order_rule.py on the
    flag bytes the launch reads, and leaves a busy env in a late rank only
    where a chunk has more late busy ranks than early idle ones. Both
    directions occur; where there are tail ranks (n >= 8) some launch
    exchanges envs and some launch reads a busy flag."""
    a = _env(row, n, 2)
    step = _Stepper(a)
    upward, swaps, busy_seen = set(), 0, 0
    for t in range(STEPS):
        m, flags = _launch_map(a)
        parity = t & 1
        assert np.array_equal(np.sort(m), np.arange(n)), t
        assert set(np.unique(flags)) <= {0, 1}, t
        want = R.env_of_block(n, parity, flags)
        assert np.array_equal(m, want), (t, np.flatnonzero(m != want)[:8])
        assert R.late_busy_left(n, parity, flags, m) == R.late_busy_expected(n, parity, flags), t
        upward.add(bool((m == np.arange(n)).sum() > (m == np.arange(n)[::-1]).sum()))
        swaps += int((m != R.position(n, parity, np.arange(n))).any())
        busy_seen += int(flags.any())
        step()
    assert upward == {True, False}  # the blocks outside the tails walk the envs both ways
    if R.tail(n) > 0:
        assert swaps > 0 and busy_seen > 0, (swaps, busy_seen)
    else:
        assert swaps == 0
    a.close()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_mixed_launch_kinds_keep_twins_equal(row, n):
    """Mode 2 against index order through everything that leaves the flags
    stale or starts them at zero: a masked reset, a step with external actions,
    a 3-step fused rollout, eval mode on and off, and a snapshot restored into
    a fresh handle. Equal outputs at every launch, equal state after each part."""
    a, b = _env(row, n, 2), _env(row, n, 0)
    sa, sb = _Stepper(a), _Stepper(b)
    keep = _snapshot_mask(row, n)
    t = 0

    def run(k, what):
        nonlocal t
        for _ in range(k):
            _same_outputs(sa(), sb(), (what, t))
            t += 1
        _same_state(a, b, keep, (what,))

    run(40, "start")
    mask = torch.arange(n, device=DEV) % 3 == 0
    seeds = 1000 + 4 * np.arange(n, dtype=np.int64)
    # (a masked reset writes the observation rows of the envs it resets only)
    assert torch.equal(a.reset(seeds, mask=mask)[mask], b.reset(seeds, mask=mask)[mask])
    run(30, "after masked reset")
    for k in range(3):  # external actions: the heuristic's own, then one launch each
        act = a.heuristic_act("firstfit")
        assert torch.equal(act, b.heuristic_act("firstfit")), ("act", k)
        sa.poison()
        sb.poison()
        xa = a.step(act, obs=sa.obs, reward=sa.rew, done=sa.done, bool_done=False)
        xb = b.step(act, obs=sb.obs, reward=sb.rew, done=sb.done, bool_done=False)
        _same_outputs(xa, xb, ("external", k))
        assert torch.equal(xa[3], xb[3]), ("valid", k)
    run(30, "after external actions")
    ra, rb = a.rollout("firstfit", 3), b.rollout("firstfit", 3)
    assert torch.equal(ra[0], rb[0]) and torch.equal(ra[1], rb[1])
    run(30, "after fused rollout")
    a.eval(True)
    b.eval(True)
    run(30, "eval mode")
    a.eval(False)
    b.eval(False)
    run(30, "training mode again")
    c = _env(row, n, 2)  # zeroed flags, launch count 0
    c.restore(a.snapshot())
    a.close()
    a, sa = c, _Stepper(c)
    run(60, "restored into a fresh handle")
    assert t == 250
    a.close()
    b.close()
