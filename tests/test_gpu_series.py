"""The per-step time series (vmp_series_*, BatchedVmEnv.series) on the GPU
against tests/series_literal: after every step the expected row is built from
the handle's own getters (counters, stats, state, rank, the step's reward), or
from the C oracle's run, and folded into a LiteralSeries. Every field must be
bit-equal, except CPU_VAR / MEM_VAR: within 1e-12 relative of np.var, the
project's bound for the kl reward's variance terms. 5 envs (not a multiple of
the 4 waves of a block), seeds 4 i, 60 steps at an arrival rate of V / 4 and a
service length of 8: the slots fill within a few steps, VMs finish from step 9
on and requests are dropped (checked on the CPU with the oracle)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import series_literal as SL

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = 5
SEEDS = np.arange(N, dtype=np.int64) * 4
STEPS = 60
EINVAL, EOOM, ESTATE = -1, -3, -4
# one slot row; full rows; a partial last row in padded blocks, P over two bitmap words and a
# pairwise split; the block kernel (dynamic LDS for the target sums); the LDS plan for the PM sums
SHAPES = [(10, 30), (100, 1000), (130, 300), (20, 1100), (2000, 500)]
BASE = dict(allow_null_action=True, training_steps=10000, eval_steps=100000, seed=0,
            sequence="uniform", cap_target_util=True, beta=0.3, service_length=8)
EXACT = [f for f in range(SL.NF) if f not in SL.VAR_FIELDS]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")


def _cfg(P, V, reward="wr", **over):
    return dict(dict(BASE, pms=P, vms=V, arrival_rate=V / 4.0, reward_function=reward), **over)


def _env(cfg, n=N, **kw):
    from vmp.batched import BatchedVmEnv
    from vmp.config import Config
    return BatchedVmEnv(Config(**cfg), n, seeds=np.arange(n, dtype=np.int64) * 4, device=DEV, **kw)


def _same_start(a, b):
    """Twin b takes twin a's snapshot, so the two hold the same bytes: the
    padded VM words behind slot V, which no kernel reads or writes, included
    (they are whatever the allocation held)."""
    b.restore(a.snapshot())


def _assert_same_snapshot(a, b, what=""):
    """snapshot() bytes equal; a difference is reported by offset and part
    (descriptor 256 B | hdr N x 256 | pm N x 2P f64 | VM words)."""
    x, y = a.snapshot().cpu().numpy(), b.snapshot().cpu().numpy()
    assert x.shape == y.shape
    bad = np.flatnonzero(x != y)
    ends = np.cumsum([256, 256 * a.n_envs, 16 * a.n_envs * a.P])
    assert bad.size == 0, (what, bad.size, bad[:8], [int(np.searchsorted(ends, o, "right")) for o in bad[:8]])


def _random_actions(g, placement, P):
    """Half of the slots keep their placement, the others draw any action in
    0..P+1: waiting VMs are placed where they fit, running VMs are suspended
    (action WAIT, valid) or sent elsewhere (invalid)."""
    a = placement.copy()
    draw = g.random(a.shape) < 0.5
    a[draw] = g.integers(0, P + 2, int(draw.sum()))
    return a


@functools.lru_cache(maxsize=None)
def _oracle_counters_move(P, V):
    """On the CPU: under first fit the workload fills, finishes and drops within
    STEPS steps; under the random actions VMs are suspended as well."""
    cfg = _cfg(P, V)
    e = O.OracleEnv(dict(cfg, seed=0))
    e.reset(0)
    for _ in range(STEPS):
        e.step(e.firstfit())
    c = e.counters()[0]
    assert c[0] > V and c[1] > 0 and c[3] > 0 and c[4] > 0 and c[5] == STEPS + 1, (P, V, c)
    e.reset(0)
    g = np.random.default_rng(11)
    for _ in range(STEPS):
        e.step(_random_actions(g, e.state()[0], P))
    c = e.counters()[0]
    assert c[1] > 0 and c[2] > 0 and c[3] > 0 and c[4] > 0, (P, V, c)
    return True


def _getter_rows(b, rew):
    """The step's expected rows [n_envs, NF] from the handle's own getters."""
    st = {k: v.cpu().numpy() for k, v in b.state().items()}
    ctr, sts, rk = b.counters().cpu().numpy(), b.stats().cpu().numpy(), b.rank().cpu().numpy()
    rew = rew.cpu().numpy()
    return np.stack([SL.row_of({k: v[i] for k, v in st.items()}, ctr[i], sts[i], int(rk[i]),
                               float(rew[i]), b.P) for i in range(b.n_envs)])


def _step(b, driver, g=None):
    """One step under `driver`; -> (obs, reward)."""
    if driver == "step":
        pl = b.state()["vm_placement"].cpu().numpy()
        a = torch.tensor(_random_actions(g, pl, b.P), dtype=torch.int32, device=DEV)
        obs, rew, _, _ = b.step(a)
        return obs, rew
    obs, rew, _, _, _ = b.heuristic_step(driver)
    return obs, rew


def _assert_rows(got, want, what=""):
    """got, want [..., NF]: bit-equal but for the variances (1e-12 relative)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for f in SL.VAR_FIELDS:
        err = np.abs(got[..., f] - want[..., f])
        rel = float(np.max(err / np.maximum(np.abs(want[..., f]), 1e-300))) if err.size else 0.0
        print("series %s field %d: max relative variance error %.3g, %d of %d values bit-equal"
              % (what, f, rel, int(np.sum(got[..., f] == want[..., f])), err.size))
        assert np.all(err <= 1e-12 * np.abs(want[..., f])), (what, f, rel)
    bad = np.argwhere(got[..., EXACT] != want[..., EXACT])
    assert bad.size == 0, (what, [(tuple(x[:-1]), EXACT[x[-1]], got[tuple(x[:-1])][EXACT[x[-1]]],
                                   want[tuple(x[:-1])][EXACT[x[-1]]]) for x in bad[:6]])


def _assert_series(b, lits, what=""):
    """The device series equals the per-env literals: meta and every row."""
    ser = b.series_read()
    for i, lit in enumerate(lits):
        assert np.array_equal(ser.meta[i], lit.meta), ("meta", what, i, ser.meta[i], lit.meta)
    _assert_rows(ser.rows, np.stack([lit.rows for lit in lits]), what)
    return ser


def _run_with_literals(b, lits, driver, steps, g=None):
    for _ in range(steps):
        _, rew = _step(b, driver, g)
        rows = _getter_rows(b, rew)
        for lit, r in zip(lits, rows):
            lit.add(r)


# ------------------------------------------------- 1: every field, every shape
@pytest.mark.parametrize("driver,reward", [("firstfit", "ut"), ("bestfit", "kl"), ("step", "wr")])
@pytest.mark.parametrize("P,V", SHAPES)
def test_every_field_vs_getters(P, V, driver, reward):
    assert _oracle_counters_move(P, V)
    b = _env(_cfg(P, V, reward))
    b.series(capacity=STEPS)
    lits = [SL.LiteralSeries(STEPS, 1) for _ in range(N)]
    _run_with_literals(b, lits, driver, STEPS, np.random.default_rng(11))
    ser = _assert_series(b, lits, "P%d V%d %s" % (P, V, driver))
    assert np.array_equal(ser.count, [STEPS] * N) and np.array_equal(ser.rows_written, [STEPS] * N)
    assert np.array_equal(ser.first, [1] * N) and not ser.lost.any() and np.all(ser.steps == 1)
    assert np.array_equal(ser.timestep, np.broadcast_to(np.arange(2, STEPS + 2), (N, STEPS)))
    # the counters moved on the device too, and the series saw the slots fill
    last = ser.rows[:, -1]
    for f in (SL.TOTAL_REQUESTS, SL.SERVED, SL.PLACE, SL.DROPPED) + ((SL.SUSPEND,) if driver == "step" else ()):
        assert np.all(last[:, f] > 0), f
    assert np.max(ser.waiting + ser.running) == V and np.all(ser.used_pm.max(axis=1) > 0)
    assert np.all(ser.used_pm + ser.empty_pm <= P) and np.all(ser.used_pm <= ser.running)
    # the independent restatement of the target means (k_target_means gave the getters' values)
    st = {k: v.cpu().numpy() for k, v in b.state().items()}
    for i in range(N):
        tm = SL.target_means({k: v[i] for k, v in st.items()}, P, True)
        assert last[i, SL.TARGET_CPU_MEAN] == tm[0] and last[i, SL.TARGET_MEM_MEAN] == tm[1], i
    if reward == "ut":  # env.py:152, of the very sums the reward kernel took; 0 with no VM at all
        ut = BASE["beta"] * ser.cpu_sum + (1 - BASE["beta"]) * ser.mem_sum
        ut = np.where(ser.waiting + ser.running > 0, ut, 0.0)
        assert np.array_equal(ser.reward, ut)
    b.close()


@pytest.mark.parametrize("reward", ["ut", "kl"])
def test_every_field_vs_the_oracles_own_run(reward):
    """ut: every field from the oracle, the reward included, bit for bit. kl:
    the step kernel's kl reward equals the oracle's only within the project's
    1e-12 (libm's log; __graft_entry__.smoke), and REWARD is the step's own
    reward, so that row takes the device step's reward (checked against the
    oracle's within that bound) and everything else from the oracle."""
    P, V = 10, 30
    cfg = _cfg(P, V, reward)
    b = _env(cfg)
    b.series(capacity=STEPS)
    oes = [O.OracleEnv(dict(cfg, seed=int(s))) for s in SEEDS]
    for e, s in zip(oes, SEEDS):
        e.reset(int(s))
    lits = [SL.LiteralSeries(STEPS, 1) for _ in range(N)]
    for t in range(STEPS):
        _, rew, _, _, act = b.heuristic_step("firstfit", want_actions=True)
        act, rew = act.cpu().numpy(), rew.cpu().numpy()
        for i, e in enumerate(oes):
            a = e.firstfit()
            assert np.array_equal(a, act[i]), (t, i)
            _, r, _, _ = e.step(a)
            if reward == "kl":
                assert abs(r - rew[i]) <= 1e-12 * max(1.0, abs(r)), (t, i, r, rew[i])
                r = float(rew[i])
            pl, vc, vm, c, m, _ = e.state()
            ctr, sts = e.counters()
            lits[i].add(SL.row_of(dict(vm_placement=pl, cpu=c, memory=m), ctr, sts, e.rank(), r, P))
    _assert_series(b, lits, "oracle")
    b.close()


# ------------------------------------------------------------------ 2: windows
def test_windows_capacity_and_poisoned_margin():
    from vmp import _lib
    P, V, S, CAP = 130, 300, 7, 5
    cfg = _cfg(P, V, "kl")
    b, one = _env(cfg), _env(cfg)
    b.series(capacity=CAP, stride=S)
    one.series(capacity=STEPS, stride=1)
    lits = [SL.LiteralSeries(CAP, S) for _ in range(N)]
    for _ in range(STEPS):
        _, rew = _step(b, "bestfit")
        _step(one, "bestfit")
        for lit, r in zip(lits, _getter_rows(b, rew)):
            lit.add(r)
    ser = _assert_series(b, lits, "windows")   # STEPS, COUNT, LOST, sums, last-step counters
    assert np.array_equal(ser.meta, [[1, STEPS, STEPS - CAP * S]] * N)
    assert np.all(ser.steps == S) and np.array_equal(ser.rows_written, [CAP] * N)
    assert np.array_equal(ser.timestep, np.broadcast_to(1 + S * np.arange(1, CAP + 1), (N, CAP)))
    # the device's own per-step values (the stride-1 twin), added one after another: every
    # field bit for bit, the variances included
    steps = one.series_read()
    for i in range(N):
        lit = SL.LiteralSeries(CAP, S)
        for r in steps.rows[i]:
            lit.add(r)
        assert np.array_equal(ser.rows[i], lit.rows) and np.array_equal(ser.meta[i], lit.meta), i
    # nothing beyond the capacity: read into the prefix of larger poisoned buffers
    n = N * CAP * SL.NF
    buf = torch.full((n + 4096,), -7.5, dtype=torch.float64, device=DEV)
    meta = torch.full((N * 3 + 64,), -7, dtype=torch.int64, device=DEV)
    _lib.check(_lib.lib().vmp_series_read(b._bind(), _lib.ptr(buf), None, _lib.ptr(meta)))
    buf, meta = buf.cpu().numpy(), meta.cpu().numpy()
    assert np.array_equal(buf[:n].reshape(N, CAP, SL.NF), ser.rows) and np.all(buf[n:] == -7.5)
    assert np.array_equal(meta[:N * 3].reshape(N, 3), ser.meta) and np.all(meta[N * 3:] == -7)
    b.close()
    one.close()


# ------------------------------------------------------------------ 3: PM rows
@pytest.mark.parametrize("P,V", [(130, 300), (20, 1100)])
def test_pm_rows_are_the_last_observation_of_each_window(P, V):
    from vmp import _lib
    S, CAP = 7, 7   # 60 steps: 7 rows kept (49 steps), 11 steps lost
    b, one = _env(_cfg(P, V)), _env(_cfg(P, V))
    b.series(capacity=CAP, stride=S, pm_rows=True)
    one.series(capacity=STEPS, pm_rows=True)
    obs = []
    for _ in range(STEPS):
        o, _ = _step(b, "firstfit")
        _step(one, "firstfit")
        obs.append(o[:, 3 * V:].cpu().numpy())
    obs = np.stack(obs, axis=1)   # [N, STEPS, 2P]
    ser, steps = b.series_read(), one.series_read()
    assert steps.pm.shape == (N, STEPS, 2 * P) and np.array_equal(steps.pm, obs)
    assert np.array_equal(ser.pm, obs[:, S - 1:S * CAP:S]) and np.any(obs[:, S * CAP - 1] != obs[:, -1])
    assert np.array_equal(ser.pm_cpu, ser.pm[:, :, :P]) and np.array_equal(ser.pm_mem, ser.pm[:, :, P:])
    assert np.array_equal(ser.lost, [STEPS - S * CAP] * N) and ser.pm_cpu.max() > 0
    assert np.array_equal(ser.rows, b.series_read().rows)   # a read changes nothing
    # the PM buffer has no slack either
    n = N * CAP * 2 * P
    buf = torch.full((n + 4096,), -7.5, dtype=torch.float32, device=DEV)
    _lib.check(_lib.lib().vmp_series_read(b._bind(), None, _lib.ptr(buf), None))
    got = buf.cpu().numpy()
    assert np.array_equal(got[:n].reshape(N, CAP, 2 * P), ser.pm) and np.all(got[n:] == -7.5)
    # a series without PM rows has none to read
    one.series(capacity=4)
    assert one.series_read().pm is None
    assert _lib.lib().vmp_series_read(one._bind(), None, _lib.ptr(buf), None) == ESTATE
    b.close()
    one.close()


# --------------------------------------------------------------- 4: neutrality
@pytest.mark.parametrize("observed", [False, True])
@pytest.mark.parametrize("P,V,reward", [(10, 30, "wr"), (20, 1100, "kl")])
def test_series_changes_nothing_of_the_run(P, V, reward, observed):
    """Twins, one with the series on: every step's obs / reward / done and the
    final snapshot are equal (P 10 / wr: the idle-step path of the per-step
    kernel stays in use, the series asks for no actions or validity flags);
    with recorder and request log on in both, their outputs are equal too."""
    a, b = _env(_cfg(P, V, reward)), _env(_cfg(P, V, reward))
    for e in (a, b):
        e.eval(True)
        e.reset(torch.tensor(SEEDS))
        if observed:
            e.record(True)
            e.request_log(capacity=4000)
    _same_start(a, b)   # before the series: a restore restarts it
    b.series(stride=3, capacity=40, pm_rows=True)
    for t in range(STEPS):
        (o1, r1, d1, _, _), (o2, r2, d2, _, _) = a.heuristic_step("bestfit"), b.heuristic_step("bestfit")
        assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2), t
    _assert_same_snapshot(a, b, "after the run")
    if observed:   # record_summary calls the stats getter: on both twins
        np.testing.assert_equal(a.record_summary(), b.record_summary())
        la, lb = a.request_log_read(), b.request_log_read()
        assert np.array_equal(la.rows, lb.rows) and np.array_equal(la.meta, lb.meta)
        assert la.meta[:, 1].min() > V
        _assert_same_snapshot(a, b, "after the stats getter on both")
    ser = b.series_read()
    assert np.array_equal(ser.count, [STEPS] * N) and np.all(ser.steps[:, :20] == 3)
    assert np.all(ser.dropped[:, 19] > 0)
    a.close()
    b.close()


# ------------------------------------------------------------- 5: launch kinds
def test_rollout_call_gives_a_row_per_step():
    cfg = _cfg(10, 30)
    b, twin = _env(cfg), _env(cfg)
    b.series(capacity=40)
    twin.series(capacity=40)
    rew, _ = b.rollout("firstfit", 25)
    for _ in range(25):
        twin.heuristic_step("firstfit")
    got, want = b.series_read(), twin.series_read()
    assert np.array_equal(got.count, [25] * N) and np.array_equal(got.rows_written, [25] * N)
    assert np.array_equal(got.rows, want.rows) and np.array_equal(got.meta, want.meta)
    assert np.array_equal(got.reward[:, :25], rew.cpu().numpy().T) and not got.rows[:, 25:].any()
    b.close()
    twin.close()


def test_graph_captured_after_enable_advances_on_replay():
    cfg = _cfg(130, 300, "ut")
    b = _env(cfg)
    b.series(capacity=30, stride=2, pm_rows=True)
    b.heuristic_step("firstfit")  # a launch outside the capture first
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(10):
            b.heuristic_step("firstfit")
    b.reset(torch.tensor(SEEDS))   # restarts the series
    for _ in range(2):
        g.replay()
    got = b.series_read()
    del g
    twin = _env(cfg)
    twin.series(capacity=30, stride=2, pm_rows=True)
    for _ in range(20):
        twin.heuristic_step("firstfit")
    want = twin.series_read()
    assert np.array_equal(got.count, [20] * N) and np.array_equal(got.rows_written, [10] * N)
    assert np.array_equal(got.rows, want.rows) and np.array_equal(got.meta, want.meta)
    assert np.array_equal(got.pm, want.pm) and got.cpu_sum[:, 9].min() > 0
    b.close()
    twin.close()


def test_traced_handle_follows_the_traces_offsets():
    from vmp.config import Config
    from vmp.trace import Trace
    P, V = 10, 30
    cfg = _cfg(P, V)
    traces = []
    for i in range(N):   # a first step of 50 requests for 30 slots, then a synthetic trace
        t = Trace.synthetic(Config(**dict(cfg, arrival_rate=3.0)), 30, seed=i)
        traces.append(Trace(np.r_[0, t.offs + 50], np.r_[np.full(50, 10 + i), t.cpu],
                            np.r_[np.full(50, 20), t.mem], np.r_[np.full(50, 3), t.runtime]))
    b = _env(cfg)
    b.set_trace(traces, np.arange(N))
    b.reset()
    b.series(capacity=40)
    lits = [SL.LiteralSeries(40, 1) for _ in range(N)]
    _run_with_literals(b, lits, "firstfit", 40)   # 31 trace steps, then no requests
    ser = _assert_series(b, lits, "traced")
    for i, t in enumerate(traces):
        offs = np.r_[t.offs[1:], np.full(40, t.offs[-1])][:40]
        assert np.array_equal(ser.total_requests[i], offs), i
        assert ser.dropped[i, 0] == 50 - V and np.all(np.diff(ser.dropped[i]) >= 0)
        assert np.all(np.diff(ser.dropped[i]) <= np.diff(offs)) and ser.dropped[i, -1] == ser.dropped[i, 31]
        assert ser.waiting[i, 0] + ser.running[i, 0] == V
    b.close()


def test_per_env_workload_handle():
    P, V = 10, 30
    b = _env(_cfg(P, V, "ut"), arrival_rate=[0.0, 0.5, 4.0, 12.0, 25.0],
             service_length=[5.0, 30.0, 8.0, 12.0, 2.0])
    b.series(capacity=40)
    lits = [SL.LiteralSeries(40, 1) for _ in range(N)]
    _run_with_literals(b, lits, "bestfit", 40)
    ser = _assert_series(b, lits, "workload")
    assert not ser.total_requests[0].any() and not ser.reward[0].any()
    assert np.all(ser.total_requests[1:, -1] > 0) and ser.dropped[4, -1] > ser.dropped[2, -1] >= 0
    b.close()


# ---------------------------------------------------------------- 6: lifecycle
def _info(b):
    from vmp import _lib
    c, s, p = ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int32()
    _lib.check(_lib.lib().vmp_series_info(b._bind(), ctypes.byref(c), ctypes.byref(s), ctypes.byref(p)))
    return c.value, s.value, p.value


def test_masked_reset_restore_mid_run_enable_reenable_disable():
    from vmp import _lib
    from vmp._lib import VmpError
    L = _lib.lib()
    P, V = 10, 30
    cfg = _cfg(P, V, "kl", training_steps=200, eval_steps=300)
    live = L.vmp_debug_live_allocs()
    b = _env(cfg)
    base = L.vmp_debug_live_allocs()
    b.series(capacity=100)
    assert _info(b) == (100, 1, 0) and L.vmp_debug_live_allocs() == base + 3   # rows, meta, reward
    lits = [SL.LiteralSeries(100, 1) for _ in range(N)]
    _run_with_literals(b, lits, "firstfit", 10)
    _assert_series(b, lits, "start")
    mask = torch.zeros(N, dtype=torch.uint8)
    mask[3] = 1
    b.reset(torch.full((N,), 99, dtype=torch.int64), mask=mask)   # only env 3 restarts
    lits[3].restart(1)
    _assert_series(b, lits, "after the masked reset")
    _run_with_literals(b, lits, "firstfit", 5)
    ser = _assert_series(b, lits, "env 3 reset")
    assert np.array_equal(ser.count, [15, 15, 15, 5, 15]) and ser.timestep[3, 4] == 6
    snap = b.snapshot()
    ts = b.counters()[:, 5].cpu().numpy()
    _run_with_literals(b, lits, "firstfit", 3)
    b.restore(snap)   # every env's series restarts, FIRST = the restored timestep
    for lit, t in zip(lits, ts):
        lit.restart(int(t))
    _assert_series(b, lits, "restored")
    _run_with_literals(b, lits, "firstfit", 4)
    ser = _assert_series(b, lits, "after the restore")
    assert np.array_equal(ser.first, [16, 16, 16, 6, 16]) and np.array_equal(ser.count, [4] * N)
    b.close()
    assert L.vmp_debug_live_allocs() == live
    # a mid-run enable with the default capacity, then another stride, then off
    c = _env(cfg)
    for _ in range(12):
        c.heuristic_step("firstfit")
    c.series(stride=2)
    assert _info(c) == ((200 - 12 + 1) // 2, 2, 0)   # the steps left to training_steps
    lits = [SL.LiteralSeries(94, 2, 13) for _ in range(N)]
    _run_with_literals(c, lits, "firstfit", 7)
    ser = _assert_series(c, lits, "mid-run")
    assert np.array_equal(ser.first, [13] * N) and np.array_equal(ser.rows_written, [4] * N)
    assert np.array_equal(ser.steps[:, :5], [[2, 2, 2, 1, 0]] * N)
    c.eval(True)
    c.series(stride=7, pm_rows=True)   # reallocates and restarts
    assert _info(c) == (-(-(300 - 19) // 7), 7, 1)
    lits = [SL.LiteralSeries(41, 7, 20) for _ in range(N)]
    _assert_series(c, lits, "re-enabled")
    _run_with_literals(c, lits, "firstfit", 9)
    ser = _assert_series(c, lits, "second stride")
    assert np.array_equal(ser.steps[:, :3], [[7, 2, 0]] * N)
    c.series(False)
    assert _info(c) == (0, 0, 0) and L.vmp_debug_live_allocs() == base
    with pytest.raises(VmpError):
        c.series_read()
    assert L.vmp_series_read(c._bind(), None, None, None) == ESTATE
    c.series(False)   # off while off
    c.close()
    assert L.vmp_debug_live_allocs() == live


def test_failure_paths_leave_the_handle_as_it_was():
    from vmp import _lib
    L = _lib.lib()
    cfg = _cfg(10, 30)
    b, twin = _env(cfg), _env(cfg)
    _same_start(b, twin)
    h = b._bind()
    base = L.vmp_debug_live_allocs()
    assert L.vmp_series_read(h, None, None, None) == ESTATE
    for args in ((-1, 1, 0), (1 << 31, 1, 0), (1 << 62, 1, 0), (10, 0, 0), (10, -2, 0), (10, 1, 2),
                 (10, 1, -1)):
        assert L.vmp_series_enable(h, *args) == EINVAL, args
    assert L.vmp_series_enable(None, 10, 1, 0) == EINVAL and L.vmp_series_info(None, None, None, None) == EINVAL
    assert L.vmp_series_enable(h, 0, 1, 0) == 0 and _info(b) == (0, 0, 0)
    assert L.vmp_debug_live_allocs() == base
    for pm_rows, n_alloc in ((0, 3), (1, 4)):   # rows (, PM rows), meta, the scratch reward
        for nth in range(1, n_alloc + 1):
            _lib.check(L.vmp_debug_fail_alloc(nth))
            rc = L.vmp_series_enable(h, 50, 2, pm_rows)
            _lib.check(L.vmp_debug_fail_alloc(0))
            assert rc == EOOM, (pm_rows, nth, rc)
            assert L.vmp_debug_live_allocs() == base and _info(b) == (0, 0, 0)
            assert L.vmp_series_read(h, None, None, None) == ESTATE
            b.heuristic_step("firstfit")   # the handle works
            twin.heuristic_step("firstfit")
        _lib.check(L.vmp_debug_fail_alloc(n_alloc + 1))   # one more than it makes: succeeds
        assert L.vmp_series_enable(h, 50, 2, pm_rows) == 0
        _lib.check(L.vmp_debug_fail_alloc(0))
        assert L.vmp_debug_live_allocs() == base + n_alloc and _info(b) == (50, 2, pm_rows)
        b.heuristic_step("firstfit")
        twin.heuristic_step("firstfit")
        # a failed re-enable (the scratch reward stays: one allocation fewer) leaves the series it had
        for nth in range(1, n_alloc):
            _lib.check(L.vmp_debug_fail_alloc(nth))
            assert L.vmp_series_enable(h, 70, 3, pm_rows) == EOOM
            _lib.check(L.vmp_debug_fail_alloc(0))
            assert L.vmp_debug_live_allocs() == base + n_alloc and _info(b) == (50, 2, pm_rows)
        assert L.vmp_series_enable(h, 10, 0, 0) == EINVAL and _info(b) == (50, 2, pm_rows)
        b.heuristic_step("firstfit")
        twin.heuristic_step("firstfit")
        ser = b.series_read()
        assert np.array_equal(ser.count, [2] * N) and np.all(ser.steps[:, 0] == 2)
        assert L.vmp_series_enable(h, 70, 3, pm_rows) == 0 and _info(b) == (70, 3, pm_rows)
        assert L.vmp_debug_live_allocs() == base + n_alloc
        assert not b.series_read().count.any()
        b.series(False)
        assert L.vmp_debug_live_allocs() == base and _info(b) == (0, 0, 0)
    # after all of it the env steps as an untouched twin does
    for _ in range(20):
        o1, r1, _, _, _ = b.heuristic_step("bestfit")
        o2, r2, _, _, _ = twin.heuristic_step("bestfit")
        assert torch.equal(o1, o2) and torch.equal(r1, r2)
    _assert_same_snapshot(b, twin)
    b.close()
    twin.close()


# -------------------------------------------------------------------- 7: sweep
def _cells(seeds=(0, 4)):
    from vmp import exp
    return [exp.Cell(agent, 1.0, 8, seeds, cfg=_cfg(10, 30, "ut", arrival_rate=rate), name="%s-%g" % (agent, rate))
            for agent, rate in (("firstfit", 7.5), ("firstfit", 2.0), ("bestfit", 7.5))]


def test_run_cells_series_csv_is_numpy_over_the_per_env_series(tmp_path):
    from vmp import exp
    from vmp.series import FIELDS
    cells, S = _cells(), 5
    path = str(tmp_path / "series.csv")
    res = exp.run_cells(cells, eval_steps=50, graph_steps=10, device=DEV, series=(S, path))
    plain = exp.run_cells(cells, eval_steps=50, graph_steps=10, device=DEV)
    np.testing.assert_equal(res, plain)   # the summaries are those of a run without the series
    lines = open(path).read().splitlines()
    assert lines[0] == exp.series_header() and len(lines) == 1 + 3 * 10
    hdr = lines[0].split(", ")
    for ci, cell in enumerate(cells):
        b = _env(dict(cell.cfg, eval_steps=50), n=2)
        b.eval(True)
        b.reset(torch.tensor(cell.seeds))
        b.series(stride=S)
        assert _info(b) == (10, S, 0)
        b.rollout(cell.agent, 50)
        ser = b.series_read()
        b.close()
        for r in range(10):
            c = lines[1 + ci * 10 + r].split(",")
            assert c[:5] == [str(ci), cell.name, "2", str(r), str(1 + S * (r + 1))], (ci, r, c[:5])
            for k in range(5, len(hdr), 2):
                name = hdr[k][:-len(" Mean")]
                x = ser.rows[:, r, FIELDS.index(name)]
                x = x / S if name in FIELDS[1:13] else x
                assert float(c[k]) == x.mean() and float(c[k + 1]) == x.std(), (ci, r, name)
    # merged cells (one handle per agent, a per-env workload) still report their own envs
    merged = str(tmp_path / "merged.csv")
    exp.run_cells(cells, eval_steps=50, graph_steps=10, device=DEV, merge=True, series=(S, merged))
    assert open(merged).read() == open(path).read()


def test_cli_series_flag_leaves_the_output_as_it_was(tmp_path, capsys):
    from vmp import exp
    args = ["suspension", "--lengths", "100", "--loads", "1.0", "--eval-steps", "40"]
    exp.main(args)
    plain = capsys.readouterr().out
    out = str(tmp_path / "s.csv")
    exp.main(args + ["--series", out, "--series-stride", "8"])
    assert capsys.readouterr().out == plain and plain.count("\n") == 1 + 4
    lines = open(out).read().splitlines()
    assert lines[0] == exp.series_header() and len(lines) == 1 + 4 * 5
    assert [ln.split(",")[:5] for ln in lines[1:6]] == [["0", "firstfit", "1", str(r), str(1 + 8 * (r + 1))]
                                                        for r in range(5)]
