"""Trace-driven workloads (vmp_set_trace, BatchedVmEnv.set_trace) on the GPU.

The oracle fixture is tests/test_gpu_workload.py's (P12/V90, its 8 (lambda, L)
pairs, seeds 4 i, 200 oracle steps per (policy, reward)): every oracle env's
run is turned into the trace it accepted (tests/trace_literal.derive_trace),
and a handle replaying trace i on env i must reproduce the oracle's run bit
for bit although it draws nothing. Generated traces, for which no oracle run
exists, are checked against the numpy literal (tests/trace_literal.TraceEnv,
itself pinned against the oracle in tests/test_trace_cpu.py)."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import trace_literal as TL
from tests.test_gpu_workload import (BASE, DEV, LAM, N, SEEDS, STATE_KEYS, WL, _check_end,
                                     _check_steps, _config, _ref, _rew_equal)

pytestmark = pytest.mark.gpu

EINVAL, EOOM, ESTATE = -1, -3, -4
P, V = BASE["pms"], BASE["vms"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")


@functools.lru_cache(maxsize=None)
def _traces(policy, reward):
    """One derived trace per env of the fixture's oracle run."""
    from vmp.trace import Trace
    ref = _ref(policy, reward)
    pre = (np.full(V, P + 1),)
    out = []
    for i in range(N):
        offs, cpu, mem, rt = TL.derive_trace(
            P, pre, ref["act"][:, i], ref["valid"][:, i], [s[i] for s in ref["state"]],
            ref["ctr"][:, i])
        out.append(Trace(offs, cpu, mem, rt))
    return tuple(out)


def _env(reward, n=N, **over):
    from vmp.batched import BatchedVmEnv
    # the config's own workload is never drawn from on a traced env
    return BatchedVmEnv(_config(reward, **over), n, seeds=np.arange(n, dtype=np.int64) * 4,
                        device=DEV)


def _traced(policy, reward):
    b = _env(reward)
    b.set_trace(_traces(policy, reward), np.arange(N))
    return b


def _literals(cfg, traces, trace_of_env):
    return [TL.TraceEnv(cfg, *(getattr(traces[j], k) for k in ("offs", "cpu", "mem", "runtime")))
            for j in trace_of_env]


def _check_vs_literal(b, lits, policy, steps, kl=False, arrivals=None):
    """The GPU's own heuristic actions are fed to the literals; everything a
    step returns, and counters / state at the end, must agree."""
    req0 = np.zeros(len(lits), np.int64)
    for t in range(steps):
        obs, rew, done, valid, act = b.heuristic_step(policy, want_actions=True, want_valid=True)
        obs, rew, done = obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy()
        valid, act = valid.cpu().numpy(), act.cpu().numpy()
        for i, e in enumerate(lits):
            o, r, d, v = e.step(act[i])
            assert np.array_equal(v, valid[i]), ("valid", t, i)
            assert np.array_equal(o, obs[i]), ("obs", t, i)
            assert _rew_equal([rew[i]], [r], kl), ("reward", t, i, rew[i], r)
            assert bool(done[i]) == d, ("done", t, i)
        if arrivals is not None:  # the paired-workload property
            req = b.counters().cpu().numpy()[:, 0]
            assert np.array_equal(req - req0, arrivals(t)), ("arrivals", t)
            req0 = req
    st = {k: v.cpu().numpy() for k, v in b.state().items()}
    ctr, stats = b.counters().cpu().numpy(), b.stats().cpu().numpy()
    for i, e in enumerate(lits):
        assert np.array_equal(ctr[i], e.counters()), ("counters", i, ctr[i], e.counters())
        assert np.array_equal(stats[i][[0, 3, 4]], e.stats()[[0, 3, 4]]), ("stats", i)
        for k, x in zip(STATE_KEYS, e.state()):
            assert np.array_equal(st[k][i], x), (k, i)


# ------------------------------------------------------------ 1: per-step heuristic
@pytest.mark.parametrize("policy,reward", [("firstfit", "wr"), ("firstfit", "ut"),
                                           ("bestfit", "wr"), ("bestfit", "ut"),
                                           ("bestfit", "kl")])
def test_per_step_heuristic_vs_oracle(policy, reward):
    ref = _ref(policy, reward)
    b = _traced(policy, reward)
    _check_steps(b, ref, policy, reward == "kl", 0, 200)
    _check_end(b, ref, 200)
    # stats(): the literal's, fed the same trace and the oracle's actions
    lits = _literals(dict(BASE, reward_function=reward), _traces(policy, reward), range(N))
    for t in range(200):
        for i, e in enumerate(lits):
            e.step(ref["act"][t, i])
    stats = b.stats().cpu().numpy()
    for i, e in enumerate(lits):
        assert np.array_equal(stats[i][[0, 3, 4]], e.stats()[[0, 3, 4]]), ("stats", i)
        if reward == "kl":
            assert np.array_equal(stats[i][1:3], e.stats()[1:3]), ("target means", i)
    b.close()


# ------------------------------------------------------------ 2: external actions
def test_external_actions_vs_oracle():
    ref = _ref("firstfit", "wr")
    b = _traced("firstfit", "wr")
    for t in range(100):
        a = torch.tensor(ref["act"][t], dtype=torch.int32, device=DEV)
        obs, rew, done, valid = b.step(a)
        assert np.array_equal(rew.cpu().numpy(), ref["rew"][t]), ("reward", t)
        assert np.array_equal(obs.cpu().numpy(), ref["obs"][t]), ("obs", t)
        assert np.array_equal(done.cpu().numpy(), ref["done"][t]), ("done", t)
        assert np.array_equal(valid.cpu().numpy(), ref["valid"][t]), ("valid", t)
    _check_end(b, ref, 100)
    b.close()


# ------------------------------------------------------------ 3: fused rollout
@pytest.mark.parametrize("policy", ["firstfit", "bestfit"])
def test_fused_rollout_then_headline_variant(policy):
    ref = _ref(policy, "wr")
    b = _traced(policy, "wr")
    for j in range(3):
        rs, _ = b.rollout(policy, 37)
        assert np.array_equal(rs.cpu().numpy(), ref["rew"][37 * j:37 * (j + 1)]), j
    _check_steps(b, ref, policy, False, 111, 171, full=False)
    _check_end(b, ref, 171)
    b.close()


# ------------------------------------------------------------ 4: block kernel
@pytest.mark.parametrize("policy,reward", [("firstfit", "wr"), ("bestfit", "kl")])
def test_block_kernel_forced(policy, reward, monkeypatch):
    ref = _ref(policy, reward)
    monkeypatch.setenv("VMP_BIG_KERNEL", "1")
    b = _traced(policy, reward)
    monkeypatch.delenv("VMP_BIG_KERNEL")
    _check_steps(b, ref, policy, reward == "kl", 0, 100)
    _check_end(b, ref, 100)
    b.close()


def test_block_kernel_large_v_burst():
    """A real V > 1024 handle whose step 0 carries 1 100 requests: k exceeds
    64, the event-list capacity (512) and the accepted sizes held in LDS."""
    from vmp.batched import BatchedVmEnv
    from vmp.config import Config
    from vmp.trace import Trace
    cfg = dict(BASE, pms=20, vms=1100, reward_function="wr", arrival_rate=8.0, service_length=6.0)
    rng = np.random.default_rng(3)
    traces = []
    for i in range(4):
        t = Trace.synthetic(Config(**cfg), 40, seed=i)
        n0 = 1100 if i < 2 else 700
        burst = (rng.integers(1, 101, n0), rng.integers(1, 101, n0), rng.integers(1, 9, n0))
        traces.append(Trace(np.r_[0, t.offs + n0], np.r_[burst[0], t.cpu], np.r_[burst[1], t.mem],
                            np.r_[burst[2], t.runtime]))
    b = BatchedVmEnv(Config(**cfg), 4, seeds=np.arange(4, dtype=np.int64) * 4, device=DEV)
    b.set_trace(traces, np.arange(4))
    _check_vs_literal(b, _literals(cfg, traces, range(4)), "firstfit", 30)
    assert int(b.counters()[0, 0]) >= 1100
    b.close()


# ------------------------------------------------------------ 5: generated traces
def _generated(kind):
    from vmp.config import Config
    from vmp.trace import Trace
    if kind == "drops":   # lambda 25, L 2: drops on most steps consume requests
        return [Trace.synthetic(Config(**dict(BASE, arrival_rate=25.0, service_length=2.0)), 150, s)
                for s in range(4)]
    if kind == "burst":   # 80 requests at step 0: k > 64 on the wave kernel
        out = []
        for s in range(4):
            t = Trace.synthetic(Config(**dict(BASE, arrival_rate=3.0, service_length=10.0)), 149, s)
            g = np.random.default_rng(100 + s)
            out.append(Trace(np.r_[0, t.offs + 80], np.r_[g.integers(1, 101, 80), t.cpu],
                             np.r_[g.integers(1, 101, 80), t.mem],
                             np.r_[g.integers(1, 30, 80), t.runtime]))
        return out
    if kind == "short":   # T = 40: arrivals stop, total_requests is frozen from step 40
        return [Trace.synthetic(Config(**dict(BASE, arrival_rate=4.0, service_length=30.0)), 40, s)
                for s in range(4)]
    assert kind == "empty"
    return [Trace([0], [], [], [])] + [Trace(np.zeros(s + 1, np.int64), [], [], []) for s in (1, 5, 300)]


@pytest.mark.parametrize("kind", ["drops", "burst", "short", "empty"])
@pytest.mark.parametrize("policy", ["firstfit", "bestfit"])
def test_generated_traces_vs_literal(kind, policy):
    traces = _generated(kind)
    reward = "kl" if kind == "drops" else "wr"
    b = _env(reward, n=4)
    b.set_trace(traces, np.arange(4))

    def arrivals(t):  # the same for every policy: the trace's own counts
        return np.array([tr.arrivals()[t] if t < tr.steps else 0 for tr in traces])
    _check_vs_literal(b, _literals(dict(BASE, reward_function=reward), traces, range(4)), policy,
                      150, kl=reward == "kl", arrivals=arrivals)
    ctr = b.counters().cpu().numpy()
    assert np.array_equal(ctr[:, 0], [tr.requests for tr in traces])
    if kind == "drops":
        assert np.all(ctr[:, 4] > 1000)
    b.close()


# ------------------------------------------------------------ 6: shared trace, masked reset
def test_shared_trace_and_masked_reset():
    tr = _traces("firstfit", "wr")[3]
    ref = _ref("firstfit", "wr")
    from vmp.batched import BatchedVmEnv
    b = BatchedVmEnv(_config("wr"), 8, seeds=np.arange(8, dtype=np.int64) * 7 + 1, device=DEV)
    b.set_trace(tr)  # every env replays trace 0, whatever its seed
    first = []
    for t in range(50):
        obs, rew, done, _, _ = b.heuristic_step("firstfit")
        assert np.array_equal(obs.cpu().numpy(), np.broadcast_to(ref["obs"][t, 3], (8, obs.shape[1]))), t
        assert np.all(rew.cpu().numpy() == ref["rew"][t, 3]), t
        first.append((obs[3].clone(), rew[3].clone()))
    mask = torch.zeros(8, dtype=torch.uint8)
    mask[3] = 1
    b.reset(torch.full((8,), 99, dtype=torch.int64), mask=mask)
    for t in range(50):
        obs, rew, done, _, _ = b.heuristic_step("firstfit")
        assert torch.equal(obs[3], first[t][0]) and torch.equal(rew[3], first[t][1]), t
        others = np.delete(obs.cpu().numpy(), 3, axis=0)
        assert np.array_equal(others, np.broadcast_to(ref["obs"][50 + t, 3], others.shape)), t
    b.close()


# ------------------------------------------------------------ 7: streams untouched
def test_rng_streams_rest_under_a_trace():
    from vmp.trace import Trace
    cfg = dict(BASE, reward_function="wr", arrival_rate=4.0, service_length=30.0)
    b = _env("wr", n=4, arrival_rate=4.0, service_length=30.0)
    b.set_trace(Trace([0], [], [], []))
    for _ in range(25):
        b.heuristic_step("firstfit")
    assert int(b.counters()[:, 0].sum()) == 0
    b.clear_trace()
    assert b.trace_info() is None
    oes = []
    for i in range(4):
        e = O.OracleEnv(dict(cfg, seed=4 * i))
        e.reset(4 * i)
        oes.append(e)
    for t in range(100):
        obs, rew, _, _, _ = b.heuristic_step("firstfit")
        for i, e in enumerate(oes):
            o, r, _, _ = e.step(e.firstfit())
            assert np.array_equal(obs[i].cpu().numpy(), o) and float(rew[i]) == r, (t, i)
    ctr = b.counters().cpu().numpy()
    for i, e in enumerate(oes):
        c = e.counters()[0]
        assert np.array_equal(ctr[i, :5], c[:5]) and ctr[i, 5] == c[5] + 25
    assert ctr[:, 0].min() > 0
    b.close()


# ------------------------------------------------------------ 8: arguments, failure paths
def test_arguments_and_failure_paths():
    import ctypes
    from vmp import _lib
    from vmp._lib import VmpError
    from vmp.trace import Trace
    L = _lib.lib()
    ref = _ref("firstfit", "wr")
    traces = _traces("firstfit", "wr")
    b = _env("wr")
    assert b.trace_info() is None

    def raw(offs, cpu, mem, rt, m=None, n=1):
        offs = np.asarray(offs, np.int64)
        cpu, mem = np.asarray(cpu, np.uint8), np.asarray(mem, np.uint8)
        rt = np.asarray(rt, np.uint32)
        c = (_lib.VmpTrace * n)()
        for x in c:
            x.steps = offs.size - 1
            x.offs, x.cpu, x.mem, x.runtime = (offs.ctypes.data, cpu.ctypes.data, mem.ctypes.data,
                                               rt.ctypes.data)
        mp = None if m is None else np.asarray(m, np.int32).ctypes.data_as(ctypes.c_void_p)
        return L.vmp_set_trace(b._bind(), n, ctypes.cast(c, ctypes.c_void_p), mp)

    def all_einval():
        assert raw([1, 2], [1, 1], [1, 1], [1, 1]) == EINVAL          # offs[0] != 0
        assert raw([0, 2, 1], [1, 1], [1, 1], [1, 1]) == EINVAL       # decreasing
        assert raw([0, 1], [0], [1], [1]) == EINVAL                   # size 0
        assert raw([0, 1], [1], [101], [1]) == EINVAL                 # size above 100
        assert raw([0, 1], [1], [1], [0]) == EINVAL                   # runtime 0
        assert raw([0, 1], [1], [1], [(1 << 30) + 1]) == EINVAL       # runtime above 2^30
        assert raw([0, 1], [1], [1], [1], m=[0] * (N - 1) + [1]) == EINVAL   # map out of range
        assert raw([0, 1], [1], [1], [1], m=[-1] + [0] * (N - 1)) == EINVAL
        assert L.vmp_set_trace(b._bind(), 1, None, None) == EINVAL    # null pointers
        assert L.vmp_set_trace(b._bind(), 0, None, None) == EINVAL
        c = (_lib.VmpTrace * 1)()
        c[0].steps = 1
        assert L.vmp_set_trace(b._bind(), 1, ctypes.cast(c, ctypes.c_void_p), None) == EINVAL
        assert L.vmp_set_trace(None, 1, ctypes.cast(c, ctypes.c_void_p), None) == EINVAL
    all_einval()
    assert b.trace_info() is None  # still an RNG handle
    with pytest.raises(ValueError):
        b.set_trace([])
    with pytest.raises(ValueError):
        b.set_trace(traces, np.arange(N - 1))
    # the first set_trace fails on its first and on its second device allocation
    live = L.vmp_debug_live_allocs()
    for nth in (1, 2):
        _lib.check(L.vmp_debug_fail_alloc(nth))
        with pytest.raises(VmpError) as ei:
            b.set_trace(traces, np.arange(N))
        _lib.check(L.vmp_debug_fail_alloc(0))
        assert "error %d" % EOOM in str(ei.value)
        assert L.vmp_debug_live_allocs() == live and b.trace_info() is None
    b.set_trace(traces, np.arange(N))
    assert L.vmp_debug_live_allocs() == live + 2
    _check_steps(b, ref, "firstfit", False, 0, 30)
    # failures on a traced handle leave its traces in place
    all_einval()
    _lib.check(L.vmp_debug_fail_alloc(1))
    with pytest.raises(VmpError) as ei:
        b.set_trace(traces[::-1], np.arange(N))
    _lib.check(L.vmp_debug_fail_alloc(0))
    assert "error %d" % EOOM in str(ei.value) and L.vmp_debug_live_allocs() == live + 2
    with pytest.raises(VmpError) as ei:
        b.set_workload(arrival_rate=1.0)
    assert "error %d" % ESTATE in str(ei.value)
    _check_steps(b, ref, "firstfit", False, 30, 60)
    _check_end(b, ref, 60)
    # trace_info round trip
    m = np.array([7, 6, 5, 4, 3, 2, 1, 0], np.int32)
    b.set_trace(traces, m)
    info = b.trace_info()
    assert info["n_traces"] == N and np.array_equal(info["trace_of_env"], m)
    assert np.array_equal(info["steps"], [t.steps for t in traces])
    assert np.array_equal(info["requests"], [t.requests for t in traces])
    b.set_trace(traces[2])
    info = b.trace_info()
    assert info["n_traces"] == 1 and np.all(info["trace_of_env"] == 0)
    assert L.vmp_debug_live_allocs() == live + 2
    b.clear_trace()
    assert L.vmp_debug_live_allocs() == live and b.trace_info() is None
    b.set_workload(arrival_rate=1.0)  # allowed again
    b.close()
    # a trace on a handle that has a per-env workload: dormant, then back
    w = _env("wr")
    w.set_workload(LAM, [x[1] for x in WL])
    w.set_trace(Trace([0], [], [], []))
    w.heuristic_step("firstfit")
    w.clear_trace()
    lam, _ = w.workload()
    assert np.array_equal(lam, LAM)
    w.heuristic_step("firstfit")
    w.close()


# ------------------------------------------------------------ 9: graph stability
def test_graph_survives_later_set_trace():
    ref = _ref("firstfit", "wr")
    b = _traced("firstfit", "wr")
    rew = torch.empty((10, N), dtype=torch.float64, device=DEV)
    b.heuristic_step("firstfit")  # a launch outside the capture first
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for k in range(10):
            _, r, _, _, _ = b.heuristic_step("firstfit")
            rew[k].copy_(r)
    b.reset(torch.tensor(SEEDS))
    for j in range(5):
        g.replay()
        assert np.array_equal(rew.cpu().numpy(), ref["rew"][10 * j:10 * (j + 1)]), j
    _check_end(b, ref, 50)
    # other traces, rewritten in place under the captured graph
    other = _generated("drops")
    m = np.arange(N) % 4
    b.set_trace(other, m)
    b.reset(torch.tensor(SEEDS))
    g.replay()
    g.replay()
    ctr = b.counters().cpu().numpy()
    assert np.array_equal(ctr[:, 0], [other[j].offs[20] for j in m]) and np.all(ctr[:, 5] == 21)
    lits = _literals(dict(BASE, reward_function="wr"), other, m)
    del g
    b.reset(torch.tensor(SEEDS))
    _check_vs_literal(b, lits, "firstfit", 20)
    b.close()


# ------------------------------------------------------------ 10: snapshot
def test_snapshot_restore_traced():
    from vmp import _lib
    from vmp._lib import VmpError
    ref = _ref("bestfit", "wr")
    a = _traced("bestfit", "wr")
    plain = _env("wr")
    n_plain = plain.snapshot().numel()
    _check_steps(a, ref, "bestfit", False, 0, 80)
    snap = a.snapshot()
    assert snap.numel() == n_plain  # the flag and hash live in the descriptor
    a.close()
    b = _traced("bestfit", "wr")
    b.restore(snap)
    _check_steps(b, ref, "bestfit", False, 80, 160)
    _check_end(b, ref, 160)
    b.set_trace(_traces("bestfit", "wr"), np.arange(N)[::-1].copy())  # same traces, other map
    with pytest.raises(VmpError) as ei:
        b.restore(snap)
    assert "error %d" % EINVAL in str(ei.value)
    b.set_trace(_traces("firstfit", "wr"), np.arange(N))  # other traces
    with pytest.raises(VmpError) as ei:
        b.restore(snap)
    assert "error %d" % EINVAL in str(ei.value)
    assert _lib.lib().vmp_restore(plain._bind(), _lib.ptr(snap)) == EINVAL       # traced into plain
    assert _lib.lib().vmp_restore(b._bind(), _lib.ptr(plain.snapshot())) == EINVAL  # plain into traced
    torch.cuda.synchronize()
    b.close()
    plain.close()


# ------------------------------------------------------------ 11: recorder
@pytest.mark.parametrize("fused", [False, True])
def test_recorder_summary_equals_the_rng_run(fused):
    from vmp.batched import BatchedVmEnv
    rng_env = BatchedVmEnv(_config("wr"), N, seeds=SEEDS, device=DEV, arrival_rate=LAM,
                           service_length=[x[1] for x in WL])
    tr_env = _traced("firstfit", "wr")
    out = []
    for b in (rng_env, tr_env):
        b.eval(True)
        b.reset(torch.tensor(SEEDS))
        b.record(True)
        if fused:
            b.rollout("firstfit", 150)
        else:
            for _ in range(150):
                b.heuristic_step("firstfit")
        out.append(b.record_summary())
        b.close()
    np.testing.assert_equal(out[1], out[0])
    assert any(s["total requests"] > 0 for s in out[1])


# ------------------------------------------------------------ 13: PPO
def _learn_traced():
    from vmp import ppo
    from vmp.batched import BatchedVmEnv
    from vmp.config import Config
    from vmp.trace import Trace
    cfg = Config(pms=10, vms=30, service_length=1000, arrival_rate=0.0182, training_steps=20,
                 eval_steps=100000, seed=1, reward_function="kl", cap_target_util=True,
                 sequence="uniform", beta=0.5, allow_null_action=True)
    busy = Config(**dict(cfg.__dict__, arrival_rate=1.5, service_length=15))
    traces = [Trace.synthetic(busy, 20, s) for s in range(16)]
    torch.manual_seed(0)
    env = BatchedVmEnv(cfg, 16, device=DEV)
    env.set_trace(traces, np.arange(16))
    agent = ppo.PPOAgent(env, ppo.PPOConfig(episodes=1, hidden_size=64, batch_size=20,
                                            minibatch_size=5, training_progress_bar=False))
    seen = []  # the counters every reset wipes: an episode's totals
    real = env.reset
    env.reset = lambda *a, **kw: (seen.append(env.counters().cpu().numpy()), real(*a, **kw))[1]
    rets = agent.trainer().learn()
    env.reset = real
    ctr = max(seen, key=lambda c: int(c[:, 5].sum()))
    params = torch.cat([p.detach().flatten() for p in agent.model.parameters()]).cpu()
    with pytest.raises(ValueError):
        ppo.PPOAgent(env, ppo.PPOConfig(episodes=1, hidden_size=64, batch_size=20, minibatch_size=5,
                                        training_progress_bar=False,
                                        load_range=(0.2, 1.0))).trainer()
    env.close()
    return traces, ctr, np.asarray(rets), params


def test_ppo_learns_on_a_traced_env():
    traces, ctr, rets, params = _learn_traced()
    # every env was offered its trace's requests, however the policy placed them
    steps = ctr[:, 5] - 1
    assert np.all(steps == 20)  # the episode: training_steps
    assert np.array_equal(ctr[:, 0], [t.offs[min(int(s), t.steps)] for t, s in zip(traces, steps)])
    assert ctr[:, 0].min() > 0 and len(set(rets.ravel())) > 1
    _, ctr2, rets2, params2 = _learn_traced()
    assert np.array_equal(ctr2, ctr) and np.array_equal(rets2, rets) and torch.equal(params, params2)


# ------------------------------------------------------------ 12: paired sweep, CLI
@pytest.mark.parametrize("policy", ["firstfit", "bestfit"])
def test_paired_sweep_rows_equal_untraced_runs(policy):
    from vmp import exp
    from vmp.batched import BatchedVmEnv
    traces = _traces(policy, "wr")
    cfg = dict(BASE, reward_function="wr")
    rows = exp.paired_sweep(traces, agents=(policy,), config=cfg, eval_steps=150, device=DEV)
    b = BatchedVmEnv(_config("wr"), N, seeds=SEEDS, device=DEV, arrival_rate=LAM,
                     service_length=[x[1] for x in WL])
    b.eval(True)
    b.reset(torch.tensor(SEEDS))
    b.record(True)
    b.rollout(policy, 150)
    summ = b.record_summary()
    b.close()
    assert rows == [exp.paired_row(policy, i, t, s) for i, (t, s) in enumerate(zip(traces, summ))]
    assert len(rows) == N and len({r.split(",", 4)[4] for r in rows}) > 1
    assert all(len(r.split(",")) == len(exp.PAIRED_HEADER.split(",")) for r in rows)


def test_cli_eval_replays_a_trace_file(tmp_path):
    from vmp.config import Config
    from vmp.main import Args, parse, run
    from vmp.trace import Trace
    env10 = dict(pms=10, vms=30, service_length=1000, arrival_rate=0.0182, training_steps=10000,
                 eval_steps=300, seed=1, reward_function="kl", cap_target_util=True,
                 sequence="uniform", beta=0.5, allow_null_action=True)
    t = Trace.synthetic(Config(**dict(env10, arrival_rate=0.6, service_length=25)), 200, seed=3)
    path = str(tmp_path / "t.npz")
    t.save(path)
    yml = tmp_path / "10.yml"
    yml.write_text("environment:\n" + "".join("  %s: %s\n" % kv for kv in env10.items())
                   + "agents: {}\n")
    args = parse(["-a", "firstfit", "-c", str(yml), "-r", "wr", "-e", "-s", "--trace", path,
                  "-o", str(tmp_path / "out.json")])
    assert args.trace == path and args.config["environment"]["vms"] == 30
    rec = run(args)
    assert len(rec.rewards) == 300
    assert rec.get_summary()["total requests"] == t.requests > 50
    # the config's own workload (12 requests in 1 000 steps) was not drawn from
    rec0 = run(Args(agent="firstfit", reward="wr", config=args.config, eval=True, silent=True))
    assert rec0.get_summary()["total requests"] < 20
