"""Per-env workload (vmp_set_workload, BatchedVmEnv.set_workload): one handle
whose envs run different arrival rates and service lengths, checked bit for
bit against one C oracle env per env built with that env's own pair. The
fixture mixes the three Poisson samplers (lam == 0, mult < 10, PTRS >= 10) on
both streams, sits on the lam = 10 boundary from both sides, and gives the
PTRS envs different table lengths under the one shared loggam table."""
import csv
import functools
import os

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import traj as T

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")

BASE = dict(pms=12, vms=90, allow_null_action=True, training_steps=10000, eval_steps=100000,
            seed=0, sequence="uniform", cap_target_util=True, beta=0.5,
            arrival_rate=1.0, service_length=50)
WL = [(0.0, 5.0), (0.3, 60.0), (4.0, 30.0), (12.0, 25.0), (9.99, 9.99), (10.0, 10.0),
      (2.0, 1000.0), (25.0, 2.0)]
N = len(WL)
SEEDS = np.arange(N, dtype=np.int64) * 4
LAM = np.array([w[0] for w in WL])
LEN = np.array([w[1] for w in WL])
STATE_KEYS = ("vm_placement", "vm_cpu", "vm_memory", "cpu", "memory", "vm_remaining_runtime")
EINVAL, EOOM = -1, -3


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")


def _config(reward, **over):
    from vmp.config import Config
    return Config(**dict(BASE, reward_function=reward, **over))


def _env(reward, workload=True, **over):
    from vmp.batched import BatchedVmEnv
    if workload:
        return BatchedVmEnv(_config(reward, **over), N, seeds=SEEDS, device=DEV,
                            arrival_rate=LAM, service_length=LEN)
    return BatchedVmEnv(_config(reward, **over), N, seeds=SEEDS, device=DEV)


def _oracles(base, wl, seeds):
    out = []
    for (lam, sl), s in zip(wl, seeds):
        e = O.OracleEnv(dict(base, arrival_rate=lam, service_length=sl, seed=int(s)))
        e.reset(int(s))
        out.append(e)
    return out


@functools.lru_cache(maxsize=None)
def _ref(policy, reward, steps=200):
    """`steps` heuristic steps of the fixture's N oracle envs, everything the
    tests compare, recorded once per (policy, reward) and never modified."""
    oes = _oracles(dict(BASE, reward_function=reward), WL, SEEDS)
    V, D = BASE["vms"], 3 * BASE["vms"] + 2 * BASE["pms"]
    r = dict(act=np.zeros((steps, N, V), np.int64), obs=np.zeros((steps, N, D), np.float32),
             rew=np.zeros((steps, N)), done=np.zeros((steps, N), bool),
             valid=np.zeros((steps, N, V), np.uint8), ctr=np.zeros((steps, N, 6), np.int64),
             state=[])
    for t in range(steps):
        states = []
        for i, e in enumerate(oes):
            a = e.firstfit() if policy == "firstfit" else e.bestfit()
            o, rew, done, valid = e.step(a)
            r["act"][t, i], r["obs"][t, i], r["rew"][t, i] = a, o, rew
            r["done"][t, i], r["valid"][t, i] = done, valid
            r["ctr"][t, i] = e.counters()[0]
            states.append(e.state())
        r["state"].append(states)
    for k, v in r.items():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    # the comparison is not vacuous: every env with lam > 0 receives requests
    assert np.all(r["ctr"][-1, LAM > 0, 0] > 0) and np.all(r["ctr"][-1, LAM == 0, 0] == 0)
    return r


def _rew_equal(got, exp, kl):
    """wr / ut rewards bit for bit; kl with the bound of the kl cases of
    tests/test_gpu_env.py (tests.traj.kl_close: device log / exp vs glibc)."""
    got, exp = np.asarray(got), np.asarray(exp)
    if not kl:
        return np.array_equal(got, exp)
    return all(T.kl_close(g, e) for g, e in zip(got.ravel(), exp.ravel()))


def _check_end(b, ref, t):
    """state() and counters() after t steps equal the oracle's."""
    st = {k: v.cpu().numpy() for k, v in b.state().items()}
    ctr = b.counters().cpu().numpy()
    assert np.all(ctr[LAM > 0, 0] > 0)
    for i in range(N):
        assert np.array_equal(ctr[i], ref["ctr"][t - 1, i]), ("counters", i)
        for k, x in zip(STATE_KEYS, ref["state"][t - 1][i]):
            assert np.array_equal(st[k][i], x), (k, i)


def _check_steps(b, ref, policy, kl, t0, t1, full=True):
    for t in range(t0, t1):
        obs, rew, done, valid, act = b.heuristic_step(policy, want_actions=full, want_valid=full)
        assert _rew_equal(rew.cpu().numpy(), ref["rew"][t], kl), ("reward", t)
        assert np.array_equal(obs.cpu().numpy(), ref["obs"][t]), ("obs", t)
        assert np.array_equal(done.cpu().numpy(), ref["done"][t]), ("done", t)
        if full:
            assert np.array_equal(act.cpu().numpy(), ref["act"][t]), ("actions", t)
            assert np.array_equal(valid.cpu().numpy(), ref["valid"][t]), ("valid", t)


# ------------------------------------------------------------ 1: per-step heuristic
@pytest.mark.parametrize("policy,reward", [("firstfit", "wr"), ("firstfit", "ut"),
                                           ("bestfit", "wr"), ("bestfit", "ut"),
                                           ("bestfit", "kl")])
def test_per_step_heuristic_vs_oracle(policy, reward):
    ref = _ref(policy, reward)
    b = _env(reward)
    _check_steps(b, ref, policy, reward == "kl", 0, 200)
    _check_end(b, ref, 200)
    b.close()


# ------------------------------------------------------------ 2: external actions
def test_external_actions_vs_oracle():
    """k_env_ext: the oracle's own FirstFit action fed through step()."""
    ref = _ref("firstfit", "wr")
    b = _env("wr")
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
    """k_env<VPT,false> three times, then per-step launches that ask for no
    actions or validity flags (the bit-60 / time-word-skip variant)."""
    ref = _ref(policy, "wr")
    b = _env("wr")
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
    b = _env(reward)
    monkeypatch.delenv("VMP_BIG_KERNEL")
    _check_steps(b, ref, policy, reward == "kl", 0, 100)
    _check_end(b, ref, 100)
    b.close()


def test_block_kernel_large_v():
    """A real V > 1024 handle (k_env_big without the override)."""
    from vmp.batched import BatchedVmEnv
    from vmp.config import Config
    base = dict(BASE, pms=20, vms=1100, reward_function="wr")
    wl = [(30.0, 20.0), (3.0, 20.0), (30.0, 200.0), (0.0, 20.0)]
    seeds = np.arange(4, dtype=np.int64) * 4
    lam = np.array([w[0] for w in wl])
    b = BatchedVmEnv(Config(**base), 4, seeds=seeds, device=DEV, arrival_rate=lam,
                     service_length=[w[1] for w in wl])
    oes = _oracles(base, wl, seeds)
    for t in range(60):
        obs, rew, done, valid, act = b.heuristic_step("firstfit", want_actions=True,
                                                      want_valid=True)
        obs, rew, done = obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy()
        valid, act = valid.cpu().numpy(), act.cpu().numpy()
        for i, e in enumerate(oes):
            a = e.firstfit()
            o, r, d, v = e.step(a)
            assert np.array_equal(a, act[i]) and np.array_equal(v, valid[i]), (t, i)
            assert rew[i] == r and bool(done[i]) == d and np.array_equal(o, obs[i]), (t, i)
    st = {k: v.cpu().numpy() for k, v in b.state().items()}
    ctr = b.counters().cpu().numpy()
    assert np.all(ctr[lam > 0, 0] > 0)
    for i, e in enumerate(oes):
        assert np.array_equal(ctr[i], e.counters()[0]), i
        for k, x in zip(STATE_KEYS, e.state()):
            assert np.array_equal(st[k][i], x), (k, i)
    b.close()


# ------------------------------------------------------------ 5: homogeneous equivalence
def test_homogeneous_workload_equals_untouched_handle():
    """The headline config: a handle given the config's own values for every
    env computes exactly what an untouched handle does."""
    from vmp.batched import BatchedVmEnv
    from vmp.config import Config
    cfg = Config(pms=100, vms=1000, arrival_rate=1.8182, service_length=1000,
                 training_steps=10000, eval_steps=100000, seed=0, reward_function="wr",
                 sequence="uniform", cap_target_util=True, beta=0.5, allow_null_action=True)
    a = BatchedVmEnv(cfg, 64, device=DEV)
    b = BatchedVmEnv(cfg, 64, device=DEV)
    b.set_workload(np.full(64, 1.8182), np.full(64, 1000.0))
    ra, _ = a.rollout("firstfit", 100)
    rb, _ = b.rollout("firstfit", 100)
    assert torch.equal(ra, rb)
    for _ in range(20):
        oa, wa, da, _, _ = a.heuristic_step("firstfit")
        ob, wb, db, _, _ = b.heuristic_step("firstfit")
        assert torch.equal(oa, ob) and torch.equal(wa, wb) and torch.equal(da, db)
    sa, sb = a.state(), b.state()
    for k in STATE_KEYS:
        assert torch.equal(sa[k], sb[k]), k
    assert torch.equal(a.counters(), b.counters())
    assert int(a.counters()[:, 0].min()) > 0
    a.close()
    b.close()


# ------------------------------------------------------------ 6: mid-run change
def test_mid_run_change():
    ref = _ref("firstfit", "wr")
    b = _env("wr")
    _check_steps(b, ref, "firstfit", False, 0, 50)
    b.set_workload(LAM, LEN)  # the current values: nothing changes
    _check_steps(b, ref, "firstfit", False, 50, 100)
    _check_end(b, ref, 100)
    b.set_workload(arrival_rate=0)
    lam, sl = b.workload()
    assert np.all(lam == 0) and np.array_equal(sl, LEN)
    c0 = b.counters().cpu().numpy()
    for _ in range(40):
        b.heuristic_step("firstfit")
    c1 = b.counters().cpu().numpy()
    assert np.array_equal(c1[:, 0], c0[:, 0])  # total_requests stopped at once
    assert c1[:, 1].sum() > c0[:, 1].sum()     # running VMs still finish: served grows
    assert np.all(c1[:, 1] >= c0[:, 1]) and np.all(c1[:, 5] == c0[:, 5] + 40)
    b.close()


# ------------------------------------------------------------ 7: arguments, failure paths
def test_arguments_and_failure_paths():
    from vmp import _lib
    from vmp._lib import VmpError
    L = _lib.lib()
    ref = _ref("firstfit", "wr")
    b = _env("wr", workload=False, arrival_rate=WL[2][0], service_length=WL[2][1])
    lam, sl = b.workload()
    assert np.all(lam == WL[2][0]) and np.all(sl == WL[2][1])  # the config's values
    for bad in (-1.0, float("nan"), float("inf")):
        for kw in ("arrival_rate", "service_length"):
            x = LAM.copy()
            x[3] = bad
            with pytest.raises(VmpError) as ei:
                b.set_workload(**{kw: x})
            assert "error %d" % EINVAL in str(ei.value)
    with pytest.raises((ValueError, VmpError)):
        b.set_workload(arrival_rate=np.ones(N + 1))
    with pytest.raises((ValueError, VmpError)):
        b.set_workload(service_length=np.ones(N - 1))
    # the first set_workload fails on its first device allocation
    live = L.vmp_debug_live_allocs()
    _lib.check(L.vmp_debug_fail_alloc(1))
    with pytest.raises(VmpError) as ei:
        b.set_workload(LAM, LEN)
    _lib.check(L.vmp_debug_fail_alloc(0))
    assert "error %d" % EOOM in str(ei.value)
    assert L.vmp_debug_live_allocs() == live
    lam, sl = b.workload()
    assert np.all(lam == WL[2][0]) and np.all(sl == WL[2][1])
    # ... and the handle goes on stepping with the config's workload: env 2 of
    # the fixture has exactly that pair (and seed 8)
    b.reset(torch.full((N,), int(SEEDS[2]), dtype=torch.int64))
    for t in range(30):
        obs, rew, _, _, _ = b.heuristic_step("firstfit")
        assert np.all(rew.cpu().numpy() == ref["rew"][t, 2]), t
        assert np.array_equal(obs[5].cpu().numpy(), ref["obs"][t, 2]), t
    # round trip, bit for bit (values that are not exact in binary)
    x = np.array([0.1, 1 / 3, 9.99, 10.0, 1e-300, 123.456, 0.0, 7.0])
    y = np.array([1e3, 2 / 3, 0.0, 10.000000000000002, 5.0, 1.5, 1e-5, 9.999999999999998])
    b.set_workload(x, y)
    lam, sl = b.workload()
    assert lam.dtype == np.float64 and sl.dtype == np.float64
    assert lam.tobytes() == x.tobytes() and sl.tobytes() == y.tobytes()
    b.set_workload(service_length=3.0)  # a scalar; the other quantity is kept
    lam, sl = b.workload()
    assert lam.tobytes() == x.tobytes() and np.all(sl == 3.0)
    b.close()


# ------------------------------------------------------------ 8: snapshot
def test_snapshot_restore_with_workload():
    from vmp import _lib
    from vmp._lib import VmpError
    ref = _ref("bestfit", "wr")
    a = _env("wr")
    plain = _env("wr", workload=False)
    n_plain = plain.snapshot().numel()
    _check_steps(a, ref, "bestfit", False, 0, 80)
    snap = a.snapshot()
    assert snap.numel() == n_plain + 16 * N  # f64 [N][2] appended; plain handles keep their size
    a.close()
    b = _env("wr")
    b.restore(snap)
    _check_steps(b, ref, "bestfit", False, 80, 160)
    _check_end(b, ref, 160)
    # another workload
    b.set_workload(service_length=LEN + 1.0)
    with pytest.raises(VmpError) as ei:
        b.restore(snap)
    assert "error %d" % EINVAL in str(ei.value)
    b.close()
    # none: the C entry point itself refuses it (it reads the descriptor only)
    rc = _lib.lib().vmp_restore(plain._bind(), _lib.ptr(snap))
    assert rc == EINVAL
    # ... and a plain snapshot into a handle with a workload
    c = _env("wr")
    rc = _lib.lib().vmp_restore(c._bind(), _lib.ptr(plain.snapshot()))
    assert rc == EINVAL
    torch.cuda.synchronize()
    c.close()
    plain.close()


# ------------------------------------------------------------ 9: graph stability
def test_graph_survives_later_set_workload():
    ref = _ref("firstfit", "wr")
    b = _env("wr")
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
    c0 = b.counters().cpu().numpy()
    b.set_workload(arrival_rate=0)  # rewrites the per-env array in place
    g.replay()
    g.replay()
    c1 = b.counters().cpu().numpy()
    assert np.array_equal(c1[:, 0], c0[:, 0]) and np.all(c1[:, 5] == c0[:, 5] + 20)
    del g
    b.close()


# ------------------------------------------------------------ 10: merged sweep
def test_merged_suspension_sweep_rows_match_published(monkeypatch):
    from vmp import exp
    with open(os.path.join(GOLDEN, "exp_suspension_data.csv")) as f:
        pub = {(r[0], r[1], r[2]): ",".join(x.strip() for x in r) for r in csv.reader(f)}
    made = []
    real = exp.BatchedVmEnv

    def counting(*a, **kw):
        made.append(a[1])
        return real(*a, **kw)
    monkeypatch.setattr(exp, "BatchedVmEnv", counting)
    rows = exp.suspension_sweep(agents=("firstfit", "bestfit"), loads=[0.5], lengths=[100],
                                merge=True)
    assert made == [2, 2]  # two handles of two envs instead of four of one
    assert len(rows) == 4
    for row in rows:
        a, ld, sr = row.split(",")[:3]
        assert row == pub[(a, ld, sr)], (row, pub[(a, ld, sr)])


# ------------------------------------------------------------ 11: PPO
def _learn_once():
    from vmp import ppo
    from vmp.batched import BatchedVmEnv
    from vmp.config import Config
    cfg = Config(pms=10, vms=30, service_length=1000, arrival_rate=0.0182, training_steps=20,
                 eval_steps=100000, seed=1, reward_function="kl", cap_target_util=True,
                 sequence="uniform", beta=0.5, allow_null_action=True)
    torch.manual_seed(0)
    env = BatchedVmEnv(cfg, 16, device=DEV)
    agent = ppo.PPOAgent(env, ppo.PPOConfig(episodes=1, hidden_size=64, batch_size=20,
                                            minibatch_size=5, training_progress_bar=False,
                                            load_range=(0.2, 1.0)))
    tr = agent.trainer()
    seen = []
    real = env.set_workload
    env.set_workload = lambda *a, **kw: (seen.append(kw["arrival_rate"].copy()), real(*a, **kw))
    rets = tr.learn()
    lam, sl = env.workload()
    params = torch.cat([p.detach().flatten() for p in agent.model.parameters()]).cpu()
    env.close()
    return seen, lam, sl, np.asarray(rets), params


def test_ppo_load_range():
    from vmp import ppo
    seen, lam, sl, rets, params = _learn_once()
    # episode 0's loads before its reset, episode 1's when episode 0 ends
    assert len(seen) == 2
    for ep in (0, 1):
        loads = np.random.default_rng([1, ep, 0]).uniform(0.2, 1.0, 16)
        assert np.array_equal(ppo.episode_loads(1, ep, 0, 16, (0.2, 1.0)), loads)
        assert np.array_equal(seen[ep], 10 / 0.55 / 1000 * loads), ep
    assert lam.tobytes() == seen[1].tobytes() and np.all(sl == 1000.0)
    assert rets.shape == (1, 16) and len(set(rets[0])) > 1
    seen2, lam2, _, rets2, params2 = _learn_once()
    assert lam2.tobytes() == lam.tobytes() and np.array_equal(rets2, rets)
    assert torch.equal(params, params2)
