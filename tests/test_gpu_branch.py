"""vmp_branch / BatchedVmEnv.branch on the GPU against tests/branch_literal.py
(snapshot bytes), against the source env and the C oracle (continuation),
against numpy's own generators (reseeding), tests/trace_literal.py (another
trace on the target) and twin handles (observers, graph replay).

Common setup: src has 7 envs and dst 5 (neither a multiple of 4), seeds 4 i,
arrival rate V / 4 and service length 8 as in tests/test_gpu_series.py (whose
docstring records that this workload fills, finishes and drops within 60
steps, checked on the CPU with the oracle); src is advanced 40 FirstFit steps
and dst 25 BestFit steps, so a kept env differs from every source env. Shapes:
one slot row; a padded pitch with P over two bitmap words; full rows; the
block kernel (V > 1024, more than one 16-byte-unit chunk boundary inside the
VM row)."""
import ctypes
import gc

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import branch_literal as BL
from tests import trace_literal as TL

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NS, ND = 7, 5
SHAPES = [(10, 30), (130, 300), (100, 1000), (20, 1100)]
BASE = dict(allow_null_action=True, training_steps=10000, eval_steps=100000, seed=0,
            sequence="uniform", cap_target_util=True, beta=0.3, service_length=8)
MAP = [3, -1, 0, 3, 6]
KEYS = ("vm_placement", "vm_cpu", "vm_memory", "cpu", "memory", "vm_remaining_runtime")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")


def _cfg(P, V, reward="wr", **over):
    return dict(dict(BASE, pms=P, vms=V, arrival_rate=V / 4.0, reward_function=reward), **over)


def _env(cfg, n, **kw):
    from vmp.batched import BatchedVmEnv
    from vmp.config import Config
    return BatchedVmEnv(Config(**cfg), n, seeds=np.arange(n, dtype=np.int64) * 4, device=DEV, **kw)


def _advance(b, policy, steps):
    """Per-step launches without actions or validity flags: the launches that
    write and read the step hints."""
    for _ in range(steps):
        b.heuristic_step(policy, want_obs=False)


def _pair(cfg, traces=None):
    src, dst = _env(cfg, NS), _env(cfg, ND)
    if traces is not None:
        src.set_trace(traces[0])
        dst.set_trace(traces[1])
    _advance(src, "firstfit", 40)
    _advance(dst, "bestfit", 25)
    return src, dst


def _bytes(b):
    return b.snapshot().cpu().numpy()


def _assert_bytes(got, want, n, P, V, what):
    bad = np.flatnonzero(got != want)
    ends = np.array(BL.parts(n, P, V))
    assert bad.size == 0, (what, bad.size, bad[:8], [int(np.searchsorted(ends, o, "right")) for o in bad[:8]])


def _rows_equal(dst, i, src, s, what):
    """env i of dst and env s of src hold the same three rows of snapshot bytes."""
    for a, b, part in zip(BL.rows(_bytes(dst), dst.n_envs, dst.P, dst.V),
                          BL.rows(_bytes(src), src.n_envs, src.P, src.V), ("hdr", "pm", "vmw")):
        assert np.array_equal(a[i], b[s]), (what, part, i, s)


# ------------------------------------------------------------------ bytes
@pytest.mark.parametrize("P,V", SHAPES)
def test_bytes_equal_the_literal(P, V):
    src, dst = _pair(_cfg(P, V))
    s0, d0 = _bytes(src), _bytes(dst)
    assert not np.array_equal(BL.rows(s0, NS, P, V)[0][:ND], BL.rows(d0, ND, P, V)[0])
    # host lists, with seeds: a reseeded copy, two copies of one env, a kept env with a seed
    seeds = [-1, 5, 9, 9, -1]
    dst.branch(src, MAP, seeds)
    d1 = _bytes(dst)
    _assert_bytes(d1, BL.branch(s0, d0, NS, ND, P, V, MAP, seeds), ND, P, V, "between handles")
    _assert_bytes(_bytes(src), s0, NS, P, V, "the source is untouched")
    # out of range on both sides, from device tensors (the host cannot see them): kept
    m = torch.tensor([NS, 2, -5, -1, 1 << 30], dtype=torch.int32, device=DEV)
    sd = torch.tensor([3, -7, 3, 3, 3], dtype=torch.int64, device=DEV)
    dst.branch(src, m, sd)
    d2 = _bytes(dst)
    _assert_bytes(d2, BL.branch(s0, d1, NS, ND, P, V, m.cpu().numpy(), sd.cpu().numpy()), ND, P, V,
                  "out-of-range entries")
    assert np.array_equal(BL.rows(d2, ND, P, V)[2][1], BL.rows(s0, NS, P, V)[2][2])
    # in place: overlaps (2 -> 0 and 1 while 0 -> 2), a swap (5 <-> 6), one env to several
    inplace = [2, 2, 0, 1, 1, 6, 5]
    src.branch(src, inplace)
    s1 = _bytes(src)
    _assert_bytes(s1, BL.branch(s0, s0, NS, NS, P, V, inplace), NS, P, V, "in place")
    # ... again with out-of-range entries, a reseed, and the swap undone
    m = torch.tensor([NS, -5, -1, 0, 4, 6, 5], dtype=torch.int32, device=DEV)
    sd = torch.tensor([1, 1, 1, 12, -1, -1, -1], dtype=torch.int64, device=DEV)
    src.branch(src, m, sd)
    _assert_bytes(_bytes(src), BL.branch(s1, s1, NS, NS, P, V, m.cpu().numpy(), sd.cpu().numpy()),
                  NS, P, V, "in place, out of range")
    src.close()
    dst.close()


def test_host_arguments_are_range_checked():
    src, dst = _env(_cfg(10, 30), NS), _env(_cfg(10, 30), ND)
    for bad in ([0, 1, 2, 3, NS], [0, 1, 2, 3, -2], [0, 1, 2, 3], [[0, 1, 2, 3, 4]],
                [0.5, 1, 2, 3, 4], np.array([0, 1, 2, 3, NS]), torch.tensor([0, 1, 2, 3, -2])):
        with pytest.raises(ValueError):
            dst.branch(src, bad)
    with pytest.raises(ValueError):
        dst.branch(src, MAP, seeds=[1, 2, 3])
    with pytest.raises(ValueError):
        dst.branch(src, torch.zeros(ND + 1, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        dst.branch("src", MAP)
    src.close()
    dst.close()


# ----------------------------------------------------------- continuation
def _oracles(cfg, envs, pre_steps):
    out = []
    for s in envs:
        e = O.OracleEnv(dict(cfg, seed=4 * s))
        e.reset(4 * s)
        for _ in range(pre_steps):
            e.step(e.firstfit())
        out.append(e)
    return out


def _close(a, b):
    return a == b or abs(a - b) <= 1e-12 * max(1.0, abs(b))


@pytest.mark.parametrize("driver", ["heuristic_step", "rollout", "step"])
@pytest.mark.parametrize("P,V", SHAPES)
def test_copies_continue_as_their_sources(P, V, driver):
    """dst env i and src env MAP[i] give bit-equal obs, reward, done and
    counters for 30 steps, and dst equals an OracleEnv seeded as the source
    env and replayed to the same age (obs bit for bit; the reward within the
    project's 1e-12, as __graft_entry__.smoke holds the kl reward)."""
    cfg = _cfg(P, V, "kl")
    src, dst = _pair(cfg)
    dst.branch(src, MAP)
    pairs = [(i, s) for i, s in enumerate(MAP) if s >= 0]
    for i, s in pairs:
        _rows_equal(dst, i, src, s, "after the branch")
    oes = _oracles(cfg, [s for _, s in pairs], 40)
    g = np.random.default_rng(7)
    T = 30
    if driver == "rollout":
        rs, _ = src.rollout("firstfit", T)
        rd, dd = dst.rollout("firstfit", T)
        rs, rd = rs.cpu().numpy(), rd.cpu().numpy()
        for (i, s), e in zip(pairs, oes):
            assert np.array_equal(rd[:, i], rs[:, s]), (i, s)
            for t in range(T):
                _, r, _, _ = e.step(e.firstfit())
                assert _close(rd[t, i], r), (t, i, rd[t, i], r)
    else:
        for t in range(T):
            if driver == "heuristic_step":
                # no actions, no validity flags: the variant that takes the hint-driven paths
                os_, rs, ds, _, _ = src.heuristic_step("firstfit")
                od, rd, dd, _, _ = dst.heuristic_step("firstfit")
                acts = None
            else:
                pl = src.state()["vm_placement"].cpu().numpy()
                a = pl.copy()
                draw = g.random(a.shape) < 0.5
                a[draw] = g.integers(0, P + 2, int(draw.sum()))
                ad = dst.state()["vm_placement"].cpu().numpy()
                for i, s in pairs:
                    ad[i] = a[s]
                acts = a
                os_, rs, ds, vs = src.step(torch.tensor(a, dtype=torch.int32, device=DEV))
                od, rd, dd, vd = dst.step(torch.tensor(ad, dtype=torch.int32, device=DEV))
                for i, s in pairs:
                    assert torch.equal(vd[i], vs[s]), ("valid", t, i)
            cs, cd = src.counters(), dst.counters()
            for (i, s), e in zip(pairs, oes):
                assert torch.equal(od[i], os_[s]), ("obs", t, i)
                assert torch.equal(rd[i], rs[s]) and torch.equal(dd[i], ds[s]), ("reward", t, i)
                assert torch.equal(cd[i], cs[s]), ("counters", t, i)
                o, r, d, _ = e.step(e.firstfit() if acts is None else acts[s])
                assert np.array_equal(od[i].cpu().numpy(), o), ("oracle obs", t, i)
                assert _close(float(rd[i]), r) and bool(dd[i]) == d, ("oracle reward", t, i)
    cd = dst.counters().cpu().numpy()
    sd = {k: v.cpu().numpy() for k, v in dst.state().items()}
    for (i, s), e in zip(pairs, oes):
        assert np.array_equal(cd[i], e.counters()[0]), ("oracle counters", i)
        for j, k in enumerate(KEYS):
            assert np.array_equal(sd[k][i], e.state()[j]), ("oracle state", k, i)
        _rows_equal(dst, i, src, s, "after %d steps" % T)
    src.close()
    dst.close()


def test_headline_config_quiet_envs_continue():
    """P100 / V1000, lambda 1.8182, L 1000 at age 2 500, where
    profiles/idle_step_stats.txt finds 0.998 of the env-steps quiet: the hint
    word travels with the state. The fast-forward is fused rollouts and then a
    few per-step launches, which are the ones that write the quiet bit."""
    cfg = dict(BASE, pms=100, vms=1000, arrival_rate=1.8182, service_length=1000,
               reward_function="kl")
    n = 8
    src, dst = _env(cfg, n), _env(cfg, n)
    src.rollout("firstfit", 2496)
    _advance(src, "firstfit", 4)
    pad = BL.hdr_words(_bytes(src), n, 100, 1000)[:, BL.W_PAD]
    ts = BL.hdr_words(_bytes(src), n, 100, 1000)[:, BL.W_TIMESTEP]
    print("pad words: " + " ".join("%016x" % int(x) for x in pad))
    assert np.all(ts == 2501)
    assert np.any((pad >> np.uint64(62)) & np.uint64(1)), "no source env carries the quiet bit"
    m = [7, 6, 5, 4, 3, 2, 1, 0]
    dst.branch(src, m)
    for t in range(100):
        os_, rs, ds, _, _ = src.heuristic_step("firstfit")
        od, rd, dd, _, _ = dst.heuristic_step("firstfit")
        ix = torch.tensor(m, device=DEV)
        assert torch.equal(od, os_[ix]) and torch.equal(rd, rs[ix]) and torch.equal(dd, ds[ix]), t
    assert torch.equal(dst.counters(), src.counters()[ix])
    for i, s in enumerate(m):
        _rows_equal(dst, i, src, s, "final")
    src.close()
    dst.close()


# ---------------------------------------------------------------- reseed
def _run_and_collect(b, steps):
    """Per step and env: the requests offered and the (slot-ordered) sizes and
    runtimes of the VMs accepted. A slot is a new arrival iff it stands at
    WAIT after the step and did not after the action phase (the rule of
    tests/trace_literal.derive_trace)."""
    n = b.n_envs
    offered = np.zeros((steps, n), np.int64)
    cpu, mem, rt = ([[] for _ in range(n)] for _ in range(3))
    st = {k: v.cpu().numpy() for k, v in b.state().items()}
    tot = b.counters().cpu().numpy()[:, 0]
    for t in range(steps):
        _, _, _, valid, act = b.heuristic_step("firstfit", want_actions=True, want_valid=True)
        valid, act = valid.cpu().numpy(), act.cpu().numpy()
        mid = np.where(valid != 0, act, st["vm_placement"])
        st = {k: v.cpu().numpy() for k, v in b.state().items()}
        c = b.counters().cpu().numpy()[:, 0]
        offered[t] = c - tot
        tot = c
        for i in range(n):
            new = np.flatnonzero((st["vm_placement"][i] == b.P) & (mid[i] != b.P))
            cpu[i] += st["vm_cpu"][i][new].tolist()
            mem[i] += st["vm_memory"][i][new].tolist()
            rt[i] += st["vm_remaining_runtime"][i][new].tolist()
    return offered, cpu, mem, rt


def _assert_fresh_streams(seed, rate, L, offered, cpu, mem, rt, skip_sizes=0, skip_steps=0, skip_rt=0):
    """What numpy's four generators of reset(seed) give (env.py:172-178, 271-293)."""
    n = len(cpu)
    assert n > 0, "no VM was accepted: the check would be empty"
    assert np.array_equal(offered,
                          np.random.default_rng(seed + 2).poisson(rate, skip_steps + len(offered))[skip_steps:])
    assert np.array_equal(cpu, np.around(np.random.default_rng(seed).uniform(0.1, 1.0, skip_sizes + n), 2)[skip_sizes:])
    assert np.array_equal(mem, np.around(np.random.default_rng(seed + 1).uniform(0.1, 1.0, skip_sizes + n), 2)[skip_sizes:])
    assert np.array_equal(rt, (np.random.default_rng(seed + 3).poisson(L, skip_rt + n) + 1)[skip_rt:])


@pytest.mark.parametrize("P,V", SHAPES)
def test_reseeded_copies_draw_from_numpys_generators(P, V):
    cfg = _cfg(P, V)
    src, dst = _pair(cfg)
    seeds = [11, 11, 23, -1, 40]
    dst.branch(src, [0] * ND, seeds)
    T = 30
    offered, cpu, mem, rt = _run_and_collect(dst, T)
    for i, s in enumerate(seeds):
        if s >= 0:
            _assert_fresh_streams(s, V / 4.0, 8, offered[:, i], cpu[i], mem[i], rt[i])
    # equal seeds: equal trajectories; other seeds: others
    _rows_equal(dst, 1, dst, 0, "equal seeds")
    assert not np.array_equal(offered[:, 2], offered[:, 0])
    # the -1 env is src env 0 continuing
    for _ in range(T):
        src.heuristic_step("firstfit", want_actions=True, want_valid=True)
    _rows_equal(dst, 3, src, 0, "kept streams")
    src.close()
    dst.close()


def test_reset_without_seed_restarts_the_sequence_behind_the_new_base():
    """eval_steps = training_steps = 50, so M2 = 100: after reset(seeds=None) the
    sizes of a reseeded env go on at draw 100 of default_rng(s) / (s + 1), while
    the arrival and runtime streams continue where they stood."""
    P, V = 10, 30
    cfg = _cfg(P, V, training_steps=50, eval_steps=50)
    src, dst = _pair(cfg)
    s = 17
    dst.branch(src, [2, -1, -1, -1, -1], [s, -1, -1, -1, -1])
    off1, cpu1, mem1, rt1 = _run_and_collect(dst, 6)
    _assert_fresh_streams(s, V / 4.0, 8, off1[:, 0], cpu1[0], mem1[0], rt1[0])
    mask = torch.tensor([1, 0, 0, 0, 0], dtype=torch.uint8, device=DEV)
    dst.reset(seeds=None, mask=mask)
    assert int(dst.counters()[0, 5]) == 1
    off2, cpu2, mem2, rt2 = _run_and_collect(dst, 6)
    _assert_fresh_streams(s, V / 4.0, 8, off2[:, 0], cpu2[0], mem2[0], rt2[0], skip_sizes=100,
                          skip_steps=6, skip_rt=len(rt1[0]))
    src.close()
    dst.close()


# ---------------------------------------------------------------- traces
def _traces(cfg):
    from vmp.config import Config
    from vmp.trace import Trace
    return Trace.synthetic(Config(**cfg), 90, 1), Trace.synthetic(Config(**cfg), 90, 2)


def test_traced_copy_continues_on_the_same_trace():
    cfg = _cfg(130, 300)
    ta, _ = _traces(cfg)
    src, dst = _pair(cfg, (ta, ta))
    dst.branch(src, MAP)
    for t in range(30):
        os_, rs, ds, _, _ = src.heuristic_step("firstfit")
        od, rd, dd, _, _ = dst.heuristic_step("firstfit")
        for i, s in enumerate(MAP):
            if s >= 0:
                assert torch.equal(od[i], os_[s]) and torch.equal(rd[i], rs[s]), (t, i)
    cs, cd = src.counters(), dst.counters()
    for i, s in enumerate(MAP):
        if s >= 0:
            assert torch.equal(cd[i], cs[s])
            _rows_equal(dst, i, src, s, "traced")
    assert int(cs[0, 0]) == int(ta.offs[70])  # every request of 70 steps was offered
    src.close()
    dst.close()


def test_traced_copy_replays_the_targets_own_trace():
    """dst replays another trace: a copied env is offered dst's trace at the
    copied timestep. tests/trace_literal.TraceEnv, started from the state the
    device holds after the branch and fed the device's actions, gives every
    step's obs, reward and counters."""
    P, V = 130, 300
    cfg = _cfg(P, V)
    ta, tb = _traces(cfg)
    src, dst = _pair(cfg, (ta, tb))
    dst.branch(src, MAP)
    st = {k: v.cpu().numpy() for k, v in dst.state().items()}
    ctr, sts = dst.counters().cpu().numpy(), dst.stats().cpu().numpy()
    lits = {}
    for i, s in enumerate(MAP):
        if s < 0:
            continue
        assert ctr[i, 5] == 41
        e = TL.TraceEnv(cfg, tb.offs, tb.cpu, tb.mem, tb.runtime)
        for k in TL.STATE_KEYS:
            setattr(e, k, st[k][i].copy())
        (e.total_requests, e.served, e.suspend_action, e.place_action, e.dropped,
         e.timestep) = (int(x) for x in ctr[i])
        (e.waiting_ratio, e.tcm, e.tmm, e.total_cpu_requested,
         e.total_memory_requested) = (float(x) for x in sts[i])
        lits[i] = e
    offered = {i: [] for i in lits}
    for t in range(25):
        obs, rew, done, valid, act = dst.heuristic_step("firstfit", want_actions=True, want_valid=True)
        obs, rew, act = obs.cpu().numpy(), rew.cpu().numpy(), act.cpu().numpy()
        ctr = dst.counters().cpu().numpy()
        for i, e in lits.items():
            before = e.total_requests
            o, r, d, v = e.step(act[i])
            assert np.array_equal(obs[i], o), (t, i)
            assert rew[i] == r and np.array_equal(valid[i].cpu().numpy(), v), (t, i)
            assert np.array_equal(ctr[i], e.counters()), (t, i)
            offered[i].append(e.total_requests - before)
    for i in lits:  # timestep 41 is trace step 40
        assert offered[i] == np.diff(tb.offs)[40:65].tolist() and sum(offered[i]) > 0
    assert not np.array_equal(np.diff(ta.offs)[40:65], np.diff(tb.offs)[40:65])
    src.close()
    dst.close()


def test_traced_and_plain_do_not_mix():
    from vmp._lib import VmpError
    cfg = _cfg(10, 30)
    ta, _ = _traces(cfg)
    a, b = _env(cfg, NS), _env(cfg, ND)
    a.set_trace(ta)
    before = _bytes(a), _bytes(b)
    for dst, src, n in ((b, a, ND), (a, b, NS)):
        with pytest.raises(VmpError, match="libvmp error -4"):
            dst.branch(src, [0] * n)
    assert np.array_equal(_bytes(a), before[0]) and np.array_equal(_bytes(b), before[1])
    a.close()
    b.close()


# ------------------------------------------------------------- observers
def _observe(b):
    b.record(True)
    b.request_log(capacity=20000)  # ids are ordinals since the reset: 61 steps of V / 4 fit
    b.series(capacity=40, pm_rows=True)


def _readings(b):
    hist, sums = b.record_read()
    rq, sr = b.request_log_read(), b.series_read()
    return dict(hist=hist.cpu().numpy(), sums=sums.cpu().numpy(), rq_rows=rq.rows, rq_meta=rq.meta,
                sr_rows=sr.rows, sr_meta=sr.meta, sr_pm=sr.pm)


@pytest.mark.parametrize("P,V", [(130, 300), (20, 1100)])
def test_observers_restart_for_overwritten_envs_only(P, V):
    """dst has the recorder, the request log and the series on. After a branch
    the overwritten envs read back as those of a twin restored to the same
    bytes (vmp_restore restarts every env's observers) and stepped alike; the
    kept env reads back as that of a twin that made the same steps and was
    never branched. The recorder's VMP_REC_XMEM sums over the handle's envs, so
    it is compared where all envs hold the same state (the restored twin)."""
    cfg = _cfg(P, V)
    src = _env(cfg, NS)
    _advance(src, "firstfit", 40)
    dst, kept = _env(cfg, ND), _env(cfg, ND)
    for b in (dst, kept):
        _advance(b, "bestfit", 15)
        _observe(b)
        _advance(b, "bestfit", 10)
    dst.branch(src, MAP)
    twin = _env(cfg, ND)
    _observe(twin)
    twin.restore(dst.snapshot())
    for b in (dst, kept, twin):
        _advance(b, "firstfit", 20)
    rd, rk, rt = _readings(dst), _readings(kept), _readings(twin)
    for i, s in enumerate(MAP):
        ref = rt if s >= 0 else rk
        for key in rd:
            x, y = rd[key][i], ref[key][i]
            if key == "sums" and s < 0:
                x, y = x[:18], y[:18]
            assert np.array_equal(x, y), (key, i, s)
    # the kept env's observers went on: they hold the 10 steps before the branch too
    assert rd["sr_meta"][1].tolist() == [16, 30, 0] and rd["sr_meta"][0].tolist() == [41, 20, 0]
    assert rd["sums"][1, 0] == 30 and rd["sums"][0, 0] == 20
    for b in (src, dst, kept, twin):
        b.close()


# ---------------------------------------------------------------- errors
def test_refusals_leave_both_handles_usable_and_nothing_allocated():
    from vmp._lib import VmpError, lib
    gc.collect()
    torch.cuda.synchronize()
    lib().vmp_debug_live_allocs.restype = ctypes.c_int64
    base = lib().vmp_debug_live_allocs()
    cfg = _cfg(10, 30)
    dst = _env(cfg, ND)
    _advance(dst, "bestfit", 25)
    d0 = _bytes(dst)
    others = [_env(_cfg(11, 30), NS), _env(_cfg(10, 31), NS), _env(_cfg(10, 30, "ut"), NS)]
    for o in others:
        _advance(o, "firstfit", 5)
        o0 = _bytes(o)
        for a, b, n in ((dst, o, ND), (o, dst, NS)):
            with pytest.raises(VmpError, match="libvmp error -1"):
                a.branch(b, [0] * n)
        assert np.array_equal(_bytes(dst), d0) and np.array_equal(_bytes(o), o0)
    # both sides step on as the oracle does
    for b, c, pre, pol in ((dst, cfg, 25, "bestfit"), (others[2], _cfg(10, 30, "ut"), 5, "firstfit")):
        e = O.OracleEnv(dict(c, seed=4))
        e.reset(4)
        for _ in range(pre):
            e.step(getattr(e, pol)())
        for t in range(10):
            obs, rew, _, _, _ = b.heuristic_step("firstfit")
            o, r, _, _ = e.step(e.firstfit())
            assert np.array_equal(obs[1].cpu().numpy(), o) and _close(float(rew[1]), r), t
    # the in-place staging and the observers' mask are the handle's: freed with it
    live = lib().vmp_debug_live_allocs()
    dst.branch(dst, [1, 0, 3, 2, 4])
    assert lib().vmp_debug_live_allocs() == live + 1
    dst.branch(dst, [1, 0, 3, 2, 4])
    assert lib().vmp_debug_live_allocs() == live + 1
    dst.series(capacity=8)
    live = lib().vmp_debug_live_allocs()
    dst.branch(dst, [1, 0, 3, 2, 4])
    assert lib().vmp_debug_live_allocs() == live + 1
    # a failed staging allocation: VMP_EOOM, the handle as it was
    o = others[2]
    o0 = _bytes(o)
    lib().vmp_debug_fail_alloc(1)
    try:
        with pytest.raises(VmpError, match="libvmp error -3"):
            o.branch(o, [1, 0, 2, 3, 4, 5, 6])
    finally:
        lib().vmp_debug_fail_alloc(0)
    assert np.array_equal(_bytes(o), o0)
    o.branch(o, [1, 0, 2, 3, 4, 5, 6])
    assert np.array_equal(BL.rows(_bytes(o), NS, 10, 30)[0][0], BL.rows(o0, NS, 10, 30)[0][1])
    for b in others + [dst]:
        b.close()
    assert lib().vmp_debug_live_allocs() == base


# ----------------------------------------------------------------- graph
def test_branch_and_rollout_replay_in_a_graph():
    P, V, K = 130, 300, 8
    src, dst = _pair(_cfg(P, V))
    eager = _env(_cfg(P, V), ND)
    m = torch.tensor(MAP, dtype=torch.int32, device=DEV)
    sd = torch.tensor([-1, 5, 9, 9, -1], dtype=torch.int64, device=DEV)
    rew = torch.empty((K, ND), dtype=torch.float64, device=DEV)
    dc = torch.zeros(ND, dtype=torch.int64, device=DEV)
    dst.branch(src, m, sd)  # launches outside the capture first
    dst.rollout("firstfit", K, rewards=rew, done_count=dc)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dst.branch(src, m, sd)
        dst.rollout("firstfit", K, rewards=rew, done_count=dc)
    eager.restore(dst.snapshot())
    for maps in (MAP, [-1, 6, 6, 0, NS]):
        m.copy_(torch.tensor(maps, dtype=torch.int32))
        g.replay()
        eager.branch(src, m.clone(), sd.clone())
        want, _ = eager.rollout("firstfit", K)
        assert torch.equal(rew, want), maps
        _assert_bytes(_bytes(dst), _bytes(eager), ND, P, V, "replay %s" % (maps,))
    for b in (src, dst, eager):
        b.close()
