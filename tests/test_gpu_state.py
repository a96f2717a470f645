"""vmp_set_state / BatchedVmEnv.set_state on the GPU against
tests/state_literal.py (snapshot bytes and status codes), against twin handles
(identity imports continue bit for bit, observers, graph replay), against
tests/trace_literal.py (hand-made states under a hand-made trace) and against
numpy's own generators (reseeding).

Shapes (P, V): one slot row; a full row; one slot past it; 5 blocks padded to
8; the widest wave kernel; the block kernel's first V and one with a ragged
last block; and once the project's largest config, P 1000 / V 10000."""
import ctypes
import gc

import numpy as np
import pytest
import torch

from tests import branch_literal as BL
from tests import state_literal as SL
from tests import trace_literal as TL
from tests.env_cases import ext_actions

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = 6
SHAPES = [(3, 5), (4, 64), (4, 65), (100, 300), (7, 1024), (7, 1025), (20, 2049)]
REWARDS = ("wr", "ut", "kl")
BASE = dict(allow_null_action=True, training_steps=10000, eval_steps=100000, seed=0,
            sequence="uniform", cap_target_util=True, beta=0.3, service_length=8)
KEYS = ("vm_placement", "vm_cpu", "vm_memory", "cpu", "memory", "vm_remaining_runtime")


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


def _advance(b, policy, steps):
    for _ in range(steps):
        b.heuristic_step(policy, want_obs=False)


def _bytes(b):
    return b.snapshot().cpu().numpy()


def _rows(b):
    return BL.rows(_bytes(b), b.n_envs, b.P, b.V)


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _export(b):
    """state(), counters() and the two totals as device tensors: what an identity import takes."""
    return b.state(), b.counters(), b.stats()[:, 3:5].contiguous()


def _slot_words(vmw, V):
    """The slot and time words of slots 0..V-1 out of VM rows [n, 4 pitch] (bytes). The
    words behind slot V are whatever the allocation held: two handles differ in them."""
    v = np.arange(V)
    at = ((v >> 6) << 7) | (v & 63)
    u = vmw.view(np.uint32)
    return np.concatenate([u[:, at], u[:, at | 64]], axis=1)


def _rows_nopad(b):
    """_rows after stats() has derived the target means of the current state,
    with the hint word cleared (a function of the path, not of the state) and
    the VM row cut down to its V slots."""
    b.stats()
    hdr, pm, vmw = _rows(b)
    hdr = hdr.copy()
    hdr.view(np.uint64)[:, SL.W_PAD] = 0
    return hdr, pm, _slot_words(vmw, b.V)


def _expected_rows(before, i, pk):
    """The three snapshot rows env i must hold after importing `pk` (SL.pack)
    over the rows `before`: untouched streams, target means and padded words."""
    hdr, pm, vmw = (r[i].copy() for r in before)
    w = hdr.view(np.uint64)
    if pk["counters"] is not None:
        w[BL.W_TOTAL:BL.W_TOTAL + 5] = pk["counters"][:5].astype(np.uint64)
        w[BL.W_TIMESTEP] = np.uint64(pk["counters"][5])
    if pk["totals"] is not None:
        hdr.view(np.float64)[SL.W_CPU_REQ:SL.W_MEM_REQ + 1] = pk["totals"]
    hdr.view(np.float64)[SL.W_WAITING] = pk["waiting_ratio"]
    w[SL.W_PAD] = 0
    u = vmw.view(np.uint32)
    u[pk["slot_at"]] = pk["slot"]
    u[pk["time_at"]] = pk["time"]
    return hdr, pk["pm"].view(np.uint8), vmw


# ------------------------------------------------------------------ 1: bytes
@pytest.mark.parametrize("loads", [True, False], ids=["loads", "sums"])
@pytest.mark.parametrize("P,V,n", [s + (N,) for s in SHAPES] + [(1000, 10000, 2)])
def test_bytes_equal_the_literal(P, V, n, loads):
    cfg = _cfg(P, V, "kl")
    b = _env(cfg, n)
    _advance(b, "bestfit", 12)  # hint words, counters and every row hold something
    before = _rows(b)
    if V <= 1024:  # the wave kernels' per-step launches leave hints (the block kernel writes 0)
        assert np.any(before[0].view(np.uint64)[:, SL.W_PAD] != 0)
    g = np.random.default_rng([P, V, int(loads)])
    sts = [SL.random_state(g, P, V, fill=(0.5, 0.95, 0.1)[i % 3], loads=loads) for i in range(n)]
    mask = np.ones(n, np.uint8)
    mask[n // 3] = 0
    d = SL.stack(sts)
    status = b.set_state({k: d[k] for k in d if k not in ("counters", "totals")}, mask=mask,
                         counters=d["counters"], totals=d["totals"])
    assert status.cpu().numpy().tolist() == mask.tolist()
    after = _rows(b)
    for i in range(n):
        want = _expected_rows(before, i, SL.pack(sts[i], P, V)) if mask[i] else [r[i] for r in before]
        for part, got, w in zip(("hdr", "pm", "vmw"), after, want):
            bad = np.flatnonzero(got[i] != w)
            assert bad.size == 0, (part, i, bad[:8])
    # stats() right after the call: what the literal computes from the state
    stats = b.stats().cpu().numpy()
    for i in np.flatnonzero(mask):
        ex = sts[i]["vm_placement"] <= P
        tcm = min(1.0, np.sum(sts[i]["vm_cpu"][ex]) / P)
        tmm = min(1.0, np.sum(sts[i]["vm_memory"][ex]) / P)
        want = [SL.pack(sts[i], P, V)["waiting_ratio"], tcm, tmm] + sts[i]["totals"].tolist()
        assert stats[i].tolist() == want, (i, stats[i], want)
    # ... and state() / counters() give the arrays back
    got, ctr = _np(b.state()), b.counters().cpu().numpy()
    for i in np.flatnonzero(mask):
        for k in ("vm_placement", "vm_cpu", "vm_memory", "vm_remaining_runtime"):
            assert np.array_equal(got[k][i], sts[i][k]), (k, i)
        assert np.array_equal(ctr[i], sts[i]["counters"])
    # without counters and totals the env keeps its own, the timestep among them
    mid = _rows(b)
    ts = b.counters().cpu().numpy()[:, 5]
    sts2 = [SL.random_state(g, P, V, loads=loads, counters=False) for _ in range(n)]
    b.set_state(SL.stack(sts2))
    after = _rows(b)
    for i in range(n):
        want = _expected_rows(mid, i, SL.pack(sts2[i], P, V, timestep=int(ts[i])))
        for part, got_, w in zip(("hdr", "pm", "vmw"), after, want):
            assert np.array_equal(got_[i], w), ("kept counters", part, i)
    b.close()


# -------------------------------------------------------------- 2: refusals
def _rich_state(g, P, V):
    """A valid state with loads, an empty slot and two VMs."""
    while True:
        st = SL.random_state(g, P, V, fill=0.6, loads=True)
        pl = st["vm_placement"]
        if np.count_nonzero(pl == P + 1) and np.count_nonzero(pl <= P) >= 2:
            return st


def _break(st, code, P):
    pl = st["vm_placement"]
    null, ex = np.flatnonzero(pl == P + 1), np.flatnonzero(pl <= P)
    if code == SL.PLACEMENT:
        pl[null[-1]] = P + 2
    elif code == SL.NULL_SLOT:
        st["vm_cpu"][null[0]] = 0.5
    elif code == SL.VM_SIZE:
        st["vm_memory"][ex[-1]] = 0.1 + 0.2
    elif code == SL.RUNTIME:
        st["vm_remaining_runtime"][ex[0]] = (1 << 30) + 1
    elif code == SL.TIMESTEP:
        st["counters"][5] = 0
    elif code == SL.COUNTER:
        st["counters"][2] = -1
    elif code == SL.CAPACITY:
        for v in ex[:2]:
            pl[v], st["vm_cpu"][v] = 0, 0.51
    elif code == SL.LOAD_FLOOR:
        st["cpu"][P - 1] = 9.9e-8
    elif code == SL.LOAD_MAX:
        st["memory"][0] = np.nextafter(1.0, 2.0)
    elif code == SL.LOAD_SUM:
        k = SL._sums(st, P)[P - 1]
        st["cpu"][P - 1] = k / 100.0 + (2e-7 if k < 100 else -2e-7)
    return st


@pytest.mark.parametrize("P,V", SHAPES)
def test_every_refusal_leaves_the_env_untouched(P, V):
    from vmp.state import RULES
    codes = list(range(2, 12))
    n = len(codes) + 2  # env i breaks rule codes[i]; then a valid env and an unselected one
    b = _env(_cfg(P, V), n)
    _advance(b, "firstfit", 12)
    before = _rows(b)
    g = np.random.default_rng([P, V, 2])
    sts = [_rich_state(g, P, V) for _ in range(n)]
    for i, c in enumerate(codes):
        _break(sts[i], c, P)
    want = [SL.validate(s, P) for s in sts]
    assert want[:len(codes)] == codes and want[-2:] == [SL.IMPORTED] * 2  # not vacuous
    mask = [1] * (n - 1) + [0]
    want[-1] = SL.SKIPPED
    d = SL.stack(sts)
    arrays = {k: d[k] for k in d if k not in ("counters", "totals")}
    status = b.set_state(arrays, mask=mask, counters=d["counters"], totals=d["totals"], check=False)
    assert status.dtype == torch.uint8 and status.cpu().numpy().tolist() == want
    after = _rows(b)
    for i in range(n):
        same = all(np.array_equal(x[i], y[i]) for x, y in zip(before, after))
        assert same == (i != n - 2), i
    with pytest.raises(ValueError) as err:
        b.set_state(arrays, mask=mask, counters=d["counters"], totals=d["totals"])
    for i, c in enumerate(codes):
        assert "%d: %s" % (i, RULES[c]) in str(err.value), (i, str(err.value))
    assert "%d:" % (n - 2) not in str(err.value) and "%d:" % (n - 1) not in str(err.value)
    # host-side refusals: shapes, dtypes and the cpu / memory pair
    for bad in (dict(arrays, vm_cpu=d["vm_cpu"][:, :-1]), dict(arrays, vm_placement=d["vm_placement"][1:]),
                {k: v for k, v in arrays.items() if k != "cpu"},
                dict(arrays, memory=[["x"] * P] * n)):
        with pytest.raises(ValueError):
            b.set_state(bad, mask=mask)
    with pytest.raises(ValueError):
        b.set_state(arrays, counters=d["counters"][:, :5])
    for x, y in zip(after, _rows(b)):
        assert np.array_equal(x, y)
    b.close()


# ------------------------------------------------ 3: identity import, RNG workload
def _assert_twins(a, b, what):
    for x, y in ((a.counters(), b.counters()), (a.stats(), b.stats())):
        assert torch.equal(x, y), what
    sa, sb = a.state(), b.state()
    for k in KEYS:
        assert torch.equal(sa[k], sb[k]), (what, k)


@pytest.mark.parametrize("P,V", SHAPES)
def test_identity_import_continues_as_its_twin(P, V):
    """Two handles of equal seeds; one re-imports its own exported state (loads
    verbatim, counters, totals, streams kept) before each of four drivers, and
    must then return what its untouched twin returns, bit for bit."""
    k = SHAPES.index((P, V))
    reward, policy = REWARDS[k % 3], ("firstfit", "bestfit")[k % 2]
    cfg = _cfg(P, V, reward)
    a, b = _env(cfg), _env(cfg)
    g = np.random.default_rng([P, V, 3])

    def ext_step():
        heur = a.heuristic_act(policy).cpu().numpy().astype(np.int64)
        pl = a.state()["vm_placement"].cpu().numpy()
        act = np.stack([ext_actions(g, P, P + 2, pl[i], heur[i]) for i in range(N)])
        t = torch.tensor(act, dtype=torch.int32, device=DEV)
        return a.step(t), b.step(t)

    a.rollout(policy, 20)
    b.rollout(policy, 20)
    for _ in range(8):
        ext_step()
    for driver in ("bare", "actions", "ext", "rollout"):
        st, ctr, tot = _export(b)
        b.set_state(st, counters=ctr, totals=tot)
        a.stats()  # as _export did on b: both headers hold the means of this state
        ra, rb = _rows(a), _rows(b)
        assert np.array_equal(ra[1], rb[1]), driver
        assert np.array_equal(_slot_words(ra[2], V), _slot_words(rb[2], V)), driver
        wa, wb = ra[0].view(np.uint64), rb[0].view(np.uint64)
        assert np.array_equal(wa[:, :SL.W_PAD], wb[:, :SL.W_PAD]) and np.all(wb[:, SL.W_PAD] == 0)
        if driver == "rollout":
            (ra_, da), (rb_, db) = a.rollout(policy, 40), b.rollout(policy, 40)
            assert torch.equal(ra_, rb_) and torch.equal(da, db)
            _assert_twins(a, b, driver)
            continue
        for t in range(40):
            if driver == "ext":
                xa, xb = ext_step()
            else:
                kw = dict(want_actions=True, want_valid=True) if driver == "actions" else {}
                xa, xb = a.heuristic_step(policy, **kw), b.heuristic_step(policy, **kw)
            for p, q in zip(xa, xb):
                assert (p is None and q is None) or torch.equal(p, q), (driver, t)
            _assert_twins(a, b, (driver, t))
    assert int(a.counters()[:, 1].sum()) > 0 and int(a.counters()[:, 2].sum()) > 0  # served, suspended
    a.close()
    b.close()


# ---------------------------------------------------- 4: headline config, quiet envs
def test_headline_config_quiet_envs_continue():
    """P100 / V1000, lambda 1.8182, L 1000 at age 2 500, where nearly every
    env-step is quiet: the import writes the hint word as 0, the next launch
    takes the general path once and the idle path after it must be the twin's."""
    cfg = dict(BASE, pms=100, vms=1000, arrival_rate=1.8182, service_length=1000,
               reward_function="kl")
    n = 64
    a, b = _env(cfg, n), _env(cfg, n)
    for e in (a, b):
        e.rollout("firstfit", 2496)
        _advance(e, "firstfit", 4)
    pad = _rows(a)[0].view(np.uint64)[:, SL.W_PAD]
    assert np.any((pad >> np.uint64(62)) & np.uint64(1)), "no env carries the quiet bit"
    st, ctr, tot = _export(b)
    b.set_state(st, counters=ctr, totals=tot)
    assert np.all(_rows(b)[0].view(np.uint64)[:, SL.W_PAD] == 0)
    for t in range(200):
        oa, ra, da, _, _ = a.heuristic_step("firstfit")
        ob, rb, db, _, _ = b.heuristic_step("firstfit")
        assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db), t
    _assert_twins(a, b, "final")
    assert all(np.array_equal(x, y) for x, y in zip(_rows_nopad(a), _rows_nopad(b)))
    a.close()
    b.close()


# ------------------------------------- 5: hand-made states vs the literal env, traced
def _hand_made(P, V):
    """Four states no reset reaches, each with counters (their timestep picks
    the trace step) and without loads."""
    g = np.random.default_rng([P, V, 5])
    null = lambda: dict(vm_placement=np.full(V, P + 1, np.int64), vm_cpu=np.zeros(V),  # noqa: E731
                        vm_memory=np.zeros(V), vm_remaining_runtime=np.zeros(V, np.int64))
    full = null()  # every PM exactly full in cpu: 4 VMs of 25, memory 4 x 20; the rest wait
    n_run = min(V, 4 * P)
    full["vm_placement"][:n_run] = np.arange(n_run) % P
    full["vm_cpu"][:n_run], full["vm_memory"][:n_run] = 0.25, 0.2
    full["vm_remaining_runtime"][:n_run] = g.integers(1, 30, n_run)
    rest = np.arange(n_run, V)
    full["vm_placement"][rest] = P
    full["vm_cpu"][rest], full["vm_memory"][rest] = 0.5, 0.5
    full["vm_remaining_runtime"][rest] = g.integers(1, 9, rest.size)
    frag = SL.random_state(g, P, V, fill=0.9, wait=0.2, counters=False, max_rt=12)  # odd sizes all over
    waiting = null()
    waiting["vm_placement"][:] = P
    waiting["vm_cpu"][:] = g.integers(1, 101, V) / 100.0
    waiting["vm_memory"][:] = g.integers(1, 101, V) / 100.0
    waiting["vm_remaining_runtime"][:] = g.integers(1, 20, V)
    out = [full, frag, waiting, null()]
    for st, ts in zip(out, (3, 40, 120, 500)):
        st["counters"] = np.array([7, 2, 1, 4, 0, ts], np.int64)
        st["totals"] = np.array([12.5, 9.75])
    return out


@pytest.mark.parametrize("P,V,reward", [(4, 65, "wr"), (7, 1025, "ut"), (4, 64, "kl")])
def test_hand_made_states_under_a_trace_vs_the_literal(P, V, reward):
    from vmp.trace import Trace
    cfg = _cfg(P, V, reward)
    g = np.random.default_rng([P, V, 55])
    steps = 600
    arrivals = g.poisson(max(1.0, V / 30.0), steps)
    tot = int(arrivals.sum())
    tr = Trace(np.r_[0, np.cumsum(arrivals)], g.integers(1, 101, tot), g.integers(1, 101, tot),
               g.integers(1, 15, tot))
    sts = _hand_made(P, V)
    n = len(sts)
    b = _env(cfg, n)
    b.set_trace(tr)
    _advance(b, "firstfit", 5)
    d = SL.stack(sts)
    b.set_state({k: d[k] for k in d if k not in ("counters", "totals")}, counters=d["counters"],
                totals=d["totals"])
    lits = [SL.into_trace_env(TL.TraceEnv(cfg, tr.offs, tr.cpu, tr.mem, tr.runtime), s) for s in sts]
    obs0 = b.obs().cpu().numpy()
    for i, e in enumerate(lits):
        assert np.array_equal(obs0[i], e.obs()), ("imported obs", i)
    ga = np.random.default_rng([P, V, 56])
    policy = "bestfit" if reward == "kl" else "firstfit"
    offered = [[] for _ in lits]
    n_invalid = n_susp = 0
    for t in range(60):
        heur = b.heuristic_act(policy).cpu().numpy().astype(np.int64)
        act = np.stack([ext_actions(ga, P, P + 2, e.vm_placement, heur[i]) for i, e in enumerate(lits)])
        act[act < 0] = P + 2  # out of range at the top only: the literal indexes its PMs with it
        obs, rew, done, valid = b.step(torch.tensor(act, dtype=torch.int32, device=DEV))
        obs, rew, valid = obs.cpu().numpy(), rew.cpu().numpy(), valid.cpu().numpy()
        for i, e in enumerate(lits):
            before, susp = e.total_requests, e.suspend_action
            o, r, dn, v = e.step(act[i])
            assert np.array_equal(valid[i], v), ("valid", t, i)
            assert np.array_equal(obs[i], o), ("obs", t, i)
            assert abs(rew[i] - r) <= 1e-5, ("reward", t, i, rew[i], r)
            assert bool(done[i]) == dn, ("done", t, i)
            offered[i].append(e.total_requests - before)
            n_invalid += int(np.count_nonzero(v == 0))
            n_susp += e.suspend_action - susp
    assert n_invalid > 0 and n_susp > 0
    ctr, stats, st = b.counters().cpu().numpy(), b.stats().cpu().numpy(), _np(b.state())
    for i, e in enumerate(lits):
        assert np.array_equal(ctr[i], e.counters()), ("counters", i, ctr[i], e.counters())
        assert np.array_equal(stats[i][[0, 3, 4]], e.stats()[[0, 3, 4]]), ("stats", i)
        for k, x in zip(TL.STATE_KEYS, e.state()):
            assert np.array_equal(st[k][i], x), (k, i)
        ts = int(sts[i]["counters"][5])  # timestep ts is trace step ts - 1
        assert offered[i] == arrivals[ts - 1:ts + 59].tolist() and sum(offered[i]) > 0, i
    b.close()


# ---------------------------------------------------------------- 6: reseed
@pytest.mark.parametrize("P,V", [(100, 300), (7, 1025)])
def test_reseeded_import_draws_from_numpys_generators(P, V):
    from tests.test_gpu_branch import _assert_fresh_streams, _run_and_collect
    cfg = _cfg(P, V)
    n = 5
    a, b = _env(cfg, n), _env(cfg, n)
    _advance(a, "firstfit", 25)
    _advance(b, "firstfit", 25)
    seeds = [11, 11, 23, -1, 40]
    st, ctr, tot = _export(b)
    st = {k: v.clone() for k, v in st.items()}
    for k in st:  # envs 0 and 1 start from one state: equal seeds, equal futures
        st[k][1] = st[k][0]
    ctr[1], tot[1] = ctr[0], tot[0]
    before = _rows(b)[0].view(np.uint64)
    b.set_state(st, counters=ctr, totals=tot, seeds=seeds)
    w = _rows(b)[0].view(np.uint64)
    for i, s in enumerate(seeds):
        want = BL.stream_words(s) if s >= 0 else before[i, :20]
        assert np.array_equal(w[i, :20], want), i
    T = 30
    offered, cpu, mem, rt = _run_and_collect(b, T)
    for i, s in enumerate(seeds):
        if s >= 0:
            _assert_fresh_streams(s, V / 4.0, 8, offered[:, i], cpu[i], mem[i], rt[i])
    rb = _rows_nopad(b)
    assert all(np.array_equal(r[1], r[0]) for r in rb)
    assert not np.array_equal(offered[:, 2], offered[:, 0])
    for _ in range(T):  # the -1 env is its twin continuing
        a.heuristic_step("firstfit", want_actions=True, want_valid=True)
    ra = _rows_nopad(a)
    assert all(np.array_equal(x[3], y[3]) for x, y in zip(ra, rb))
    a.close()
    b.close()


# ------------------------------------------------------------- 7: observers
def _observe(b):
    b.record(True)
    b.request_log(capacity=20000)
    b.series(capacity=40, pm_rows=True)


def _readings(b):
    hist, sums = b.record_read()
    rq, sr = b.request_log_read(), b.series_read()
    return dict(hist=hist.cpu().numpy(), sums=sums.cpu().numpy(), rq_rows=rq.rows, rq_meta=rq.meta,
                sr_rows=sr.rows, sr_meta=sr.meta, sr_pm=sr.pm)


@pytest.mark.parametrize("P,V", [(100, 300), (20, 2049)])
def test_observers_restart_for_imported_envs_only(P, V):
    """Recorder, request log and series on. Env 2 is not selected and env 3 is
    refused: both read back as those of a twin that made the same steps and
    never imported; the imported envs as those of a twin restored to the same
    bytes (vmp_restore restarts every env's observers). VMP_REC_XMEM sums over
    the handle's envs, so it is compared on the restored twin only."""
    cfg = _cfg(P, V)
    n = 5
    dst, kept = _env(cfg, n), _env(cfg, n)
    for b in (dst, kept):
        _advance(b, "bestfit", 15)
        _observe(b)
        _advance(b, "bestfit", 10)
    st, ctr, tot = _export(dst)
    st["vm_placement"][3, V - 1] = P + 2
    status = dst.set_state(st, mask=[1, 1, 0, 1, 1], counters=ctr, totals=tot, check=False)
    assert status.cpu().numpy().tolist() == [1, 1, 0, SL.PLACEMENT, 1]
    twin = _env(cfg, n)
    _observe(twin)
    twin.restore(dst.snapshot())
    for b in (dst, kept, twin):
        _advance(b, "firstfit", 20)
    rd, rk, rt = _readings(dst), _readings(kept), _readings(twin)
    for i in range(n):
        went_on = i in (2, 3)
        ref = rk if went_on else rt
        for key in rd:
            x, y = rd[key][i], ref[key][i]
            if key == "sums" and went_on:
                x, y = x[:18], y[:18]
            assert np.array_equal(x, y), (key, i)
    assert rd["sr_meta"][2].tolist() == [16, 30, 0] and rd["sr_meta"][0].tolist() == [26, 20, 0]
    assert rd["sums"][3, 0] == 30 and rd["sums"][1, 0] == 20
    for b in (dst, kept, twin):
        b.close()


# ----------------------------------------------------------------- 8: graph
def test_set_state_and_rollout_replay_in_a_graph():
    from vmp._lib import lib
    P, V, K, n = 100, 300, 8, 5
    cfg = _cfg(P, V)
    dst, eager = _env(cfg, n), _env(cfg, n)
    _advance(dst, "bestfit", 10)
    g = np.random.default_rng(8)

    def arrays(break_env=None):
        sts = [SL.random_state(g, P, V, loads=True) for _ in range(n)]
        if break_env is not None:
            sts[break_env]["vm_remaining_runtime"][:] = 0
        d = SL.stack(sts)
        return {k: torch.tensor(v, device=DEV) for k, v in d.items()}, [SL.validate(s, P) for s in sts]

    buf, _ = arrays()
    st = {k: buf[k] for k in buf if k not in ("counters", "totals")}
    sd = torch.tensor([-1, 5, 9, 9, -1], dtype=torch.int64, device=DEV)
    rew = torch.empty((K, n), dtype=torch.float64, device=DEV)
    dc = torch.zeros(n, dtype=torch.int64, device=DEV)

    def call(env, state, ctr, tot, seeds, **kw):
        status = env.set_state(state, counters=ctr, totals=tot, seeds=seeds, check=False)
        return status, env.rollout("firstfit", K, **kw)

    call(dst, st, buf["counters"], buf["totals"], sd, rewards=rew, done_count=dc)  # outside first
    torch.cuda.synchronize()
    gc.collect()
    lib().vmp_debug_live_allocs.restype = ctypes.c_int64
    live = lib().vmp_debug_live_allocs()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        status, _ = call(dst, st, buf["counters"], buf["totals"], sd, rewards=rew, done_count=dc)
    eager.restore(dst.snapshot())
    for break_env in (None, 2, None):
        new, want_status = arrays(break_env)
        for k in buf:
            buf[k].copy_(new[k])
        graph.replay()
        s2, (want, _) = call(eager, {k: new[k] for k in st}, new["counters"], new["totals"], sd.clone())
        assert status.cpu().numpy().tolist() == want_status == s2.cpu().numpy().tolist()
        assert (break_env is None) == (want_status == [1] * n)
        assert torch.equal(rew, want), break_env
        assert np.array_equal(_bytes(dst), _bytes(eager)), break_env
    assert lib().vmp_debug_live_allocs() == live
    dst.close()
    eager.close()


# ------------------------------------------------------------------- 9: CLI
def _first_fit(e):
    """FirstFitAgent.act on the literal env's state (sizes far from any border)."""
    a = e.vm_placement.copy()
    cpu, mem = e.cpu.copy(), e.memory.copy()
    for v in np.flatnonzero(e.vm_placement == e.WAIT):
        for q in range(e.P):
            if cpu[q] + e.vm_cpu[v] <= 1 and mem[q] + e.vm_memory[v] <= 1:
                a[v] = q
                cpu[q] += e.vm_cpu[v]
                mem[q] += e.vm_memory[v]
                break
    return a


def test_cli_main_starts_from_a_state_file(tmp_path):
    """python -m vmp.main --state --trace: on a trace of three short requests,
    what the run serves and places beyond them is what the state file brought
    (the counts tests/trace_literal.py gives, see the paired test below)."""
    from vmp.main import Args, parse, run
    from vmp.state import State
    from vmp.trace import Trace
    P, V, steps = 4, 10, 20
    env = dict(BASE, pms=P, vms=V, arrival_rate=0.5, reward_function="wr", eval_steps=steps)
    tr = str(tmp_path / "t.npz")
    Trace([0, 1, 1, 3] + [3] * (steps - 3), [50, 30, 20], [50, 10, 40], [4, 3, 2]).save(tr)
    yml = tmp_path / "tiny.yml"
    yml.write_text("environment:\n" + "".join("  %s: %s\n" % kv for kv in env.items())
                   + "agents: {}\n")
    st = dict(vm_placement=np.array([0, 0, 2, P] + [P + 1] * 6, np.int64),
              vm_cpu=np.array([0.3, 0.7, 0.55, 0.25] + [0.0] * 6),
              vm_memory=np.array([0.2, 0.1, 0.45, 0.5] + [0.0] * 6),
              vm_remaining_runtime=np.array([5, 1, 30, 7] + [0] * 6, np.int64))
    path = str(tmp_path / "s.npz")
    State(P, **st).save(path)
    args = parse(["-a", "firstfit", "-c", str(yml), "-r", "wr", "-e", "-s", "--state", path,
                  "--trace", tr, "-o", str(tmp_path / "out.json")])
    assert args.state == path
    summ = run(args).get_summary()
    # the trace's three VMs, and of the state: slots 0, 1 finish, slot 3 is placed and
    # finishes, slot 2 outlives the 20 steps
    assert (summ["total served VMs"], summ["total place actions"], summ["total requests"]) == (6, 4, 3)
    plain = run(Args(agent="firstfit", reward="wr", config=args.config, eval=True, silent=True,
                     trace=tr, output=str(tmp_path / "out0.json"))).get_summary()
    assert (plain["total served VMs"], plain["total place actions"]) == (3, 3)


def test_cli_paired_starts_from_a_state_file(tmp_path, capsys):
    from vmp import exp
    from vmp.state import State
    from vmp.trace import Trace
    P, V, steps = 4, 10, 20
    cfg = dict(BASE, pms=P, vms=V, arrival_rate=0.5, reward_function="wr", eval_steps=steps)
    yml = tmp_path / "tiny.yml"
    yml.write_text("environment:\n" + "".join("  %s: %s\n" % kv for kv in cfg.items()))
    tr = Trace([0, 1, 1, 3] + [3] * (steps - 3), [50, 30, 20], [50, 10, 40], [4, 3, 2])
    tr.save(str(tmp_path / "t.npz"))
    st = dict(vm_placement=np.array([0, 0, 2, P] + [P + 1] * 6, np.int64),
              vm_cpu=np.array([0.3, 0.7, 0.55, 0.25] + [0.0] * 6),
              vm_memory=np.array([0.2, 0.1, 0.45, 0.5] + [0.0] * 6),
              vm_remaining_runtime=np.array([5, 1, 30, 7] + [0] * 6, np.int64))
    State(P, **st).save(str(tmp_path / "s.npz"))
    argv = ["paired", "--trace", str(tmp_path / "t.npz"), "--config", str(yml), "--agents",
            "firstfit", "--eval-steps", str(steps)]
    exp.main(argv)
    plain = capsys.readouterr().out.splitlines()
    exp.main(argv + ["--state", str(tmp_path / "s.npz")])
    started = capsys.readouterr().out.splitlines()
    assert plain[0] == started[0] == exp.PAIRED_HEADER and len(plain) == len(started) == 2

    def predict(state):
        e = TL.TraceEnv(cfg, tr.offs, tr.cpu, tr.mem, tr.runtime)
        if state is not None:
            SL.into_trace_env(e, state)
        for _ in range(steps):
            e.step(_first_fit(e))
        return e.served, e.suspend_action, e.suspend_action + e.place_action

    for line, state in ((plain[1], None), (started[1], st)):
        col = line.split(",")
        assert col[:4] == ["firstfit", "0", str(steps), "3"]
        assert tuple(int(x) for x in col[4:7]) == predict(state), line
    # the trace's 3 VMs are placed and served in both; the state adds two running VMs that
    # finish and a waiting one that is placed and finishes (its fourth VM outlives the run)
    assert predict(None) == (3, 0, 3) and predict(st) == (6, 0, 4)
