"""The C oracle (oracle/vmp_oracle.c) pinned against the reference's own
outputs: numpy RNG KATs, golden lock-step trajectories, and the published
exp_suspension rows (data/exp_suspension/data.csv). CPU only."""
import csv
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import prims_cases as C
from tests import traj as T
from tests.golden_hash import obs_hash, state_hash

KAT = np.load(os.path.join(T.GOLDEN, "rng_kat.npz"))


def test_seed_state_matches_numpy():
    out = np.zeros(4, np.uint64)
    for s, exp in zip(KAT["seeds"], KAT["state_inc"]):
        O.lib().oracle_pcg_seed(int(s), O._p(out))
        assert np.array_equal(out, exp), int(s)


def test_raw_double_around():
    for i, s in enumerate(KAT["seeds"]):
        raw = np.zeros(8, np.uint64)
        O.lib().oracle_pcg_raw(int(s), 8, O._p(raw))
        assert np.array_equal(raw, KAT["raw"][i])
        dbl = np.zeros(8)
        O.lib().oracle_pcg_double(int(s), 8, O._p(dbl))
        assert np.array_equal(dbl, KAT["dbl"][i])
        ar = np.zeros(16)
        O.lib().oracle_pcg_around(int(s), 16, 0.1, 1.0, O._p(ar))
        assert np.array_equal(ar, KAT["around"][i])


def test_poisson_streams():
    for i, s in enumerate(KAT["seeds"]):
        for j, lam in enumerate(KAT["lams"]):
            out = np.zeros(40, np.int64)
            after = O.lib().oracle_pcg_poisson(int(s), float(lam), 40, O._p(out))
            assert np.array_equal(out, KAT["poisson"][i, j]), (int(s), lam)
            assert after == int(KAT["raw_after"][i, j]), (int(s), lam)


def test_advance_matches_stepping():
    for s in (0, 7, 2**40 + 3):
        raw = np.zeros(1001, np.uint64)
        O.lib().oracle_pcg_raw(s, 1001, O._p(raw))
        assert O.lib().oracle_pcg_advance_raw(s, 1000) == int(raw[1000])


def test_pairwise_sum_matches_numpy():
    """np.sum of a contiguous float64 array, bit for bit, through every plan
    border of the device's sum and across numpy's reduction buffer of 8192
    elements (pairwise per buffer, the buffers added in order), for summands
    whose order of addition shows (tests/prims_cases.py)."""
    rng = np.random.default_rng(3)
    for n in list(range(0, 40)) + [127, 128, 129, 255, 256, 300, 1000, 1037, 4099]:
        a = np.around(rng.uniform(0.1, 1, n), 2)
        assert O.lib().oracle_pw_sum(O._p(a), n) == np.sum(a), n
    bad = []
    for fam in C.PW_FAMILIES:
        pool = C.pw_values(fam)
        for off, n in C.pw_cases():
            a = np.ascontiguousarray(pool[off:off + n])
            got, exp = O.lib().oracle_pw_sum(O._p(a), n), float(np.sum(a))
            if np.float64(got).view(np.uint64) != np.float64(exp).view(np.uint64):
                bad.append((fam, off, n, got, exp))
    assert not bad, (len(bad), bad[:8])


def test_mean_var_match_numpy_past_one_buffer():
    """The oracle's np_mean / np_var (the kl reward's moments of the existing
    VMs) against np.mean / np.var at more than 8192 elements."""
    bad = []
    for fam in C.PW_FAMILIES:
        pool = C.pw_values(fam)
        for off, n in C.pw_cases():
            if n < 8184:
                continue
            a = np.ascontiguousarray(pool[off:off + n])
            tmp, out = np.zeros(n), np.zeros(2)
            O.lib().oracle_mean_var(O._p(a), n, O._p(tmp), O._p(out))
            exp = np.array([np.mean(a), np.var(a)])
            if not np.array_equal(out.view(np.uint64), exp.view(np.uint64)):
                bad.append((fam, off, n, out.tolist(), exp.tolist()))
    assert not bad, (len(bad), bad[:8])


def test_argsort_is_a_permutation_sorting_keys():
    rng = np.random.default_rng(4)
    for n in (1, 2, 10, 16, 17, 50, 100, 1000):
        v = (rng.integers(0, 30, n) / 10).astype(np.float32)
        out = np.zeros(n, np.int64)
        O.lib().oracle_argsort_f32(O._p(v), n, O._p(out))
        assert sorted(out.tolist()) == list(range(n))
        assert np.all(np.diff(v[out]) >= 0)
        if n <= 16:  # insertion sort only: stable
            assert np.array_equal(out, np.argsort(v, kind="stable"))


def replay(d, reward_idx):
    cfg = dict(d["config"])
    cfg["reward_function"] = d["rewards"][reward_idx]
    env = O.OracleEnv(cfg)
    env.eval(bool(d["eval_mode"]))
    env.reset(cfg["seed"])
    acts = T.sparse_actions(d)
    masks = {int(t): i for i, t in enumerate(d["mask_at"])}
    n_kl_exact = 0
    for t in range(d["T"]):
        if t == d["reset_none_at"]:
            env.reset(None)
        if t in masks:
            m = env.mask()
            assert np.array_equal(np.packbits(m), d["masks"][masks[t]]), ("mask", t)
        pl = env.state()[0]
        a = pl.copy()
        if t in acts:
            vm, tg, va = acts[t]
            a[vm] = tg
        obs, r, done, valid = env.step(a)
        if t in acts:
            assert np.array_equal(valid[acts[t][0]], acts[t][2]), ("valid", t)
        exp_r = d["reward"][reward_idx, t]
        if cfg["reward_function"] == "kl":
            assert T.kl_close(r, exp_r), (t, r, exp_r)
            n_kl_exact += r == exp_r
        else:
            assert r == exp_r, (t, r, exp_r)
        st = env.state()
        assert state_hash(*st) == d["state_hash"][t], ("state", t)
        assert obs_hash(obs) == d["obs_hash"][t], ("obs", t)
        c, misc = env.counters()
        assert np.array_equal(c, d["counters"][t]), ("counters", t, c, d["counters"][t])
        assert np.array_equal(misc, d["misc"][t]), ("misc", t, misc, d["misc"][t])
        assert int(done) == d["done"][t]
        if "rank" in d:
            assert env.rank() == d["rank"][t]
    return n_kl_exact


@pytest.mark.parametrize("name", T.traj_names())
def test_trajectory_replay(name):
    d = T.load(name)
    for k in range(len(d["rewards"])):
        n_exact = replay(d, k)
        if d["rewards"][k] == "kl":
            # libm log vs numpy/OpenBLAS bit paths: report, bar is 1e-12
            assert n_exact >= 0.5 * d["T"], n_exact


@pytest.mark.parametrize("name", [n for n in T.traj_names() if n.endswith("pure")] +
                         ["c1_10yml_ff"])
def test_heuristic_proposals(name):
    d = T.load(name)
    env = O.OracleEnv(d["config"])
    env.eval(True)
    env.reset(d["config"]["seed"])
    acts = T.sparse_actions(d)
    for t in range(d["T"]):
        a = env.firstfit() if d["policy"] == "ff" else env.bestfit()
        pl = env.state()[0]
        nz = np.flatnonzero(a != pl)
        exp = acts.get(t, (np.zeros(0, int), np.zeros(0, int), None))
        assert np.array_equal(nz, exp[0]) and np.array_equal(a[nz], exp[1]), t
        env.step(a)


def _kat_rows():
    rows = []
    with open(os.path.join(T.GOLDEN, "exp_suspension_data.csv")) as f:
        for r in csv.reader(f):
            if r[0] in ("firstfit", "bestfit"):
                rows.append((r[0], float(r[1]), int(r[2]), int(r[3]), int(r[4]), int(r[5])))
    return rows


@pytest.mark.parametrize("row", _kat_rows(),
                         ids=lambda r: "%s-load%.1f-L%d" % (r[0], r[1], r[2]))
def test_published_exp_suspension_rows(row):
    """exp_suspension.py:12-60: config/100.yml, reward wr, seed 0, 100k eval
    steps, arrival_rate = round(100/0.55/L*load, 3); columns served, valid
    suspends, valid actions (data/exp_suspension/data.csv)."""
    agent, load, L, served, susp, valid = row
    cfg = dict(pms=100, vms=300, service_length=L, training_steps=10000, eval_steps=100000,
               seed=0, reward_function="wr", sequence="uniform", cap_target_util=True,
               beta=0.5, allow_null_action=True,
               arrival_rate=float(np.round(100 / 0.55 / L * load, 3)))
    _, ctr = O.rollout(cfg, 1, 0, 1, 100000, policy=0 if agent == "firstfit" else 1)
    assert ctr[0, 1] == served and ctr[0, 2] == susp and ctr[0, 2] + ctr[0, 3] == valid, ctr[0]


def test_rollout_timed_passes_repeat_the_same_window():
    """bench.py cpu_baseline: every timed pass restarts from the post-warm-up
    state, so the passes do identical work (same per-env reward sums), and
    they equal a plain OracleEnv FirstFit rollout of the same seeds."""
    cfg = dict(pms=10, vms=30, arrival_rate=0.3, service_length=20, reward_function="wr")
    secs, rs = O.rollout_timed(cfg, 4, 7, 3, 25, 40, 0, 2, reps=3)
    assert secs.shape == (3,) and (secs > 0).all()
    np.testing.assert_array_equal(rs[0], rs[1])
    np.testing.assert_array_equal(rs[0], rs[2])
    for i in range(4):
        e = O.OracleEnv(dict(cfg, seed=7 + 3 * i))
        tot = 0.0
        for s in range(65):
            _, r, _, _ = e.step(e.firstfit())
            if s >= 25:
                tot += r
        assert tot == rs[0, i]


# ------------------------------- the models of branch / set_state / set_workload
_API_CFG = dict(pms=6, vms=40, arrival_rate=2.0, service_length=9, training_steps=60,
                eval_steps=100000, seed=5, reward_function="kl", sequence="uniform",
                cap_target_util=True, beta=0.3, allow_null_action=True)


def _random_ext(g, e):
    a = e.state()[0].copy()
    draw = g.random(e.V) < 0.5
    a[draw] = g.integers(0, e.P + 2, int(draw.sum()))
    return a


def _drive(e, driver, g):
    return e.firstfit() if driver == "firstfit" else e.bestfit() if driver == "bestfit" \
        else _random_ext(g, e)


def _same_env(a, b, what):
    for x, y in zip(a.state(), b.state()):
        assert np.array_equal(x, y), what
    for x, y in zip(a.counters(), b.counters()):
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64)), what
    assert a.rank() == b.rank(), what


def _lockstep(a, b, driver, steps, seed=1):
    """a and b step under the same driver and must return the same values, bit for bit."""
    ga, gb = np.random.default_rng(seed), np.random.default_rng(seed)
    for t in range(steps):
        xa, xb = _drive(a, driver, ga), _drive(b, driver, gb)
        assert np.array_equal(xa, xb), (driver, t)
        (oa, ra, da, va), (ob, rb, db, vb) = a.step(xa), b.step(xb)
        assert np.array_equal(oa, ob) and np.array_equal(va, vb) and da == db, (driver, t)
        assert np.float64(ra).view(np.uint64) == np.float64(rb).view(np.uint64), (driver, t)
        _same_env(a, b, (driver, t))


@pytest.mark.parametrize("driver", ["firstfit", "bestfit", "ext"])
def test_assigned_env_continues_as_its_source(driver):
    """assign copies the whole state, the streams and the sequence bases (a
    reset(None) inside the 100 steps rewinds both alike), not the eval mode."""
    src = O.OracleEnv(_API_CFG)
    g = np.random.default_rng(2)
    for _ in range(37):
        src.step(_drive(src, driver, g))
    dst = O.OracleEnv(dict(_API_CFG, seed=99))
    dst.eval(True)
    for _ in range(5):
        dst.step(dst.firstfit())
    dst.assign(src)
    _same_env(src, dst, "assigned")
    # eval mode stayed dst's own: at timestep 60 the source is done, the copy is not
    a, b = O.OracleEnv(_API_CFG), O.OracleEnv(_API_CFG)
    a.assign(src)
    b.assign(dst)
    b.eval(True)
    for t in range(38, 61):
        da, db = a.step(a.firstfit())[2], b.step(b.firstfit())[2]
        assert (da, db) == (t >= 60, False), t
    src.eval(True)  # both in eval mode from here: no episode end decides anything
    for k in range(2):
        _lockstep(src, dst, driver, 50, seed=3 + k)
        src.reset(None)
        dst.reset(None)


@pytest.mark.parametrize("loads", [True, False])
def test_set_state_of_the_exported_state_is_an_identity(loads):
    """state(), counters and totals imported back: the env continues as its
    twin, with the loads verbatim; as sums of hundredths when no step has yet
    left rounding residue in them (a fresh placement of every VM)."""
    a, b = O.OracleEnv(_API_CFG), O.OracleEnv(_API_CFG)
    g = np.random.default_rng(4)
    for e in (a, b):
        ge = np.random.default_rng(4)
        for _ in range(30 if loads else 1):
            e.step(_random_ext(ge, e) if loads else e.firstfit())
    if not loads:  # one more step places the first arrivals: every load is one exact sum
        for e in (a, b):
            e.step(e.firstfit())
    pl, vc, vm, c, m, rem = b.state()
    ctr, st = b.counters()
    if not loads:
        from tests import state_literal as SL
        s = SL._sums(dict(vm_placement=pl, vm_cpu=vc, vm_memory=vm), b.P)
        assert np.array_equal(np.array(s, np.float64) / 100.0, np.r_[c, m]) and sum(s) > 0
    # poison first: set_state must write every array and recompute the stats
    z = np.zeros(b.V)
    b.set_state(np.full(b.V, b.P + 1), z, z, z.astype(np.int64), counters=np.arange(6) + 1,
                totals=[1.0, 2.0])
    assert b.counters()[0].tolist() == [1, 2, 3, 4, 5, 6] and b.counters()[1].tolist() == [0, 0, 0, 1, 2]
    b.set_state(pl, vc, vm, rem, c if loads else None, m if loads else None, ctr, st[3:5])
    _same_env(a, b, "imported")
    _lockstep(a, b, "ext", 100)
    # without counters and totals the env keeps its own
    pl, vc, vm, c, m, rem = b.state()
    before = b.counters()
    b.set_state(pl, vc, vm, rem, c, m)
    assert all(np.array_equal(x, y) for x, y in zip(before, b.counters()))
    del g


def test_reseeded_env_draws_from_the_fresh_streams():
    """reseed(s) on an env in mid-run: its state stays, and what it then draws
    (arrivals, sizes, runtimes) is what the streams of a fresh reset(s) env
    give; a later reset(None) rewinds to that seed's second sequence."""
    s = (1 << 33) + 7
    cfg = dict(_API_CFG, vms=400, pms=40)  # room for every arrival: draws are not cut by drops
    a = O.OracleEnv(cfg)
    for _ in range(20):
        a.step(a.firstfit())
    before = a.state()
    ctr0 = a.counters()[0].copy()
    a.reseed(s)
    assert all(np.array_equal(x, y) for x, y in zip(before, a.state()))
    fresh = O.OracleEnv(dict(cfg, seed=s))
    for t in range(25):
        pa, pf = a.state()[0], fresh.state()[0]
        a.step(pa)  # nothing is placed: every accepted VM stays where its draw put it
        fresh.step(pf)
        na, nf = a.state(), fresh.state()
        # (a slot freed by a finisher is refilled in the same step)
        new_a = np.flatnonzero((pa != a.P) & (na[0] == a.P))
        new_f = np.flatnonzero((pf != a.P) & (nf[0] == a.P))
        assert new_a.size == new_f.size, t
        assert a.counters()[0][0] - ctr0[0] == fresh.counters()[0][0], t
        for k in (1, 2, 5):
            assert np.array_equal(na[k][new_a], nf[k][new_f]), (t, k)
    assert fresh.counters()[0][0] > 30
    a.reset(None)
    fresh.reset(None)
    _lockstep(a, fresh, "firstfit", 30)


def test_set_workload_mid_run_equals_an_env_created_with_it():
    a = O.OracleEnv(_API_CFG)
    for _ in range(25):
        a.step(a.bestfit())
    for lam, L in ((11.0, 3.0), (0.0, 5.0), (0.7, 40.0)):
        b = O.OracleEnv(dict(_API_CFG, arrival_rate=lam, service_length=L, seed=77))
        b.assign(a)
        a.set_workload(lam, L)
        _lockstep(a, b, "bestfit", 40)
