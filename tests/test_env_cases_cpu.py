"""The cases of tests/env_cases.py are not vacuous (CPU, the C oracle alone).

tests/test_gpu_env_instances.py compares every env step kernel instantiation
with the oracle over each case's plan. A comparison proves something only if
the run it compares goes where the kernels can go wrong: these tests walk the
oracle through every plan and assert that it does, and that the table as a
whole selects all 45 wave and 24 block instantiations by the host's own
selection rule. They are conditions on the inputs: a case that misses one gets
other inputs."""
import numpy as np
import pytest

from tests import env_cases as C

IDS = [c.name for c in C.CASES]


def test_selection_rules():
    assert [C.wave_vpt(v) for v in (1, 64, 65, 128, 129, 256, 257, 512, 513, 1024)] == \
        [1, 1, 2, 2, 4, 4, 8, 8, 16, 16]
    assert [C.big_spt(v) for v in (1, 1024, 1025, 2048, 2049, 4096, 4097, 10240)] == \
        [4, 4, 8, 8, 16, 16, 40, 40]


def test_table_selects_every_instantiation():
    sel = set().union(*(c.selects() for c in C.CASES))
    sources = ("config", "workload", "trace")
    wave = {("wave", vpt, kind, s) for vpt in (1, 2, 4, 8, 16) for kind in ("ext", "one", "multi")
            for s in sources}
    block = {("block", spt, one, s) for spt in (4, 8, 16, 40) for one in (True, False)
             for s in sources}
    assert len(wave) == 45 and len(block) == 24
    assert sel == wave | block, sorted(map(str, (wave | block) ^ sel))
    # every VPT and every SPT meets all three (reward, policy) combinations
    met = {}
    for c in C.CASES:
        if c.group in "ab":
            key = ("block", C.big_spt(c.V)) if c.block else ("wave", C.wave_vpt(c.V))
            met.setdefault(key, set()).add((c.reward, c.policy))
    assert len(met) == 9 and all(m == set(C.COMBOS) for m in met.values()), met


def test_table_holds_the_cases_of_every_group():
    by = {}
    for c in C.CASES:
        by.setdefault(c.group, []).append(c)
    a = {(c.V, c.source) for c in by["a"]}
    assert a == {(v, s) for v in C.WAVE_V + C.BLOCK_V for s in ("config", "workload", "trace")}
    assert all(c.P <= 40 for c in by["a"] if c.V > 1024)
    assert {c.V for c in by["b"] if c.source == "config"} == set(C.FORCED_V)
    assert all(c.big for c in by["b"])
    assert {(c.P, c.V, c.lam, c.L, c.source) for c in by["c"]} >= {
        (400, 1024, lam, 2.0, s) for lam in (100.0, 200.0) for s in ("config", "workload")}
    assert any(c.V == 512 and abs(c.lam - 100) <= 10 for c in by["c"])
    assert {(c.P, c.null) for c in by["d"]} == {(p, n) for p in C.MASK_P for n in (True, False)}
    assert all(c.V == 65 for c in by["d"] + by["e"])
    assert {c.policy for c in by["e"]} == {"firstfit", "bestfit"}
    assert all(c.rolls == (1, 2, 256, 257) for c in by["e"])
    for c in C.CASES:
        assert len(c.seeds) == C.N_ENV and max(c.seeds) > 1 << 32 and len(set(c.seeds)) == C.N_ENV
        if c.wl is not None and c.group in "ab":
            lam = [w[0] for w in c.wl]
            assert len(set(c.wl)) == 6 and min(lam) == 0 and any(0 < x < 10 for x in lam) \
                and any(x >= 10 for x in lam)
        # the standard plan unless the case says why not
        std = (c.n_full, c.n_ext, c.rolls, c.n_bare) == (C.N_FULL, C.N_EXT, (C.K_ROLL,), C.N_BARE)
        assert std or c.note or c.group == "e", c.name


@pytest.mark.parametrize("case", C.CASES, ids=IDS)
def test_case_is_not_vacuous(case):
    r = C.run_oracle(case)
    P, V = case.P, case.V
    lam = np.array([w[0] for w in case.workload()])
    live = lam > 0
    acc, drop = r.accepted(), r.dropped()
    # every env with lam > 0: requests arrive, a VM runs, slot V - 1 is occupied on some step
    assert np.all(r.ctr[-1, live, 0] > 0) and np.all(r.ctr[-1, ~live, 0] == 0)
    assert np.all(r.n_run[:, live].max(0) > 0), r.n_run.max(0)
    assert np.all((r.last_pl[:, live] != P + 1).any(0)), (r.last_pl != P + 1).sum(0)
    # over the envs: full and not full, drops and none
    if V > 2:
        assert (r.n_null == 0).any() and (r.n_null > 0).any()
    assert (drop[:, live] > 0).any() and (drop[:, live] == 0).any()
    # episodes end inside the plan: both values of done are compared
    assert r.done.any() and not r.done.all()
    if case.n_ext:
        ext = slice(case.n_full, case.n_full + case.n_ext)
        assert (r.last_pl[ext] < P).any(), "slot V - 1 never runs in the external segment"
        n_rej = n_susp = 0
        for k, t in enumerate(range(ext.start, ext.stop)):
            n_rej += int((r.valid[t] == 0).sum())
            n_susp += int(((r.ext_pre_pl[k] < P) & (r.act[t] == P) & (r.valid[t] != 0)).sum())
        assert n_rej > 0 and n_susp > 0, (n_rej, n_susp)
    if case.group == "c":
        assert np.all((acc > 64).sum(0) >= 3), (acc > 64).sum(0)
        if case.lam >= 200:
            assert np.all((acc > 128).sum(0) >= 2), (acc > 128).sum(0)
    if case.group == "d":
        # the last mask word of a slot: columns 32 (W32 - 1) .. A - 1. Column A - 1 is
        # seen set and clear; where the word has a second column, so is its neighbour,
        # and some slot's word holds a set and a clear bit at once.
        A = case.A
        lo = 32 * ((A + 31) // 32 - 1)
        m = np.concatenate([x.reshape(-1, A) for x in r.ext_mask + [r.mid["mask"]]])
        assert m[:, A - 1].any() and not m[:, A - 1].all()
        if A - lo > 1:
            assert m[:, A - 2].any() and not m[:, A - 2].all()
            w = m[:, lo:]
            assert (w.any(1) & ~w.all(1)).any()
    if case.source == "trace":
        for i, tr in enumerate(r.traces):
            assert (tr[0][-1] > 0) == bool(live[i]), i
            assert tr[0].size == case.steps + 1 and tr[0][-1] == r.ctr[-1, i, 0]
