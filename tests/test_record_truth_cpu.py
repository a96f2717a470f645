"""tests/record_truth.py on its own, without a GPU: the kernel's rule restated
(RuleRec) equals the ground truth (RecEnv) on every case of the table that
tests/test_gpu_record_truth.py runs on the device; three defective rules are
told apart; no case is vacuous; summary_from_device on the truth's raw
read-out gives the truth's summary; the comparison rule rejects what it must."""
import warnings

import numpy as np
import pytest

from tests import record_literal
from tests import record_truth as R

MIXED = [k for k, c in R.CASES.items() if c["workload"] == "mixed"]


def _rule(r, first=0, **defect):
    """RuleRec per env fed the run's (prev, action, valid, new placement) from step `first` on."""
    c = r.case
    rules = [R.RuleRec(c["P"], c["V"], r.pre[first, i], **defect) for i in range(c["N"])]
    for s in range(first, r.acts.shape[0]):
        for i, q in enumerate(rules):
            assert np.array_equal(q.prev, r.pre[s, i]), ("the rule's prev is the env's", s, i)
            q.update(r.acts[s, i], r.valids[s, i], r.post[s, i])
    return rules


def _differs(rules, envs):
    out = []
    for q, e in zip(rules, envs):
        hist, ls, lc = q.read()
        t = e.raw()
        out.append(not (np.array_equal(hist, t["hist"]) and ls == t["sums"][R.LIFE_SUM]
                        and lc == t["sums"][R.LIVES]))
    return out


# ---------------------------------------------------------------- rule == truth
@pytest.mark.parametrize("name", list(R.CASES))
def test_rule_equals_truth(name):
    r = R.run_case(name)
    assert not any(_differs(_rule(r), r.envs))


def test_rule_equals_truth_after_reset_and_restore():
    r = R.run_reset()
    c = r.case
    for i, e in enumerate(r.envs):
        first = R.RESET_AT if i in R.RESET_ENVS else 0
        q = R.RuleRec(c["P"], c["V"], r.pre[first, i])
        for s in range(first, R.RESET_STEPS):
            q.update(r.acts[s, i], r.valids[s, i], r.post[s, i])
        assert not _differs([q], [e])[0], i
        assert e.raw()["sums"][R.STEPS] == R.RESET_STEPS - first
    r = R.run_restore()
    assert all(e.mid_start for e in r.envs)
    assert not any(_differs(_rule(r, first=R.RESTORE_AT), r.envs))


# ------------------------------------------------------------------ sensitivity
@pytest.mark.parametrize("name,defect", [("waves-N5", "no_susp"), ("waves-N5-churn", "no_placed"),
                                         ("ties", "half_away")])
def test_a_defective_rule_is_told_apart(name, defect):
    r = R.run_case(name)
    assert all(_differs(_rule(r, **{defect: True}), r.envs)), (name, defect)


# --------------------------------------------------------------------- vacuity
@pytest.mark.parametrize("name", MIXED)
def test_mixed_is_not_vacuous(name):
    """Per env: >= 20 closed lives that ran, >= 10 valid suspensions, >= 5
    never-run lives, >= 1 life open at the read. The one-slot shape (P 1 / V 1)
    cannot hold them: random_actions places a waiting VM with probability
    1/2 * 1/3 a step, so 120 steps see about 20 placements in all, and 25 lives
    each need one. There the thresholds are those one slot can meet: >= 5
    closed lives that ran, >= 1 valid suspension, >= 2 never-run lives, and
    the open life."""
    r = R.run_case(name)
    need = (5, 1, 2, 1) if r.case["V"] == 1 else (20, 10, 5, 1)
    for i, e in enumerate(r.envs):
        ran, never, opened = e.life_stats()
        got = (ran, e.n_susp, never, opened)
        assert all(g >= n for g, n in zip(got, need)), (name, i, got, need)


def test_churn_refills_slots_in_the_step_that_frees_them():
    for i, e in enumerate(R.run_case("waves-N5-churn").envs):
        # an arrival with prev < P and no suspension; one with prev == WAIT and `placed`
        assert e.n_refill_run + e.n_refill_placed >= 50, i
        assert e.n_refill_run > 0 and e.n_refill_placed > 0, i


@pytest.mark.parametrize("name", ["drops", "pitch-V1025"])
def test_drops_drop_in_most_steps(name):
    for i, e in enumerate(R.run_case(name).envs):
        d = np.diff(np.r_[0, e.tr["dropped_requests"]])
        assert np.count_nonzero(d > 0) > d.size / 2, (name, i)


def test_ties_sit_on_the_half():
    for i, e in enumerate(R.run_case("ties").envs):
        n = {len(s) for s in e.closed}
        assert n >= {16, 80}, n
        # unrounded rates of the closed lives
        p_half = s_half = 0
        for s in e.closed:
            f = record_literal._first_run(s, e.WAIT)
            if f is None:
                continue
            p_half += R.on_half((f + 1.0) / len(s))
            life = len(s) - f - 1
            s_half += life > 0 and R.on_half(np.count_nonzero(s[f:] == e.WAIT) / life)
        assert p_half >= 8 and s_half >= 4, (i, p_half, s_half)


@pytest.mark.parametrize("name", [k for k in R.CASES if k.startswith("border")])
def test_p_borders_are_reached(name):
    r = R.run_case(name)
    P = r.case["P"]
    for i, e in enumerate(r.envs):
        assert e.max_pm == P - 1, (name, i, e.max_pm)  # PM P-1 is used at some step,
        assert P <= 64 or e.max_pm >= 64               # so is a PM of the second bitmap word
        assert P <= 128 or e.max_pm >= 128             # and of the third


@pytest.mark.parametrize("name", [k for k, c in R.CASES.items()
                                  if c["N"] > 1 and c["workload"] != "empty"])
def test_envs_of_a_handle_differ(name):
    raws = [e.raw() for e in R.run_case(name).envs[:2]]
    assert not np.array_equal(raws[0]["sums"], raws[1]["sums"])
    assert not np.array_equal(raws[0]["hist"], raws[1]["hist"]) or name == "ties"


def test_reset_scenario_can_see_a_stale_prev():
    """In env 1 or 3 some slot stands at WAIT just before the reset and takes
    an arrival in the first step after it: a recorder that kept its `prev`
    would merge that arrival into the old life."""
    r = R.run_reset()
    hit = [v for i in R.RESET_ENVS for v in r.waiting_before[i]
           if r.envs[i].arrival_steps[v][:1] == [2]]
    assert hit


# ---------------------------------------------- summary_from_device on the truth
def _summary_from_raw(e, raw):
    from vmp.record import summary_from_device
    return summary_from_device(raw["hist"], raw["sums"], e.counters(), e.stats(), e.P)


@pytest.mark.parametrize("name", list(R.CASES))
def test_summary_from_device_on_the_truth(name):
    r = R.run_case(name)
    for i, (e, raw) in enumerate(zip(r.envs, R.handle_raw(r.envs))):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)  # means of nothing: the empty trace
            lit = e.summary()
        assert not R.summary_mismatch(_summary_from_raw(e, raw), lit, e.exact_means()), (name, i)
    if name == "empty":
        assert raw["sums"][R.LIVES] == 0 and not raw["hist"].any()
        assert np.isnan(lit["average VM life"]) and lit["max pending"] == 0


def test_total_rewards_rule_on_synthetic_sums():
    """Record.total_rewards (record.py:103-108): rewards below -1e7 are replaced
    by the mean of those above, rewards of exactly -1e7 stay. No env reward
    reaches -1e7, so the device cannot take this branch through an env; the
    sums are made by hand here, as k_record would accumulate them."""
    from vmp.record import summary_from_device
    rw = [-0.25, -2e7, -1e7, -0.5, -3e7, -1e7, -0.125]
    s = np.zeros(R.NREC)
    s[R.STEPS] = len(rw)
    s[R.REWARD] = R.seq_sum(rw)
    s[R.REWARD_OK] = R.seq_sum(x for x in rw if x > -1e7)
    s[R.N_OK] = sum(x > -1e7 for x in rw)
    s[R.N_BAD] = sum(x < -1e7 for x in rw)
    assert s[R.N_BAD] == 2 and s[R.STEPS] - s[R.N_OK] - s[R.N_BAD] == 2
    got = summary_from_device(np.zeros((2, R.BINS), np.uint32), s, np.zeros(6, np.int64), np.zeros(5), 12)
    r = np.array(rw)
    r[r < -1e7] = np.mean(r[r > -1e7])  # record_literal.summary's rule
    assert got["total rewards"] == np.round(np.sum(r), 3)


# ----------------------------------------------------------- the comparison rule
@pytest.mark.parametrize("name", ["waves-N5", "border-P129-V257", "cross-N64", "cross-N65", "pitch-V1025"])
def test_comparison_rule(name):
    r = R.run_case(name)
    c = r.case
    truth = R.handle_raw(r.envs)
    naive = R.handle_raw(r.envs, naive=True)
    dims = (c["P"], c["V"], c["N"])
    for i in (0, c["N"] - 1):
        t = truth[i]
        assert R.judge(t["hist"], t["sums"], t, *dims) == []
        assert R.judge(naive[i]["hist"], naive[i]["sums"], t, *dims) == [], "np.sum is within the bound"
        h = t["hist"].copy()
        h[0, int(np.flatnonzero(h[0])[0])] += 1
        assert len(R.judge(h, t["sums"], t, *dims)) == 1
        for k in (R.RANK,) + R.BOUNDED:
            s = t["sums"].copy()
            s[k] = s[k] + 1 if k == R.RANK else s[k] * (1 + 1e-9)
            if k == R.XMEM and c["N"] > R.XMAX:
                assert t["sums"][k] == 0 and t["M"][k] == 0
                s[k] = 1e-300  # anything but 0 is rejected
            assert len(R.judge(t["hist"], s, t, *dims)) == 1, R.NAMES[k]
    R.RATIOS.clear()
