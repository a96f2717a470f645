"""Ground truth, rule and comparison rule of the device recorder (vmp_record_*,
csrc/vmp_record.hip), in numpy.

TEST INFRASTRUCTURE ONLY. Imports without a GPU. Three independent statements:

RecEnv     a tests/trace_literal.TraceEnv that knows the arrivals because it
           watches its own _accept (the slots that went NULL -> WAIT in this
           step); it reads neither actions nor validity flags to find them.
           After every step it appends what record.py keeps. summary() is
           tests/record_literal.summary on those traces; raw() is what
           vmp_record_read must return for this env: the two histograms and the
           19 sums of include/vmp.h VMP_REC_*, every sum exact (integer
           arithmetic on the f64 terms, rounded once at the end), together with
           the magnitudes M of the comparison rule.
RuleRec    k_record's update and k_record_close restated on the kernel's inputs
           alone (per slot the previous and the new placement, the action and
           its validity), as reqlog_literal.RuleLog does for the request log;
           three switchable defects show that the workloads can tell a wrong
           rule from the right one.
judge      the comparison rule: which of the device's numbers must be
           bit-exact and which are held to a derived bound gamma(n) * M
           (DESIGN.md section 5.3).

tests/test_record_truth_cpu.py holds RecEnv and RuleRec equal and checks that
no case is vacuous; tests/test_gpu_record_truth.py judges the device.
"""
import copy
import functools
import math
from fractions import Fraction

import numpy as np

from tests import record_literal
from tests.reqlog_literal import random_actions
from tests.trace_literal import TraceEnv

BINS, NREC, XMAX = 1001, 19, 64
(STEPS, REWARD, CPU, CPU2, MEM, MEM2, RANK, DROP, TCM, TMM, WAITING, LIFE_SUM, LIVES, REWARD_OK,
 N_OK, N_BAD, CPUVAR, MEMVAR, XMEM) = range(NREC)
NAMES = ("STEPS", "REWARD", "CPU", "CPU2", "MEM", "MEM2", "RANK", "DROP", "TCM", "TMM", "WAITING",
         "LIFE_SUM", "LIVES", "REWARD_OK", "N_OK", "N_BAD", "CPUVAR", "MEMVAR", "XMEM")
EXACT = (STEPS, REWARD, RANK, DROP, WAITING, LIFE_SUM, LIVES, REWARD_OK, N_OK, N_BAD)
BOUNDED = (CPU, CPU2, MEM, MEM2, TCM, TMM, CPUVAR, MEMVAR, XMEM)

U = 2.0 ** -53
_ONE = 1 << 1074  # every finite f64 is an integer multiple of 1 / _ONE


def gamma(n):
    return n * U / (1.0 - n * U)


def _i(x):
    """The f64 x as an exact integer multiple of 1 / _ONE."""
    n, d = float(x).as_integer_ratio()
    return n * (_ONE // d)


def _f(num, den=1, pw=1):
    """num / (den * _ONE**pw) rounded once to f64."""
    return float(Fraction(num, den * _ONE ** pw))


def seq_sum(terms):
    """s += term in f64, in order: what lane 0 of k_record does over the steps."""
    s = 0.0
    for t in terms:
        s = s + float(t)
    return s


def rate_bin(x, half_away=False):
    x = float(x) * 1000.0
    return int(math.floor(x + 0.5)) if half_away else int(np.rint(x))


def on_half(x):
    """The rate x, times 1000 in f64, sits exactly between two integers."""
    return (float(x) * 1000.0) % 1.0 == 0.5


def hist_of(pend, slow):
    h = np.zeros((2, BINS), np.uint32)
    for row, vals in ((0, pend), (1, slow)):
        for x in vals:
            h[row, rate_bin(x)] += 1
    return h


class RecEnv(TraceEnv):
    """TraceEnv with the ground-truth Record traces since reset / record_start."""

    def reset(self):
        obs = super().reset()
        self.record_start()
        return obs

    def record_start(self):
        """What vmp_record_enable / a reset / a restore does (k_record_init):
        nothing recorded, no open life. A VM present now is recorded from the
        next step on, as a life that starts there with length 0; the reference
        has no such case (Base.test records from reset), so for a recorder
        started mid-episode only raw() is defined, not summary()."""
        self.tr = {k: [] for k in (
            "vm_placements", "cpu", "memory", "waiting_ratio", "rewards", "dropped_requests",
            "total_requests", "served_requests", "suspended", "placed", "rank",
            "target_cpu_mean", "target_memory_mean", "sz_cpu", "sz_mem")}
        self.arrival_steps = [[] for _ in range(self.V)]
        self.closed = []                           # status arrays of the closed lives
        self.open = [[] for _ in range(self.V)]    # statuses of each slot's current life
        self.mid_start = bool(np.any(self.vm_placement <= self.WAIT))
        # events the vacuity conditions count
        self.n_susp = self.n_refill_run = self.n_refill_placed = 0
        self.max_pm = -1

    def step(self, action):
        self._pre = self.vm_placement.copy()
        out = super().step(action)
        self._record(out[1])
        return out

    def _run(self):
        self._mid = self.vm_placement.copy()       # after the action phase
        super()._run()

    def _accept(self):
        before = self.vm_placement.copy()
        super()._accept()
        self._new = (before == self.NULL) & (self.vm_placement == self.WAIT)

    def _record(self, reward):
        t, row = self.tr, len(self.tr["vm_placements"])
        pl = self.vm_placement.copy()
        for v in np.flatnonzero(self._new):
            if self.open[v]:
                self.closed.append(np.array(self.open[v], np.int64))
            self.open[v] = []
            self.arrival_steps[v].append(row + 2)  # the post-step timestep of a run from reset
        for v in np.flatnonzero(pl <= self.WAIT):
            self.open[v].append(int(pl[v]))
        ran = self._mid < self.WAIT
        self.n_susp += int(np.count_nonzero((self._pre < self.WAIT) & (self._mid == self.WAIT)))
        self.n_refill_run += int(np.count_nonzero(self._new & ran & (self._pre < self.WAIT)))
        self.n_refill_placed += int(np.count_nonzero(self._new & ran & (self._pre == self.WAIT)))
        used = pl[pl < self.P]
        if used.size:
            self.max_pm = max(self.max_pm, int(used.max()))
        ex = pl <= self.WAIT
        t["vm_placements"].append(pl)
        t["cpu"].append(self.cpu.copy())
        t["memory"].append(self.memory.copy())
        t["waiting_ratio"].append(self.waiting_ratio)
        t["rewards"].append(float(reward))
        t["dropped_requests"].append(self.dropped)
        t["total_requests"].append(self.total_requests)
        t["served_requests"].append(self.served)
        t["suspended"].append(self.suspend_action)
        t["placed"].append(self.place_action)
        t["rank"].append(int(np.unique(used).size))
        t["target_cpu_mean"].append(self.tcm)
        t["target_memory_mean"].append(self.tmm)
        t["sz_cpu"].append(self.vm_cpu[ex].copy())
        t["sz_mem"].append(self.vm_memory[ex].copy())

    # ------------------------------------------------------------- read-outs
    def lives(self):
        """Every life so far as its status array, the open ones included."""
        return self.closed + [np.array(o, np.int64) for o in self.open if o]

    def life_stats(self):
        """(closed lives that ran, never-run lives, open lives) for the vacuity conditions."""
        ran = sum(1 for s in self.closed if record_literal._first_run(s, self.WAIT) is not None)
        never = sum(1 for s in self.lives() if record_literal._first_run(s, self.WAIT) is None)
        return ran, never, sum(1 for o in self.open if o)

    def traces(self):
        t = dict(self.tr)
        t["vm_arrival_steps"] = self.arrival_steps
        t["total_cpu_requested"] = self.total_cpu_requested
        t["total_memory_requested"] = self.total_memory_requested
        return t

    def summary(self):
        assert not self.mid_start, "summary() is defined for a recorder started at reset only"
        return record_literal.summary(self.traces(), self.WAIT)

    def exact_means(self):
        """The means get_summary rounds, as exact fractions (None: no terms)."""
        pend, slow, life = record_literal.life_metrics(self.lives(), self.WAIT)

        def mean(vals, scale):
            vals = [int(np.rint(float(x) * scale)) for x in vals]
            return Fraction(sum(vals), scale * len(vals)) if vals else None

        return {"average VM life": mean(life, 1), "average pending": mean(pend, 1000),
                "average slowdown": mean(slow, 1000), "rank mean": mean(self.tr["rank"], 1)}

    def raw(self, rewards=None, naive=False):
        """dict(hist u32 [2, 1001], sums f64 [19], M f64 [19]) for this env. XMEM
        is left 0 (handle_raw fills it). rewards: the per-step rewards to sum
        (default: the literal's own). naive=True computes the bounded sums with
        np.sum in f64 instead of exactly."""
        t, P = self.tr, self.P
        T = len(t["vm_placements"])
        pend, slow, life = record_literal.life_metrics(self.lives(), self.WAIT)
        if not any(record_literal._first_run(s, self.WAIT) is not None for s in self.lives()):
            slow = []  # life_metrics' [0] default is summary_from_device's business
        s, M = np.zeros(NREC), np.zeros(NREC)
        rw = [float(x) for x in (t["rewards"] if rewards is None else rewards)]
        assert len(rw) == T
        s[STEPS] = T
        s[REWARD] = seq_sum(rw)
        s[REWARD_OK] = seq_sum(x for x in rw if x > -1e7)
        s[N_OK] = sum(1 for x in rw if x > -1e7)
        s[N_BAD] = sum(1 for x in rw if x < -1e7)
        s[RANK] = sum(t["rank"])
        s[DROP] = seq_sum(d / n if n else 0.0 for d, n in zip(t["dropped_requests"], t["total_requests"]))
        s[WAITING] = seq_sum(t["waiting_ratio"])
        s[LIFE_SUM] = sum(life)
        s[LIVES] = len(pend)
        cap = self.cfg.get("cap_target_util", True)
        for key, k1, k2, kv in (("cpu", CPU, CPU2, CPUVAR), ("memory", MEM, MEM2, MEMVAR)):
            if naive:
                x = np.array(t[key], np.float64).reshape(T, P)
                s[k1], s[k2], s[kv] = np.sum(x), np.sum(x * x), np.sum(np.var(x, axis=1))
                continue
            a1 = a2 = 0          # sum x, sum x^2            (units 1/_ONE, 1/_ONE^2)
            var = mag = 0        # sum_t sum_p (P x - S)^2, sum_t sum_p (P |x| + |S|)^2   (/ P^3 _ONE^2)
            for x in t[key]:
                xi = [_i(v) for v in x]
                S = sum(xi)
                a1 += S
                a2 += sum(v * v for v in xi)
                var += sum((P * v - S) ** 2 for v in xi)
                mag += sum((P * abs(v) + abs(S)) ** 2 for v in xi)
            s[k1], s[k2], s[kv] = _f(a1), _f(a2, 1, 2), _f(var, P ** 3, 2)
            M[k1] = _f(sum(abs(_i(v)) for x in t[key] for v in x))
            M[k2], M[kv] = s[k2], _f(mag, P ** 3, 2)
        for key, k in (("sz_cpu", TCM), ("sz_mem", TMM)):
            if naive:
                per = [np.sum(x) / P for x in t[key]]
                s[k] = np.sum([min(v, 1.0) if cap else v for v in per])
                continue
            tot = mag = 0        # units 1 / (P _ONE)
            for x in t[key]:
                S = sum(_i(v) for v in x)
                mag += S
                tot += min(S, P * _ONE) if cap else S
            s[k], M[k] = _f(tot, P), _f(mag, P)
        return dict(hist=hist_of(pend, slow), sums=s, M=M)


def xmem(envs, naive=False, mem=None, first=None):
    """VMP_REC_XMEM of every env of a handle and its magnitude: the sum over
    the env's recorded steps and the PMs of mem[e][p] * sum_s mem[s][p]; zeros
    for more than 64 envs. mem (default: each env's recorded rows): per env the
    memory rows of every step of the handle; first: per env the first of those
    steps that its recorder saw (a reset restarts one env's recorder while the
    others' go on, and every env's rows enter every other env's sum)."""
    N = len(envs)
    out, mag = np.zeros(N), np.zeros(N)
    if N > XMAX:
        return out, mag
    mem = [e.tr["memory"] for e in envs] if mem is None else mem
    first = [0] * N if first is None else first
    T, P = len(mem[0]), envs[0].P
    assert all(len(m) == T for m in mem)
    if naive:
        m = np.array(mem, np.float64).reshape(N, T, P)
        prod = m * m.sum(axis=0)
        out = np.array([np.sum(prod[e, first[e]:]) for e in range(N)])
        return out, np.abs(out)
    acc, amag = [0] * N, [0] * N
    for t in range(T):
        mi = [[_i(v) for v in m[t]] for m in mem]
        for p in range(P):
            col = sum(m[p] for m in mi)
            acol = sum(abs(m[p]) for m in mi)
            for e in range(N):
                if t >= first[e]:
                    acc[e] += mi[e][p] * col
                    amag[e] += abs(mi[e][p]) * acol
    return (np.array([_f(a, 1, 2) for a in acc]), np.array([_f(a, 1, 2) for a in amag]))


def handle_raw(envs, rewards=None, naive=False, mem=None, first=None):
    """raw() of every env of a handle with XMEM filled in. rewards: [T, N] or
    None; mem, first: see xmem (env i sums rewards[first[i]:, i])."""
    xs, xm = xmem(envs, naive, mem, first)
    out = []
    for i, e in enumerate(envs):
        f = 0 if first is None else first[i]
        r = e.raw(None if rewards is None else np.asarray(rewards)[f:, i], naive)
        r["sums"][XMEM], r["M"][XMEM] = xs[i], xm[i]
        out.append(r)
    return out


# ---------------------------------------------------------------- the kernel's rule
class RuleRec:
    """k_record's per-slot update and k_record_close for one env, on the
    kernel's inputs alone. no_susp / no_placed / half_away: the rule with one
    clause dropped, or rounding half away from zero: each must be told apart
    from the truth by some workload."""

    def __init__(self, P, V, placement, no_susp=False, no_placed=False, half_away=False):
        self.P, self.V = int(P), int(V)
        self.no_susp, self.no_placed, self.half_away = no_susp, no_placed, half_away
        self.prev = np.asarray(placement, np.int64).copy()
        self.n = np.zeros(V, np.int64)
        self.al = np.full(V, -1, np.int64)
        self.wt = np.zeros(V, np.int64)
        self.hist = np.zeros((2, BINS), np.uint32)
        self.life_sum = self.lives = 0

    def _close(self, n, al, w, hist):
        if n == 0:
            return 0, 0
        if al > 0:
            hist[0, rate_bin((al + 1.0) / float(n), self.half_away)] += 1
            life = n - al - 1
            hist[1, 0 if life == 0 else rate_bin(float(w) / float(life), self.half_away)] += 1
            return life, 1
        hist[0, 1000] += 1
        return 0, 1

    def update(self, action, valid, placement):
        P, WAIT = self.P, self.P
        for v in range(self.V):
            pv, a, ok, st = int(self.prev[v]), int(action[v]), bool(valid[v]), int(placement[v])
            placed = pv == WAIT and ok and 0 <= a < P and not self.no_placed
            susp = pv < P and ok and a == WAIT and not self.no_susp
            arrival = st == WAIT and not (pv == WAIT and not placed) and not susp
            if arrival:
                ls, lc = self._close(int(self.n[v]), int(self.al[v]), int(self.wt[v]), self.hist)
                self.life_sum += ls
                self.lives += lc
                self.n[v], self.al[v], self.wt[v] = 1, -1, 0
            elif st <= WAIT:
                idx = int(self.n[v])
                self.n[v] += 1
                if st < WAIT:
                    if self.al[v] < 0:
                        self.al[v] = idx
                elif self.al[v] >= 0:
                    self.wt[v] += 1
            self.prev[v] = st

    def read(self):
        """(hist, LIFE_SUM, LIVES) as vmp_record_read shows them: the open lives
        closed into a copy."""
        hist, ls, lc = self.hist.copy(), self.life_sum, self.lives
        for v in range(self.V):
            a, b = self._close(int(self.n[v]), int(self.al[v]), int(self.wt[v]), hist)
            ls, lc = ls + a, lc + b
        return hist, ls, lc


# ------------------------------------------------------------- the comparison rule
def bound_n(k, P, V, N, T):
    if k in (CPU, MEM, CPU2, MEM2):
        return P + T + 8
    if k in (TCM, TMM):
        return V + T + 8
    if k in (CPUVAR, MEMVAR):
        return 2 * (P + T + 8)
    assert k == XMEM
    return N + P + T + 8


RATIOS = {}  # quantity -> [max |device - truth|, its bound, max err / bound]


def judge(hist, sums, truth, P, V, N, what=""):
    """The device's (hist, sums) of one env against truth = raw(): a list of
    mismatch descriptions (empty: accepted). hist and the EXACT sums must be
    bit-exact; a BOUNDED sum k must lie within gamma(bound_n(k)) * M[k] of the
    truth. Records max error / bound per quantity in RATIOS."""
    bad = []
    hist, sums = np.asarray(hist).view(np.uint32).reshape(2, BINS), np.asarray(sums, np.float64)
    T = int(truth["sums"][STEPS])
    for row, name in ((0, "pending"), (1, "slowdown")):
        d = np.flatnonzero(hist[row] != truth["hist"][row])
        if d.size:
            bad.append(f"{what} hist {name} bins {d[:6]}: {hist[row][d[:6]]} != {truth['hist'][row][d[:6]]}")
    for k in EXACT:
        if not sums[k] == truth["sums"][k]:
            bad.append(f"{what} {NAMES[k]}: {sums[k]!r} != {truth['sums'][k]!r} (bit-exact)")
    for k in BOUNDED:
        err = abs(float(sums[k]) - float(truth["sums"][k]))
        bound = gamma(bound_n(k, P, V, N, T)) * float(truth["M"][k])
        ratio = err / bound if bound > 0 else (0.0 if err == 0 else math.inf)
        rec = RATIOS.setdefault(NAMES[k], [0.0, 0.0, 0.0])
        if ratio >= rec[2]:
            rec[0], rec[1], rec[2] = err, bound, ratio
        if not ratio <= 1.0:
            bad.append(f"{what} {NAMES[k]}: |{sums[k]!r} - {truth['sums'][k]!r}| = {err:.3e} > "
                       f"bound {bound:.3e} (ratio {ratio:.3f})")
    return bad


def summary_mismatch(dev, lit, exact_means=None):
    """record_summary()'s dict against RecEnv.summary(): integer and rounded
    rate keys equal, the rest within the 1e-3 tests/test_gpu_record.py allows.
    exact_means (RecEnv.exact_means()): where the exact mean of a key, times
    1000, lies exactly between two integers, the reference's own rounded value
    is decided by the rounding noise of its np.mean (summation order), so
    either neighbour is accepted there, and nowhere else."""
    bad = []
    equal = ("average VM life", "average pending", "median pending", "max pending", "average slowdown",
             "median slowdown", "max slowdown", "drop rate", "rank mean")
    for k, v in lit.items():
        d = dev[k]
        if isinstance(v, (int, np.integer)) or k in equal:
            tie = exact_means is not None and exact_means.get(k) is not None and \
                (exact_means[k] * 1000) % 1 == Fraction(1, 2)
            if tie and abs(float(d) - float(v)) <= 1.0000001e-3:
                continue
            if not (d == v or (np.isnan(float(d)) and np.isnan(float(v)))):
                bad.append((k, d, v))
        elif np.isnan(float(v)) or np.isnan(float(d)):
            if not (np.isnan(float(v)) and np.isnan(float(d))):
                bad.append((k, d, v))
        elif abs(float(d) - float(v)) > 1e-3 + 1e-9 * abs(float(v)):
            bad.append((k, d, v))
    return bad


# ------------------------------------------------------------------ workloads
BASE = dict(pms=12, vms=90, allow_null_action=True, training_steps=10000, eval_steps=100000, seed=0,
            sequence="uniform", cap_target_util=True, beta=0.5, arrival_rate=1.0, service_length=50)


def _trace(per, g, size, runtime):
    from vmp.trace import Trace
    n = int(np.sum(per))
    return Trace(np.r_[0, np.cumsum(per)].astype(np.int64), g.integers(size[0], size[1] + 1, n),
                 g.integers(size[0], size[1] + 1, n), runtime(n))


def mixed(P, V, n, steps, seed=0):
    """Moderate load, service lengths of tens of steps (one request in six
    runs for a single step: placed and finished at once, a life that never
    ran), so random suspensions hit running VMs and waiting VMs queue up. One
    slot (V 1) gets a request every step and runtimes 1..4."""
    out = []
    for i in range(n):
        g = np.random.default_rng(1000 * seed + 7 * i + P + V)
        if V == 1:
            out.append(_trace(np.ones(steps, np.int64), g, (5, 100),
                              lambda m: np.where(g.random(m) < 0.3, 1, g.integers(2, 5, m))))
            continue
        rate = min(V / 15.0, P / 3.5)
        out.append(_trace(g.poisson(rate, steps), g, (5, 40),
                          lambda m: np.where(g.random(m) < 1 / 6, 1, g.integers(5, 31, m))))
    return out


def churn(n, steps=150):
    """As reqlog_literal.extra_traces('churn'), for n envs: 6 requests a step
    with runtimes 1..3."""
    out = []
    for i in range(n):
        g = np.random.default_rng(500 + i)
        out.append(_trace(np.full(steps, 6), g, (5, 40), lambda m: g.integers(1, 4, m)))
    return out


def drops(V, n, steps):
    """V / 3 requests a step with runtimes 1..12: more than the NULL slots in most steps."""
    out = []
    for i in range(n):
        g = np.random.default_rng(900 + i + V)
        out.append(_trace(np.full(steps, max(2, V // 3)), g, (5, 60), lambda m: g.integers(1, 13, m)))
    return out


def empty(n, steps):
    from vmp.trace import Trace
    z = np.zeros(0, np.int64)
    return [Trace(np.zeros(steps + 1, np.int64), z, z, z) for _ in range(n)]


TIES_STEPS, TIES_BATCH2 = 120, 85


def _ties_plans(i):
    """The hand-made plans of env i, one per VM of a batch, as (hold, n, w, a):
    the VM waits `hold` statuses (the arrival's included), is placed and runs.
    w == 0: a life of n statuses, hold + 1 odd, n 16 or 80: pending ends in .5.
    w > 0: 16 statuses after the first running one, w of them (odd) suspended
    from offset a: slowdown w / 16 ends in .5."""
    plans = [(h, 16, 0, 0) for h in (2, 4, 6, 8, 10, 12, 14)]
    plans += [(h, 80, 0, 0) for h in (2, 6, 10, 22, 38, 54)]   # (h + 1) * 12.5 ends in .5
    plans += [(1 + (k + i) % 3, 0, w, a) for k, (w, a) in enumerate(((1, 3), (3, 2), (5, 4), (7, 1),
                                                                     (9, 5), (11, 2), (13, 1)))]
    return plans[i % len(plans):] + plans[:i % len(plans)]  # the envs differ in slot order


def _plan_statuses(plan, pm):
    """(the desired status per row of the life, the runtime that ends it there)."""
    h, n, w, a = plan
    if w == 0:
        return [-1] * h + [pm] * (n - h), n - h + 1
    seq = [-1] * h + [pm] + [pm] * 16
    for j in range(a, a + w):
        seq[h + j] = -1
    return seq, 18 - w


def ties(n):
    """Two batches of hand-planned VMs, the second refilling the slots of the
    first at step TIES_BATCH2 (its arrivals close the first batch's lives), 1 %
    sizes so every placement is valid. Driven by ties_actions."""
    from vmp.trace import Trace
    out = []
    for i in range(n):
        plans = _ties_plans(i)
        rt = [_plan_statuses(p, 0)[1] for p in plans]
        per = np.zeros(TIES_STEPS, np.int64)
        per[0] = per[TIES_BATCH2] = len(plans)
        one = np.ones(2 * len(plans), np.int64)
        out.append(Trace(np.r_[0, np.cumsum(per)], one, one, np.array(rt + rt, np.int64)))
    return out


def ties_actions(env, i, step):
    """The driver's actions of env i for 0-based step `step` (it writes row `step`)."""
    a = env.vm_placement.copy()
    plans = _ties_plans(i)
    for v, plan in enumerate(plans):
        if a[v] > env.WAIT:
            continue
        seq, _ = _plan_statuses(plan, v % env.P)
        j = step - (TIES_BATCH2 if step > TIES_BATCH2 else 0)  # row of the life: arrival = row 0
        if 0 < j < len(seq):
            a[v] = env.WAIT if seq[j] < 0 else seq[j]
    return a.astype(np.int64)


# ------------------------------------------------------------------ the case table
def _case(P, V, N, workload, steps, reward):
    return dict(P=P, V=V, N=N, workload=workload, steps=steps, reward=reward)


CASES = {}
for _P, _V in ((1, 1), (63, 63), (64, 64), (65, 65), (128, 129), (129, 257)):
    CASES[f"border-P{_P}-V{_V}"] = _case(_P, _V, 5, "mixed", 120, "kl")
for _N in (1, 3, 4, 5, 9):
    CASES[f"waves-N{_N}"] = _case(12, 90, _N, "mixed", 120, "ut")
CASES["waves-N5-churn"] = _case(12, 90, 5, "churn", 120, "ut")
CASES["cross-N64"] = _case(12, 90, 64, "mixed", 40, "wr")
CASES["cross-N65"] = _case(12, 90, 65, "mixed", 40, "wr")
CASES["pitch-V1025"] = _case(20, 1025, 3, "drops", 40, "wr")
CASES["ties"] = _case(12, 90, 4, "ties", TIES_STEPS, "wr")
CASES["empty"] = _case(12, 90, 4, "empty", 20, "wr")
CASES["drops"] = _case(12, 90, 4, "drops", 60, "wr")


def case_cfg(c):
    return dict(BASE, pms=c["P"], vms=c["V"], reward_function=c["reward"])


def case_traces(c):
    w = c["workload"]
    if w == "mixed":
        return mixed(c["P"], c["V"], c["N"], c["steps"])
    if w == "churn":
        return churn(c["N"], c["steps"])
    if w == "drops":
        return drops(c["V"], c["N"], c["steps"])
    if w == "empty":
        return empty(c["N"], c["steps"])
    assert w == "ties", w
    return ties(c["N"])


def make_envs(c, traces=None):
    traces = case_traces(c) if traces is None else traces
    envs = [RecEnv(case_cfg(c), t.offs, t.cpu, t.mem, t.runtime) for t in traces]
    for e in envs:
        e.eval_mode = True
    return envs


class Run:
    """One case run on the literal alone: acts / valids [T, N, V], the
    placements before every step (pre [T, N, V]), the envs at the end and deep
    copies of them after the steps listed in `snaps`."""


def run(c, snaps=(), seed=11, traces=None, steps=None, before_step=None):
    """Drive make_envs(c) with the case's seeded actions. before_step(envs, s):
    a hook run before step s (a reset, a restore)."""
    r = Run()
    r.case, r.traces = c, case_traces(c) if traces is None else traces
    r.envs = make_envs(c, r.traces)
    g = np.random.default_rng(seed)
    T = c["steps"] if steps is None else steps
    N, V = c["N"], c["V"]
    r.acts, r.valids, r.pre = (np.zeros((T, N, V), np.int64), np.zeros((T, N, V), np.uint8),
                               np.zeros((T, N, V), np.int64))
    r.post = np.zeros((T, N, V), np.int64)
    r.snaps = {}
    for s in range(T):
        if before_step is not None:
            before_step(r.envs, s)
        for i, e in enumerate(r.envs):
            a = ties_actions(e, i, s) if c["workload"] == "ties" else random_actions(g, e)
            r.pre[s, i] = e.vm_placement
            r.acts[s, i] = a
            r.valids[s, i] = e.step(a)[3]
            r.post[s, i] = e.vm_placement
        if s + 1 in snaps:
            r.snaps[s + 1] = copy.deepcopy(r.envs)
    return r


@functools.lru_cache(maxsize=None)
def run_case(name, snaps=()):
    """run(CASES[name]), computed once per process and left unchanged by its users."""
    return run(CASES[name], snaps)


# --------------------------------------------------- reset and restore scenarios
FURTHER = "waves-N5"  # 12 / 90, N 5, mixed: the shape of the further tests
RESET_AT, RESET_ENVS, RESET_STEPS = 40, (1, 3), 100
SNAP_AT, RESTORE_AT, RESTORE_STEPS = 20, 50, 90


@functools.lru_cache(maxsize=None)
def run_reset():
    """RESET_AT steps, envs RESET_ENVS reset (their truth and their trace
    position restart), then on to RESET_STEPS. r.waiting_before[i]: the slots of
    env i that stood at WAIT just before its reset; r.mem, r.first: for xmem."""
    waiting, before = {}, {}

    def hook(envs, s):
        if s == RESET_AT:
            for i in RESET_ENVS:
                waiting[i] = np.flatnonzero(envs[i].vm_placement == envs[i].WAIT)
                before[i] = list(envs[i].tr["memory"])
                envs[i].reset()

    r = run(CASES[FURTHER], steps=RESET_STEPS, before_step=hook)
    r.waiting_before = waiting
    r.first = [RESET_AT if i in RESET_ENVS else 0 for i in range(len(r.envs))]
    r.mem = [before.get(i, []) + e.tr["memory"] for i, e in enumerate(r.envs)]
    return r


@functools.lru_cache(maxsize=None)
def run_restore():
    """Snapshot before step SNAP_AT, restore before step RESTORE_AT: the envs
    go back to the snapshot and their truth starts recording there
    (record_start), then on to RESTORE_STEPS steps in all."""
    saved = {}

    def hook(envs, s):
        if s == SNAP_AT:
            saved["envs"] = copy.deepcopy(envs)
        if s == RESTORE_AT:
            envs[:] = copy.deepcopy(saved["envs"])
            for e in envs:
                e.record_start()

    return run(CASES[FURTHER], steps=RESTORE_STEPS, before_step=hook)
