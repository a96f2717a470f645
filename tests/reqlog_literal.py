"""Ground truth and rule of the per-request outcome log (include/vmp.h,
vmp_reqlog_*), in numpy.

TEST INFRASTRUCTURE ONLY. Two independent statements of one log:

LogEnv     a tests/trace_literal.TraceEnv that knows which slot took which
           request, because it watches its own action phase, _run and _accept:
           the ground truth. It reads neither actions nor validity flags.
RuleLog    the device kernel's rule (k_reqlog, csrc/vmp_reqlog.hip) restated:
           it sees only what the kernel sees, per slot the previous and the
           new post-step placement, the action and its validity, and per env
           the timestep and total_requests, and derives arrivals, ranks,
           finishes and drops from them. open_counts=True keeps WAIT_STEPS as
           the kernel stores it (written at events only, an open stretch of
           waiting closed by read(), as vmp_reqlog_read closes it in its copy).

tests/test_reqlog_cpu.py holds the two equal on workloads with churn, bursts,
drops and suspensions; tests/test_gpu_reqlog.py compares the device log with
LogEnv. A row is int32 [6]: SLOT, ARRIVED, PLACED, FINISHED, SUSPENDS,
WAIT_STEPS; meta is int64 [3]: FIRST, NEXT, LOST (include/vmp.h VMP_RQ_*).
"""
import numpy as np

from tests.trace_literal import TraceEnv

SLOT, ARRIVED, PLACED, FINISHED, SUSPENDS, WAIT_STEPS, NF = 0, 1, 2, 3, 4, 5, 6
FIRST, NEXT, LOST = 0, 1, 2


def empty_rows(capacity):
    rows = np.zeros((int(capacity), NF), np.int32)
    rows[:, SLOT] = -2
    return rows


class LogEnv(TraceEnv):
    """TraceEnv with the ground-truth request log of `capacity` rows (default:
    the trace's request count, at least 1)."""

    def __init__(self, cfg, offs, cpu, mem, runtime, capacity=None):
        self.capacity = max(1, int(np.asarray(offs)[-1])) if capacity is None else int(capacity)
        super().__init__(cfg, offs, cpu, mem, runtime)

    def reset(self):
        obs = super().reset()
        self.log_start()
        return obs

    def log_start(self):
        """What vmp_reqlog_enable / a reset does: nothing observed, nothing tracked."""
        self.rows = empty_rows(self.capacity)
        self.meta = np.array([self.total_requests, self.total_requests, 0], np.int64)
        self.slot_req = np.full(self.V, -1, np.int64)

    def step(self, action):
        self._t = self.timestep
        self._pre = self.vm_placement.copy()
        return super().step(action)

    def _tracked(self, mask):
        v = np.flatnonzero(mask & (self.slot_req >= 0))
        return v, self.slot_req[v]

    def _run(self):
        # the action phase is over: what it did to the slots
        now = self.vm_placement
        _, ids = self._tracked((self._pre == self.WAIT) & (now < self.WAIT))
        first = ids[self.rows[ids, PLACED] == 0]
        self.rows[first, PLACED] = self._t
        _, ids = self._tracked((self._pre < self.WAIT) & (now == self.WAIT))
        self.rows[ids, SUSPENDS] += 1
        before = now.copy()
        super()._run()
        v, ids = self._tracked((before < self.WAIT) & (self.vm_placement == self.NULL))
        self.rows[ids, FINISHED] = self._t
        self.slot_req[v] = -1

    def _accept(self):
        before = self.vm_placement.copy()
        id0 = self.total_requests
        super()._accept()
        slots = np.flatnonzero((before == self.NULL) & (self.vm_placement == self.WAIT))
        for k, v in enumerate(slots):  # ascending slots take the step's first requests in order
            rid = id0 + k
            if rid < self.capacity:
                self.slot_req[v] = rid
                self.rows[rid] = (v, self._t, 0, 0, 0, 0)
        for rid in range(id0 + slots.size, self.total_requests):  # dropped and consumed
            if rid < self.capacity:
                self.rows[rid, SLOT], self.rows[rid, ARRIVED] = -1, self._t
        self.meta[NEXT] = self.total_requests
        self.meta[LOST] += sum(1 for rid in range(id0, self.total_requests) if rid >= self.capacity)
        _, ids = self._tracked(self.vm_placement == self.WAIT)
        self.rows[ids, WAIT_STEPS] += 1


class RuleLog:
    """The kernel's update rule for one env, on the kernel's inputs alone."""

    def __init__(self, P, V, capacity, placement, total_requests, open_counts=False):
        self.P, self.V, self.cap = int(P), int(V), int(capacity)
        self.open = bool(open_counts)
        self.rows = empty_rows(capacity)
        self.meta = np.array([total_requests, total_requests, 0], np.int64)
        self.ids = np.full(V, -1, np.int64)
        self.prev = np.asarray(placement, np.int64).copy()

    def update(self, t, action, valid, placement, total_requests):
        P, WAIT, NULL = self.P, self.P, self.P + 1
        prev_total = int(self.meta[NEXT])
        rank = 0
        for v in range(self.V):
            pv, a, ok, st, i = (int(self.prev[v]), int(action[v]), bool(valid[v]),
                                int(placement[v]), int(self.ids[v]))
            placed = pv == WAIT and ok and 0 <= a < P
            susp = pv < P and ok and a == WAIT
            arrival = st == WAIT and not (pv == WAIT and not placed) and not susp
            if i >= 0:
                r = self.rows[i]
                if placed and r[PLACED] == 0:
                    r[PLACED] = t
                if susp:
                    r[SUSPENDS] += 1
                if self.open:  # a stretch of waiting from step s to a placement in p: p - s
                    r[WAIT_STEPS] += (t - 1 if placed else 0) + (1 - t if susp else 0)
                running = placed or (pv < P and not susp)
                if running and (st == NULL or arrival):
                    r[FINISHED] = t
                    i = -1
                elif st == WAIT and not self.open:
                    r[WAIT_STEPS] += 1
            if arrival:
                rid = prev_total + rank
                rank += 1
                i = -1
                if rid < self.cap:
                    i = rid
                    self.rows[rid, SLOT], self.rows[rid, ARRIVED] = v, t
                    self.rows[rid, WAIT_STEPS] = 1 - t if self.open else 1
            self.ids[v] = i
            self.prev[v] = st
        for rid in range(prev_total + rank, min(int(total_requests), self.cap)):
            self.rows[rid, SLOT], self.rows[rid, ARRIVED] = -1, t
        self.meta[LOST] += max(0, int(total_requests) - max(prev_total, self.cap))
        self.meta[NEXT] = total_requests

    def read(self, last_t):
        """The rows as a read shows them after the step that started at timestep
        last_t: the open stretches of the VMs waiting now closed in a copy."""
        rows = self.rows.copy()
        if self.open:
            ids = self.ids[(self.ids >= 0) & (self.prev == self.P)]
            rows[ids, WAIT_STEPS] += last_t
        return rows


# ------------------------------------------------------------------ workloads
def extra_traces(kind):
    """Two workloads beyond tests/test_gpu_trace._generated, four traces each:
    'churn'    6 requests a step with runtimes 1..3: VMs placed and finished in
               one step, their slots refilled in the same step;
    'burst200' 200 requests in the first step (V 90: 110 drops, more than one
               wave of dropped ids), then a light workload."""
    from vmp.trace import Trace
    out = []
    for s in range(4):
        g = np.random.default_rng(500 + s)
        if kind == "churn":
            n = 6 * 150
            out.append(Trace(np.arange(151) * 6, g.integers(5, 41, n), g.integers(5, 41, n),
                             g.integers(1, 4, n)))
        else:
            assert kind == "burst200"
            per = g.poisson(3.0, 149)
            n = int(per.sum())
            out.append(Trace(np.r_[0, 200, 200 + np.cumsum(per)],
                             np.r_[g.integers(1, 101, 200), g.integers(10, 101, n)],
                             np.r_[g.integers(1, 101, 200), g.integers(10, 101, n)],
                             np.r_[g.integers(1, 30, 200), g.integers(1, 20, n)]))
    return out


def random_actions(g, env):
    """External actions that exercise the rule's ambiguities: half of the slots
    keep their placement (always valid), the others draw any action in
    0..P+1, so waiting VMs are placed (if the PM has room), running VMs are
    suspended (action WAIT) or sent to another PM (invalid), empty slots are
    mostly addressed invalidly."""
    a = env.vm_placement.copy()
    draw = g.random(env.V) < 0.5
    a[draw] = g.integers(0, env.P + 2, int(draw.sum()))
    return a.astype(np.int64)


def first_fit(env):
    """Sequential first fit on the literal's f64 loads; other slots stay."""
    a = env.vm_placement.copy()
    cpu, mem = env.cpu.copy(), env.memory.copy()
    for v in np.flatnonzero(env.vm_placement == env.WAIT):
        fit = np.flatnonzero((cpu + env.vm_cpu[v] <= 1) & (mem + env.vm_memory[v] <= 1))
        if fit.size:
            a[v] = fit[0]
            cpu[fit[0]] += env.vm_cpu[v]
            mem[fit[0]] += env.vm_memory[v]
    return a.astype(np.int64)


def identities(rows, counters):
    """The four counter identities of a log that saw every request of the env:
    counters = (total_requests, served, suspend_action, place_action, dropped, ...)."""
    total, served, susp, _, dropped = (int(x) for x in counters[:5])
    return (np.count_nonzero(rows[:, SLOT] >= 0) == total - dropped
            and np.count_nonzero(rows[:, SLOT] == -1) == dropped
            and np.count_nonzero(rows[:, FINISHED] > 0) == served
            and int(rows[:, SUSPENDS].sum()) == susp)
