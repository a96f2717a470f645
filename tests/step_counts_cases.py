"""The cases of tests/test_step_counts_cpu.py and tests/test_gpu_step_counts.py
(test infrastructure, numpy and the C oracle only: importable without a GPU).

The wave env kernels take the VM counts of a step's stats (existing VMs n_ex,
waiting VMs n_w, "a NULL slot is left") from the step's events: the NULL count
before the accept phase, the accepted requests k, the accepted placements and
the suspensions. The cases below walk the oracle through steps of every kind
those counts can go wrong at; `classes(walk)` counts them.

A case fixes P, V and the workload; a walk adds the policy, the reward and who
chooses the actions ("heur": the policy itself; "ext": ext_actions below, random
and mostly invalid, suspensions included). The oracle never sees a device value.
"""
from dataclasses import dataclass

import numpy as np

from oracle import oracle as O
from tests import trace_literal as TL

N_ENV = 6
SEEDS = (4, 11, (1 << 32) + 5, 1234567, 0, (1 << 40) + 3)  # one seed above 2^32
POLICIES = ("firstfit", "bestfit")
REWARDS = ("wr", "ut", "kl")
ROLLS = (1, 7, 100)  # the fused drive repeats these launch lengths
MIN_OCCURRENCES = 5


@dataclass(frozen=True)
class Case:
    name: str
    P: int
    V: int
    lam: float
    L: float
    steps: int
    exhausts: bool = True  # the NULL slots run out within the plan
    note: str = ""

    def cfg(self, reward):
        return dict(pms=self.P, vms=self.V, arrival_rate=self.lam, service_length=self.L,
                    training_steps=10000, eval_steps=100000, seed=0, reward_function=reward,
                    sequence="uniform", cap_target_util=True, beta=0.5, allow_null_action=True)


# lam and L (where the cases' definition leaves them open) are chosen so that
# the PMs saturate, VMs wait, the table fills and finishers free slots again
# within the plan; tests/test_step_counts_cpu.py holds every class to at least
# MIN_OCCURRENCES env-steps per walk.
# The two P100 / V1000 cases cannot exhaust their NULL slots: a walk has at
# most 400 steps, which at lam 1.8182 offer about 730 requests to 1000 slots
# (at lam 0.182 about 73; that case is there because they never run out). The
# exhaustion classes at VPT 16 are p50v1024's.
CASES = (
    Case("p10v30", 10, 30, 2.0, 12.0, 220, note="VPT 1"),
    Case("p20v64", 20, 64, 3.0, 16.0, 220, note="VPT 1, full row"),
    Case("p20v65", 20, 65, 3.0, 16.0, 220, note="VPT 2, one live slot in the last row"),
    Case("p100v1000", 100, 1000, 1.8182, 150.0, 400, exhausts=False,
         note="VPT 16, 24 pad lanes; the headline's instantiation"),
    Case("p100v1000-low", 100, 1000, 0.182, 150.0, 400, exhausts=False,
         note="NULL slots never run out"),
    Case("p50v1024", 50, 1024, 40.0, 30.0, 220, note="VPT 16, no pad lane"),
)
BY_NAME = {c.name: c for c in CASES}
TRACE_CASES = ("p20v65", "p100v1000")


def ext_actions(rng, P, A, placement, heur):
    """One env's proposed actions for an external step, from the oracle's state
    alone: the policy's action, then 15 % of the running VMs sent to WAIT, and
    half of all slots given any index in [-1, A] (out of range at both ends,
    migrations, placements of NULL slots and on full PMs: mostly invalid)."""
    V = placement.size
    a = heur.copy()
    a[(placement < P) & (rng.random(V) < 0.15)] = P
    rnd = rng.random(V) < 0.5
    a[rnd] = rng.integers(-1, A + 1, size=int(rnd.sum()))
    return a


@dataclass
class Walk:
    case: Case
    policy: str
    reward: str
    mode: str
    obs: np.ndarray      # [T, N, D] f32
    rew: np.ndarray      # [T, N]
    done: np.ndarray     # [T, N]
    act: np.ndarray      # [T, N, V] the actions stepped with
    valid: np.ndarray    # [T, N, V]
    pre_pl: np.ndarray   # [T, N, V] placement before the step
    ctr: np.ndarray      # [T, N, 6] counters after the step
    n_null: np.ndarray   # [T, N] NULL slots after the step
    n_wait: np.ndarray   # [T, N] waiting VMs after the step
    state: list          # per env: state() at the end
    stats: np.ndarray    # [N, 5] at the end
    traces: list = None  # per env (offs, cpu, mem, runtime), want_trace only


def walk(case, policy, reward, mode, want_trace=False):
    """The oracle's record of `case.steps` steps of every env."""
    rng = np.random.default_rng([77, CASES.index(case), POLICIES.index(policy), mode == "ext"])
    T, N, V, P = case.steps, N_ENV, case.V, case.P
    oes = []
    for s in SEEDS:
        e = O.OracleEnv(dict(case.cfg(reward), seed=int(s)))
        e.reset(int(s))
        oes.append(e)
    A = oes[0].A
    heur = (lambda e: e.firstfit()) if policy == "firstfit" else (lambda e: e.bestfit())
    w = Walk(case, policy, reward, mode,
             obs=np.zeros((T, N, 3 * V + 2 * P), np.float32), rew=np.zeros((T, N)),
             done=np.zeros((T, N), bool), act=np.zeros((T, N, V), np.int64),
             valid=np.zeros((T, N, V), np.uint8), pre_pl=np.zeros((T, N, V), np.int64),
             ctr=np.zeros((T, N, 6), np.int64), n_null=np.zeros((T, N), np.int64),
             n_wait=np.zeros((T, N), np.int64), state=None, stats=None)
    pre = [e.state() for e in oes]
    pl = [p[0] for p in pre]
    states = [[] for _ in oes]
    for t in range(T):
        for i, e in enumerate(oes):
            a = heur(e)
            if mode == "ext":
                a = ext_actions(rng, P, A, pl[i], a)
            w.pre_pl[t, i] = pl[i]
            w.act[t, i] = a
            w.obs[t, i], w.rew[t, i], w.done[t, i], w.valid[t, i] = e.step(a)
            st = e.state()
            if want_trace:
                states[i].append(st)
            pl[i] = st[0]
            w.ctr[t, i] = e.counters()[0]
            w.n_null[t, i] = np.count_nonzero(pl[i] == P + 1)
            w.n_wait[t, i] = np.count_nonzero(pl[i] == P)
    w.state = [e.state() for e in oes]
    w.stats = np.stack([e.counters()[1] for e in oes])
    if want_trace:
        w.traces = [TL.derive_trace(P, pre[i], w.act[:, i], w.valid[:, i], states[i], w.ctr[:, i])
                    for i in range(N)]
    return w


def classes(w):
    """How many env-steps of the walk fall into each class (see the module's
    docstring and tests/test_step_counts_cpu.py)."""
    P, V = w.case.P, w.case.V
    d = np.diff(np.concatenate([np.zeros((1,) + w.ctr.shape[1:], np.int64), w.ctr]), axis=0)
    arrivals, served, susp, placed, dropped = (d[:, :, j] for j in range(5))
    k = arrivals - dropped
    null_pre = w.n_null + k  # NULL slots when the accept phase began
    proposed = (w.pre_pl == P) & (w.act >= 0) & (w.act < P)
    out = {
        "finisher": served > 0,
        "no_finisher": served == 0,
        "placed_no_finisher": (placed > 0) & (served == 0),
        "leaves_null": w.n_null > 0,
        "fills_last_null": (k > 0) & (w.n_null == 0),
        "arrivals_over_nulls": (arrivals > null_pre) & (null_pre > 0),
        # counting the padded rows as VMs would change waiting / existing
        "pad_rows_matter": (w.n_wait > 0) & (V % 64 != 0),
        "suspension": susp > 0,
        "rejected_placement": (proposed & (w.valid == 0)).any(axis=2),
        "carried_wait": w.n_wait > 0,
    }
    return {name: int(np.count_nonzero(m)) for name, m in out.items()}


def required(case, mode):
    """The classes a walk of `case` must show at least MIN_OCCURRENCES times."""
    req = ["finisher", "no_finisher", "placed_no_finisher", "leaves_null", "carried_wait"]
    if case.exhausts:
        req += ["fills_last_null", "arrivals_over_nulls"]
    if case.V % 64 != 0:
        req.append("pad_rows_matter")
    if mode == "ext":
        req += ["suspension", "rejected_placement"]
    return req
