"""The case table of tests/test_env_cases_cpu.py and tests/test_gpu_env_instances.py
(test infrastructure, numpy and the C oracle only: importable without a GPU).

Every env step kernel instantiation (k_env / k_env_ext / k_env_tr / k_env_ext_tr
for VPT 1 / 2 / 4 / 8 / 16, k_env_big for SPT 4 / 8 / 16 / 40, each with the
config's, a per-env or a trace workload) is selected by at least one case, at
the smallest V on either side of every slot border.

A case fixes the config, the seeds, the request source and a segment plan:

  1. n_full  per-step heuristic steps, actions and validity requested
  2. n_ext   external-action steps (ext_actions below), mask_out requested
  3.         mask / mask_bits / obs / act-only, without a step
  4. rolls   fused rollouts of K steps, one after the other
  5. n_bare  per-step heuristic steps with nothing requested

`run_oracle(case)` walks the C oracle alone through the plan and records what
the GPU test compares with, and what the CPU test needs to show that the case
is not vacuous. It never sees a device value: the external actions are built
from the oracle's own state with the case's seeded generator, and a trace case
replays the trace its own oracle run accepted (tests.trace_literal.derive_trace,
which takes the validity flags and so supports rejected proposals: the trace
handle is fed the same proposed actions, the rejected ones included).
"""
import math
from dataclasses import dataclass, field

import numpy as np

from oracle import oracle as O
from tests import trace_literal as TL

N_ENV = 6
# one seed above 2^32 in every case (the seeding reads all 64 bits)
SEEDS = (4, 11, (1 << 32) + 5, 1234567, 0, (1 << 40) + 3)
COMBOS = (("wr", "firstfit"), ("ut", "bestfit"), ("kl", "bestfit"))
N_FULL, N_EXT, K_ROLL, N_BARE = 30, 25, 23, 15
# episodes end inside the external-action segment: `done` is compared on both sides of it
TRAINING_STEPS = 50

WAVE_V = (1, 2, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1024)
BLOCK_V = (1025, 2048, 2049, 4096, 4097)
FORCED_V = (1, 255, 256, 257, 1024)
MASK_P = (1, 2, 30, 31, 32, 62, 63, 64, 65)
SPLIT_K = (1, 2, 256, 257)

K_BIG_NT = 256          # csrc/vmp_carve.h kBigNT
K_MAX_WAVE_V = 16 * 64  # csrc/vmp_layout.h kMaxVPT * kWaveSize


def wave_vpt(V):
    """launch_env (csrc/vmp_capi.cpp): the fewest of 1 / 2 / 4 / 8 / 16 slot rows that hold V."""
    need = (V + 63) // 64
    return 1 if need <= 1 else 2 if need <= 2 else 4 if need <= 4 else 8 if need <= 8 else 16


def big_spt(V):
    """big_spt (csrc/vmp_carve.h): k_env_big's slots per thread."""
    return 4 if V <= 4 * K_BIG_NT else 8 if V <= 8 * K_BIG_NT else 16 if V <= 16 * K_BIG_NT else 40


@dataclass(frozen=True)
class Case:
    name: str
    group: str
    P: int
    V: int
    lam: float
    L: float
    reward: str
    policy: str
    null: bool = True
    source: str = "config"       # "config" | "workload" | "trace"
    wl: tuple = None             # six (lam, L) pairs for "workload" / "trace"
    big: bool = False            # VMP_BIG_KERNEL=1
    ext_hold: bool = False       # external segment: no waiting VM below slot V - 1 is placed
    n_full: int = N_FULL
    n_ext: int = N_EXT
    rolls: tuple = (K_ROLL,)
    n_bare: int = N_BARE
    seeds: tuple = SEEDS
    note: str = ""

    @property
    def A(self):
        return self.P + 2 if self.null else self.P + 1

    @property
    def block(self):
        return self.big or self.V > K_MAX_WAVE_V

    @property
    def steps(self):
        return self.n_full + self.n_ext + sum(self.rolls) + self.n_bare

    def cfg(self):
        return dict(pms=self.P, vms=self.V, arrival_rate=self.lam, service_length=self.L,
                    training_steps=TRAINING_STEPS, eval_steps=100000, seed=0,
                    reward_function=self.reward, sequence="uniform", cap_target_util=True,
                    beta=0.5, allow_null_action=self.null)

    def workload(self):
        """The (lam, L) pair of every env."""
        return self.wl if self.wl is not None else ((self.lam, self.L),) * N_ENV

    def selects(self):
        """The kernel instantiations the plan launches: ("wave", VPT, kind, source) with
        kind ext (k_env_ext*), one (per-step launch, k_steps == 1) or multi (fused rollout
        and act-only, k_steps != 1); ("block", SPT, ONE, source)."""
        kinds = set()
        if self.n_full or self.n_bare or 1 in self.rolls:
            kinds.add("one")
        if self.n_ext:
            kinds.add("ext")
        kinds.add("multi")  # the act-only launch of segment 3
        if self.block:
            return {("block", big_spt(self.V), k != "multi", self.source) for k in kinds}
        return {("wave", wave_vpt(self.V), k, self.source) for k in kinds}


def _pms(V):
    return min(40, max(3, V // 12))


def _lam(V):
    """The table fills within the first segment: slot V - 1 waits when the
    external-action segment begins."""
    return max(0.8, V / 18.0)


def _pairs(V):
    """Six (lam, L) pairs as tests/test_gpu_workload.py's WL mixes them: lam = 0, the
    multiplication sampler (lam < 10) and PTRS (lam >= 10, from 10.0 itself) on the
    arrival stream, and both on the service stream. The rates grow with V so that
    every env with lam > 0 fills its table inside the plan."""
    lo = min(9.5, max(0.6, V / 40.0))
    return ((0.0, 5.0), (lo, 300.0), (max(10.0, V / 18.0), 9.99), (max(12.0, V / 14.0), 25.0),
            (min(9.99, max(0.9, V / 30.0)), 1000.0), (max(25.0, V / 10.0), 2.0))


def _rolls(V, pairs):
    """The fused segment of a per-env / trace case: 23 steps, or as many as the env
    with the lowest rate needs to fill V slots (a rate below 10 cannot fill V > 880
    slots in the 93 steps of the standard plan; the fused rollout is the cheapest
    launch kind to spend the extra steps on, and past 256 steps it is split by the host)."""
    lo = min(l for l, _ in pairs if l > 0)
    need = int(math.ceil(1.25 * V / lo)) + 10 - (N_FULL + N_EXT + N_BARE)
    return (max(K_ROLL, need),)


def _build():
    cases = []
    # a. slot borders x source
    for vi, V in enumerate(WAVE_V + BLOCK_V):
        P = _pms(V)
        for si, source in enumerate(("config", "workload", "trace")):
            reward, policy = COMBOS[(vi + si) % 3]
            kw = {}
            if source != "config":
                kw = dict(wl=_pairs(V), rolls=_rolls(V, _pairs(V)))
                if kw["rolls"] != (K_ROLL,):
                    kw["note"] = ("fused segment of %d steps: the envs with lam < 10 need them "
                                  "to fill %d slots" % (kw["rolls"][0], V))
            cases.append(Case("a-v%d-%s" % (V, source), "a", P, V, _lam(V), 8.0, reward, policy,
                              source=source, **kw))
    # b. forced block kernel at small V (threads without a slot; SPT 4 with its last row
    # full or nearly empty); V 257 also with the other two sources, so that every
    # (SPT 4, ONE, source) instantiation is selected here
    for vi, V in enumerate(FORCED_V):
        reward, policy = COMBOS[vi % 3]
        cases.append(Case("b-v%d-config" % V, "b", _pms(V), V, _lam(V), 8.0, reward, policy,
                          big=True))
    for si, source in enumerate(("workload", "trace")):
        reward, policy = COMBOS[(si + 1) % 3]
        cases.append(Case("b-v257-%s" % source, "b", _pms(257), 257, _lam(257), 8.0, reward, policy,
                          source=source, wl=_pairs(257), big=True))
    # c. more than 64 (128) accepted requests in one step on the wave kernel. At
    # P400 / V1024 / L2 the heuristics keep up with both rates (the oracle never has
    # fewer than 245 NULL slots): every heuristic step accepts its whole draw, ~100 or
    # ~200 requests, so the standard plan keeps the arrival condition. The table fills
    # only where the external segment withholds the placements (ext_hold); the fused
    # rollout that follows then places several hundred waiting VMs in its first step.
    note = "standard plan; ext_hold: the table fills in the external segment only"
    for lam in (100.0, 200.0):
        for si, source in enumerate(("config", "workload")):
            reward, policy = COMBOS[(si + (lam > 100)) % 3]
            cases.append(Case("c-v1024-lam%d-%s" % (lam, source), "c", 400, 1024, lam, 2.0, reward,
                              policy, source=source, wl=((lam, 2.0),) * N_ENV if si else None,
                              ext_hold=True, note=note))
    # V 512: 100 PMs serve ~60 VMs a step, so the table fills by itself within segment 1
    cases.append(Case("c-v512-lam100-config", "c", 100, 512, 100.0, 2.0, "kl", "bestfit"))
    # d. mask borders: W32 = (A + 31) / 32 words per slot, A = P + 2 or P + 1
    # (from 30 PMs on every VM finds room: the table fills only when lam (L + 1) > V; just
    # above V it goes on filling and emptying, so that NULL slots come and go)
    for pi, P in enumerate(MASK_P):
        for null in (True, False):
            reward, policy = COMBOS[(pi + null) % 3]
            lam, L = (4.0, 17.0) if P > 2 else (4.0, 2.0)
            cases.append(Case("d-p%d-%s" % (P, "null" if null else "nonull"), "d", P, 65,
                              lam, L, reward, policy, null=null))
    # e. the host's split of a rollout at kMaxStepsPerLaunch = 256
    for policy in ("firstfit", "bestfit"):
        cases.append(Case("e-v65-%s" % policy, "e", 6, 65, 4.0, 8.0, "ut" if policy == "bestfit" else "wr",
                          policy, rolls=SPLIT_K))
    return tuple(cases)


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def ext_actions(rng, P, A, placement, heur, hold=False):
    """The proposed actions of one external step of one env, from the oracle's
    state alone: the heuristic's action with some running VMs sent to WAIT, some
    slots given any index in [-1, A] (out of range at both ends included), and
    slot V - 1 given a PM whenever it waits. That PM is emptied for it: the VMs
    running on it are suspended (the action phase goes in slot order, so they
    leave first) and no lower slot is placed on it, so the placement is valid
    and slot V - 1 runs. hold: the heuristic's placements are withheld first
    (waiting VMs keep waiting), so that a table the heuristic would keep half
    empty fills up."""
    V = placement.size
    WAIT = P
    a = heur.copy()
    if hold:
        a[placement == WAIT] = WAIT
    a[(placement < P) & (rng.random(V) < 0.15)] = WAIT
    rnd = rng.random(V) < 0.1
    a[rnd] = rng.integers(-1, A + 1, size=int(rnd.sum()))
    last = V - 1
    if placement[last] == WAIT:
        q = int(rng.integers(0, P))
        head, pl = a[:last], placement[:last]
        head[(head == q) & (pl != q)] = pl[(head == q) & (pl != q)]
        head[pl == q] = WAIT
        a[last] = q
    return a


@dataclass
class Ref:
    """What the oracle did over a case's plan. Step-indexed arrays cover every
    step; act / obs / valid only the steps of segments 1, 2 and 5 (None inside a
    fused rollout, where the device returns rewards only)."""
    rew: np.ndarray            # [T, N]
    done: np.ndarray           # [T, N]
    ctr: np.ndarray            # [T, N, 6] counters after the step
    last_pl: np.ndarray        # [T, N] placement of slot V - 1 after the step
    n_null: np.ndarray         # [T, N] NULL slots after the step
    n_run: np.ndarray          # [T, N] running VMs after the step
    act: list = field(default_factory=list)
    obs: list = field(default_factory=list)
    valid: list = field(default_factory=list)
    ext_pre_pl: list = field(default_factory=list)   # per external step: placement before it [N, V]
    ext_mask: list = field(default_factory=list)     # per external step: mask() after it [N, V, A]
    mid: dict = None           # segment 3: mask, obs, act of the policy
    state: list = None         # per env: state() at the end
    traces: list = None        # per env (offs, cpu, mem, runtime), trace cases only

    def accepted(self):
        """[T, N] requests accepted per step: d total_requests - d dropped."""
        c = np.concatenate([np.zeros((1,) + self.ctr.shape[1:], np.int64), self.ctr])
        d = np.diff(c, axis=0)
        return d[:, :, 0] - d[:, :, 4]

    def dropped(self):
        c = np.concatenate([np.zeros((1,) + self.ctr.shape[1:], np.int64), self.ctr])
        return np.diff(c, axis=0)[:, :, 4]


def oracle_envs(case):
    out = []
    for (lam, sl), s in zip(case.workload(), case.seeds):
        e = O.OracleEnv(dict(case.cfg(), arrival_rate=lam, service_length=sl, seed=int(s)))
        e.reset(int(s))
        out.append(e)
    return out


def run_oracle(case, case_index=None):
    """-> Ref. The generator of the external actions is seeded by the case's
    position in CASES."""
    if case_index is None:
        case_index = CASES.index(case)
    rng = np.random.default_rng([2024, case_index])
    oes = oracle_envs(case)
    T, N, V, P = case.steps, N_ENV, case.V, case.P
    r = Ref(rew=np.zeros((T, N)), done=np.zeros((T, N), bool), ctr=np.zeros((T, N, 6), np.int64),
            last_pl=np.zeros((T, N), np.int64), n_null=np.zeros((T, N), np.int64),
            n_run=np.zeros((T, N), np.int64))
    want_trace = case.source == "trace"
    pre_pl = [np.full(V, P + 1, np.int64) for _ in range(N)]
    req0 = [0] * N
    parts = [([0], [], [], []) for _ in range(N)]
    heur = (lambda e: e.firstfit()) if case.policy == "firstfit" else (lambda e: e.bestfit())

    def step(t, kind):
        keep = kind != "roll"
        acts, obss, valids = [], [], []
        if kind == "ext":
            r.ext_pre_pl.append(np.stack(pre_pl))
        for i, e in enumerate(oes):
            a = heur(e)
            if kind == "ext":
                a = ext_actions(rng, P, case.A, pre_pl[i], a, case.ext_hold)
            o, rew, done, valid = e.step(a)
            st = e.state()
            ctr = e.counters()[0]
            r.rew[t, i], r.done[t, i], r.ctr[t, i] = rew, done, ctr
            r.last_pl[t, i] = st[0][V - 1]
            r.n_null[t, i] = np.count_nonzero(st[0] == P + 1)
            r.n_run[t, i] = np.count_nonzero(st[0] < P)
            if want_trace:
                offs, cpu, mem, rt = TL.derive_trace(P, (pre_pl[i],), [a], [valid], [st],
                                                     [[int(ctr[0]) - req0[i]]])
                parts[i][0].append(parts[i][0][-1] + int(offs[1]))
                for dst, src in zip(parts[i][1:], (cpu, mem, rt)):
                    dst.append(src)
                req0[i] = int(ctr[0])
            pre_pl[i] = st[0]
            if keep:
                acts.append(a)
                obss.append(o)
                valids.append(valid)
        r.act.append(np.stack(acts) if keep else None)
        r.obs.append(np.stack(obss) if keep else None)
        r.valid.append(np.stack(valids) if keep else None)
        if kind == "ext":
            r.ext_mask.append(np.stack([e.mask() for e in oes]))

    t = 0
    for _ in range(case.n_full):
        step(t, "full")
        t += 1
    for _ in range(case.n_ext):
        step(t, "ext")
        t += 1
    r.mid = dict(mask=np.stack([e.mask() for e in oes]), obs=np.stack([e.obs() for e in oes]),
                 act=np.stack([heur(e) for e in oes]))
    for _ in range(sum(case.rolls)):
        step(t, "roll")
        t += 1
    for _ in range(case.n_bare):
        step(t, "bare")
        t += 1
    assert t == T
    r.state = [e.state() for e in oes]
    if want_trace:
        r.traces = [(np.asarray(p[0], np.int64),
                     np.concatenate(p[1]) if p[1] else np.zeros(0, np.uint8),
                     np.concatenate(p[2]) if p[2] else np.zeros(0, np.uint8),
                     np.concatenate(p[3]) if p[3] else np.zeros(0, np.uint32)) for p in parts]
    return r
