"""Call sequences against a model of the batched handle.

TEST INFRASTRUCTURE ONLY: numpy, the C oracle and the literals of tests/; it
imports without a GPU. tests/test_seq_cases_cpu.py shows on the model alone
that the sequences go where the device can go wrong, tests/test_gpu_sequences.py
walks the device handles and the model through the same op list and compares
every value the device returns.

  ModelHandle   one env model per env (the C oracle, or tests/trace_literal's
                TraceEnv for a traced handle, behind one adapter interface) plus
                the handle's own state: eval flag, start state, series, request
                log. Every op of BatchedVmEnv that changes or reads env state,
                with the semantics its docstrings state.
  gen_ops       the seeded op list of one (case, seed), built by walking the
                model only: no device value ever enters a sequence.
  run_model     the model's outputs of an op list, op by op.

Replay aid:  python -m tests.seq_cases --case A --seed 2 [--upto K]
prints the op list with every argument; a failing GPU assertion names the case,
the seed and the op index.
"""
import argparse
import copy
import sys
from dataclasses import dataclass

import numpy as np

from oracle import oracle as O
from tests import env_cases as EC
from tests import reqlog_literal as RL
from tests import series_literal as SR
from tests import state_literal as SL
from tests import trace_literal as TL
from tests.act_literal import literal_act

N_MAIN, N_SECOND = 6, 5          # 6: not a multiple of a block's 4 waves
SEEDS_MAIN = EC.SEEDS            # one seed above 2^32
SEEDS_SECOND = (21, (1 << 33) + 9, 333, 8, 77)
TRAINING_STEPS = 50              # episodes end inside a sequence
SEQ_SEEDS = (0, 1, 2)
STATE_KEYS = TL.STATE_KEYS
VM_KEYS = ("vm_placement", "vm_cpu", "vm_memory", "vm_remaining_runtime")
TRACE_STEPS = 600
TRACE_MAP = ((0, 1, 2, 3, 4, 6), (6, 6, 5, 0, 1))  # one trace per env plus a shared one (6)

LAUNCHES = ("step_ext", "hstep_full", "hstep_bare", "rollout")
READERS = ("mask", "mask_bits", "obs", "heuristic_act", "getters")
MUTATORS = ("reset_seeds", "reset_none", "eval", "snapshot", "restore", "branch_self",
            "branch_from_second", "branch_into_second", "set_state_identity", "set_state_random",
            "set_state_invalid", "set_start_state", "set_workload")
OBSERVERS = ("series_on", "series_off", "series_read", "reqlog_on", "reqlog_off", "reqlog_read",
             "record_on", "record_off")
OTHERS = ("h2_step", "set_start_none")  # the second handle's own steps; start state off again
ROLLOUT_K = (1, 2, 7, 23)
PER_STEP = ("step_ext", "hstep_full", "hstep_bare", "h2_step")


@dataclass(frozen=True)
class SeqCase:
    name: str
    cid: int
    P: int
    V: int
    lam: float
    L: float
    reward: str
    policy: str
    source: str = "config"   # "config" | "workload" | "trace"
    wl: tuple = None         # the six (lam, L) pairs of a "workload" case

    @property
    def A(self):
        return self.P + 2

    def cfg(self):
        return dict(pms=self.P, vms=self.V, arrival_rate=self.lam, service_length=self.L,
                    training_steps=TRAINING_STEPS, eval_steps=100000, seed=0,
                    reward_function=self.reward, sequence="uniform", cap_target_util=True,
                    beta=0.5, allow_null_action=True)

    def mutators(self):
        return tuple(m for m in MUTATORS if m != "set_workload" or self.source == "workload")

    def kinds(self):
        return LAUNCHES + READERS + self.mutators() + OBSERVERS + OTHERS

    def workload(self, which):
        """The (lam, L) pair of every env of handle `which` at creation."""
        n = (N_MAIN, N_SECOND)[which]
        if self.wl is None:
            return ((self.lam, self.L),) * n
        return tuple(self.wl[(i + which) % len(self.wl)] for i in range(n))

    def traces(self):
        """Seven Poisson traces as (offs, cpu, mem, runtime): rate lam, runtimes 1 .. 2 L - 1."""
        out = []
        for k in range(7):
            g = np.random.default_rng([self.cid, 55, k])
            arrivals = g.poisson(self.lam, TRACE_STEPS)
            tot = int(arrivals.sum())
            out.append((np.r_[0, np.cumsum(arrivals)].astype(np.int64), g.integers(1, 101, tot),
                        g.integers(1, 101, tot), g.integers(1, int(2 * self.L), tot)))
        return out


CASES = (
    # tests/test_gpu_idle_step.py row p4v65: VPT 2 with 63 padded lanes; idle path, bits 60 / 62
    # and skip_time all fire
    SeqCase("A", 1, 4, 65, 1.0, 40.0, "wr", "firstfit"),
    # VPT 1; lam = 0, the multiplication and the PTRS sampler; set_workload mid-run; BestFit ties
    SeqCase("B", 2, 10, 30, 0.182, 100.0, "kl", "bestfit", source="workload", wl=EC._pairs(30)),
    # k_env_big at the smallest V over the wave limit; a pitch that is no power of two; the
    # last slot row holds one slot
    SeqCase("C", 3, 7, 1025, EC._lam(1025), 8.0, "ut", "bestfit"),
    # the trace kernels: nothing is drawn, the step follows the copied / imported timestep into
    # the target's own trace; idle path eligible
    SeqCase("D", 4, 4, 64, 1.0, 40.0, "wr", "firstfit", source="trace"),
)
BY_NAME = {c.name: c for c in CASES}


# ----------------------------------------------------------------- env models
class OracleModel:
    """One env on the C oracle."""

    def __init__(self, cfg, seed):
        self.e = O.OracleEnv(dict(cfg, seed=int(seed)))
        self.P, self.V = self.e.P, self.e.V

    def eval(self, mode):
        self.e.eval(mode)

    def reset(self, seed):
        self.e.reset(seed)

    def step(self, action):
        return self.e.step(action)

    def obs(self):
        return self.e.obs()

    def mask(self):
        return self.e.mask()

    def act(self, policy):
        return self.e.firstfit() if policy == "firstfit" else self.e.bestfit()

    def rank(self):
        return int(self.e.rank())

    def state(self):
        return dict(zip(STATE_KEYS, self.e.state()))

    def counters(self):
        return self.e.counters()

    def clone(self):
        c = OracleModel(self.e.cfg, 0)
        c.e.assign(self.e)
        return c

    def assign(self, other):
        self.e.assign(other.e)

    def reseed(self, seed):
        self.e.reseed(seed)

    def set_state(self, st):
        self.e.set_state(st["vm_placement"], st["vm_cpu"], st["vm_memory"],
                         st["vm_remaining_runtime"], st.get("cpu"), st.get("memory"),
                         st.get("counters"), st.get("totals"))

    def set_workload(self, lam, L):
        self.e.set_workload(lam, L)

    def workload(self):
        return (self.e.cfg["arrival_rate"], self.e.cfg["service_length"])


class TraceModel:
    """One traced env on tests/trace_literal.TraceEnv: copy.deepcopy stands for
    assign (the trace stays the target's own), state_literal.into_trace_env for
    set_state, act_literal.literal_act on the literal's own obs for the
    heuristic. Seeds change nothing a traced env shows."""

    def __init__(self, cfg, trace):
        self.t = TL.TraceEnv(cfg, *trace)
        self.P, self.V = self.t.P, self.t.V

    def eval(self, mode):
        self.t.eval_mode = bool(mode)

    def reset(self, seed):
        self.t.reset()

    def step(self, action):
        obs, r, done, valid = self.t.step(action)
        return obs, float(r), done, valid

    def obs(self):
        return self.t.obs()

    def mask(self):
        t = self.t
        return np.array([[not t._valid(v, t.vm_placement[v], a) for a in range(self.P + 2)]
                         for v in range(self.V)], bool)

    def act(self, policy):
        return literal_act(self.t.obs(), self.P, self.V, policy)

    def rank(self):
        pl = self.t.vm_placement
        return int(np.unique(pl[pl < self.P]).size)

    def state(self):
        return dict(zip(STATE_KEYS, self.t.state()))

    def counters(self):
        st = self.t.stats().astype(np.float64)
        st[1:3] = SR.target_means(self.state(), self.P, self.t.cfg.get("cap_target_util", True))
        return self.t.counters(), st

    def clone(self):
        c = copy.copy(self)
        c.t = copy.deepcopy(self.t)
        return c

    def assign(self, other):
        mine = self.t
        self.t = copy.deepcopy(other.t)
        for k in ("cfg", "offs", "rq_cpu", "rq_mem", "rq_rt", "eval_mode"):
            setattr(self.t, k, getattr(mine, k))

    def reseed(self, seed):
        pass

    def set_state(self, st):
        SL.into_trace_env(self.t, st)

    def workload(self):
        return None


def _state_idle(st, P):
    """The state part of the idle predicate (tools/idle_step_stats.py) and of the
    hand-overs: no slot is NULL, no running VM finishes next step and no
    waiting VM fits a PM."""
    pl, rem = st["vm_placement"], st["vm_remaining_runtime"]
    if (pl == P + 1).any():
        return False
    run = pl < P
    if run.any() and int(rem[run].min()) <= 1:
        return False
    w = pl == P
    fits = ((st["cpu"][None, :] + st["vm_cpu"][w, None] <= 1)
            & (st["memory"][None, :] + st["vm_memory"][w, None] <= 1))
    return not fits.any()


# --------------------------------------------------------------- the handle
class ModelHandle:
    def __init__(self, case, which):
        self.case, self.which = case, which
        self.n = (N_MAIN, N_SECOND)[which]
        self.P, self.V, self.A = case.P, case.V, case.A
        seeds = (SEEDS_MAIN, SEEDS_SECOND)[which]
        if case.source == "trace":
            tr = case.traces()
            self.envs = [TraceModel(case.cfg(), tr[k]) for k in TRACE_MAP[which]]
        else:
            self.envs = [OracleModel(dict(case.cfg(), arrival_rate=lam, service_length=L), s)
                         for (lam, L), s in zip(case.workload(which), seeds)]
        self.eval_mode = False
        self.start = None      # per-env state dicts: what reset() leaves
        self.series = None     # dict(capacity, stride, lits)
        self.reqlog = None     # dict(capacity, logs)
        self.record = False
        self.snap = None       # (env clones, workload) of the latest snapshot
        # what the CPU half counts (never compared with the device)
        self.quiet = [False] * self.n        # the env's last launch was a per-step launch that
        #                                      placed, finished and accepted nothing, and
        #                                      nothing has written the env since
        self.last_pred = [False] * self.n    # idle predicate at the env's last per-step launch
        self.post_idle = [False] * self.n    # _state_idle after the env's last launch
        self.written = [False] * self.n      # a mutator wrote the env since its last launch
        self.track_idle = case.name in ("A", "D")
        self.moved = np.zeros((self.n, 6), np.int64)  # what the steps added to the counters
        self.stats = dict(bare_steps=0, bare_idle=0, dangerous=0, opposite=0, done_training=0,
                          last_row_accept=0, bestfit_tie=0, refused=0, imported=0, env_steps=0)

    # -- observers
    def _restart(self, envs):
        for i in envs:
            ctr = self.envs[i].counters()[0]
            if self.series:
                self.series["lits"][i].restart(int(ctr[5]))
            if self.reqlog:
                self.reqlog["logs"][i] = RL.RuleLog(self.P, self.V, self.reqlog["capacity"],
                                                    self.envs[i].state()["vm_placement"], int(ctr[0]))
            self.written[i] = True
            self.quiet[i] = False

    def series_on(self, capacity, stride):
        self.series = dict(capacity=capacity, stride=stride,
                           lits=[SR.LiteralSeries(capacity, stride, int(e.counters()[0][5]))
                                 for e in self.envs])

    def reqlog_on(self, capacity):
        self.reqlog = dict(capacity=capacity, logs=[None] * self.n)
        for i, e in enumerate(self.envs):
            self.reqlog["logs"][i] = RL.RuleLog(self.P, self.V, capacity, e.state()["vm_placement"],
                                                int(e.counters()[0][0]))

    def series_read(self):
        s = self.series
        return dict(series_rows=np.stack([x.rows for x in s["lits"]]),
                    series_meta=np.stack([x.meta for x in s["lits"]]))

    def reqlog_read(self):
        q = self.reqlog
        return dict(reqlog_rows=np.stack([x.read(0) for x in q["logs"]]),
                    reqlog_meta=np.stack([x.meta for x in q["logs"]]))

    # -- launches
    def _pred(self, i, st):
        pl, rem = st["vm_placement"], st["vm_remaining_runtime"]
        run = pl < self.P
        soon = int(rem[run].min()) if run.any() else 0
        return (self.quiet[i] and not (pl == self.P + 1).any() and soon > 1
                and self.reqlog is None and not self.record)

    def _launch(self, kind, actions=None, policy=None, rew=None):
        """One step of every env. actions [n, V] or None (the heuristic's). rew
        [n]: the rewards the series rows take (the device's own under kl).
        -> obs, reward, done, valid, actions."""
        out = [[], [], [], [], []]
        for i, e in enumerate(self.envs):
            st0 = e.state()
            c0 = e.counters()[0]
            if kind in PER_STEP or kind == "rollout":
                pred = self._pred(i, st0)
                if kind == "hstep_bare":
                    s = self.stats
                    s["bare_steps"] += 1
                    s["bare_idle"] += pred
                    if self.written[i] and self.track_idle:
                        now = _state_idle(st0, self.P)
                        s["dangerous"] += self.last_pred[i] and not now
                        s["opposite"] += (not self.post_idle[i]) and now
            if actions is None:
                a = e.act(policy)
                if policy == "bestfit" and (st0["vm_placement"] == self.P).any():
                    key = st0["cpu"].astype(np.float32) + st0["memory"].astype(np.float32)
                    self.stats["bestfit_tie"] += np.unique(key).size < key.size
            else:
                a = np.asarray(actions[i], np.int64)
            obs, r, done, valid = e.step(a)
            st1 = e.state()
            c1, sts = e.counters()
            if self.series:
                used = r if rew is None else float(rew[i])
                self.series["lits"][i].add(SR.row_of(st1, c1, sts, e.rank(), used, self.P))
            if self.reqlog:
                self.reqlog["logs"][i].update(int(c0[5]), a, valid, st1["vm_placement"], int(c1[0]))
            d = c1 - c0
            per_step = kind in PER_STEP
            self.quiet[i] = bool(per_step and d[3] == 0 and d[1] == 0 and d[0] - d[4] == 0)
            if per_step:
                self.last_pred[i] = pred
            self.post_idle[i] = self.track_idle and _state_idle(st1, self.P)
            self.moved[i] += d
            self.written[i] = False
            s = self.stats
            s["env_steps"] += 1
            s["done_training"] += bool(done) and not self.eval_mode
            s["last_row_accept"] += bool(st0["vm_placement"][-1] == self.P + 1
                                         and st1["vm_placement"][-1] == self.P)
            for k, x in zip(range(5), (obs, r, done, valid, a)):
                out[k].append(x)
        return (np.stack(out[0]), np.array(out[1], np.float64), np.array(out[2], bool),
                np.stack(out[3]).astype(np.uint8), np.stack(out[4]).astype(np.int64))

    # -- readers
    def observe(self):
        """What is compared after every op: counters, stats, the six state arrays, rank."""
        ctr = [e.counters() for e in self.envs]
        sts = [e.state() for e in self.envs]
        out = dict(counters=np.stack([c[0] for c in ctr]),
                   stats=np.stack([np.asarray(c[1], np.float64) for c in ctr]),
                   rank=np.array([e.rank() for e in self.envs], np.int64))
        for k in STATE_KEYS:
            out[k] = np.stack([s[k] for s in sts])
        return out

    def mask(self):
        return np.stack([e.mask() for e in self.envs])

    # -- mutators
    def set_eval(self, mode):
        self.eval_mode = bool(mode)
        for e in self.envs:
            e.eval(mode)

    def reset(self, seeds, mask):
        sel = [i for i in range(self.n) if mask is None or mask[i]]
        for i in sel:
            self.envs[i].reset(None if seeds is None else int(seeds[i]))
            if self.start is not None:
                self.envs[i].set_state(self.start[i])
        self._restart(sel)

    def snapshot(self):
        self.snap = ([e.clone() for e in self.envs], [e.workload() for e in self.envs])

    def snapshot_fits(self):
        return self.snap is not None and self.snap[1] == [e.workload() for e in self.envs]

    def restore(self):
        assert self.snapshot_fits()
        for e, s in zip(self.envs, self.snap[0]):
            e.assign(s)
        self._restart(range(self.n))

    def branch(self, src, index, seeds):
        sources = [e.clone() for e in src.envs]  # a staging copy: any map is correct in place
        sel = []
        for i, k in enumerate(index):
            if k < 0:
                continue
            self.envs[i].assign(sources[int(k)])
            if seeds is not None and seeds[i] >= 0:
                self.envs[i].reseed(int(seeds[i]))
            sel.append(i)
        self._restart(sel)

    def set_state(self, states, mask, seeds):
        """states: per-env dicts (counters / totals inside). -> status u8 [n]."""
        status = np.zeros(self.n, np.uint8)
        sel = []
        for i, st in enumerate(states):
            if mask is not None and not mask[i]:
                continue
            status[i] = SL.validate(st, self.P, int(self.envs[i].counters()[0][5]))
            if status[i] != SL.IMPORTED:
                self.stats["refused"] += 1
                continue
            self.stats["imported"] += 1
            self.envs[i].set_state(st)
            if seeds is not None and seeds[i] >= 0:
                self.envs[i].reseed(int(seeds[i]))
            sel.append(i)
        self._restart(sel)
        return status

    def set_workload(self, lam, L):
        for e, a, s in zip(self.envs, lam, L):
            e.set_workload(float(a), float(s))


def unstack(d, n):
    """The op's stacked arrays -> per-env state dicts."""
    return [{k: (None if v is None else v[i]) for k, v in d.items()} for i in range(n)]


class Model:
    """The two handles of a case and the dispatch of an op to them."""

    def __init__(self, case):
        self.case = case
        self.h = [ModelHandle(case, 0), ModelHandle(case, 1)]

    def apply(self, op, rew=None):
        """-> dict of the values the op returns (empty for most mutators). rew
        [K, n]: the device's rewards of a launch, for the series rows under kl."""
        k = op["op"]
        main, second = self.h
        c = self.case
        if k == "step_ext":
            obs, r, done, valid, _ = main._launch(k, actions=op["actions"],
                                                  rew=None if rew is None else rew[0])
            out = dict(obs=obs, reward=r, done=done, valid=valid)
            if op["mask_out"]:
                out["mask_out"] = main.mask()
            return out
        if k in ("hstep_full", "h2_step", "hstep_bare"):
            h = second if k == "h2_step" else main
            obs, r, done, valid, act = h._launch(k, policy=c.policy, rew=None if rew is None else rew[0])
            out = dict(obs=obs, reward=r, done=done)
            if k != "hstep_bare":
                out.update(valid=valid, actions=act)
            return out
        if k == "rollout":
            K = op["K"]
            rs, dc = np.zeros((K, main.n)), np.zeros(main.n, np.int64)
            for j in range(K):
                # observed, the device makes K per-step launches (vmp_rollout_heuristic)
                kind = "hstep_full" if main.series or main.reqlog or main.record else "rollout"
                _, rs[j], done, _, _ = main._launch(kind, policy=c.policy,
                                                    rew=None if rew is None else rew[j])
                dc += done
            return dict(rewards=rs, done_count=dc)
        if k in ("mask", "mask_bits"):
            return {k: main.mask()}
        if k == "obs":
            return dict(obs=np.stack([e.obs() for e in main.envs]))
        if k == "heuristic_act":
            return dict(actions=np.stack([e.act(c.policy) for e in main.envs]).astype(np.int64))
        if k == "getters":
            return {}
        if k in ("reset_seeds", "reset_none"):
            main.reset(op.get("seeds"), op["mask"])
            return dict(obs=np.stack([e.obs() for e in main.envs]))
        if k == "eval":
            main.set_eval(op["mode"])
        elif k == "snapshot":
            main.snapshot()
        elif k == "restore":
            main.restore()
        elif k == "branch_self":
            main.branch(main, op["index"], op["seeds"])
        elif k == "branch_from_second":
            main.branch(second, op["index"], op["seeds"])
        elif k == "branch_into_second":
            second.branch(main, op["index"], op["seeds"])
        elif k in ("set_state_identity", "set_state_random", "set_state_invalid"):
            d = dict(op["state"], counters=op["counters"], totals=op["totals"])
            return dict(status=main.set_state(unstack(d, main.n), op["mask"], op["seeds"]))
        elif k == "set_start_state":
            d = dict(op["state"], counters=op["counters"], totals=op["totals"])
            main.start = unstack(d, main.n)
        elif k == "set_start_none":
            main.start = None
        elif k == "set_workload":
            main.set_workload(op["arrival_rate"], op["service_length"])
        elif k == "series_on":
            main.series_on(op["capacity"], op["stride"])
        elif k == "series_off":
            main.series = None
        elif k == "series_read":
            return main.series_read()
        elif k == "reqlog_on":
            main.reqlog_on(op["capacity"])
        elif k == "reqlog_off":
            main.reqlog = None
        elif k == "reqlog_read":
            return main.reqlog_read()
        elif k == "record_on":
            main.record = True
        elif k == "record_off":
            main.record = False
        else:
            raise ValueError(k)
        return {}

    def final(self):
        """The observers' readings at the end of a sequence."""
        out = {}
        if self.h[0].series:
            out.update(self.h[0].series_read())
        if self.h[0].reqlog:
            out.update(self.h[0].reqlog_read())
        return out


# ------------------------------------------------------------ the generator
def _export(h):
    """state(), counters and totals of every env of a model handle, stacked."""
    o = h.observe()
    st = {k: o[k].copy() for k in STATE_KEYS}
    return st, o["counters"].copy(), o["stats"][:, 3:5].copy()


def _mask(g, n, p):
    m = (g.random(n) < p).astype(np.uint8)
    m[int(g.integers(0, n))] = 1
    return m


def _seeds_or_keep(g, n):
    """Entries >= 0 reseed, negative ones keep the streams; None sometimes."""
    if g.random() < 0.5:
        return None
    s = g.integers(0, 1 << 41, n).astype(np.int64)
    s[g.random(n) < 0.4] = -1
    return s


def _ext_actions(g, h):
    """reqlog_literal.random_actions on the model's placements: half keep, half any
    action in 0..P+1; now and then entries out of range at the top end."""
    acts = []
    for e in h.envs:
        pl = e.state()["vm_placement"]
        a = pl.copy()
        draw = g.random(h.V) < 0.5
        a[draw] = g.integers(0, h.P + 2, int(draw.sum()))
        if g.random() < 0.15:
            a[g.random(h.V) < 0.05] = h.P + 2 + int(g.integers(0, 3))
        acts.append(a.astype(np.int64))
    return np.stack(acts)


def _no_room(st, P):
    """Edit a state without loads so that nothing can happen in it but arrivals
    being dropped (the state part of the idle predicate): a waiting VM that
    fits a PM is given a cpu size of 1.0 where no PM is empty, a running VM
    about to finish one more step."""
    pl = st["vm_placement"]
    s = SL._sums(st, P)
    if min(s[:P]) == 0:
        return
    for v in np.flatnonzero(pl == P):
        kc, km = SL._k(st["vm_cpu"][v]), SL._k(st["vm_memory"][v])
        if any(s[q] + kc <= 100 and s[P + q] + km <= 100 for q in range(P)):
            st["vm_cpu"][v] = 1.0
    rem = st["vm_remaining_runtime"]
    rem[(pl < P) & (rem == 1)] = 2


def _random_states(g, h, loads, counters, fills=(0.5, 0.95, 1.0)):
    sts = []
    for _ in range(h.n):
        full = h.track_idle and g.random() < 0.5
        st = SL.random_state(g, h.P, h.V, fill=1.0 if full else float(g.choice(fills)),
                             loads=loads and not full, counters=counters, max_rt=60)
        if full:
            _no_room(st, h.P)
            if loads:  # the exact sums: valid loads of the edited state
                x = np.array(SL._sums(st, h.P), np.float64) / 100.0
                st["cpu"], st["memory"] = x[:h.P].copy(), x[h.P:].copy()
        if counters:  # ages inside and around an episode of 50 steps
            st["counters"][5] = int(g.integers(1, 60))
        sts.append(st)
    d = SL.stack(sts)
    return ({k: d[k] for k in d if k not in ("counters", "totals")}, d.get("counters"),
            d.get("totals"))


_RULES = (SL.PLACEMENT, SL.NULL_SLOT, SL.VM_SIZE, SL.RUNTIME, SL.TIMESTEP, SL.COUNTER,
          SL.CAPACITY, SL.LOAD_MAX)


def _break(g, st, ctr, i, P):
    """Make env i of the stacked arrays break one rule (tests/test_gpu_state.py's breakages)."""
    pl = st["vm_placement"][i]
    null, ex = np.flatnonzero(pl == P + 1), np.flatnonzero(pl <= P)
    rule = int(g.choice(_RULES))
    if rule == SL.NULL_SLOT and null.size:
        st["vm_cpu"][i, null[0]] = 0.5
    elif rule == SL.VM_SIZE and ex.size:
        st["vm_memory"][i, ex[-1]] = 0.1 + 0.2
    elif rule == SL.RUNTIME and ex.size:
        st["vm_remaining_runtime"][i, ex[0]] = (1 << 30) + 1
    elif rule == SL.TIMESTEP:
        ctr[i, 5] = 0
    elif rule == SL.COUNTER:
        ctr[i, 2] = -1
    elif rule == SL.CAPACITY and ex.size >= 2:
        for v in ex[:2]:
            pl[v], st["vm_cpu"][i, v] = 0, 0.51
    elif rule == SL.LOAD_MAX:
        st["memory"][i, 0] = np.nextafter(1.0, 2.0)
    else:
        pl[int(g.integers(0, pl.size))] = P + 2


def _make(kind, m, g):
    """The op of `kind` with its arguments, from the model's present state."""
    c, main, second = m.case, m.h[0], m.h[1]
    op = dict(op=kind)
    if kind == "step_ext":
        op.update(actions=_ext_actions(g, main), mask_out=bool(g.random() < 0.4))
    elif kind == "rollout":
        op.update(K=int(g.choice(ROLLOUT_K)))
    elif kind in ("reset_seeds", "reset_none"):
        if kind == "reset_seeds":
            op.update(seeds=g.integers(0, 1 << 41, main.n).astype(np.int64))
        # an emptied table takes V / lam steps to fill again: where the idle path is the
        # subject, most resets take one or two envs
        p_all, p_env = (0.1, 0.1) if main.track_idle else (0.2, 0.3)
        op.update(mask=None if g.random() < p_all else _mask(g, main.n, p_env))
    elif kind == "eval":
        op.update(mode=not main.eval_mode)
    elif kind in ("branch_self", "branch_from_second", "branch_into_second"):
        dst, src = (second, main) if kind == "branch_into_second" else \
            (main, second if kind == "branch_from_second" else main)
        idx = g.integers(-1, src.n, dst.n).astype(np.int64)
        a, b, k = (int(x) for x in g.permutation(dst.n)[:3])
        idx[a] = -1
        idx[b] = idx[k] = int(g.integers(0, src.n))  # a repeated source
        op.update(index=idx, seeds=_seeds_or_keep(g, dst.n))
    elif kind == "set_state_identity":
        st, ctr, tot = _export(main)
        op.update(state=st, counters=ctr, totals=tot, mask=_mask(g, main.n, 0.5),
                  seeds=_seeds_or_keep(g, main.n))
    elif kind == "set_state_random":
        st, ctr, tot = _random_states(g, main, bool(g.random() < 0.5), bool(g.random() < 0.6))
        op.update(state=st, counters=ctr, totals=tot,
                  mask=None if g.random() < 0.2 else _mask(g, main.n, 0.6),
                  seeds=_seeds_or_keep(g, main.n))
    elif kind == "set_state_invalid":
        st, ctr, tot = _export(main)
        if g.random() < 0.5:  # random valid states around the broken ones
            st, ctr, tot = _random_states(g, main, True, True)
        mask = _mask(g, main.n, 0.8)
        bad = g.permutation(main.n)[:int(g.integers(2, 4))]
        for i in bad:
            mask[i] = 1
            _break(g, st, ctr, int(i), main.P)
        op.update(state=st, counters=ctr, totals=tot, mask=mask, seeds=_seeds_or_keep(g, main.n))
    elif kind == "set_start_state":
        st, ctr, tot = _random_states(g, main, bool(g.random() < 0.5), bool(g.random() < 0.5),
                                      fills=(0.9, 1.0))
        if ctr is not None:
            ctr[:, 5] = g.integers(1, 30, main.n)
        op.update(state=st, counters=ctr, totals=tot)
    elif kind == "set_workload":
        perm = g.permutation(len(c.wl))
        op.update(arrival_rate=np.array([c.wl[k][0] for k in perm], np.float64),
                  service_length=np.array([c.wl[k][1] for k in perm], np.float64))
    elif kind == "series_on":
        op.update(capacity=int(g.choice((2, 6, 40, 2000))), stride=int(g.integers(1, 6)))
    elif kind == "reqlog_on":
        op.update(capacity=int(g.choice((3, 50, max(5000, int(c.lam * 400))))))
    return op


def _plan(case, seed, g):
    """The op kinds of one sequence, in order. Units are kept whole: a mutator
    and the launch that follows it; observer windows. Every (mutator, launch)
    pair is dealt to one of the three seeds, and so is every mutator's unit that
    runs while the series and the request log are on."""
    muts = case.mutators()
    pairs = [(mu, la) for mu in muts for la in LAUNCHES]
    deal = np.random.default_rng([case.cid, 999]).permutation(len(pairs))
    mine = [pairs[k] for j, k in enumerate(deal) if j % len(SEQ_SEEDS) == SEQ_SEEDS.index(seed)]
    idle_case = case.name in ("A", "D")

    def unit(mu, la):
        u = []
        if idle_case and g.random() < 0.7:  # per-step launches first: the env may go idle
            u += ["hstep_bare"] * int(g.integers(2, 5))
        if mu == "restore":
            u += ["snapshot?"]  # only if the handle has no snapshot that fits
        u += [mu, la]
        if mu == "set_start_state":
            u += [str(g.choice(("reset_seeds", "reset_none"))), str(g.choice(LAUNCHES)),
                  "set_start_none"]
        return u

    units = {mu: [] for mu in muts}
    for mu, la in mine:
        units[mu].append(unit(mu, la))
    for mu in muts:
        while len(units[mu]) < (4 if mu == "eval" else 3):
            la = "hstep_bare" if idle_case and g.random() < 0.6 else str(g.choice(LAUNCHES))
            units[mu].append(unit(mu, la))
    observed, free = [], []
    for j, mu in enumerate(muts):  # a third of the mutators per seed: the observed window is
        if j % len(SEQ_SEEDS) == SEQ_SEEDS.index(seed):  # short, valid is requested throughout it
            observed.append(units[mu].pop(int(g.integers(0, len(units[mu])))))
        free += units[mu]
    extra = [[k] for k in READERS for _ in range(3)] + [["h2_step"]] * 4
    extra += [[k] for k in LAUNCHES for _ in range(2)]
    extra += [["hstep_bare"] * 3 for _ in range(2 if idle_case else 1)]
    if idle_case:  # idle envs and busy ones change places, a bare launch on either side
        extra += [["hstep_bare"] * 3 + ["branch_self", "hstep_bare", "hstep_bare"] for _ in range(3)]
    observed += [extra.pop(int(g.integers(0, len(extra)))) for _ in range(4)]
    observed += [["series_read"], ["reqlog_read"]]
    free += extra
    for _ in range(2):  # the observers' second and third windows, short ones
        free.append(["series_on", str(g.choice(LAUNCHES)), "rollout", "series_read", "series_off"])
        free.append(["reqlog_on", str(g.choice(LAUNCHES)), "step_ext", "reqlog_read", "reqlog_off"])
        free.append(["record_on", str(g.choice(LAUNCHES)), "record_off"])
    observed = [observed[k] for k in g.permutation(len(observed))]
    free = [free[k] for k in g.permutation(len(free))]
    cut = int(g.integers(2, 6))
    seq = free[:cut] + [["series_on", "reqlog_on", "record_on"]] + observed \
        + [["reqlog_off", "record_off", "series_read", "series_off"]] + free[cut:]
    return [k for u in seq for k in u]


def gen_ops(case, seed):
    """The op list of (case, seed): deterministic, from the model alone."""
    g = np.random.default_rng([case.cid, seed])
    m = Model(case)
    ops = []
    for kind in _plan(case, seed, g):
        if kind == "snapshot?":
            if m.h[0].snapshot_fits():
                continue
            kind = "snapshot"
        if kind == "restore" and not m.h[0].snapshot_fits():
            kind = "snapshot"
        op = _make(kind, m, g)
        m.apply(op)
        ops.append(op)
    return ops


def run_model(case, ops):
    """-> (model, [(outputs, observe(main), observe(second)) per op])."""
    m = Model(case)
    rec = []
    for op in ops:
        out = m.apply(op)
        rec.append((out, m.h[0].observe(), m.h[1].observe()))
    return m, rec


# ---------------------------------------------------------------- replay aid
def _fmt(v):
    if isinstance(v, np.ndarray):
        return np.array2string(v, threshold=10 ** 6, max_line_width=10 ** 6, separator=",")
    if isinstance(v, dict):
        return "{" + ", ".join("%s=%s" % (k, _fmt(x)) for k, x in v.items()) + "}"
    return repr(v)


def describe(op, short=False):
    args = {k: v for k, v in op.items() if k != "op"}
    if short:
        args = {k: v for k, v in args.items() if not isinstance(v, (dict, np.ndarray)) or
                (isinstance(v, np.ndarray) and v.ndim == 1)}
    return "%s(%s)" % (op["op"], ", ".join("%s=%s" % (k, _fmt(v)) for k, v in args.items()))


def main(argv=None):
    ap = argparse.ArgumentParser(description="print the op list of one call sequence")
    ap.add_argument("--case", required=True, choices=sorted(BY_NAME))
    ap.add_argument("--seed", type=int, required=True)
    ap.add_argument("--upto", type=int, default=None, help="ops 0 .. K only")
    ap.add_argument("--short", action="store_true", help="leave out the large arrays")
    a = ap.parse_args(argv)
    ops = gen_ops(BY_NAME[a.case], a.seed)
    for k, op in enumerate(ops[:None if a.upto is None else a.upto + 1]):
        print("%4d %s" % (k, describe(op, a.short)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
