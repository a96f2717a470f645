"""Agent base and the heuristic agents on the GPU env.

Reference: src/agents/base.py:13-136 (Base: set_log / test / record_testing_step),
src/agents/firstfit.py:21-38 and src/agents/bestfit.py:21-40. Same constructor
signatures and methods; act(observation) runs the heuristic scan in a HIP
kernel on the observation it is given (vmp_heuristic_act_obs).
"""
from dataclasses import asdict, dataclass, is_dataclass
from time import gmtime, strftime

import numpy as np

from .record import Record


@dataclass
class Config:
    pass


def _asdict(c):
    return asdict(c) if is_dataclass(c) else dict(vars(c))


def batched_env(env):
    """The BatchedVmEnv behind a vmp.VmEnv (or the env itself)."""
    return getattr(env, "_b", env)


class Base:
    def __init__(self, name: str, env, config):
        self.name = name
        self.env = env
        self.config = Config() if config is None else config
        self.record = Record(self.name, _asdict(self.env.config), _asdict(self.config))
        self.writer = None
        self.total_steps = 0
        self.rng = np.random.default_rng(self.env.config.seed)

    def set_log(self, jobname, logdir):
        """base.py:30-44; tensorboard is optional in this image (no-op without it)."""
        if not logdir:
            return
        try:
            from torch.utils.tensorboard import SummaryWriter
        except Exception:
            print("tensorboard is not installed: logging disabled")
            return
        self.writer = SummaryWriter(f"{logdir}/{strftime('%Y%m%d', gmtime())}-{self.name}-{jobname}")

    def learn(self):
        raise NotImplementedError

    def act(self, observation):
        raise NotImplementedError

    def save_model(self, modelpath):
        raise NotImplementedError

    def load_model(self, modelpath):
        raise NotImplementedError

    def eval(self, mode=True):
        raise NotImplementedError

    def test(self, show: bool = False, output: str = None, debug: bool = False):
        """base.py:63-118: one eval episode (eval_steps) from reset(seed=config.seed),
        every step recorded; returns the Record (saved to `output` if given). The
        Record metrics are accumulated on the device during the episode
        (vmp_record_*); the host keeps the per-step traces of the JSON. Each
        call starts a fresh Record (the reference appends the traces of every
        call while replacing vm_arrival_steps, so a second test() would pair
        two episodes' placements with one episode's arrivals): the saved
        traces and the summary always describe the same episode."""
        self.record.clear()
        self.env.eval()
        self.eval()
        obs, info = self.env.reset(seed=self.env.config.seed)
        dev = batched_env(self.env)
        dev.record(True)  # right after reset, as base.py:67-71 records from there
        done = False
        while not done:
            if debug:
                self.env.render()
            action = self.act(obs)
            obs, reward, done, _, info = self.env.step(action)
            if debug:
                print("action: \t\t%s" % (np.asarray(action).flatten()))
                print("validity: \t\t%s" % (info["valid"]))
                print("reward: \t\t%.2f" % (reward))
                print("")
            self.record_testing_step(reward, info)
        self.record.set_device_summary(dev.record_summary()[0])
        dev.record(False)
        summary = self.record.get_summary()
        if show:
            print(self.env.config)
            for k, v in summary.items():
                print("%s: %.2f" % (k, v))
            print("cpu: %s" % (info["cpu"]))
            print("memory: %s" % (info["memory"]))
        if output:
            self.record.save(output)
        return self.record

    def end_log(self):
        if self.writer:
            self.writer.close()

    def record_testing_step(self, reward: float, info):  # base.py:120-136
        r = self.record
        r.cpu.append(info["cpu"])
        r.memory.append(info["memory"])
        r.used_pm.append(len(info["cpu"]) - np.count_nonzero(info["cpu"]))  # empty PMs (quirk 12)
        r.vm_placements.append(info["vm_placement"])
        r.waiting_ratio.append(info["waiting_ratio"])
        r.actions.append(info["action"])
        r.rewards.append(reward)
        r.dropped_requests.append(info["dropped_requests"])
        r.total_requests.append(info["total_requests"])
        r.vm_arrival_steps = info["vm_arrival_steps"]
        r.target_cpu_mean.append(info["target_cpu_mean"])
        r.target_memory_mean.append(info["target_memory_mean"])
        r.served_requests.append(int(info["served_requests"]))
        r.total_cpu_requested = info["total_cpu_requested"]
        r.total_memory_requested = info["total_memory_requested"]
        r.suspended.append(info["suspend_actions"])
        r.placed.append(info["place_actions"])
        r.rank.append(info["rank"])


ACT_OBS_MAX_P = 9045  # vmp_heuristic_act_obs: 18 P + 1024 B of LDS <= 160 KB


class _HeuristicAgent(Base):
    POLICY = None

    def __init__(self, env):
        super().__init__(type(self).__name__, env, None)

    def learn(self):
        pass

    def load_model(self, modelpath):
        pass

    def save_model(self, modelpath):
        pass

    def eval(self, mode=True):
        pass

    def act(self, observation):
        """The heuristic's action computed from `observation` -> int64 [V] (or
        [N, V] for a BatchedVmEnv's [N, D] observations), as the reference
        reads only the obs it is passed (firstfit.py:22-28): an edited or stale
        observation gets its own action, not the env's. The scan runs in the
        HIP kernel (vmp_heuristic_act_obs); Base.test's fused act+step path
        (vmp_heuristic_step) acts on the env state, which is that obs."""
        b = batched_env(self.env)
        if b.P > ACT_OBS_MAX_P:
            # k_act_obs holds the PM view in one workgroup's LDS; beyond that the
            # env-state scan (vmp_heuristic_act) serves the env's own observation
            import torch
            o = torch.as_tensor(observation, dtype=torch.float32, device=b.device)
            if not torch.equal(o.reshape(b.n_envs, b.D), b.obs()):
                raise ValueError(f"act() on an edited observation supports P <= {ACT_OBS_MAX_P} "
                                 f"(this env has P = {b.P}); pass the env's own observation")
            a = b.heuristic_act(self.POLICY).cpu().numpy().astype(np.int64)
        else:
            a = b.heuristic_act_obs(observation, self.POLICY).cpu().numpy().astype(np.int64)
        return a[0] if b is not self.env else a


class FirstFitAgent(_HeuristicAgent):
    """firstfit.py:21-38: first PM (index order) that fits in f32, cpu-only update."""
    POLICY = "firstfit"


class BestFitAgent(_HeuristicAgent):
    """bestfit.py:21-40: feasible PM with the largest f32 cpu+mem, numpy scalar
    introsort tie order."""
    POLICY = "bestfit"


def choose_candidates(returns):
    """The rollout agent's choice: returns [n, C] (any float tensor, CPU or
    device) -> int64 [n], the candidate with the largest return of each row,
    the LOWEST index among equal ones. A candidate wins only by being strictly
    greater than every earlier one, so a NaN return never wins against a
    number before it. A fixed chain of comparisons: no host round trip."""
    import torch
    if returns.dim() != 2 or returns.shape[1] < 1:
        raise ValueError("returns must be [n, C] with C >= 1")
    best = returns[:, 0]
    idx = torch.zeros(returns.shape[0], dtype=torch.int64, device=returns.device)
    for c in range(1, returns.shape[1]):
        better = returns[:, c] > best
        idx = torch.where(better, torch.full_like(idx, c), idx)
        best = torch.where(better, returns[:, c], best)
    return idx


class RolloutAgent:
    """A rollout (policy-switching) agent between the heuristics and PPO: at
    every step each env tries every candidate action on copies of its own
    state, lets the `base` heuristic play `horizon` further steps, and takes
    the candidate with the best mean return.

    env: a BatchedVmEnv (or a vmp.VmEnv) of n envs. candidates: "firstfit" /
    "bestfit" (the heuristic's action on the current state) and "wait" (every
    VM's current placement: nothing is placed or moved this step). The agent
    holds a scratch BatchedVmEnv of n * C * futures envs of the same config,
    given the parent's per-env workload rows once, or the parent's traces and
    map when the parent is traced; a trace has one future, so futures is then 1.
    Scratch env (i * C + c) * M + m is env i's future m under candidate c.

    step():
      1. the scratch envs take their env's state (BatchedVmEnv.branch); on an
         RNG workload future m of env i at the agent's step t gets fresh
         streams from the counter-based seed
         seed + 4 * ((t * n + i) * M + m), the same for every candidate
         (common random numbers: candidates are compared on equal arrivals);
      2. candidate c's action is applied as one external step;
      3. rollout(base, horizon);
      4. the rewards are added in step order, the first step's included, then
         averaged over the M futures;
      5. choose_candidates: argmax per env, ties to the lowest index;
      6. the real env steps with that candidate's action.
    Everything runs on the device on the current stream; nothing is read back."""
    CANDIDATES = ("firstfit", "bestfit", "wait")

    def __init__(self, env, candidates=("firstfit", "bestfit", "wait"), horizon=10, futures=1,
                 base="firstfit", seed=None):
        import torch

        from . import _lib
        from .batched import BatchedVmEnv
        b = batched_env(env)
        candidates = tuple(candidates)
        if not candidates or any(c not in self.CANDIDATES for c in candidates):
            raise ValueError(f"candidates must be a non-empty choice of {self.CANDIDATES}")
        if base not in _lib.POLICIES:
            raise ValueError(f"base must be one of {tuple(_lib.POLICIES)}")
        if int(horizon) < 0 or int(futures) < 1:
            raise ValueError("horizon must be >= 0 and futures >= 1")
        self.env, self.b = env, b
        self.candidates, self.base, self.K = candidates, base, int(horizon)
        self.traced = b._traces is not None
        self.C, self.M = len(candidates), 1 if self.traced else int(futures)
        n, per = b.n_envs, self.C * self.M
        self.seed = int(b.config.seed if seed is None else seed)
        if self.seed < 0:
            raise ValueError("seed must be non-negative")
        self.t = 0
        self.scratch = BatchedVmEnv(b.config, n * per, device=b.device)
        try:
            if self.traced:
                traces, tmap = b._traces
                self.scratch.set_trace(traces, np.repeat(tmap, per))
            else:
                a, s = b.workload()
                if np.any(a != float(b.config.arrival_rate)) or np.any(s != float(b.config.service_length)):
                    self.scratch.set_workload(np.repeat(a, per), np.repeat(s, per))
        except Exception:
            self.scratch.close()
            raise
        dev = b.device
        j = torch.arange(n * per, device=dev)
        self._src = (j // per).to(torch.int32)
        # (i * M + m) of every scratch env: the same for all candidates
        self._future = (j // per) * self.M + j % self.M
        self._rows = torch.arange(n, device=dev)

    def close(self):
        self.scratch.close()

    def candidate_actions(self):
        """int32 [n, C, V]: every candidate's action on the env's current state."""
        import torch
        acts = []
        for c in self.candidates:
            if c == "wait":
                acts.append(self.b.state()["vm_placement"].to(torch.int32))
            else:
                acts.append(self.b.heuristic_act(c))
        return torch.stack(acts, dim=1)

    def future_seeds(self):
        """int64 [n * C * M] seeds of this step's futures, None on a traced env."""
        if self.traced:
            return None
        n = self.b.n_envs
        s = self.seed + 4 * (self.t * n * self.M + self._future)
        return s & ((1 << 62) - 1)

    def returns(self, acts):
        """f64 [n, C]: the mean over the futures of the summed rewards of
        candidate c's action followed by `horizon` steps of the base policy."""
        n, per, sc = self.b.n_envs, self.C * self.M, self.scratch
        if sc.eval_mode != self.b.eval_mode:  # the termination limit is no part of the state
            sc.eval(self.b.eval_mode)
        sc.branch(self.b, self._src, self.future_seeds())
        a = acts.unsqueeze(2).expand(n, self.C, self.M, self.b.V).reshape(n * per, self.b.V)
        _, total, _, _ = sc.step(a.contiguous(), want_valid=False, bool_done=False)
        if self.K:
            rew, _ = sc.rollout(self.base, self.K)
            for k in range(self.K):
                total = total + rew[k]
        total = total.view(n, self.C, self.M)
        ret = total[:, :, 0]
        for m in range(1, self.M):
            ret = ret + total[:, :, m]
        return ret / self.M if self.M > 1 else ret

    def act(self):
        """(actions int32 [n, V], choice int64 [n]) for the env's current state."""
        acts = self.candidate_actions()
        choice = choose_candidates(self.returns(acts))
        self.t += 1
        return acts[self._rows, choice], choice

    def step(self):
        """One agent step of every env -> (obs, reward, done, valid, choice)."""
        action, choice = self.act()
        obs, reward, done, valid = self.b.step(action)
        return obs, reward, done, valid, choice
