"""Experiment sweeps of the reference (exp_suspension.py, exp.py) as batched GPU
runs: every (agent, load, service length) cell is one BatchedVmEnv whose envs
are the cell's seeds, all cells advance side by side on their own streams, and
the Record metrics are kept on the device (vmp_record_*), so nothing per step
comes back to the host. This replaces the reference's process fan-out
(exp.py:1-2, 8 processes of one env each) and its per-step host Record.

    python -m vmp.exp suspension --out data.csv            # heuristic rows
    python -m vmp.exp suspension --merge                   # one handle per agent, per-env workload
    python -m vmp.exp suspension --agents ppo --weights w.pt --out ppo.csv
    python -m vmp.exp performance --loads 1.0,0.6          # exp_performance.py summary
    python -m vmp.exp performance_small                    # exp_performance_small.py
    python -m vmp.exp vm_size                              # exp_vm_size.py summary
    python -m vmp.exp reward --agents ppo --weights 'w/ppo-{reward}.pt'   # exp_reward.py
    python -m vmp.exp migration_ratio --agents bestfit,ppo --weights 'w/ppo-{reward}.pt'
    python -m vmp.exp paired --trace a.npz,b.npz           # every agent on the same requests
    python -m vmp.exp paired --trace a.npz --requests r.csv   # ... and what became of each request
    python -m vmp.exp paired --trace a.npz --state s.npz      # ... from a saved cluster state
    python -m vmp.exp suspension --series s.csv --series-stride 100   # any experiment: curves over time

Rows are printed in exp_suspension.py's CSV layout (exp_suspension.py:51-58):
Agent, Load, Service Length, Total Served, Valid Suspend Actions, Valid
Actions, Life, Average Pending, Average Slowdown, Max Slowdown.
"""
import argparse
from dataclasses import dataclass

import numpy as np
import torch

from .batched import BatchedVmEnv
from .config import Config

SUSPENSION_HEADER = ("Agent, Load, Service Length, Total Served, Valid Suspend Actions, "
                     "Valid Actions, Life, Average Pending, Average Slowdown, Max Slowdown")

# config/100.yml's environment section (the sweeps override reward / arrival rate)
ENV100 = dict(pms=100, vms=300, service_length=1000, arrival_rate=1.8182, training_steps=10000,
              eval_steps=100000, seed=0, reward_function="kl", cap_target_util=True,
              sequence="uniform", beta=0.5, allow_null_action=True)
PPO100 = dict(episodes=100, hidden_size=512, masked=True, batch_size=100, minibatch_size=25,
              migration_ratio=0.002)


@dataclass
class Cell:
    agent: str
    load: float
    service_length: int
    seeds: tuple = (0,)
    weights: str = None
    cfg: dict = None   # the cell's environment config (else make_config(load, length))
    ppo: dict = None   # PPOConfig overrides (exp_performance.py:28-33)
    name: str = None   # row label (jobname)


def suspension_config(load, sr, env=ENV100):
    """exp_suspension.py:13-19: reward wr, uniform sizes, the given service length,
    arrival_rate = round(pms / 0.55 / sr * load, 3)."""
    c = dict(env)
    c.update(reward_function="wr", sequence="uniform", service_length=sr,
             arrival_rate=float(np.round(c["pms"] / 0.55 / sr * load, 3)))
    return c


class _RecordedRollout:
    """`g_steps` recorded heuristic steps (act+step, then the recorder: two
    launches per step) of one env captured as a HIP graph, so a long eval costs
    one graph launch per g_steps steps instead of 2 * g_steps kernel launches."""

    def __init__(self, env, policy, g_steps):
        self.env, self.policy, self.g = env, policy, g_steps
        n = env.n_envs
        self.rew = torch.empty((g_steps, n), dtype=torch.float64, device=env.device)
        self.dc = torch.zeros(n, dtype=torch.int64, device=env.device)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            env.rollout(policy, g_steps, rewards=self.rew, done_count=self.dc)

    def run(self, k):
        for _ in range(k // self.g):
            self.graph.replay()
        if k % self.g:
            self.env.rollout(self.policy, k % self.g)


HEURISTICS = ("firstfit", "bestfit")
WORKLOAD_KEYS = ("arrival_rate", "service_length")


def merge_groups(cells, cfgs, merge=True):
    """Which cells share one handle: a list of lists of cell indices, in order
    of first appearance. Without `merge` every cell is its own group. With it,
    heuristic cells of the same agent whose configs differ only in
    arrival_rate / service_length (and the config seed, which the explicit
    per-cell seeds override) form one group: their seeds become the envs of one
    handle with a per-env workload. PPO cells, and cells that differ in
    anything else, stay alone."""
    groups, by_key = [], {}
    for i, (cell, cfg) in enumerate(zip(cells, cfgs)):
        if cell.agent != "ppo" and cell.agent not in HEURISTICS:
            raise ValueError(f"agent {cell.agent!r} has no batched GPU path")
        if not merge or cell.agent == "ppo":
            groups.append([i])
            continue
        rest = tuple(sorted((k, repr(v)) for k, v in cfg.items()
                            if k not in WORKLOAD_KEYS and k != "seed"))
        key = (cell.agent, rest)
        if key in by_key:
            by_key[key].append(i)
        else:
            by_key[key] = [i]
            groups.append(by_key[key])
    return groups


# ------------------------------------------------------------ time series
def _series_fields():
    from .series import COUNTERS, SUMMED
    return SUMMED + tuple(c for c in COUNTERS if c != "timestep")


def series_header():
    return "Cell, Agent, Envs, Window, Timestep" + "".join(
        ", %s Mean, %s Std" % (f, f) for f in _series_fields())


def series_rows(index, name, ser):
    """One CSV row per window of a cell's `vmp.series.Series` (its envs are the
    cell's seeds): the cell's index and name, its env count, the window, the
    timestep counter after the window's last step, then the mean and the std
    over the envs of every field's window mean (Series.band; floats in repr)."""
    bands = [ser.band(f) for f in _series_fields()]
    ts = ser.timestep[0] if ser.n_envs else []
    rows = []
    for r in range(len(bands[0][0])):
        rows.append("%d,%s,%d,%d,%d" % (index, name, ser.n_envs, r, int(ts[r])) + "".join(
            ",%r,%r" % (float(m[r]), float(sd[r])) for m, sd in bands))
    return rows


def _series_request(series):
    """(stride, path) of a `series=` argument, None for none."""
    if series is None:
        return None
    stride, path = series
    if int(stride) < 1:
        raise ValueError("series stride must be >= 1")
    return int(stride), path


def _write_series(path, rows):
    with open(path, "w") as f:
        f.write("\n".join([series_header()] + rows) + "\n")


def run_cells(cells, make_config=None, eval_steps=None, chunk=2000, device="cuda:0",
              graph_steps=100, merge=False, series=None):
    """Evaluate every cell (Base.test per seed, base.py:63-118) for its eval_steps
    and return one list of Record summaries per cell (one dict per seed). All
    seeds of a cell are the envs of one handle, so the recorder's cross-env sums
    (VMP_REC_XMEM) span exactly the cell's seeds. Heuristic cells replay a
    captured graph of graph_steps recorded steps (0 = plain launches).
    merge=True: the cells of one merge_groups group are the envs of ONE handle
    (their seeds concatenated, each env at its cell's arrival rate and service
    length), with one recorder and one captured rollout; the return value keeps
    its shape, except that `_xmem` (a sum over a handle's envs) is NaN.
    series=(stride, path): also keep the per-step time series of every env on
    the device (BatchedVmEnv.series, `stride` steps a window) and write one
    row per cell and window to the CSV `path` (series_header / series_rows);
    merged cells still report their own envs."""
    series = _series_request(series)
    series_out = {}
    cfgs = []
    for cell in cells:
        cfg = dict(cell.cfg) if cell.cfg is not None else make_config(cell.load, cell.service_length)
        if eval_steps is not None:
            cfg["eval_steps"] = int(eval_steps)
        cfgs.append(cfg)
    groups = merge_groups(cells, cfgs, merge)
    envs, agents, streams, steps = [], [], [], []
    for g in groups:
        cell, cfg = cells[g[0]], cfgs[g[0]]
        seeds = [int(s) for i in g for s in cells[i].seeds]
        s = torch.cuda.Stream(device=device)
        with torch.cuda.stream(s):
            env = BatchedVmEnv(Config(**cfg), len(seeds), seeds=seeds, device=device)
            if len(g) > 1:  # before the capture: the first call moves the kernels' constants
                env.set_workload(
                    [cfgs[i]["arrival_rate"] for i in g for _ in cells[i].seeds],
                    [cfgs[i]["service_length"] for i in g for _ in cells[i].seeds])
            env.eval(True)
            env.reset(torch.tensor(seeds, dtype=torch.int64))
            env.record(True)  # before the graph capture, so replays are recorded too
            if series:
                env.series(True, capacity=-(-int(cfg["eval_steps"]) // series[0]), stride=series[0])
            agent = None
            if cell.agent == "ppo":
                from .ppo import ActStepGraph, PPOAgent, PPOConfig
                ag = PPOAgent(env, PPOConfig(**dict(PPO100, **(cell.ppo or {}))))
                ag.load_model(cell.weights)
                ag.eval(True)
                agent = ActStepGraph(ag, warmup=0)
            elif graph_steps:
                agent = _RecordedRollout(env, cell.agent, int(graph_steps))
        envs.append(env)
        agents.append(agent)
        streams.append(s)
        steps.append(int(cfg["eval_steps"]))
    done = [0] * len(groups)
    while any(d < t for d, t in zip(done, steps)):
        for i, (g, env, agent, s) in enumerate(zip(groups, envs, agents, streams)):
            k = min(chunk, steps[i] - done[i])
            if k <= 0:
                continue
            with torch.cuda.stream(s):
                if agent is None:
                    env.rollout(cells[g[0]].agent, k)
                elif isinstance(agent, _RecordedRollout):
                    agent.run(k)
                else:
                    for _ in range(k):
                        agent.replay()
            done[i] += k
    out = [None] * len(cells)
    for g, env, s in zip(groups, envs, streams):
        with torch.cuda.stream(s):
            summ = env.record_summary()
            ser = env.series_read() if series else None
        env.close()
        at = 0
        for i in g:
            out[i] = summ[at:at + len(cells[i].seeds)]
            if series:
                series_out[i] = series_rows(i, cells[i].name or cells[i].agent,
                                            ser.env(slice(at, at + len(cells[i].seeds))))
            at += len(cells[i].seeds)
    if series:
        _write_series(series[1], [r for i in sorted(series_out) for r in series_out[i]])
    if merge:
        for summ in out:
            for d in summ:
                d["_xmem"] = float("nan")
    return out


def suspension_row(cell, summaries):
    """exp_suspension.py:51-58 for one cell (mean over its seeds)."""
    f = lambda k: float(np.mean([s[k] for s in summaries]))  # noqa: E731
    name = cell.agent if cell.weights is None else cell.weights.split("/")[-1].split(".")[0]
    susp, placed = f("total suspend actions"), f("total place actions")
    return "%s,%.1f,%d,%d,%d,%d,%d,%.3f,%.3f,%.3f" % (
        name, cell.load, cell.service_length, f("total served VMs"), susp, susp + placed,
        f("_mean_life"), f("_mean_pending"), f("_mean_slowdown"), f("_max_slowdown"))


def suspension_sweep(agents=("firstfit", "bestfit"), loads=None, lengths=None, seeds=(0,),
                     weights=None, eval_steps=None, merge=False, series=None):
    """The exp_suspension.py grid (load 1.0 x service lengths 100..3900 step 200,
    then service length 1000 x loads 0.2..1.0) for the given agents. merge=True
    runs each heuristic agent's whole grid as the envs of one handle (run_cells)."""
    if lengths is None:
        lengths = list(range(100, 4100, 200))
    if loads is None:
        loads = [float(x) for x in np.arange(0.2, 1.1, 0.1)]
    cells = [Cell(a, 1.0, int(sr), tuple(seeds), weights if a == "ppo" else None)
             for sr in lengths for a in agents]
    cells += [Cell(a, float(ld), 1000, tuple(seeds), weights if a == "ppo" else None)
              for ld in loads for a in agents]
    res = run_cells(cells, suspension_config, eval_steps=eval_steps, merge=merge, series=series)
    return [suspension_row(c, r) for c, r in zip(cells, res)]


# ------------------------------------------------------------ paired comparison
PAIRED_HEADER = ("Agent, Trace, Steps, Requests, Total Served, Valid Suspend Actions, "
                 "Valid Actions, Life, Average Pending, Average Slowdown, Max Slowdown")


def paired_row(agent, index, trace, summary):
    """One (agent, trace) row: suspension_row's metric columns for one env."""
    susp, placed = summary["total suspend actions"], summary["total place actions"]
    life = summary["_mean_life"]  # NaN for an env no VM ever lived in (an empty trace)
    return "%s,%d,%d,%d,%d,%d,%d,%s,%.3f,%.3f,%.3f" % (
        agent, index, trace.steps, trace.requests, summary["total served VMs"], susp,
        susp + placed, "%d" % life if life == life else "nan", summary["_mean_pending"],
        summary["_mean_slowdown"], summary["_max_slowdown"])


def paired_sweep(traces, agents=("firstfit", "bestfit"), config=None, eval_steps=None,
                 weights=None, device="cuda:0", series=None, state=None):
    """Every agent on the SAME requests: one handle per agent whose env i replays
    traces[i] (BatchedVmEnv.set_trace), the device recorder on, eval_steps steps
    (default: the longest trace). A traced env's requests do not depend on what
    the policy did with the earlier ones, so the rows of one trace compare the
    agents on one workload. One CSV row per (agent, trace), see PAIRED_HEADER.
    series=(stride, path): also write the time series CSV, one row per agent
    and window over the agent's envs (run_cells). state: a vmp.state.State the
    envs start from instead of an empty env (BatchedVmEnv.set_start_state); a
    state with counters brings its timestep, which selects the trace step."""
    return _paired_run(traces, agents, config, eval_steps, weights, device, False, series,
                       state)[0]


def _paired_run(traces, agents, config, eval_steps, weights, device, log, series=None,
                state=None):
    """paired_sweep's runs; log=True: with the per-request outcome log on;
    state: a vmp.state.State every env starts from (one env row serves all).
    Returns (rows, {agent: RequestLog})."""
    series = _series_request(series)
    series_out = []
    traces = list(traces)
    cfg = dict(ENV100, reward_function="wr") if config is None else dict(config)
    steps = int(eval_steps) if eval_steps is not None else max(t.steps for t in traces)
    cfg["eval_steps"] = max(int(cfg.get("eval_steps", 0)), steps)
    rows, logs = [], {}
    for name in agents:
        if name != "ppo" and name not in HEURISTICS:
            raise ValueError(f"agent {name!r} has no batched GPU path")
        env = BatchedVmEnv(Config(**cfg), len(traces), device=device)
        env.set_trace(traces, np.arange(len(traces)))  # before any capture: it switches kernels
        env.eval(True)
        env.set_start_state(state)
        env.reset()
        env.record(True)
        if log:  # before the capture below: a graph captured earlier would not log
            env.request_log(True)
        if series:
            env.series(True, capacity=-(-steps // series[0]), stride=series[0])
        if name == "ppo":
            from .ppo import ActStepGraph, PPOAgent, PPOConfig
            ag = PPOAgent(env, PPOConfig(**PPO100))
            ag.load_model(weights)
            ag.eval(True)
            graph = ActStepGraph(ag, warmup=0)
            for _ in range(steps):
                graph.replay()
        else:
            env.rollout(name, steps)
        summ = env.record_summary()
        if log:
            logs[name] = env.request_log_read()
        if series:
            series_out += series_rows(list(agents).index(name), name, env.series_read())
        env.close()
        rows += [paired_row(name, i, t, s) for i, (t, s) in enumerate(zip(traces, summ))]
    if series:
        _write_series(series[1], series_out)
    return rows, logs


def paired_requests_header(agents):
    return "Trace, Request, Arrival Step, CPU, Memory, Runtime" + "".join(
        ", %s Slot, %s Placed, %s Finished, %s Suspends, %s Wait Steps" % ((a,) * 5)
        for a in agents)


def paired_requests(traces, agents=("firstfit", "bestfit"), config=None, eval_steps=None,
                    weights=None, device="cuda:0", logs=None):
    """What became of every request under every agent: paired_sweep's runs with
    the per-request outcome log on (BatchedVmEnv.request_log), one CSV row per
    (trace, request) in paired_requests_header's layout: the trace's arrival
    step, cpu, mem (hundredths) and runtime of the request, then per agent its
    slot status (-2 not observed, -1 dropped, else the slot), the timesteps of
    its first placement and of its finish (0 = not yet), its valid suspensions
    and its waiting steps. logs ({agent: RequestLog} of earlier runs on these
    traces, env i = trace i): format those, run nothing."""
    traces = list(traces)
    if logs is None:
        logs = _paired_run(traces, agents, config, eval_steps, weights, device, True)[1]
    rows = []
    for i, t in enumerate(traces):
        step_of = np.repeat(np.arange(t.steps), t.arrivals())
        for j in range(t.requests):
            row = "%d,%d,%d,%d,%d,%d" % (i, j, step_of[j], t.cpu[j], t.mem[j], t.runtime[j])
            for a in agents:
                lg = logs[a]
                r = lg.rows[i, j] if j < lg.capacity else (-2, 0, 0, 0, 0, 0)
                row += ",%d,%d,%d,%d,%d" % (r[0], r[2], r[3], r[4], r[5])
            rows.append(row)
    return rows


PAIRED_DIFF_HEADER = ("Trace, Agent A, Agent B, Placed Both, Mean Pending Difference, "
                      "Median Pending Difference, Dropped Only A, Dropped Only B, Finished Both, "
                      "Mean Sojourn Difference")


def paired_differences(traces, agents, logs):
    """Per trace and pair of agents (A before B in `agents`), over the requests
    of the trace: how many were placed under both and the mean and median of
    pending_steps(A) - pending_steps(B) over those; the requests dropped under
    A only and under B only; how many finished under both and the mean of
    sojourn(A) - sojourn(B) over those. One CSV row each (PAIRED_DIFF_HEADER);
    a mean over no request prints nan."""
    fmt = lambda x: "%.3f" % x if x == x else "nan"  # noqa: E731
    rows = []
    for i, t in enumerate(traces):
        for x in range(len(agents)):
            for y in range(x + 1, len(agents)):
                la, lb = logs[agents[x]], logs[agents[y]]
                n = min(t.requests, la.capacity, lb.capacity)
                both = la.is_placed[i, :n] & lb.is_placed[i, :n]
                d = (la.pending_steps[i, :n] - lb.pending_steps[i, :n])[both].astype(np.float64)
                fin = la.is_finished[i, :n] & lb.is_finished[i, :n]
                sj = (la.sojourn[i, :n] - lb.sojourn[i, :n])[fin].astype(np.float64)
                rows.append("%d,%s,%s,%d,%s,%s,%d,%d,%d,%s" % (
                    i, agents[x], agents[y], int(both.sum()),
                    fmt(d.mean() if d.size else float("nan")),
                    fmt(float(np.median(d)) if d.size else float("nan")),
                    int((la.dropped[i, :n] & ~lb.dropped[i, :n]).sum()),
                    int((lb.dropped[i, :n] & ~la.dropped[i, :n]).sum()), int(fin.sum()),
                    fmt(sj.mean() if sj.size else float("nan"))))
    return rows


# ------------------------------------------------------------ exp_performance
PERFORMANCE_HEADER = ("Agent, Load, Return, Drop Rate, Served VM, Suspend Actions, CPU Mean, "
                      "CPU Variance, Memory Mean, Memory Variance, Pending Rate, Waiting Ratio, "
                      "Slowdown Rate")
# config/10.yml's environment section (exp_performance_small.py:20)
ENV10 = dict(pms=10, vms=30, service_length=1000, arrival_rate=0.0182, training_steps=10000,
             eval_steps=100000, seed=1, reward_function="kl", cap_target_util=True,
             sequence="uniform", beta=0.5, allow_null_action=True)


def performance_config(load, reward="ut", env=ENV100, jobname=""):
    """exp_performance.py:20-33: the reward override, arrival_rate =
    round(pms / 0.55 / service_length * load, 4), and the -masked / -unmasked
    job suffixes (allow_null_action; the PPO mask follows via Cell.ppo)."""
    c = dict(env)
    c.update(reward_function=reward,
             arrival_rate=float(np.round(c["pms"] / 0.55 / c["service_length"] * load, 4)))
    if "-masked" in jobname:
        c["allow_null_action"] = True
    if "-unmasked" in jobname:
        c["allow_null_action"] = False
    return c


def performance_cell(agent, jobname, load, reward="ut", weights=None, small=False, seeds=None):
    """One evaluate() call of exp_performance.py (seeds 0..4) or
    exp_performance_small.py (config/10.yml, seeds 1..5)."""
    env = ENV10 if small else ENV100
    if seeds is None:
        seeds = tuple(range(1, 6)) if small else tuple(range(5))
    ppo = None
    if "-masked" in jobname:
        ppo = {"masked": True}
    if "-unmasked" in jobname:
        ppo = {"masked": False}
    return Cell(agent, float(load), env["service_length"], tuple(seeds), weights,
                cfg=performance_config(load, reward, env, jobname), ppo=ppo, name=jobname)


def performance_row(cell, summaries):
    """exp_performance.py:94-138 for one cell from its seeds' device summaries.
    Memory Variance keeps the reference's axis: np.var(memory, axis=0) is the
    variance over the seeds per (step, PM), = mean_s E[x^2] - E[(mean_s x)^2],
    the second term from the recorder's cross-env sums."""
    f = lambda k: float(np.mean([s[k] for s in summaries]))  # noqa: E731
    S = len(summaries)
    mem_var = f("_mem2") - sum(s["_xmem"] for s in summaries) / (S * S)
    return "%s,%.2f,%.3f,%.3f,%d,%d,%.3f,%.3f,%.3f,%.3f,%.3f,%.3f,%.3f" % (
        cell.name or cell.agent, cell.load, f("_return"), f("_drop_rate"), f("total served VMs"),
        f("total suspend actions"), f("_cpu_mean"), f("_cpu_var"), f("_mem_mean"), mem_var,
        f("_mean_pending"), f("_waiting"), f("_mean_slowdown"))


def performance_sweep(cells, eval_steps=None, merge=False, series=None):
    if merge:  # Memory Variance needs the recorder's sums over exactly a cell's seeds
        raise ValueError("performance_sweep cannot merge cells: its Memory Variance column "
                         "is a cross-env sum over one handle's envs (_xmem)")
    res = run_cells(cells, eval_steps=eval_steps, series=series)
    return [performance_row(c, r) for c, r in zip(cells, res)]


# ---------------------------------------------------------------- exp_vm_size
VM_SIZE_HEADER = ("Model, Return, Drop Rate, Served VM, Suspend Actions, CPU Mean, "
                  "CPU Variance, Memory Mean, Memory Variance, Waiting Ratio")


def vm_size_config(seq, env=ENV100):
    """exp_vm_size.py:12-19: config/100.yml (reward kl) with the sequence and an
    unrounded arrival rate pms / mean size / service_length."""
    c = dict(env)
    c["sequence"] = seq
    if seq == "lowuniform":
        c["arrival_rate"] = c["pms"] / 0.375 / c["service_length"]
    elif seq == "highuniform":
        c["arrival_rate"] = c["pms"] / 0.625 / c["service_length"]
    return c


def vm_size_cell(agent, seq, weights=None, seeds=tuple(range(5))):
    return Cell(agent, 1.0, ENV100["service_length"], tuple(seeds), weights,
                cfg=vm_size_config(seq), name=agent)


def vm_size_row(cell, summaries):
    """exp_vm_size.py:60-98 (variances over PMs for both resources)."""
    f = lambda k: float(np.mean([s[k] for s in summaries]))  # noqa: E731
    return "%s,%.4f,%.4f,%d,%d,%.4f,%.4f,%.4f,%.4f,%.4f" % (
        cell.name or cell.agent, f("_return"), f("_drop_rate"), f("total served VMs"),
        f("total suspend actions"), f("_cpu_mean"), f("_cpu_var"), f("_mem_mean"),
        f("_mem_var"), f("_waiting"))


def vm_size_sweep(cells, eval_steps=None, series=None):
    res = run_cells(cells, eval_steps=eval_steps, series=series)
    return [vm_size_row(c, r) for c, r in zip(cells, res)]


# ------------------------------------------------------ exp_reward / migration
REWARD_HEADER = ("Agent, Reward, Return, Drop Rate, Served VM, Suspend Actions, CPU Mean, "
                 "CPU Variance, Memory Mean, Memory Variance, Pending Rate, Waiting Ratio, "
                 "Slowdown Rate")
MIGRATION_HEADER = "Agent,Reward,Migration Ratio,CPU,Average Slowdown"


def reward_config(reward, env=ENV100):
    """exp_reward.py:24-28 / exp_migration_ratio.py:13-16: the reward, uniform
    sizes, arrival_rate = round(pms / 0.55 / service_length, 3)."""
    c = dict(env)
    c.update(reward_function=reward, sequence="uniform",
             arrival_rate=float(np.round(c["pms"] / 0.55 / c["service_length"], 3)))
    return c


def reward_cell(agent, reward, weights=None, migration_ratio=0.002, seeds=tuple(range(5))):
    """One evaluate_seeds() call of exp_reward.py (seeds 0..4)."""
    return Cell(agent, 1.0, ENV100["service_length"], tuple(seeds), weights,
                cfg=reward_config(reward), ppo={"migration_ratio": migration_ratio},
                name=agent)


def reward_row(cell, summaries):
    """exp_reward.py:108-135 (variances over PMs for both resources)."""
    f = lambda k: float(np.mean([s[k] for s in summaries]))  # noqa: E731
    return "%s,%s,%.3f,%.3f,%d,%d,%.3f,%.3f,%.3f,%.3f,%.3f,%.3f,%.3f" % (
        cell.name or cell.agent, cell.cfg["reward_function"], f("_return"), f("_drop_rate"),
        f("total served VMs"), f("total suspend actions"), f("_cpu_mean"), f("_cpu_var"),
        f("_mem_mean"), f("_mem_var"), f("_mean_pending"), f("_waiting"), f("_mean_slowdown"))


def reward_sweep(cells, eval_steps=None, series=None):
    res = run_cells(cells, eval_steps=eval_steps, series=series)
    return [reward_row(c, r) for c, r in zip(cells, res)]


def migration_cell(agent, reward, migration_ratio, weights=None):
    """One evaluate() call of exp_migration_ratio.py (config seed 0, one run)."""
    return Cell(agent, 1.0, ENV100["service_length"], (0,), weights, cfg=reward_config(reward),
                ppo={"migration_ratio": float(migration_ratio)}, name=agent)


def migration_row(cell, summaries):
    """exp_migration_ratio.py:43-48: mean CPU and mean slowdown of the one run."""
    s = summaries[0]
    return "%s,%s,%.3f,%.3f,%.3f" % (cell.name or cell.agent, cell.cfg["reward_function"],
                                     cell.ppo["migration_ratio"], s["_cpu_mean"],
                                     s["_mean_slowdown"])


def migration_sweep(cells, eval_steps=None, series=None):
    res = run_cells(cells, eval_steps=eval_steps, series=series)
    return [migration_row(c, r) for c, r in zip(cells, res)]


def arg_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("experiment", choices=["suspension", "performance", "performance_small",
                                           "vm_size", "reward", "migration_ratio", "paired"])
    ap.add_argument("--agents", default="firstfit,bestfit")
    ap.add_argument("--weights", default=None, help="PPO weights (.pt) for agent ppo")
    ap.add_argument("--seeds", default=None, help="comma list (default: the driver's seeds)")
    ap.add_argument("--loads", default=None, help="comma list (default: the reference grid)")
    ap.add_argument("--lengths", default=None, help="comma list of service lengths")
    ap.add_argument("--reward", default=None,
                    help="reward function(s): performance (default ut), reward (default wr,ut,kl)")
    ap.add_argument("--eval-steps", type=int, default=None)
    ap.add_argument("--merge", action="store_true",
                    help="suspension: one handle per heuristic agent, a per-env workload per cell")
    ap.add_argument("--trace", default=None, help="paired: comma list of Trace .npz files")
    ap.add_argument("--state", default=None,
                    help="paired: a vmp.state.State .npz every env starts from (one env row "
                         "serves all envs), not an empty env")
    ap.add_argument("--config", default=None,
                    help="paired: YAML with an `environment:` section (default config/100.yml's, wr)")
    ap.add_argument("--requests", default=None,
                    help="paired: also write one row per (trace, request) to this CSV and print "
                         "the per-request paired differences")
    ap.add_argument("--series", default=None,
                    help="any experiment: also write the per-step time series to this CSV, one "
                         "row per cell (per agent for paired) and window")
    ap.add_argument("--series-stride", type=int, default=1, help="steps per window of --series")
    ap.add_argument("--out", default=None)
    return ap


def main(argv=None):
    ap = arg_parser()
    a = ap.parse_args(argv)
    if a.series_stride < 1:
        ap.error("--series-stride must be >= 1")
    series = None if a.series is None else (a.series_stride, a.series)
    agents = a.agents.split(",")
    seeds = None if a.seeds is None else [int(x) for x in a.seeds.split(",")]
    loads = None if a.loads is None else [float(x) for x in a.loads.split(",")]
    if a.experiment == "paired":
        from .trace import Trace
        if not a.trace:
            ap.error("paired needs --trace FILE.npz[,FILE.npz...]")
        cfg = None
        if a.config:
            import yaml
            with open(a.config) as f:
                cfg = dict(yaml.safe_load(f)["environment"])
            if a.reward:
                cfg["reward_function"] = a.reward
        header = PAIRED_HEADER
        traces = [Trace.load(p) for p in a.trace.split(",")]
        state = None
        if a.state:
            from .state import State
            state = State.load(a.state)
        rows, logs = _paired_run(traces, agents, cfg, a.eval_steps, a.weights, "cuda:0",
                                 a.requests is not None, series, state)
        if a.requests is not None:
            with open(a.requests, "w") as f:
                f.write("\n".join([paired_requests_header(agents)]
                                  + paired_requests(traces, agents, logs=logs)) + "\n")
            rows = rows + [PAIRED_DIFF_HEADER] + paired_differences(traces, agents, logs)
    elif a.experiment == "suspension":
        header = SUSPENSION_HEADER
        rows = suspension_sweep(
            agents=agents, loads=loads,
            lengths=None if a.lengths is None else [int(x) for x in a.lengths.split(",")],
            seeds=seeds or [0], weights=a.weights, eval_steps=a.eval_steps, merge=a.merge,
            series=series)
    elif a.experiment in ("performance", "performance_small"):
        header = PERFORMANCE_HEADER
        small = a.experiment == "performance_small"
        reward = a.reward or "ut"
        cells = [performance_cell(ag, "ppo-" + reward if ag == "ppo" else ag, ld, reward,
                                  a.weights if ag == "ppo" else None, small, seeds)
                 for ld in (loads or [1.0]) for ag in agents]
        rows = performance_sweep(cells, eval_steps=a.eval_steps, merge=a.merge, series=series)
    elif a.experiment == "reward":
        header = REWARD_HEADER
        rewards = a.reward.split(",") if a.reward else ["wr", "ut", "kl"]
        cells = [reward_cell(ag, rw, a.weights.replace("{reward}", rw) if ag == "ppo" else None,
                             seeds=tuple(seeds) if seeds else tuple(range(5)))
                 for ag in agents for rw in rewards]
        rows = reward_sweep(cells, eval_steps=a.eval_steps, series=series)
    elif a.experiment == "migration_ratio":
        header = MIGRATION_HEADER
        ratios = [round(0.001 * i, 3) for i in range(10)]
        cells = [migration_cell(ag, rw, r, a.weights.replace("{reward}", rw)
                                if ag == "ppo" else None)
                 for r in ratios for ag in agents
                 for rw in (["ut"] if ag != "ppo" else ["wr", "ut", "kl"])]
        rows = migration_sweep(cells, eval_steps=a.eval_steps, series=series)
    else:
        header = VM_SIZE_HEADER
        cells = [vm_size_cell(ag, seq, a.weights if ag == "ppo" else None,
                              tuple(seeds) if seeds else tuple(range(5)))
                 for seq in ("lowuniform", "highuniform") for ag in agents]
        rows = vm_size_sweep(cells, eval_steps=a.eval_steps, series=series)
    text = header + "\n" + "\n".join(rows) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
