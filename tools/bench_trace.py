"""Trace-driven step against the RNG step on the headline workload.

    python tools/bench_trace.py [--envs 32768] [--steps 200] [--rounds 3]

P100 / V1000 (bench.py's CFG), FirstFit act + step, one handle. Three legs,
each fast-forwarded into the headline's staggered steady-state window
(bench.fast_forward) and snapshotted there:
  rng      the handle untraced (the config's Poisson workload)
  shared   Trace.synthetic(config, ...) replayed by every env
  per64    one synthetic trace per 64 envs (env i replays trace i // 64)
The legs alternate, `--rounds` times each, every round from its leg's snapshot
(so every round of a leg times the same window): `--steps` per-step launches
between one HIP event pair (ms per launch), then fused rollouts of
`--rollout-k` steps (env-steps/s). Prints one JSON line with mean, min and max
per leg and the traced / rng ratios of the means.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "vm-placement-migration-gym_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import bench  # noqa: E402  (CFG, fast_forward: the headline's workload and window)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=32768)
    ap.add_argument("--steps", type=int, default=200, help="timed per-step launches per round")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ff-steps", type=int, default=2500)
    ap.add_argument("--phase-groups", type=int, default=10)
    ap.add_argument("--phase-delta", type=int, default=100)
    ap.add_argument("--rollout-k", type=int, default=100)
    ap.add_argument("--rollouts", type=int, default=3, help="timed fused launches per round")
    ap.add_argument("--envs-per-trace", type=int, default=64)
    a = ap.parse_args()

    from vmp import _lib
    from vmp.batched import BatchedVmEnv
    from vmp.config import Config
    from vmp.trace import Trace

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    N, cfg = a.envs, Config(**bench.CFG)
    seeds = 4 * np.arange(N, dtype=np.int64)
    env = BatchedVmEnv(cfg, N, seeds=seeds, device=dev)
    env.eval(False)
    L, h = _lib.lib(), env._bind()
    stream = torch.cuda.current_stream(dev)
    obs = torch.empty((N, env.D), dtype=torch.float32, device=dev)
    rew = torch.empty((N,), dtype=torch.float64, device=dev)
    done = torch.empty((N,), dtype=torch.uint8, device=dev)

    # a trace outlasts the fast-forward and every timed step of a round
    total = a.ff_steps + (a.phase_groups - 1) * a.phase_delta
    t_len = total + a.warmup + a.steps + a.rollouts * a.rollout_k + 8
    n_tr = (N + a.envs_per_trace - 1) // a.envs_per_trace
    legs = {"rng": None, "shared": ([Trace.synthetic(cfg, t_len, 0)], None),
            "per64": ([Trace.synthetic(cfg, t_len, s) for s in range(n_tr)],
                      np.arange(N) // a.envs_per_trace)}

    def enter(name):
        if legs[name] is None:
            env.clear_trace()
        else:
            env.set_trace(*legs[name])

    snaps = {}
    for name in legs:
        enter(name)
        env.reset(seeds, obs=False)
        bench.fast_forward(env, "firstfit", seeds, a.ff_steps, a.phase_groups, a.phase_delta,
                           a.rollout_k)
        snaps[name] = env.snapshot()

    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn, n):
        torch.cuda.synchronize(dev)
        ev0.record(stream)
        for _ in range(n):
            fn()
        ev1.record(stream)
        torch.cuda.synchronize(dev)
        return ev0.elapsed_time(ev1)

    def one_step():
        _lib.check(L.vmp_heuristic_step(h, 0, None, _lib.ptr(obs), _lib.ptr(rew), _lib.ptr(done),
                                        None))

    ms = {k: [] for k in legs}
    rate = {k: [] for k in legs}
    requests = {}
    for _ in range(a.rounds):
        for name in legs:
            enter(name)
            env.restore(snaps[name])
            for _ in range(a.warmup):
                one_step()
            c0 = env.counters()
            ms[name].append(timed(one_step, a.steps) / a.steps)
            requests[name] = float((env.counters() - c0)[:, 0].double().mean()) / a.steps
            rews = torch.empty((a.rollout_k, N), dtype=torch.float64, device=dev)
            dc = torch.zeros(N, dtype=torch.int64, device=dev)
            t = timed(lambda: env.rollout("firstfit", a.rollout_k, rewards=rews, done_count=dc),
                      a.rollouts)
            rate[name].append(N * a.rollout_k * a.rollouts / (t * 1e-3))
    env.close()

    def stat(v):
        return {"mean": float(np.mean(v)), "min": float(np.min(v)), "max": float(np.max(v))}

    out = {"config": {"pms": cfg.pms, "vms": cfg.vms, "envs": N, "arrival_rate": cfg.arrival_rate,
                      "service_length": cfg.service_length, "steps": a.steps, "rounds": a.rounds,
                      "window": f"{a.phase_groups} groups x {a.phase_delta} steps after "
                                f"{a.ff_steps}", "trace_steps": t_len, "traces_per64": n_tr},
           "ms_per_step_launch": {k: stat(v) for k, v in ms.items()},
           "fused_env_steps_per_s": {k: stat(v) for k, v in rate.items()},
           "requests_per_env_step": requests}
    for k in ("shared", "per64"):
        out[f"{k}_over_rng_ms"] = out["ms_per_step_launch"][k]["mean"] / out["ms_per_step_launch"]["rng"]["mean"]
        out[f"{k}_over_rng_fused"] = (out["fused_env_steps_per_s"][k]["mean"]
                                      / out["fused_env_steps_per_s"]["rng"]["mean"])
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
