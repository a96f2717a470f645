"""How many env-steps of the headline window are idle (the idle
step of k_env<VPT, true>), from the C oracle (analysis only; no GPU): 12 envs
of the bench workload (P100 V1000, lambda 1.8182, L 1000, wr, training mode),
seeds 4 i, ages 2 500-3 499: one whole service period, the ages of bench.py's
staggered timed window.

An env-step is idle when, before it runs,
  - the previous step placed, finished and accepted nothing (the kernel's
    quiet bits, EnvHdr::pad 62 / 60);
  - no slot is NULL (nothing can be accepted);
  - no running VM has remaining <= 1 (nothing finishes).
Such a step only draws and drops its arrivals and advances the clock. Also
counted: the quiet steps (first condition alone) and the idle steps whose
smallest remaining runtime is 2 (the last idle step before a finisher).

Usage: python tools/idle_step_stats.py [P V lambda L [n_env t0 t1]] > profiles/idle_step_stats.txt"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from oracle import oracle as O  # noqa: E402


def config(P, V, lam, L):
    return dict(pms=P, vms=V, arrival_rate=lam, service_length=L, training_steps=10000,
                eval_steps=100000, seed=0, reward_function="wr", sequence="uniform",
                cap_target_util=True, beta=0.5, allow_null_action=True)


def replay(P, V, lam, L, n_env, t0, t1, record=False):
    """Per-step FirstFit steps 0 .. t1 - 1 of n_env oracle envs (seeds 4 i,
    training mode). Returns a dict of bool [t1 - t0, n_env] over the env-steps
    t0 .. t1 - 1: `idle`, `quiet`, `edge` (idle with smallest remaining 2);
    with record=True also every such step's `obs`, `rew`, `done` and the final
    `state` / `ctr` of each env (tests/test_gpu_idle_step.py)."""
    cfg = config(P, V, lam, L)
    T = t1 - t0
    out = {k: np.zeros((T, n_env), bool) for k in ("idle", "quiet", "edge")}
    if record:
        out.update(obs=np.zeros((T, n_env, 3 * V + 2 * P), np.float32), rew=np.zeros((T, n_env)),
                   done=np.zeros((T, n_env), bool), state=[], ctr=[])
    for i in range(n_env):
        e = O.OracleEnv(dict(cfg, seed=4 * i))
        e.eval(False)
        e.reset(4 * i)
        still = False
        c0 = e.counters()[0]
        for t in range(t1):
            if t >= t0:
                pl, _, _, _, _, rem = e.state()
                run = pl < P
                soon = int(rem[run].min()) if run.any() else 0
                out["quiet"][t - t0, i] = still
                out["idle"][t - t0, i] = still and not (pl == P + 1).any() and soon > 1
                out["edge"][t - t0, i] = out["idle"][t - t0, i] and soon == 2
            o, r, d, _ = e.step(e.firstfit())
            if record and t >= t0:
                out["obs"][t - t0, i], out["rew"][t - t0, i], out["done"][t - t0, i] = o, r, d
            c1 = e.counters()[0]
            d = c1 - c0  # total_requests, served, suspend, place, dropped
            still = d[3] == 0 and d[1] == 0 and d[0] - d[4] == 0
            c0 = c1
        if record:
            out["state"].append(e.state())
            out["ctr"].append(e.counters()[0])
    return out


def main(argv):
    P, V, lam, L = (int(argv[0]), int(argv[1]), float(argv[2]), float(argv[3])) if len(argv) >= 4 \
        else (100, 1000, 1.8182, 1000.0)
    n_env, t0, t1 = (int(x) for x in argv[4:7]) if len(argv) >= 7 else (12, 2500, 3500)
    r = replay(P, V, lam, L, n_env, t0, t1)
    idle, quiet, edge = r["idle"], r["quiet"], r["edge"]
    print(f"P{P} V{V} lambda {lam} L {L:g}, {n_env} envs (seeds 4 i), env-steps {t0}-{t1 - 1}, "
          f"per-step FirstFit, wr, training mode")
    print(f"share of env-steps: idle {idle.mean():.3f}, quiet {quiet.mean():.3f}")
    runs = int(idle[0].sum() + (idle[1:] & ~idle[:-1]).sum())
    print(f"idle runs entered {runs}, idle steps with smallest remaining 2 (last before a "
          f"finisher) {int(edge.sum())}")
    if t1 - t0 >= 200:
        print("idle share by 100-step bin:",
              " ".join(f"{idle[b:b + 100].mean():.3f}" for b in range(0, t1 - t0, 100)))


if __name__ == "__main__":
    main(sys.argv[1:])
