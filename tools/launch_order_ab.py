"""Launch order A/B ("Launch order"): 200 back-to-back per-step
FirstFit launches of the headline workload from ONE snapshot of the headline's
staggered window, for each order mode (0 index order, 1 direction, 2 direction
+ idle envs last; optionally other tail divisors), at several batch sizes.
Every mode starts from the same restored state and makes the same warm-up
launches, so the modes time the same env-steps; the rounds alternate the modes.

If Infinity-Cache reuse is what mode 1 gains from, its relative gain shrinks
as the batch grows and is about nil where a whole launch fits the cache.

Usage: python tools/launch_order_ab.py [--envs 8192,32768,65536] [--rounds 3]
           [--modes 0,1,2] > profiles/launch_order_ab.log"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import bench  # noqa: E402  (also puts the package on sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="8192,32768,65536")
    ap.add_argument("--modes", default="0,1,2")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    from vmp import _lib
    from vmp.batched import BatchedVmEnv
    from vmp.config import Config
    from vmp.replicas import shard_seeds
    dev = torch.device("cuda", 0)
    L = _lib.lib()
    modes = [int(m) for m in args.modes.split(",")]
    P, V = bench.CFG["pms"], bench.CFG["vms"]
    for N in (int(x) for x in args.envs.split(",")):
        seeds = shard_seeds(0, N)
        env = BatchedVmEnv(Config(**bench.CFG), N, seeds=seeds, device=dev)
        env.eval(False)
        bench.fast_forward(env, "firstfit", seeds, 2500, 10, 100, 100)
        snap = env.snapshot()
        obs = torch.empty((N, 3 * V + 2 * P), dtype=torch.float32, device=dev)
        rew = torch.empty((N,), dtype=torch.float64, device=dev)
        done = torch.empty((N,), dtype=torch.uint8, device=dev)
        h = env._bind()
        stream = torch.cuda.current_stream(dev)

        def step():
            _lib.check(L.vmp_heuristic_step(h, 0, None, _lib.ptr(obs), _lib.ptr(rew), _lib.ptr(done), None))

        ms = {m: [] for m in modes}
        sums = {}
        for r in range(args.rounds):
            for m in (modes if r % 2 == 0 else modes[::-1]):
                env.restore(snap)
                _lib.check(L.vmp_debug_launch_order(h, m))
                for _ in range(args.warmup):
                    step()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(dev)
                e0.record(stream)
                for _ in range(args.steps):
                    step()
                e1.record(stream)
                torch.cuda.synchronize(dev)
                ms[m].append(e0.elapsed_time(e1) / args.steps)
                # same env-steps in every mode: the last launch's outputs and the counters agree
                sums.setdefault(m, (float(rew.sum()), int(env.counters().sum())))
        assert len(set(sums.values())) == 1, sums
        base = float(np.mean(ms[modes[0]]))
        for m in modes:
            x = np.array(ms[m])
            print(json.dumps({"envs": N, "mode": m, "ms_mean": round(float(x.mean()), 5),
                              "ms_min": round(float(x.min()), 5), "ms_max": round(float(x.max()), 5),
                              "vs_first_mode_pct": round(100 * (float(x.mean()) / base - 1), 2),
                              "runs": [round(float(v), 5) for v in x]}), flush=True)
        env.close()


if __name__ == "__main__":
    main()
