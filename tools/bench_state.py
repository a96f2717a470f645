"""Time BatchedVmEnv.set_state (vmp_set_state) against the identity vmp_branch,
which writes the same state bytes.

    python tools/bench_state.py [--envs 32768] [--runs 7] [--warmup 3] [--big-envs 512] [--out FILE]

Two handles of the headline shape (P100 / V1000, bench.py's CFG), the source
advanced a few steps and its exported state, counters and totals kept as device
tensors. Legs, alternating within every run so that each sees the same
neighbours:
  given     dst.set_state(state with cpu / memory, counters, totals)
  computed  the same without cpu / memory: the kernel derives the PM loads
  branch    dst.branch(src, [0, 1, .. n-1]): the yardstick
Every leg is timed from a host clock between two device synchronises and
between two HIP events (device time); the set_state legs use check=False, the
form without a status read-back. Then the same on --big-envs envs of
P1000 / V10000. Prints (and with --out writes) one JSON line: per leg the mean,
min, max and max - min in microseconds, the bytes the leg reads and writes as
its array sizes give them, the TB/s the device mean implies, and each set_state
leg's ratio to the branch leg.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "vm-placement-migration-gym_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import bench  # noqa: E402  (CFG: the headline's workload)
from tools.bench_branch import pitch, stats  # noqa: E402


def leg_bytes(P, V, n):
    """(read, written) per leg. set_state reads 32 B per slot (the kernel's
    second pass over them is served by the caches and not counted), the
    counters, totals and, if given, 16 B per PM; it writes 8 B per slot, the PM
    row and 10 header words. The branch reads and writes the env's three rows."""
    env = 256 + 16 * P + 4 * pitch(V)
    wr = 8 * V + 16 * P + 80
    return dict(given=(n * (32 * V + 16 * P + 64), n * wr), computed=(n * (32 * V + 64), n * wr),
                branch=(n * env, n * env))


def time_legs(cfg, n, runs, warmup, dev):
    from vmp.batched import BatchedVmEnv
    seeds = 4 * np.arange(n, dtype=np.int64)
    src, dst = BatchedVmEnv(cfg, n, seeds=seeds, device=dev), BatchedVmEnv(cfg, n, seeds=seeds + 1, device=dev)
    src.rollout("firstfit", 20)
    st, ctr, tot = src.state(), src.counters(), src.stats()[:, 3:5].contiguous()
    bare = {k: v for k, v in st.items() if k not in ("cpu", "memory")}
    ident = torch.arange(n, dtype=torch.int32, device=dev)
    status = {}

    def given():
        status["given"] = dst.set_state(st, counters=ctr, totals=tot, check=False)

    def computed():
        status["computed"] = dst.set_state(bare, counters=ctr, totals=tot, check=False)

    legs = dict(given=given, computed=computed, branch=lambda: dst.branch(src, ident))
    wall, devt = {k: [] for k in legs}, {k: [] for k in legs}
    for r in range(warmup + runs):
        for name, f in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize(dev)
            t1 = time.perf_counter()
            if r >= warmup:
                wall[name].append((t1 - t0) * 1e6)
                devt[name].append(e0.elapsed_time(e1) * 1e3)
    for k, s in status.items():
        if not bool((s == 1).all()):
            raise SystemExit(f"bench_state: leg {k} did not import every env")
    P, V = int(cfg.pms), int(cfg.vms)
    nbytes = leg_bytes(P, V, n)
    out = dict(envs=n, pms=P, vms=V)
    for k in legs:
        rd, wr = nbytes[k]
        mean = float(np.mean(devt[k]))
        out[k] = dict(wall=stats(wall[k]), device=stats(devt[k]), bytes_read=rd, bytes_written=wr,
                      device_TBps=round((rd + wr) / (mean * 1e-6) / 1e12, 3))
    for k in ("given", "computed"):
        out[k]["ratio_to_branch"] = round(out[k]["device"]["mean_us"] / out["branch"]["device"]["mean_us"], 2)
    src.close()
    dst.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=32768)
    ap.add_argument("--big-envs", type=int, default=512)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.runs < 5:
        ap.error("--runs must be at least 5")
    from vmp.config import Config
    if not torch.cuda.is_available():
        raise SystemExit("bench_state needs a HIP device")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    head = time_legs(Config(**bench.CFG), a.envs, a.runs, a.warmup, dev)
    big = time_legs(Config(**dict(bench.CFG, pms=1000, vms=10000)), a.big_envs, a.runs, a.warmup, dev)
    line = json.dumps(dict(tool="bench_state", headline=head, big=big))
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
