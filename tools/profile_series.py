"""The time series' kernel beside the recorder's and the request log's, for a
kernel trace.

    rocprofv3 --kernel-trace --stats -f csv -d OUT -o series -- \
        python tools/profile_series.py [--envs 4096] [--steps 1500]

tools/profile_reqlog.py's workload (P100 / V1000, bench.py's CFG, every env
replaying Trace.synthetic of that config, FirstFit act + step) with the
recorder, the request log AND the time series on at stride 1, so one step is
four launches: the env kernel, k_record, k_reqlog, k_series. The per-launch
times are read from the trace's kernel statistics; this script times nothing
itself. It prints the bytes per env-step that k_series moves by its layout, and
checks the series against the counters at the end.
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

import bench  # noqa: E402  (CFG: the headline workload)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=1500)
    a = ap.parse_args()

    from vmp.batched import BatchedVmEnv
    from vmp.config import Config
    from vmp.trace import Trace

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = Config(**bench.CFG)
    N, V, P = a.envs, cfg.vms, cfg.pms
    trace = Trace.synthetic(cfg, a.steps, 0)
    env = BatchedVmEnv(cfg, N, seeds=4 * np.arange(N, dtype=np.int64), device=dev)
    env.set_trace(trace)
    env.eval(True)
    env.reset()
    env.record(True)
    env.request_log()
    env.series(capacity=a.steps)
    obs = torch.empty((N, env.D), dtype=torch.float32, device=dev)
    rew = torch.empty((N,), dtype=torch.float64, device=dev)
    done = torch.empty((N,), dtype=torch.uint8, device=dev)
    for _ in range(a.steps):
        env.heuristic_step("firstfit", obs=obs, reward=rew, done=done)
    torch.cuda.synchronize(dev)
    ser = env.series_read()
    ctr = env.counters().cpu().numpy()
    last = ser.rows[:, -1]
    ok = bool(np.all(ser.count == a.steps) and not ser.lost.any() and np.all(ser.steps == 1)
              and np.all(ser.rows == ser.rows[0])
              and np.array_equal(last[:, 14:19], ctr[:, :5].astype(np.float64))
              and np.array_equal(last[:, 13], ctr[:, 5].astype(np.float64))
              and np.array_equal(ser.total_requests[0], trace.offs[1:].astype(np.float64))
              and float(last[0, 1]) == float(rew[0]))
    env.close()
    # per slot: the slot word 4 B; per PM: cpu and memory 16 B (re-read from cache by the four
    # pairwise passes); per env: COUNT, reward, waiting_ratio and six counters 72 B, the
    # 152-B row, COUNT written 8 B
    print(json.dumps({"envs": N, "V": V, "P": P, "steps": a.steps, "checks_hold": ok,
                      "k_series_streamed_bytes_per_env_step": V * 4 + P * 16 + 72 + 19 * 8 + 8,
                      "k_record_streamed_bytes_per_env_step":
                          V * (4 + 2 + 2 + 4 + 1 + 3 * 8) + 4 * 8 * P + 19 * 16}),
          flush=True)
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
