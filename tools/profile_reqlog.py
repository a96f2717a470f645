"""The request log's kernel beside the recorder's, for a kernel trace.

    rocprofv3 --kernel-trace --stats -f csv -d OUT -o reqlog -- \
        python tools/profile_reqlog.py [--envs 4096] [--steps 1500]

P100 / V1000 (bench.py's CFG), every env replaying Trace.synthetic of that
config, FirstFit act + step with the recorder AND the request log on, so one
step is three launches: the env kernel, k_record, k_reqlog. The per-launch
times of the two observers are read from the trace's kernel statistics; this
script times nothing itself. It prints the bytes per env-step that k_reqlog
moves by its layout, and checks the log's counter identities at the end.
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
    N, V = a.envs, cfg.vms
    trace = Trace.synthetic(cfg, a.steps, 0)
    env = BatchedVmEnv(cfg, N, seeds=4 * np.arange(N, dtype=np.int64), device=dev)
    env.set_trace(trace)
    env.eval(True)
    env.reset()
    env.record(True)
    env.request_log()
    obs = torch.empty((N, env.D), dtype=torch.float32, device=dev)
    rew = torch.empty((N,), dtype=torch.float64, device=dev)
    done = torch.empty((N,), dtype=torch.uint8, device=dev)
    for _ in range(a.steps):
        env.heuristic_step("firstfit", obs=obs, reward=rew, done=done)
    torch.cuda.synchronize(dev)
    lg = env.request_log_read()
    ctr = env.counters().cpu().numpy()
    total, served, susp, dropped = ctr[0, 0], ctr[0, 1], ctr[0, 2], ctr[0, 4]
    ok = bool(np.all(ctr == ctr[0]) and np.all(lg.rows == lg.rows[0])
              and np.count_nonzero(lg.slot[0] >= 0) == total - dropped
              and np.count_nonzero(lg.slot[0] == -1) == dropped
              and np.count_nonzero(lg.finished[0] > 0) == served
              and int(lg.suspends[0].sum()) == susp and total == trace.requests)
    env.close()
    # per slot: slot word 4 B, prev 2 B read + 2 B written, id 4 B read + 4 B written, action
    # 4 B, validity 1 B; per env: timestep + total_requests 16 B, meta 8 B read + 16 B written;
    # per event one 24-B row, read and written
    fixed = V * (4 + 2 + 2 + 4 + 4 + 4 + 1) + 16 + 24
    # row touches: arrivals and drops, valid placements, finishes, suspensions (waiting steps
    # are not: WAIT_STEPS is written at events only and closed in the read)
    events = float(total + ctr[0, 3] + served + susp) / a.steps
    print(json.dumps({"envs": N, "V": V, "steps": a.steps, "requests_per_env": int(total),
                      "dropped_per_env": int(dropped), "served_per_env": int(served),
                      "identities_hold": ok,
                      "k_reqlog_streamed_bytes_per_env_step": fixed,
                      "k_reqlog_row_events_per_env_step": events,
                      "k_record_streamed_bytes_per_env_step":
                          V * (4 + 2 + 2 + 4 + 1 + 3 * 8) + 4 * 8 * cfg.pms + 19 * 16}),
          flush=True)
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
