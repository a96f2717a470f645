"""bench.py without --full: the result line holds the headline alone, --steps
sets the number of timed launches, and --dump-outputs holds what the last
timed launch returned."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# every key of a plain result line; a leg that --full adds is not among them
PLAIN_KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
              "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline",
              "full"}


def test_plain_run_is_headline_only_and_dumps_last_step(tmp_path):
    """The same envs stepped here (fast_forward, then warmup + steps launches)
    give the dumped obs / reward / done bit for bit: exactly warmup + steps
    launches preceded the dump, and no other leg stepped the envs before it."""
    import bench
    from vmp.batched import BatchedVmEnv
    from vmp.config import Config
    from vmp.replicas import shard_seeds

    N, K, W = 256, 3, 2
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--envs", str(N), "--steps",
                        str(K), "--warmup", str(W), "--ff-steps", "300", "--phase-delta", "10",
                        "--rollout-k", "20", "--dump-outputs", str(out)], cwd=ROOT,
                       env={k: v for k, v in os.environ.items() if k != "VMP_BENCH_FULL"},
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    d = json.loads(lines[0])
    assert set(d) == PLAIN_KEYS
    assert d["steps"] == K and d["warmup"] == W and d["full"] is False
    assert d["unit"] == "env-steps/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["ms_per_step"] > 0
    assert abs(d["value"] - N * 1e3 / d["ms_per_step"]) <= 1e-9 * d["value"]

    got = {p.stem: np.load(p) for p in out.iterdir()}
    assert sorted(got) == ["done", "obs", "obs_rows", "reward"]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 * 10**6

    seeds = shard_seeds(0, N)
    env = BatchedVmEnv(Config(**bench.CFG), N, seeds=seeds, device="cuda:0")
    env.eval(False)
    bench.fast_forward(env, "firstfit", seeds, 300, 10, 10, 20)
    for _ in range(W + K):
        obs, rew, done, _, _ = env.heuristic_step("firstfit")
    assert np.array_equal(got["obs_rows"], np.arange(N))  # 256 rows fit the sample budget
    assert np.array_equal(got["obs"], obs.cpu().numpy())
    assert np.array_equal(got["reward"], rew.cpu().numpy())
    assert np.array_equal(got["done"], done.cpu().numpy().astype(np.float32))
    env.close()
