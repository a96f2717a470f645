"""Request traces for trace-driven workloads (BatchedVmEnv.set_trace,
vmp_set_trace in include/vmp.h).

A `Trace` is T steps of VM requests: `offs` int64 [T + 1] (offs[0] = 0,
non-decreasing) and, per request, `cpu` and `mem` (uint8 hundredths, 1..100)
and `runtime` (uint32, 1..2**30). The requests of step index s are
[offs[s], offs[s+1]), in order; a traced env offers them in the step it runs
at timestep s + 1 (reset leaves timestep 1) and none from step T on.

A request that finds no NULL slot is dropped AND consumed: it is never offered
again. (The draw-based env draws a size and a runtime per accepted VM, so there
a drop consumes no draw and two policies at one seed soon face different
requests; a trace is the same request sequence whatever the policy does.)
"""
import numpy as np

MAX_RUNTIME = 1 << 30
MAX_REQUESTS = (1 << 31) - 1

SEQUENCE_RANGE = {"uniform": (0.1, 1.0), "lowuniform": (0.1, 0.65), "highuniform": (0.25, 1.0)}


class Trace:
    def __init__(self, offs, cpu, mem, runtime):
        offs = np.asarray(offs)
        cpu, mem, runtime = np.asarray(cpu), np.asarray(mem), np.asarray(runtime)
        if offs.ndim != 1 or offs.size < 1 or cpu.ndim != 1 or mem.ndim != 1 or runtime.ndim != 1:
            raise ValueError("offs must be int64 [T + 1]; cpu, mem, runtime one-dimensional")
        for name, a in (("offs", offs), ("cpu", cpu), ("mem", mem), ("runtime", runtime)):
            if a.size and not np.issubdtype(a.dtype, np.integer):
                raise ValueError(f"{name} must be integers")
        if offs[0] != 0:
            raise ValueError("offs[0] must be 0")
        if np.any(np.diff(offs.astype(np.int64)) < 0):
            raise ValueError("offs must be non-decreasing")
        n = int(offs[-1])
        if n > MAX_REQUESTS:
            raise ValueError("a trace holds at most 2**31 - 1 requests")
        if not (cpu.size == mem.size == runtime.size == n):
            raise ValueError(f"cpu, mem and runtime must hold offs[-1] = {n} requests")
        if n and (cpu.min() < 1 or cpu.max() > 100 or mem.min() < 1 or mem.max() > 100):
            raise ValueError("sizes are hundredths in 1..100")
        if n and (runtime.min() < 1 or runtime.max() > MAX_RUNTIME):
            raise ValueError("runtimes must be in 1..2**30")
        self.offs = np.ascontiguousarray(offs, dtype=np.int64)
        self.cpu = np.ascontiguousarray(cpu, dtype=np.uint8)
        self.mem = np.ascontiguousarray(mem, dtype=np.uint8)
        self.runtime = np.ascontiguousarray(runtime, dtype=np.uint32)
        for a in (self.offs, self.cpu, self.mem, self.runtime):
            a.setflags(write=False)

    @property
    def steps(self):
        return self.offs.size - 1

    @property
    def requests(self):
        return int(self.offs[-1])

    def arrivals(self):
        """Requests per step, int64 [T]."""
        return np.diff(self.offs)

    def __eq__(self, other):
        return isinstance(other, Trace) and all(
            np.array_equal(getattr(self, k), getattr(other, k))
            for k in ("offs", "cpu", "mem", "runtime"))

    def __repr__(self):
        return f"Trace(steps={self.steps}, requests={self.requests})"

    @classmethod
    def from_requests(cls, arrival_step, cpu, mem, runtime, steps=None):
        """One request per entry, arriving at step index arrival_step[i] >= 0.
        Requests of one step keep their order in the arguments (a stable sort
        by step). `steps`: the trace's length (default: last arrival + 1)."""
        a = np.asarray(arrival_step)
        if a.ndim != 1 or (a.size and not np.issubdtype(a.dtype, np.integer)):
            raise ValueError("arrival_step must be one-dimensional integers")
        a = a.astype(np.int64)
        if a.size and a.min() < 0:
            raise ValueError("arrival_step must be >= 0")
        T = int(a.max()) + 1 if a.size else 0
        if steps is not None:
            if steps < T:
                raise ValueError("steps is smaller than the last arrival step + 1")
            T = int(steps)
        order = np.argsort(a, kind="stable")
        offs = np.zeros(T + 1, np.int64)
        np.cumsum(np.bincount(a, minlength=T), out=offs[1:])
        return cls(offs, np.asarray(cpu)[order], np.asarray(mem)[order], np.asarray(runtime)[order])

    def save(self, path):
        """One .npz with the four arrays."""
        with open(path, "wb") as f:
            np.savez(f, offs=self.offs, cpu=self.cpu, mem=self.mem, runtime=self.runtime)

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            return cls(z["offs"], z["cpu"], z["mem"], z["runtime"])

    @classmethod
    def synthetic(cls, config, steps, seed):
        """The config's own workload as data, independent of any policy, drawn
        from ONE generator np.random.default_rng(seed) in this order:
          1. arrivals  = rng.poisson(config.arrival_rate, size=steps)
          2. cpu       = around(rng.uniform(lo, hi, size=n), 2)   n = arrivals.sum()
          3. mem       = around(rng.uniform(lo, hi, size=n), 2)
          4. runtime   = rng.poisson(config.service_length, size=n) + 1
        with (lo, hi) the range of config.sequence (env.py:211-219). Sizes are
        stored in hundredths; runtimes are capped at 2**30."""
        lo, hi = SEQUENCE_RANGE[config.sequence]
        rng = np.random.default_rng(seed)
        arrivals = rng.poisson(config.arrival_rate, size=int(steps)).astype(np.int64)
        n = int(arrivals.sum())
        cpu = np.rint(np.around(rng.uniform(lo, hi, size=n), 2) * 100).astype(np.int64)
        mem = np.rint(np.around(rng.uniform(lo, hi, size=n), 2) * 100).astype(np.int64)
        runtime = np.minimum(rng.poisson(config.service_length, size=n).astype(np.int64) + 1,
                             MAX_RUNTIME)
        offs = np.zeros(int(steps) + 1, np.int64)
        np.cumsum(arrivals, out=offs[1:])
        return cls(offs, cpu, mem, runtime)
