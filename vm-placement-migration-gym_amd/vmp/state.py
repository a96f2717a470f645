"""Env states as plain arrays: the container `BatchedVmEnv.set_state` takes
its input from, a file format that outlives library versions (`.npz`, no
pickles), and the rules of vmp_set_state (include/vmp.h VMP_SS_*) restated on
the host, so a state can be checked before it goes to a device.

A State holds n envs of one shape: vm_placement / vm_remaining_runtime int64
[n, V], vm_cpu / vm_memory f64 [n, V], optionally cpu / memory f64 [n, P] (the
PM loads with their rounding history; without them the device derives the
loads from the running VMs), optionally counters int64 [n, 6] (total_requests,
served, suspend, place, dropped, timestep) and totals f64 [n, 2] (total cpu /
memory requested). `pms` is P: placement P is WAIT, P + 1 an empty slot."""
import numpy as np

SKIPPED, IMPORTED = 0, 1
PLACEMENT, NULL_SLOT, VM_SIZE, RUNTIME, TIMESTEP, COUNTER = 2, 3, 4, 5, 6, 7
CAPACITY, LOAD_FLOOR, LOAD_MAX, LOAD_SUM = 8, 9, 10, 11
RULES = {
    SKIPPED: "not selected",
    IMPORTED: "imported",
    PLACEMENT: "a placement outside [0, pms + 1]",
    NULL_SLOT: "an empty slot with a size or a remaining runtime",
    VM_SIZE: "a VM size that is not k / 100 for k in 1..100",
    RUNTIME: "a VM with a remaining runtime outside [1, 2^30]",
    TIMESTEP: "a timestep outside [1, 2^31)",
    COUNTER: "a negative counter",
    CAPACITY: "a PM whose running VMs exceed its cpu or memory",
    LOAD_FLOOR: "a PM load that is neither 0 nor >= 1e-7",
    LOAD_MAX: "a PM load above 1",
    LOAD_SUM: "a PM load that differs from its running VMs' sum by 1e-7 or more",
}
MAX_RUNTIME = 1 << 30
VM_KEYS = ("vm_placement", "vm_cpu", "vm_memory", "vm_remaining_runtime")
_DTYPES = dict(vm_placement=np.int64, vm_cpu=np.float64, vm_memory=np.float64,
               vm_remaining_runtime=np.int64, cpu=np.float64, memory=np.float64,
               counters=np.int64, totals=np.float64)


def hundredths(x):
    """k where x is bitwise float64(k) / 100.0 for an integer k in 1..100, else 0."""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        ok = (x > 0.0) & (x <= 1.0)
        k = np.where(ok, np.floor(np.where(ok, x, 0.0) * 100.0 + 0.5), 0.0)
        same = (k / 100.0).view(np.int64) == x.view(np.int64)
    return np.where(ok & same & (k >= 1) & (k <= 100), k, 0).astype(np.int64)


class State:
    def __init__(self, pms, vm_placement, vm_cpu, vm_memory, vm_remaining_runtime, cpu=None,
                 memory=None, counters=None, totals=None):
        self.pms = int(pms)
        given = dict(vm_placement=vm_placement, vm_cpu=vm_cpu, vm_memory=vm_memory,
                     vm_remaining_runtime=vm_remaining_runtime, cpu=cpu, memory=memory,
                     counters=counters, totals=totals)
        if (cpu is None) != (memory is None):
            raise ValueError("cpu and memory are both given or both absent")
        for k, v in given.items():
            if v is not None:
                v = np.asarray(v)
                if v.dtype.kind not in "iufb":
                    raise ValueError(f"{k} must be numeric")
                v = np.ascontiguousarray(v, _DTYPES[k])
                v = v[None] if v.ndim == 1 else v
            setattr(self, k, v)
        n, V = self.vm_placement.shape
        want = dict(vm_placement=(n, V), vm_cpu=(n, V), vm_memory=(n, V),
                    vm_remaining_runtime=(n, V), cpu=(n, self.pms), memory=(n, self.pms),
                    counters=(n, 6), totals=(n, 2))
        for k, shape in want.items():
            v = getattr(self, k)
            if v is not None and v.shape != shape:
                raise ValueError(f"{k} must have shape {shape}, not {v.shape}")

    n_envs = property(lambda self: self.vm_placement.shape[0])
    vms = property(lambda self: self.vm_placement.shape[1])

    # ------------------------------------------------------------ sources
    @classmethod
    def of(cls, env):
        """The current state of a BatchedVmEnv (every env) or a VmEnv, PM loads,
        counters and totals included."""
        b = getattr(env, "_b", env)
        st = {k: v.cpu().numpy() for k, v in b.state().items()}
        return cls(b.P, counters=b.counters().cpu().numpy(),
                   totals=b.stats()[:, 3:5].cpu().numpy(), **st)

    @classmethod
    def from_reference(cls, ref_env):
        """The state of a reference-style VmEnv object (vmenv/envs/env.py), read
        from its attributes: the arrays, the counters and the requested totals."""
        r = ref_env
        ctr = [r.total_requests, r.served_requests, r.suspend_action, r.place_action,
               r.dropped_requests, r.timestep]
        return cls(int(r.config.pms), r.vm_placement, r.vm_cpu, r.vm_memory,
                   r.vm_remaining_runtime, cpu=r.cpu, memory=r.memory,
                   counters=np.asarray(ctr, np.int64),
                   totals=np.asarray([r.total_cpu_requested, r.total_memory_requested],
                                     np.float64))

    # --------------------------------------------------------------- file
    def save(self, path):
        """Write the state as .npz: plain arrays, readable without this library."""
        arrs = {k: getattr(self, k) for k in _DTYPES if getattr(self, k) is not None}
        with open(path, "wb") as f:
            np.savez(f, pms=np.int64(self.pms), **arrs)

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            if "pms" not in z.files or any(k not in z.files for k in VM_KEYS):
                raise ValueError(f"{path} is not a saved State")
            return cls(int(z["pms"]), **{k: z[k] for k in _DTYPES if k in z.files})

    # ---------------------------------------------------------------- use
    def broadcast(self, n):
        """A one-env state repeated for n envs (a state of n envs is returned as it is)."""
        if self.n_envs == n:
            return self
        if self.n_envs != 1:
            raise ValueError(f"a state of {self.n_envs} envs cannot serve {n} envs")
        rep = {k: None if getattr(self, k) is None else np.repeat(getattr(self, k), n, axis=0)
               for k in _DTYPES}
        return State(self.pms, **rep)

    def as_dict(self):
        """The dict `BatchedVmEnv.set_state` takes (and `state()` returns)."""
        d = {k: getattr(self, k) for k in VM_KEYS}
        if self.cpu is not None:
            d["cpu"], d["memory"] = self.cpu, self.memory
        return d

    def apply(self, env, mask=None, seeds=None, check=True):
        """set_state on a BatchedVmEnv or a VmEnv with everything the state holds."""
        b = getattr(env, "_b", env)
        s = self.broadcast(b.n_envs)
        return b.set_state(s.as_dict(), mask=mask, counters=s.counters, totals=s.totals,
                           seeds=seeds, check=check)

    def validate(self, timestep=None):
        """vmp_set_state's verdict per env, int64 [n]: IMPORTED, or the lowest
        failing rule. timestep: the envs' current timesteps (scalar or [n]),
        needed for that rule only when the state has no counters; None skips it."""
        n, P = self.n_envs, self.pms
        none = np.iinfo(np.int64).max
        code = np.full(n, none, np.int64)

        def fail(envs, c):
            code[envs & (code > c)] = c

        pl, rem = self.vm_placement, self.vm_remaining_runtime
        inside = (pl >= 0) & (pl <= P + 1)
        fail(~inside.all(axis=1), PLACEMENT)
        null, ex = inside & (pl == P + 1), inside & (pl <= P)
        empty = (self.vm_cpu == 0) & (self.vm_memory == 0) & (rem == 0)
        fail((null & ~empty).any(axis=1), NULL_SLOT)
        kc, km = hundredths(self.vm_cpu), hundredths(self.vm_memory)
        sized = (kc > 0) & (km > 0)
        fail((ex & ~sized).any(axis=1), VM_SIZE)
        timed = (rem >= 1) & (rem <= MAX_RUNTIME)
        fail((ex & sized & ~timed).any(axis=1), RUNTIME)
        ts = None
        if self.counters is not None:
            ts = self.counters[:, 5]
            fail((self.counters[:, :5] < 0).any(axis=1), COUNTER)
        elif timestep is not None:
            ts = np.broadcast_to(np.asarray(timestep, np.int64), (n,))
        if ts is not None:
            fail((ts < 1) | (ts >= 1 << 31), TIMESTEP)
        run = ex & sized & timed & (pl < P)
        for e in range(n):
            q = pl[e][run[e]]
            sc = np.bincount(q, weights=kc[e][run[e]], minlength=P).astype(np.int64)
            sm = np.bincount(q, weights=km[e][run[e]], minlength=P).astype(np.int64)
            s = np.concatenate([sc, sm])
            if (s > 100).any():
                fail(np.arange(n) == e, CAPACITY)
            if self.cpu is None:
                continue
            x = np.concatenate([self.cpu[e], self.memory[e]])
            with np.errstate(invalid="ignore"):
                cap = s <= 100
                floor = (x == 0) | (x >= 1e-7)
                top = x <= 1.0
                near = np.abs(x - s / 100.0) < 1e-7
            me = np.arange(n) == e
            if (cap & ~floor).any():
                fail(me, LOAD_FLOOR)
            if (cap & floor & ~top).any():
                fail(me, LOAD_MAX)
            if (cap & floor & top & ~near).any():
                fail(me, LOAD_SUM)
        code[code == none] = IMPORTED
        return code
