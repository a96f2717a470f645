"""Truth model of vmp_set_state (include/vmp.h), in plain numpy and Python loops.

TEST INFRASTRUCTURE ONLY. A state of ONE env is a dict with the keys of
BatchedVmEnv.state() (vm_placement, vm_cpu, vm_memory, vm_remaining_runtime;
cpu / memory optional) plus, optionally, "counters" int64 [6] (timestep last)
and "totals" f64 [2].

  validate(state, P, timestep)  the VMP_SS_* code the device must report: the
                                rules walked in their numbered order, slot by
                                slot, the first one that fails
  pack(state, P, V, timestep)   the bytes a valid state must leave: slot and time
                                words of slots 0..V-1 with their positions in the
                                env's VM row, the PM row, the header fields
  into_trace_env(env, state)    the same state put into tests/trace_literal.py's
                                TraceEnv through its attributes
  random_state(...)             valid random states for the tests

Header words written (csrc/vmp_layout.h EnvHdr, u64 index): timestep 20,
total_requests 21, served 22, suspend 23, place 24, dropped 25, total cpu / mem
requested 26 / 27 (f64), waiting_ratio 28 (f64), the hint word 31."""
import numpy as np

SKIPPED, IMPORTED = 0, 1
PLACEMENT, NULL_SLOT, VM_SIZE, RUNTIME, TIMESTEP, COUNTER = 2, 3, 4, 5, 6, 7
CAPACITY, LOAD_FLOOR, LOAD_MAX, LOAD_SUM = 8, 9, 10, 11
CODES = {"SKIPPED": 0, "IMPORTED": 1, "PLACEMENT": 2, "NULL_SLOT": 3, "VM_SIZE": 4, "RUNTIME": 5,
         "TIMESTEP": 6, "COUNTER": 7, "CAPACITY": 8, "LOAD_FLOOR": 9, "LOAD_MAX": 10,
         "LOAD_SUM": 11}
W_TIMESTEP, W_TOTAL, W_CPU_REQ, W_MEM_REQ, W_WAITING, W_PAD = 20, 21, 26, 27, 28, 31


_SIZES = {float(np.float64(k) / np.float64(100.0)): k for k in range(1, 101)}


def _k(x):
    """k if x is float(k) / 100.0 for k in 1..100 (all positive: equal values are
    equal bits), else 0."""
    return _SIZES.get(float(x), 0)


def _sums(state, P):
    pl = np.asarray(state["vm_placement"])
    s = [0] * (2 * P)
    for v in range(pl.size):
        q = int(pl[v])
        if 0 <= q < P:
            s[q] += _k(state["vm_cpu"][v])
            s[P + q] += _k(state["vm_memory"][v])
    return s


def timestep_of(state, timestep):
    return int(state["counters"][5]) if state.get("counters") is not None else int(timestep)


def validate(state, P, timestep=1):
    """timestep: the env's own, used when the state brings no counters."""
    pl = np.asarray(state["vm_placement"])
    vc, vm = np.asarray(state["vm_cpu"]), np.asarray(state["vm_memory"])
    rem = np.asarray(state["vm_remaining_runtime"])
    V = pl.size
    if any(not 0 <= int(pl[v]) <= P + 1 for v in range(V)):
        return PLACEMENT
    ex = [v for v in range(V) if int(pl[v]) <= P]
    if any(not (vc[v] == 0 and vm[v] == 0 and rem[v] == 0) for v in range(V) if int(pl[v]) == P + 1):
        return NULL_SLOT
    if any(_k(vc[v]) == 0 or _k(vm[v]) == 0 for v in ex):
        return VM_SIZE
    if any(not 1 <= int(rem[v]) <= 1 << 30 for v in ex):
        return RUNTIME
    if not 1 <= timestep_of(state, timestep) < 1 << 31:
        return TIMESTEP
    if state.get("counters") is not None and any(int(c) < 0 for c in state["counters"][:5]):
        return COUNTER
    s = _sums(state, P)
    if any(x > 100 for x in s):
        return CAPACITY
    if state.get("cpu") is not None:
        x = [float(a) for a in state["cpu"]] + [float(a) for a in state["memory"]]
        if any(not (a == 0 or a >= 1e-7) for a in x):
            return LOAD_FLOOR
        if any(not a <= 1.0 for a in x):
            return LOAD_MAX
        if any(not abs(a - np.float64(k) / np.float64(100.0)) < 1e-7 for a, k in zip(x, s)):
            return LOAD_SUM
    return IMPORTED


def pitch(V):
    b = (V + 63) >> 6
    if V <= 1024:
        q = 1
        while q < b:
            q <<= 1
        b = q
    return b << 7


def pack(state, P, V, timestep=1):
    """-> dict(slot_at, time_at: positions int [V] in the env's u32 VM row; slot,
    time: u32 [V]; pm: f64 [2 P]; counters: int64 [6] or None (kept); totals:
    f64 [2] or None (kept); waiting_ratio: f64; pad: 0)."""
    assert validate(state, P, timestep) == IMPORTED
    ts = timestep_of(state, timestep)
    pl = np.asarray(state["vm_placement"])
    v = np.arange(V)
    slot_at = ((v >> 6) << 7) | (v & 63)
    slot, time = np.zeros(V, np.uint32), np.zeros(V, np.uint32)
    for i in range(V):
        q = int(pl[i])
        if q == P + 1:
            slot[i] = q
            continue
        slot[i] = q | _k(state["vm_cpu"][i]) << 16 | _k(state["vm_memory"][i]) << 24
        rem = int(state["vm_remaining_runtime"][i])
        time[i] = ts + rem if q < P else rem
    if state.get("cpu") is not None:
        pm = np.concatenate([np.asarray(state["cpu"], np.float64),
                             np.asarray(state["memory"], np.float64)])
    else:
        pm = np.array([np.float64(k) / np.float64(100.0) for k in _sums(state, P)], np.float64)
    n_w, n_ex = int(np.count_nonzero(pl == P)), int(np.count_nonzero(pl <= P))
    ctr = state.get("counters")
    tot = state.get("totals")
    return dict(slot_at=slot_at, time_at=slot_at | 64, slot=slot, time=time, pm=pm,
                counters=None if ctr is None else np.asarray(ctr, np.int64),
                totals=None if tot is None else np.asarray(tot, np.float64),
                waiting_ratio=np.float64(n_w) / np.float64(n_ex) if n_ex else np.float64(0.0),
                pad=0)


def into_trace_env(env, state):
    """Make a tests.trace_literal.TraceEnv stand in `state` (loads not given:
    the sums of the running VMs' hundredths over 100)."""
    P = env.P
    env.vm_placement = np.asarray(state["vm_placement"], np.int64).copy()
    env.vm_cpu = np.asarray(state["vm_cpu"], np.float64).copy()
    env.vm_memory = np.asarray(state["vm_memory"], np.float64).copy()
    env.vm_remaining_runtime = np.asarray(state["vm_remaining_runtime"], np.int64).copy()
    if state.get("cpu") is not None:
        env.cpu = np.asarray(state["cpu"], np.float64).copy()
        env.memory = np.asarray(state["memory"], np.float64).copy()
    else:
        s = _sums(state, P)
        env.cpu = np.array([np.float64(k) / np.float64(100.0) for k in s[:P]])
        env.memory = np.array([np.float64(k) / np.float64(100.0) for k in s[P:]])
    if state.get("counters") is not None:
        c = [int(x) for x in state["counters"]]
        (env.total_requests, env.served, env.suspend_action, env.place_action, env.dropped,
         env.timestep) = c
    if state.get("totals") is not None:
        env.total_cpu_requested = float(state["totals"][0])
        env.total_memory_requested = float(state["totals"][1])
    pl = env.vm_placement
    n_ex = np.count_nonzero(pl <= P)
    env.waiting_ratio = np.count_nonzero(pl == P) / n_ex if n_ex else 0
    return env


def random_state(g, P, V, fill=0.7, wait=0.3, loads=False, counters=True, max_rt=50):
    """A valid state: each slot exists with probability `fill`; an existing VM
    waits with probability `wait`, else it runs on a random PM that still has
    room for it (and waits if the PM it drew has none). loads: also cpu /
    memory, the exact sums disturbed by less than 1e-7 as a run's rounding
    history would (never into (0, 1e-7) and never above 1)."""
    pl = np.full(V, P + 1, np.int64)
    vc, vm = np.zeros(V), np.zeros(V)
    rem = np.zeros(V, np.int64)
    s = [0] * (2 * P)
    for v in range(V):
        if g.random() >= fill:
            continue
        kc, km = int(g.integers(1, 101)), int(g.integers(1, 101))
        vc[v], vm[v] = np.float64(kc) / 100.0, np.float64(km) / 100.0
        rem[v] = int(g.integers(1, max_rt + 1))
        q = int(g.integers(0, P))
        if g.random() >= wait and s[q] + kc <= 100 and s[P + q] + km <= 100:
            pl[v] = q
            s[q] += kc
            s[P + q] += km
        else:
            pl[v] = P
    st = dict(vm_placement=pl, vm_cpu=vc, vm_memory=vm, vm_remaining_runtime=rem)
    if loads:
        x = np.array(s, np.float64) / 100.0
        d = g.uniform(-4e-8, 4e-8, 2 * P) * (g.random(2 * P) < 0.5)
        x = np.where(np.array(s) > 0, np.minimum(x + d, 1.0), 0.0)
        st["cpu"], st["memory"] = x[:P].copy(), x[P:].copy()
    if counters:
        c = g.integers(0, 1000, 6)
        c[5] = int(g.integers(1, 5000))
        st["counters"] = c.astype(np.int64)
        st["totals"] = g.uniform(0, 500, 2)
    return st


def stack(states, keys=("vm_placement", "vm_cpu", "vm_memory", "vm_remaining_runtime", "cpu",
                        "memory", "counters", "totals")):
    """Per-env dicts -> one dict of [n, ...] arrays (a key absent from all is left out)."""
    out = {}
    for k in keys:
        if all(s.get(k) is None for s in states):
            continue
        out[k] = np.stack([np.asarray(s[k]) for s in states])
    return out
