"""Host restatement of VmEnv.step (vmenv/envs/env.py:66-103, 108-163, 244-293)
with the trace-fed _accept_vm_requests of include/vmp.h (vmp_set_trace), in
numpy, and the derivation of a trace from a recorded run of the C oracle.

TEST INFRASTRUCTURE ONLY: the checker the trace kernels are compared against
where no oracle run exists (generated traces), itself pinned against the C
oracle in tests/test_trace_cpu.py: the oracle's run is turned into the trace
it accepted, and the literal, fed that trace and the oracle's actions, must
reproduce the run.

Semantics restated (env.py line numbers):
  action phase  66-88    per VM in index order: validate (35-42), then place
                         (f64 `cpu + vm_cpu <= 1 and memory + vm_memory <= 1`)
                         or suspend
  _run_vms      244-268  running VMs with remaining > 0 decrement; those at 0
                         finish in index order and free their PM; loads < 1e-7
                         become 0
  accept        271-293  a = the trace's count for this step (0 past its end);
                         the k = min(a, #NULL) lowest NULL slots take the
                         step's first k requests; total += a, dropped += a - k;
                         the dropped requests are consumed
  stats, reward 112-156  waiting ratio, capped target means, wr / ut / kl
  termination   160-163  timestep >= training_steps (eval_steps in eval mode),
                         tested before the timestep advances (101)
"""
import numpy as np

STATE_KEYS = ("vm_placement", "vm_cpu", "vm_memory", "cpu", "memory", "vm_remaining_runtime")


def _kl(p_mean, p_var, q_mean, q_var):
    """-KL(N(p_mean, diag p_var) || N(q_mean, diag q_var)) as env.py:8-17 evaluates it."""
    p_cov, q_cov = np.diag(p_var), np.diag(q_var)
    q_inv = np.linalg.inv(q_cov)
    tr = np.trace(np.dot(q_inv, p_cov))
    d = p_mean - q_mean
    m1 = np.dot(np.dot(d.T, q_inv), d)
    return -0.5 * (np.log(np.linalg.det(q_cov) / np.linalg.det(p_cov)) - 2 + tr + m1 - tr)


class TraceEnv:
    """One env of `cfg` (a dict with the Config fields) replaying a trace given
    as (offs, cpu, mem, runtime) arrays."""

    def __init__(self, cfg, offs, cpu, mem, runtime):
        self.cfg = dict(cfg)
        self.P, self.V = int(cfg["pms"]), int(cfg["vms"])
        self.WAIT, self.NULL = self.P, self.P + 1
        self.offs = np.asarray(offs, np.int64)
        self.rq_cpu = np.asarray(cpu, np.int64)
        self.rq_mem = np.asarray(mem, np.int64)
        self.rq_rt = np.asarray(runtime, np.int64)
        self.eval_mode = False
        self.reset()

    def reset(self):
        P, V = self.P, self.V
        self.vm_placement = np.full(V, self.NULL, np.int64)
        self.vm_cpu, self.vm_memory = np.zeros(V), np.zeros(V)
        self.cpu, self.memory = np.zeros(P), np.zeros(P)
        self.vm_remaining_runtime = np.zeros(V, np.int64)
        self.timestep = 1
        self.total_requests = self.served = self.suspend_action = self.place_action = 0
        self.dropped = 0
        self.waiting_ratio = self.tcm = self.tmm = 0.0
        self.total_cpu_requested = self.total_memory_requested = 0.0
        return self.obs()

    def obs(self):
        return np.concatenate([self.vm_placement, self.vm_cpu, self.vm_memory, self.cpu,
                               self.memory], dtype=np.float32)

    def state(self):
        return tuple(getattr(self, k).copy() for k in STATE_KEYS)

    def counters(self):
        return np.array([self.total_requests, self.served, self.suspend_action, self.place_action,
                         self.dropped, self.timestep], np.int64)

    def stats(self):
        return np.array([self.waiting_ratio, self.tcm, self.tmm, self.total_cpu_requested,
                         self.total_memory_requested])

    def _valid(self, vm, cur, to):
        if cur == to:
            return True
        if cur == self.WAIT:
            return bool(to < self.WAIT and self.cpu[to] + self.vm_cpu[vm] <= 1
                        and self.memory[to] + self.vm_memory[vm] <= 1)
        if cur < self.WAIT:
            return to == self.WAIT
        return False

    def step(self, action):
        valid = np.zeros(self.V, np.uint8)
        for vm, to in enumerate(np.asarray(action, np.int64)):
            cur = self.vm_placement[vm]
            ok = self._valid(vm, cur, to)
            valid[vm] = ok
            if not ok or to == cur:
                continue
            self.vm_placement[vm] = to
            if to == self.WAIT:
                self.cpu[cur] -= self.vm_cpu[vm]
                self.memory[cur] -= self.vm_memory[vm]
                self.suspend_action += 1
            else:
                self.cpu[to] += self.vm_cpu[vm]
                self.memory[to] += self.vm_memory[vm]
                self.place_action += 1
        self._run()
        self._accept()
        reward = self._reward()
        limit = self.cfg["eval_steps"] if self.eval_mode else self.cfg["training_steps"]
        done = self.timestep >= limit
        self.timestep += 1
        return self.obs(), reward, bool(done), valid

    def _run(self):
        running = self.vm_placement < self.WAIT
        self.vm_remaining_runtime[running & (self.vm_remaining_runtime > 0)] -= 1
        fin = np.flatnonzero(running & (self.vm_remaining_runtime == 0))
        for vm in fin:
            pm = self.vm_placement[vm]
            self.cpu[pm] -= self.vm_cpu[vm]
            self.memory[pm] -= self.vm_memory[vm]
        self.vm_placement[fin] = self.NULL
        self.vm_cpu[fin] = 0
        self.vm_memory[fin] = 0
        self.served += fin.size
        self.cpu[self.cpu < 1e-7] = 0
        self.memory[self.memory < 1e-7] = 0

    def _accept(self):
        s, T = self.timestep - 1, self.offs.size - 1
        lo, hi = (int(self.offs[s]), int(self.offs[s + 1])) if s < T else (0, 0)
        a = hi - lo
        self.total_requests += a
        slots = np.flatnonzero(self.vm_placement == self.NULL)[:a]
        k = slots.size
        self.vm_placement[slots] = self.WAIT
        c = (self.rq_cpu[lo:lo + k] / 100.0).tolist()
        m = (self.rq_mem[lo:lo + k] / 100.0).tolist()
        self.total_cpu_requested += np.sum(c)
        self.total_memory_requested += np.sum(m)
        self.vm_cpu[slots] = c
        self.vm_memory[slots] = m
        self.vm_remaining_runtime[slots] = self.rq_rt[lo:lo + k]
        self.dropped += a - k

    def _reward(self):
        ex = self.vm_placement <= self.WAIT
        n_ex = np.count_nonzero(ex)
        n_w = np.count_nonzero(self.vm_placement == self.WAIT)
        self.waiting_ratio = n_w / n_ex if n_ex > 0 else 0
        cap = self.cfg.get("cap_target_util", True)
        self.tcm = np.sum(self.vm_cpu[ex]) / self.P
        self.tmm = np.sum(self.vm_memory[ex]) / self.P
        if cap and self.tcm > 1:
            self.tcm = 1.0
        if cap and self.tmm > 1:
            self.tmm = 1.0
        if n_ex == 0:
            return 0.0
        fn = self.cfg["reward_function"]
        if fn == "wr":
            return -self.waiting_ratio
        if fn == "ut":
            beta = self.cfg.get("beta", 0.5)
            return beta * np.sum(self.cpu) + (1 - beta) * np.sum(self.memory)
        assert fn == "kl", fn
        if self.tcm == 0 or self.tmm == 0:
            return 0.0
        q_var = np.array([np.var(self.cpu) or 1e-6, np.var(self.memory) or 1e-6])
        p_var = np.array([np.var(self.vm_cpu[ex]) or 1e-6, np.var(self.vm_memory[ex]) or 1e-6])
        return float(_kl(np.array([self.tcm, self.tmm]), p_var,
                         np.array([np.mean(self.cpu), np.mean(self.memory)]), q_var))


def derive_trace(P, pre_state, acts, valids, states, ctrs, filler=(1, 1, 1)):
    """The trace one oracle env accepted over a run, as (offs, cpu, mem, runtime).

    pre_state: the env's state() before the first recorded step; acts [T, V],
    valids [T, V], states[t] = state() after step t, ctrs [T, 6] = counters
    after step t. A slot is a new arrival of step t iff its post-step placement
    is WAIT and it did not stand at WAIT after the action phase (an unplaced
    waiting VM, or one suspended by a valid action): the device recorder's rule
    (k_record), with the oracle's validity flags. Accepted requests come in
    ascending slot order with the oracle's sizes (exact hundredths) and post-step
    remaining runtimes; the step's dropped requests follow them as `filler`
    (cpu, mem, runtime) requests, which no env ever reads."""
    WAIT = P
    offs, cpu, mem, rt = [0], [], [], []
    pre_pl = np.asarray(pre_state[0])
    req0 = 0
    for t in range(len(acts)):
        pl, vc, vm, _, _, rem = states[t]
        mid = np.where(np.asarray(valids[t]) != 0, np.asarray(acts[t]), pre_pl)
        new = np.flatnonzero((np.asarray(pl) == WAIT) & (mid != WAIT))
        c100, m100 = np.rint(vc[new] * 100), np.rint(vm[new] * 100)
        assert np.array_equal(c100 / 100.0, vc[new]) and np.array_equal(m100 / 100.0, vm[new])
        total = int(ctrs[t][0]) - req0
        req0 = int(ctrs[t][0])
        assert total >= new.size, (t, total, new.size)
        n_fill = total - new.size
        cpu += c100.astype(np.int64).tolist() + [filler[0]] * n_fill
        mem += m100.astype(np.int64).tolist() + [filler[1]] * n_fill
        rt += np.asarray(rem)[new].astype(np.int64).tolist() + [filler[2]] * n_fill
        offs.append(offs[-1] + total)
        pre_pl = np.asarray(pl)
    return (np.asarray(offs, np.int64), np.asarray(cpu, np.uint8), np.asarray(mem, np.uint8),
            np.asarray(rt, np.uint32))
