"""BatchedVmEnv: N independent reference `VmEnv` instances resident on one
MI355X, stepped by libvmp.so kernels. Tensors in and out are torch tensors on
the env's device; nothing round-trips through the host on the step path.

Reference surface mapped per env (vmenv/envs/env.py):
  reset(seed)                    -> reset(seeds, mask)            env.py:180-226
  step(action)                   -> step(actions)                 env.py:66-103
  get_invalid_action_mask(True)  -> mask() / mask_bits()          env.py:45-53
  FirstFitAgent/BestFitAgent.act -> heuristic_act(policy)         firstfit.py:21, bestfit.py:21
Seeds default to config.seed + seed_stride*i (stride 4 keeps the four
per-env PCG64 streams seed+0..3 of different envs disjoint, env.py:175-178).
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import VmpError, check, lib, ptr
from .config import Config

N_COUNTERS = 6  # total_requests, served, suspend, place, dropped, timestep
N_STATS = 5     # waiting_ratio, target_cpu_mean, target_mem_mean, total_cpu_req, total_mem_req
N_REC = 19      # VMP_NREC: recorder sums (include/vmp.h VMP_REC_*)
REC_BINS = 1001


class BatchedVmEnv:
    def __init__(self, config: Config, n_envs: int, seeds=None, device="cuda", seed_stride=4,
                 arrival_rate=None, service_length=None):
        if not torch.cuda.is_available():
            raise VmpError("BatchedVmEnv needs a HIP device (MI355X); no CPU fallback exists")
        self.config = config
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.n_envs = int(n_envs)
        if seeds is None:
            seeds = int(config.seed) + int(seed_stride) * np.arange(self.n_envs, dtype=np.int64)
        seeds = np.ascontiguousarray(np.asarray(seeds, dtype=np.int64))
        if seeds.shape != (self.n_envs,):
            raise ValueError("seeds must have shape (n_envs,)")
        self._ccfg = _lib.to_c_config(config)
        self.P, self.V = int(config.pms), int(config.vms)
        self.A = self.P + 2 if config.allow_null_action else self.P + 1
        self.D = 3 * self.V + 2 * self.P
        self.W = (self.A + 31) // 32
        self.WAIT_STATUS, self.NULL_STATUS = self.P, self.P + 1
        self.eval_mode = False
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            check(lib().vmp_create(ctypes.byref(self._ccfg), self.n_envs,
                                   seeds.ctypes.data_as(ctypes.c_void_p), self.device.index,
                                   ctypes.byref(h)))
        self._h = h
        self._traces = None
        self._start = None  # set_start_state: what reset() leaves instead of an empty env
        if arrival_rate is not None or service_length is not None:
            try:
                self.set_workload(arrival_rate, service_length)
            except Exception:
                self.close()
                raise

    # ------------------------------------------------------------ plumbing
    def _bind(self):
        if self._h is None:
            raise VmpError("env is closed")
        s = torch.cuda.current_stream(self.device).cuda_stream
        check(lib().vmp_set_stream(self._h, ctypes.c_void_p(s)))
        return self._h

    def _empty(self, shape, dtype):
        return torch.empty(shape, dtype=dtype, device=self.device)

    def close(self):
        if getattr(self, "_h", None) is not None:
            torch.cuda.synchronize(self.device)
            lib().vmp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------- API
    def eval(self, mode=True):
        """VmEnv.eval (env.py:105-106): switches the termination limit to eval_steps."""
        self.eval_mode = bool(mode)
        check(lib().vmp_set_eval(self._bind(), int(self.eval_mode)))

    def _per_env(self, x, name):
        if x is None:
            return None
        if isinstance(x, torch.Tensor):
            x = x.detach().cpu().numpy()
        a = np.asarray(x, dtype=np.float64)
        if a.ndim == 0:
            a = np.full(self.n_envs, float(a))
        if a.shape != (self.n_envs,):
            raise ValueError(f"{name} must be a scalar or have n_envs = {self.n_envs} entries")
        return np.ascontiguousarray(a)

    def set_workload(self, arrival_rate=None, service_length=None):
        """Per-env workload (vmp_set_workload): env i draws its arrivals from
        Poisson(arrival_rate[i]) and its planned runtimes from
        Poisson(service_length[i]) + 1 from its next step on. Scalars or
        array-likes of n_envs; None keeps that quantity. A graph captured before
        the first call must be recaptured; later calls keep graphs valid."""
        h = self._bind()
        a = self._per_env(arrival_rate, "arrival_rate")
        s = self._per_env(service_length, "service_length")
        pa = None if a is None else a.ctypes.data_as(ctypes.c_void_p)
        ps = None if s is None else s.ctypes.data_as(ctypes.c_void_p)
        with torch.cuda.device(self.device):
            check(lib().vmp_set_workload(h, pa, ps))

    def workload(self):
        """(arrival_rate, service_length) of every env as numpy f64 [n_envs]
        (the config's values for an env never given a workload)."""
        a, s = np.empty(self.n_envs, np.float64), np.empty(self.n_envs, np.float64)
        check(lib().vmp_get_workload(self._bind(), a.ctypes.data_as(ctypes.c_void_p),
                                     s.ctypes.data_as(ctypes.c_void_p)))
        return a, s

    def set_trace(self, traces, trace_of_env=None):
        """Trace-driven workload (vmp_set_trace): env i replays
        traces[trace_of_env[i]] (a `vmp.trace.Trace`, or a list of them; None
        maps every env to trace 0) instead of drawing its requests: the step at
        timestep s + 1 is offered the requests of the trace's step s, none once
        the trace is over, and a dropped request is consumed (see vmp.trace).
        The RNG streams rest; reset() rewinds every env to step 0 of its trace.
        A graph captured before the first call must be recaptured; later calls
        keep graphs valid and make them replay the new traces."""
        from .trace import Trace
        h = self._bind()
        if isinstance(traces, Trace):
            traces = [traces]
        traces = list(traces)
        if not traces or not all(isinstance(t, Trace) for t in traces):
            raise ValueError("traces must be a Trace or a non-empty list of Trace")
        arr = (_lib.VmpTrace * len(traces))()
        for c, t in zip(arr, traces):
            c.steps = t.steps
            c.offs, c.cpu = t.offs.ctypes.data, t.cpu.ctypes.data
            c.mem, c.runtime = t.mem.ctypes.data, t.runtime.ctypes.data
        m = None
        if trace_of_env is not None:
            m = np.ascontiguousarray(np.asarray(trace_of_env), dtype=np.int32)
            if m.shape != (self.n_envs,):
                raise ValueError(f"trace_of_env must have n_envs = {self.n_envs} entries")
        pm = None if m is None else m.ctypes.data_as(ctypes.c_void_p)
        with torch.cuda.device(self.device):
            check(lib().vmp_set_trace(h, len(traces), ctypes.cast(arr, ctypes.c_void_p), pm))
        # kept for an env that is to replay the same ones (vmp.agents.RolloutAgent)
        self._traces = (traces, np.zeros(self.n_envs, np.int32) if m is None else m.copy())

    def clear_trace(self):
        """Back to the RNG workload (the per-env one if the env has it), the
        streams where they stood (vmp_clear_trace)."""
        with torch.cuda.device(self.device):
            check(lib().vmp_clear_trace(self._bind()))
        self._traces = None

    def trace_info(self):
        """None without a trace, else dict(n_traces, trace_of_env int32 [n_envs],
        steps int64 [n_traces], requests int64 [n_traces])."""
        h = self._bind()
        n = ctypes.c_int32()
        check(lib().vmp_trace_info(h, ctypes.byref(n), None, None, None))
        if n.value == 0:
            return None
        m = np.empty(self.n_envs, np.int32)
        st, rq = np.empty(n.value, np.int64), np.empty(n.value, np.int64)
        check(lib().vmp_trace_info(h, None, m.ctypes.data_as(ctypes.c_void_p),
                                   st.ctypes.data_as(ctypes.c_void_p),
                                   rq.ctypes.data_as(ctypes.c_void_p)))
        return dict(n_traces=n.value, trace_of_env=m, steps=st, requests=rq)

    def reset(self, seeds=None, mask=None, obs=True):
        """reset(seed) for every env (or those where mask is true). seeds=None is
        reset(seed=None): the RNG streams continue (env.py:181-182)."""
        h = self._bind()
        s = None
        if seeds is not None:
            s = torch.as_tensor(seeds, dtype=torch.int64, device=self.device).contiguous()
            if s.numel() != self.n_envs:
                raise ValueError("seeds must have n_envs entries")
            if bool((s < 0).any()):
                raise ValueError("seeds must be non-negative")
        m = None
        if mask is not None:
            m = torch.as_tensor(mask, device=self.device).to(torch.uint8).contiguous()
        o = self._empty((self.n_envs, self.D), torch.float32) if obs else None
        check(lib().vmp_reset(h, ptr(s), ptr(m), ptr(o)))
        if self._start is not None:  # validated on the host by set_start_state: no read-back here
            st, ctr, tot = self._start
            self.set_state(st, mask=m, counters=ctr, totals=tot, check=False)
            if o is not None:
                check(lib().vmp_get_obs(h, ptr(o)))
        return o

    def step(self, actions, obs=None, reward=None, done=None, valid=None, want_valid=True,
             bool_done=True, mask_out=None):
        """One VmEnv.step per env. actions: int tensor [N, V] on the device.
        Returns (obs f32[N,D], reward f64[N], done bool[N], valid u8[N,V]);
        bool_done=False returns the u8 done buffer itself (no conversion
        kernel: a captured step graph reads `done` in place). mask_out (int32
        [N, V, W]): also write the post-step invalid-action mask bits, what
        mask_bits() would give next (vmp_step_mask, same launch)."""
        h = self._bind()
        a = actions
        if a.dtype != torch.int32 or not a.is_contiguous() or a.device != self.device:
            a = a.to(device=self.device, dtype=torch.int32).contiguous()
        if a.shape != (self.n_envs, self.V):
            raise ValueError(f"actions must have shape ({self.n_envs}, {self.V})")
        obs = self._empty((self.n_envs, self.D), torch.float32) if obs is None else obs
        reward = self._empty((self.n_envs,), torch.float64) if reward is None else reward
        done = self._empty((self.n_envs,), torch.uint8) if done is None else done
        if want_valid and valid is None:
            valid = self._empty((self.n_envs, self.V), torch.uint8)
        if mask_out is None:
            check(lib().vmp_step(h, ptr(a), ptr(obs), ptr(reward), ptr(done), ptr(valid)))
        else:
            if (mask_out.dtype != torch.int32 or not mask_out.is_contiguous()
                    or tuple(mask_out.shape) != (self.n_envs, self.V, self.W)):
                raise ValueError(f"mask_out must be contiguous int32 {(self.n_envs, self.V, self.W)}")
            check(lib().vmp_step_mask(h, ptr(a), ptr(obs), ptr(reward), ptr(done), ptr(valid),
                                      ptr(mask_out)))
        return obs, reward, done.bool() if bool_done else done, valid

    def heuristic_act(self, policy="firstfit"):
        """FirstFitAgent.act / BestFitAgent.act for every env -> int32 [N, V]."""
        h = self._bind()
        a = self._empty((self.n_envs, self.V), torch.int32)
        check(lib().vmp_heuristic_act(h, _lib.POLICIES[policy], ptr(a)))
        return a

    def heuristic_act_obs(self, obs, policy="firstfit"):
        """FirstFitAgent.act / BestFitAgent.act on the given observations (any
        f32 [N, D], not necessarily the envs' own; firstfit.py:21-38,
        bestfit.py:21-40) -> int32 [N, V]. Reads no env state."""
        h = self._bind()
        o = torch.as_tensor(obs, dtype=torch.float32, device=self.device).reshape(
            self.n_envs, self.D).contiguous()
        a = self._empty((self.n_envs, self.V), torch.int32)
        check(lib().vmp_heuristic_act_obs(h, _lib.POLICIES[policy], ptr(o), ptr(a)))
        return a

    def heuristic_step(self, policy="firstfit", want_actions=False, want_valid=False,
                       want_obs=True, obs=None, reward=None, done=None):
        """act(obs) then step(action) in one launch (the Base.test loop body).
        obs f32[N,D] / reward f64[N] / done u8[N]: the caller's own contiguous
        output buffers (as `step` takes them); allocated here when None."""
        h = self._bind()
        a = self._empty((self.n_envs, self.V), torch.int32) if want_actions else None
        for t, shape, dt in ((obs, (self.n_envs, self.D), torch.float32),
                             (reward, (self.n_envs,), torch.float64),
                             (done, (self.n_envs,), torch.uint8)):
            if t is not None and (t.shape != shape or t.dtype != dt or not t.is_contiguous()
                                  or t.device != self.device):
                raise ValueError(f"output buffer must be contiguous {dt} {shape} on {self.device}")
        if obs is None and want_obs:
            obs = self._empty((self.n_envs, self.D), torch.float32)
        reward = self._empty((self.n_envs,), torch.float64) if reward is None else reward
        done = self._empty((self.n_envs,), torch.uint8) if done is None else done
        valid = self._empty((self.n_envs, self.V), torch.uint8) if want_valid else None
        check(lib().vmp_heuristic_step(h, _lib.POLICIES[policy], ptr(a), ptr(obs), ptr(reward),
                                       ptr(done), ptr(valid)))
        return obs, reward, done.bool(), valid, a

    def rollout(self, policy="firstfit", k_steps=1, rewards=None, done_count=None):
        """k_steps fused act+step iterations per env in one launch.
        Returns (rewards f64[k, N], done_count i64[N])."""
        h = self._bind()
        rewards = self._empty((k_steps, self.n_envs), torch.float64) if rewards is None else rewards
        if done_count is None:
            done_count = torch.zeros(self.n_envs, dtype=torch.int64, device=self.device)
        check(lib().vmp_rollout_heuristic(h, _lib.POLICIES[policy], int(k_steps), ptr(rewards),
                                          ptr(done_count)))
        return rewards, done_count

    def mask_bits(self, out=None):
        """Bit-packed invalid-action mask u32 [N, V, ceil(A/32)] (bit set = invalid)."""
        h = self._bind()
        b = self._empty((self.n_envs, self.V, self.W), torch.int32) if out is None else out
        if b.shape != (self.n_envs, self.V, self.W) or b.dtype != torch.int32 or not b.is_contiguous():
            raise ValueError("mask_bits out must be contiguous int32 [N, V, W]")
        check(lib().vmp_mask(h, ptr(b)))
        return b

    def mask(self):
        """get_invalid_action_mask(masked=True) as bool [N, V, A] (env.py:45-53)."""
        h = self._bind()
        m = self._empty((self.n_envs, self.V, self.A), torch.uint8)
        check(lib().vmp_mask_bool(h, ptr(m)))
        return m.bool()

    def obs(self):
        h = self._bind()
        o = self._empty((self.n_envs, self.D), torch.float32)
        check(lib().vmp_get_obs(h, ptr(o)))
        return o

    def counters(self):
        h = self._bind()
        c = self._empty((self.n_envs, N_COUNTERS), torch.int64)
        check(lib().vmp_get_counters(h, ptr(c)))
        return c

    def stats(self):
        h = self._bind()
        s = self._empty((self.n_envs, N_STATS), torch.float64)
        check(lib().vmp_get_stats(h, ptr(s)))
        return s

    def state(self):
        """Reference-dtype state tensors: placement/remaining int64 [N,V],
        vm_cpu/vm_mem f64 [N,V], cpu/mem f64 [N,P]."""
        h = self._bind()
        N, V, P = self.n_envs, self.V, self.P
        pl, rem = self._empty((N, V), torch.int64), self._empty((N, V), torch.int64)
        vc, vm = self._empty((N, V), torch.float64), self._empty((N, V), torch.float64)
        c, m = self._empty((N, P), torch.float64), self._empty((N, P), torch.float64)
        check(lib().vmp_get_state(h, ptr(pl), ptr(vc), ptr(vm), ptr(c), ptr(m), ptr(rem)))
        return dict(vm_placement=pl, vm_cpu=vc, vm_memory=vm, cpu=c, memory=m,
                    vm_remaining_runtime=rem)

    # ------------------------------------------------ eval-mode Record metrics
    def record(self, on=True):
        """Start (on=True, right after reset, as Base.test does) or stop recording
        the Record metrics of every env on the device (vmp_record_enable).
        reset() restarts the recorder of the envs it resets, restore() that of
        every env."""
        check(lib().vmp_record_enable(self._bind(), int(bool(on))))

    def record_read(self):
        """(hist u32 [N, 2, 1001] pending/slowdown rate counts, sums f64 [N, 19]:
        include/vmp.h VMP_REC_*). Non-destructive."""
        h = self._bind()
        hist = self._empty((self.n_envs, 2, REC_BINS), torch.int32)
        sums = self._empty((self.n_envs, N_REC), torch.float64)
        check(lib().vmp_record_read(h, ptr(hist), ptr(sums)))
        return hist, sums

    def record_summary(self):
        """Record.get_summary() (record.py:110-134) of every env -> list of dicts."""
        from .record import summary_from_device
        hist, sums = self.record_read()
        ctr, st = self.counters().cpu().numpy(), self.stats().cpu().numpy()
        hist, sums = hist.cpu().numpy().view(np.uint32), sums.cpu().numpy()
        return [summary_from_device(hist[i], sums[i], ctr[i], st[i], self.P)
                for i in range(self.n_envs)]

    # ------------------------------------------- per-request outcome log
    def request_log(self, on=True, capacity=None):
        """Start (on=True) or free the per-request outcome log of every env on
        the device (vmp_reqlog_enable): one row per request offered since the
        env's last reset, updated after every step (see vmp.reqlog). capacity:
        rows per env; a traced env defaults to the largest request count among
        the traces its envs replay, an RNG env must pass one. The log starts
        from the current state (call it right after reset); reset() restarts
        the log of the envs it resets. Not during graph capture; a graph
        captured before the call does not log."""
        h = self._bind()
        if not on:
            check(lib().vmp_reqlog_enable(h, 0))
            return
        if capacity is None:
            info = self.trace_info()
            if info is None:
                raise ValueError("request_log needs a capacity on an env without a trace")
            capacity = max(1, int(info["requests"][np.unique(info["trace_of_env"])].max()))
        if int(capacity) < 1:
            raise ValueError("capacity must be >= 1")
        with torch.cuda.device(self.device):
            check(lib().vmp_reqlog_enable(h, int(capacity)))

    def request_log_read(self):
        """The log so far as a `vmp.reqlog.RequestLog` (non-destructive)."""
        from .reqlog import NF, RequestLog
        h = self._bind()
        cap = ctypes.c_int64()
        check(lib().vmp_reqlog_info(h, ctypes.byref(cap)))
        if cap.value == 0:
            raise VmpError("the request log is not enabled (request_log())")
        rows = self._empty((self.n_envs, cap.value, NF), torch.int32)
        meta = self._empty((self.n_envs, 3), torch.int64)
        check(lib().vmp_reqlog_read(h, ptr(rows), ptr(meta)))
        return RequestLog(rows.cpu().numpy(), meta.cpu().numpy())

    # ------------------------------------------------- per-step time series
    def series(self, on=True, capacity=None, stride=1, pm_rows=False):
        """Start (on=True) or free the per-step time series of every env on the
        device (vmp_series_enable): one row per window of `stride` steps with
        the reward, waiting ratio, PM utilisation, target means, used PMs and
        counters (see vmp.series), filled after every step; pm_rows also keeps
        the PMs' cpu and memory of each window's last step. capacity: rows per
        env, by default what the steps left to eval_steps (training_steps
        outside eval mode) need. The series starts at row 0 from the current
        state; reset() restarts the series of the envs it resets. Not during
        graph capture; a graph captured before the call does not observe."""
        h = self._bind()
        if not on:
            check(lib().vmp_series_enable(h, 0, 1, 0))
            return
        if int(stride) < 1:
            raise ValueError("stride must be >= 1")
        if capacity is None:
            limit = self.config.eval_steps if self.eval_mode else self.config.training_steps
            left = int(limit) - (int(self.counters()[:, 5].min()) - 1)
            capacity = max(1, -(-left // int(stride)))
        if int(capacity) < 1:
            raise ValueError("capacity must be >= 1")
        with torch.cuda.device(self.device):
            check(lib().vmp_series_enable(h, int(capacity), int(stride), int(bool(pm_rows))))

    def series_read(self):
        """The series so far as a `vmp.series.Series` (non-destructive)."""
        from .series import NF, NMETA, Series
        h = self._bind()
        cap, stride, pmr = ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int32()
        check(lib().vmp_series_info(h, ctypes.byref(cap), ctypes.byref(stride), ctypes.byref(pmr)))
        if cap.value == 0:
            raise VmpError("the time series is not enabled (series())")
        rows = self._empty((self.n_envs, cap.value, NF), torch.float64)
        meta = self._empty((self.n_envs, NMETA), torch.int64)
        pm = self._empty((self.n_envs, cap.value, 2 * self.P), torch.float32) if pmr.value else None
        check(lib().vmp_series_read(h, ptr(rows), ptr(pm), ptr(meta)))
        return Series(rows.cpu().numpy(), meta.cpu().numpy(), stride.value,
                      None if pm is None else pm.cpu().numpy())

    def rank(self):
        h = self._bind()
        r = self._empty((self.n_envs,), torch.int64)
        check(lib().vmp_get_rank(h, ptr(r)))
        return r

    # ------------------------------------------------- checkpoint / resume
    def snapshot(self):
        """The whole batched env state (vmp_snapshot: PCG64 streams, counters,
        PM and VM words) as a device u8 tensor; `restore` on an env of the same
        config and n_envs continues bit-exactly from here. torch.save it for a
        resumable run. An env given a per-env workload appends it;
        such a snapshot restores only into an env with the same workload. A
        traced env's snapshot carries a hash of its traces and map and restores
        only into an env replaying the same ones."""
        h = self._bind()
        n = ctypes.c_int64()
        check(lib().vmp_snapshot_bytes(h, ctypes.byref(n)))
        buf = self._empty((n.value,), torch.uint8)
        check(lib().vmp_snapshot(h, ptr(buf)))
        return buf

    def restore(self, snap):
        """Load a `snapshot()` (any device or host tensor) into this env."""
        h = self._bind()
        s = torch.as_tensor(snap).to(device=self.device, dtype=torch.uint8).contiguous()
        n = ctypes.c_int64()
        check(lib().vmp_snapshot_bytes(h, ctypes.byref(n)))
        if s.numel() != n.value:
            raise ValueError(f"snapshot holds {s.numel()} bytes, this env needs {n.value}")
        check(lib().vmp_restore(h, ptr(s)))
        torch.cuda.current_stream(self.device).synchronize()  # s may be a temporary copy

    # ------------------------------------------------------------ branching
    def _branch_arg(self, x, dtype, name, lo=None, hi=None):
        """index / seeds of `branch` as a contiguous device tensor [n_envs].
        Host values are range-checked here; a device tensor is taken as it is
        (the kernel keeps an env whose entry is out of range)."""
        if isinstance(x, torch.Tensor) and x.is_cuda:
            if x.numel() != self.n_envs:
                raise ValueError(f"{name} must have n_envs = {self.n_envs} entries")
            if x.device != self.device:
                raise ValueError(f"{name} lives on {x.device}, the env on {self.device}")
            return x.reshape(-1).to(dtype).contiguous()
        a = np.asarray(x.numpy() if isinstance(x, torch.Tensor) else x)
        if a.shape != (self.n_envs,):
            raise ValueError(f"{name} must have n_envs = {self.n_envs} entries")
        if a.dtype.kind not in "iu":
            raise ValueError(f"{name} must be integers")
        a = a.astype(np.int64)
        if lo is not None and (a.min() < lo or a.max() >= hi):
            raise ValueError(f"{name} entries must be in [{lo}, {hi})")
        return torch.as_tensor(a, device=self.device).to(dtype)

    def branch(self, src, index, seeds=None):
        """Copy env states on the device (vmp_branch): env i of this env takes
        the complete state of env index[i] of `src` (streams, counters, PMs,
        VMs; bit for bit, so it continues exactly as that env would), -1 keeps
        env i as it is. `src` is a BatchedVmEnv of the same config (the seed
        and n_envs may differ) or this env itself: any map is correct in
        place. seeds (optional): where seeds[i] >= 0 the copied env gets the
        four RNG streams of reset(seed=seeds[i]) instead, i.e. its own future
        from the copied state; negative entries keep the copied streams.
        index / seeds: device tensors, host arrays or lists of n_envs entries;
        host values are range-checked (ValueError), device tensors are read by
        the kernel only, which keeps an env whose entry is out of range. Eval
        mode, the per-env workload and the trace stay this env's own. The
        recorder, request log and series restart for the overwritten envs.
        No host synchronisation; with src is not self it can be captured in a
        graph (tensor arguments are then read at every replay)."""
        if not isinstance(src, BatchedVmEnv):
            raise ValueError("src must be a BatchedVmEnv")
        if src.device != self.device:
            raise ValueError("src lives on another device")
        hd = self._bind()
        hs = src._bind()
        m = self._branch_arg(index, torch.int32, "index", -1, src.n_envs)
        s = None if seeds is None else self._branch_arg(seeds, torch.int64, "seeds")
        check(lib().vmp_branch(hd, hs, ptr(m), ptr(s)))

    # ------------------------------------------------------------ set state
    def _state_arg(self, x, dtype, shape, name):
        """An array of `set_state` as a contiguous device tensor of `shape`. A
        device tensor of the right dtype and layout is used as it is (a graph
        replays on the caller's own buffer); anything else is converted."""
        if isinstance(x, torch.Tensor):
            if x.is_cuda and x.device != self.device:
                raise ValueError(f"{name} lives on {x.device}, the env on {self.device}")
            t = x
        else:
            a = np.asarray(x)
            if a.dtype.kind not in "iufb":
                raise ValueError(f"{name} must be numeric")
            t = torch.from_numpy(np.ascontiguousarray(a))
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name} must have shape {tuple(shape)}, not {tuple(t.shape)}")
        return t.to(device=self.device, dtype=dtype).contiguous()

    def set_start_state(self, state):
        """Make every later reset() leave `state` (a vmp.state.State of n_envs
        envs, or of one env for all; None: an empty env again) instead of an
        empty env: the reset envs are reseeded or rewound as usual and then
        given the state by set_state, counters and totals included where the
        state has them. The state is validated here, on the host (ValueError),
        and kept on the device, so reset() stays free of host synchronisation."""
        if state is None:
            self._start = None
            return
        from .state import IMPORTED, RULES
        s = state.broadcast(self.n_envs)
        if s.pms != self.P or s.vms != self.V:
            raise ValueError(f"the state is of {s.pms} PMs / {s.vms} VMs, the env of "
                             f"{self.P} / {self.V}")
        code = s.validate(timestep=1)
        if (code != IMPORTED).any():
            e = int(np.flatnonzero(code != IMPORTED)[0])
            raise ValueError(f"start state refused, env {e}: {RULES[int(code[e])]}")
        dev = lambda x: None if x is None else torch.as_tensor(x, device=self.device)  # noqa: E731
        self._start = ({k: dev(v) for k, v in s.as_dict().items()}, dev(s.counters), dev(s.totals))

    def set_state(self, state, mask=None, counters=None, totals=None, seeds=None, check=True):
        """Give envs the state in the caller's arrays (vmp_set_state): the
        inverse of `state()` / `counters()`. state: the dict `state()` returns
        (vm_placement, vm_remaining_runtime int64 [N, V]; vm_cpu, vm_memory f64
        [N, V]); cpu / memory f64 [N, P] may be absent or None, the PM loads are
        then the exact sums of the running VMs' hundredths. mask [N]: the envs
        to set (None: all). counters int64 [N, 6] as `counters()` returns them
        (timestep last), totals f64 [N, 2] = total cpu / memory requested; None
        keeps the env's. seeds int64 [N]: entries >= 0 give the env the streams
        of reset(seed), negative ones and None keep its streams.
        Every selected env is validated on the device as a whole and written
        only if valid (vmp.state.RULES names the codes). check=True reads the
        status back and raises ValueError naming the refused envs and their
        rule; check=False returns the status tensor (u8 [N]: 0 not selected, 1
        imported, >= 2 refused) without a synchronise: with device tensors of
        the right dtype this is the graph-capturable form, and a replay reads
        the tensors' current contents. Host lists and arrays are converted;
        a shape mismatch raises ValueError. The recorder, request log and
        series restart for the imported envs only."""
        h = self._bind()
        N, V, P = self.n_envs, self.V, self.P
        pl = self._state_arg(state["vm_placement"], torch.int64, (N, V), "vm_placement")
        vc = self._state_arg(state["vm_cpu"], torch.float64, (N, V), "vm_cpu")
        vm = self._state_arg(state["vm_memory"], torch.float64, (N, V), "vm_memory")
        rem = self._state_arg(state["vm_remaining_runtime"], torch.int64, (N, V),
                              "vm_remaining_runtime")
        c, m = state.get("cpu"), state.get("memory")
        if (c is None) != (m is None):
            raise ValueError("cpu and memory are both given or both absent")
        if c is not None:
            c = self._state_arg(c, torch.float64, (N, P), "cpu")
            m = self._state_arg(m, torch.float64, (N, P), "memory")
        k = None if mask is None else self._state_arg(mask, torch.uint8, (N,), "mask")
        ctr = None if counters is None else self._state_arg(counters, torch.int64,
                                                            (N, N_COUNTERS), "counters")
        tot = None if totals is None else self._state_arg(totals, torch.float64, (N, 2), "totals")
        sd = None if seeds is None else self._state_arg(seeds, torch.int64, (N,), "seeds")
        status = self._empty((N,), torch.uint8)
        _lib.check(lib().vmp_set_state(h, ptr(k), ptr(pl), ptr(vc), ptr(vm), ptr(rem), ptr(c),
                                       ptr(m), ptr(ctr), ptr(tot), ptr(sd), ptr(status)))
        if not check:
            return status
        st = status.cpu().numpy()
        refused = np.flatnonzero(st >= 2)
        if refused.size:
            from .state import RULES
            raise ValueError("set_state refused env(s) " + ", ".join(
                f"{int(e)}: {RULES.get(int(st[e]), int(st[e]))}" for e in refused))
        return status
