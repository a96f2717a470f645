"""The per-step time series (include/vmp.h, VMP_SR_*) restated in numpy: what one
step contributes to its row from an env's state, counters, stats, rank and
reward (`row_of`), and how rows, COUNT and LOST develop as steps are folded in
one after another (`LiteralSeries`). tests/test_series_cpu.py checks the
literal itself; tests/test_gpu_series.py compares the device series with it."""
import numpy as np

(STEPS, REWARD, WAITING_RATIO, CPU_SUM, MEM_SUM, CPU_VAR, MEM_VAR, TARGET_CPU_MEAN,
 TARGET_MEM_MEAN, USED_PM, EMPTY_PM, WAITING, RUNNING, TIMESTEP, TOTAL_REQUESTS, SERVED, SUSPEND,
 PLACE, DROPPED, NF) = range(20)
FIRST, COUNT, LOST, NMETA = range(4)
N_SUMMED = 13  # fields below it are summed over a window, the others overwritten
VAR_FIELDS = (CPU_VAR, MEM_VAR)


def row_of(state, counters, stats, rank, reward, P):
    """One step's f64[NF] row of one env. state: dict with vm_placement [V],
    cpu [P], memory [P] (BatchedVmEnv.state()'s entries of the env); counters:
    vmp_get_counters' row (total_requests, served, suspend, place, dropped,
    timestep); stats: vmp_get_stats' row (waiting_ratio, target_cpu_mean,
    target_mem_mean, ...); rank: _get_rank; reward: the step's reward."""
    pl = np.asarray(state["vm_placement"])
    cpu = np.ascontiguousarray(state["cpu"], dtype=np.float64)
    mem = np.ascontiguousarray(state["memory"], dtype=np.float64)
    assert cpu.shape == mem.shape == (P,)
    r = np.zeros(NF, np.float64)
    r[STEPS] = 1.0
    r[REWARD] = reward
    r[WAITING_RATIO] = stats[0]
    r[CPU_SUM] = np.sum(cpu)
    r[MEM_SUM] = np.sum(mem)
    r[CPU_VAR] = np.var(cpu)
    r[MEM_VAR] = np.var(mem)
    r[TARGET_CPU_MEAN] = stats[1]
    r[TARGET_MEM_MEAN] = stats[2]
    r[USED_PM] = rank
    r[EMPTY_PM] = P - np.count_nonzero(cpu)
    r[WAITING] = np.count_nonzero(pl == P)
    r[RUNNING] = np.count_nonzero(pl < P)
    r[TIMESTEP] = counters[5]
    r[TOTAL_REQUESTS:DROPPED + 1] = counters[:5]
    return r


def target_means(state, P, cap_target_util):
    """env.py:116-121 from the state: the existing VMs' sizes summed in index
    order over P, capped at 1 under cap_target_util."""
    ex = np.asarray(state["vm_placement"]) <= P
    out = []
    for key in ("vm_cpu", "vm_memory"):
        t = np.sum(np.asarray(state[key], dtype=np.float64)[ex]) / P
        out.append(1.0 if cap_target_util and t > 1 else t)
    return out


class LiteralSeries:
    """One env's series: `capacity` rows of `stride` steps each. add(row)
    folds the next observed step in: the first step of a window stores its
    summed fields, a later one adds to them (one f64 add each), and every step
    overwrites the counters. A step whose row is >= capacity is counted in
    LOST and stored nowhere. restart(timestep) is what enable / reset /
    restore do."""

    def __init__(self, capacity, stride, timestep=1):
        assert capacity >= 1 and stride >= 1
        self.capacity, self.stride = int(capacity), int(stride)
        self.restart(timestep)

    def restart(self, timestep):
        self.rows = np.zeros((self.capacity, NF), np.float64)
        self.meta = np.array([timestep, 0, 0], np.int64)

    def add(self, row):
        row = np.asarray(row, dtype=np.float64)
        assert row.shape == (NF,)
        count = int(self.meta[COUNT])
        r, k = divmod(count, self.stride)
        self.meta[COUNT] = count + 1
        if r >= self.capacity:
            self.meta[LOST] += 1
            return
        if k == 0:
            self.rows[r, :N_SUMMED] = row[:N_SUMMED]
        else:
            for f in range(N_SUMMED):  # sequential: one add per field and step
                self.rows[r, f] = self.rows[r, f] + row[f]
        self.rows[r, N_SUMMED:] = row[N_SUMMED:]

    @property
    def rows_written(self):
        return min(-(-int(self.meta[COUNT]) // self.stride), self.capacity)
