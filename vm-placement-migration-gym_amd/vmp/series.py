"""The per-step time series (vmp_series_* in include/vmp.h) on the host.

`BatchedVmEnv.series()` switches the device series on; `series_read()` returns
a `Series`: for every env one row per window of `stride` observed steps, the
per-step lists of the reference's Record (src/record.py:13-32) for N envs at
once. Fields 1..12 of a row are sums over the window's steps, the counters are
those after the window's last step.
"""
import numpy as np

FIELDS = ("steps", "reward", "waiting_ratio", "cpu_sum", "mem_sum", "cpu_var", "mem_var",
          "target_cpu_mean", "target_mem_mean", "used_pm", "empty_pm", "waiting", "running",
          "timestep", "total_requests", "served", "suspend", "place", "dropped")  # VMP_SR_*
NF = len(FIELDS)
N_SUMMED = 13  # fields 1 .. N_SUMMED - 1 are window sums; the rest are counters
SUMMED = FIELDS[1:N_SUMMED]
COUNTERS = FIELDS[N_SUMMED:]
FIRST, COUNT, LOST = 0, 1, 2
NMETA = 3


class Series:
    """rows f64 [N, C, 19], meta int64 [N, 3] (FIRST, COUNT, LOST), optionally
    pm f32 [N, C, 2P], as vmp_series_read gives them, and the stride they were
    recorded with. Every field is an f64 [N, C] array under its name:
      steps            steps folded into the row (0: never written; below the
                       stride only in an env's last, open row)
      reward .. running   sums over the window's steps (`mean` divides them)
      timestep .. dropped the env's counters after the window's last step
                       (int64 values held as f64: exact below 2^53)
    """

    def __init__(self, rows, meta, stride=1, pm=None):
        rows, meta = np.asarray(rows), np.asarray(meta)
        if rows.ndim != 3 or rows.shape[2] != NF or meta.shape != (rows.shape[0], NMETA):
            raise ValueError("rows must be [N, C, %d] and meta [N, %d]" % (NF, NMETA))
        if int(stride) < 1:
            raise ValueError("stride must be >= 1")
        self.rows = rows.astype(np.float64, copy=False)
        self.meta = meta.astype(np.int64, copy=False)
        self.stride = int(stride)
        self.pm = None
        if pm is not None:
            pm = np.asarray(pm)
            if pm.ndim != 3 or pm.shape[:2] != rows.shape[:2] or pm.shape[2] % 2:
                raise ValueError("pm must be [N, C, 2P]")
            self.pm = pm.astype(np.float32, copy=False)
        for k, name in enumerate(FIELDS):
            setattr(self, name, self.rows[:, :, k])

    @property
    def n_envs(self):
        return self.rows.shape[0]

    @property
    def capacity(self):
        return self.rows.shape[1]

    @property
    def first(self):
        """The timestep at which each env's series started."""
        return self.meta[:, FIRST]

    @property
    def count(self):
        """Steps each env observed since then."""
        return self.meta[:, COUNT]

    @property
    def lost(self):
        """Steps per env whose row was >= capacity (counted, not stored)."""
        return self.meta[:, LOST]

    @property
    def rows_written(self):
        """Rows per env that hold at least one step: min(ceil(COUNT / stride), C)."""
        return np.minimum(-(-self.count // self.stride), self.capacity)

    def mean(self, name):
        """The window means of a field, f64 [N, C]: a summed field divided by
        `steps` (NaN in a row never written); a counter, or `steps`, as it is."""
        k = FIELDS.index(name)
        x = self.rows[:, :, k]
        if not 1 <= k < N_SUMMED:
            return x.copy()
        st = self.rows[:, :, 0]
        return np.divide(x, st, out=np.full(x.shape, np.nan), where=st > 0)

    def band(self, name):
        """(mean, std) over the envs of `mean(name)`, per row, over the rows
        every env has written: two f64 [rows] arrays (std: numpy's default,
        the population's)."""
        n = int(self.rows_written.min()) if self.n_envs else 0
        m = self.mean(name)[:, :n]
        return m.mean(axis=0), m.std(axis=0)

    @property
    def pm_cpu(self):
        """f32 [N, C, P]: the PMs' cpu after each window's last step (None
        unless recorded with pm_rows)."""
        return None if self.pm is None else self.pm[:, :, :self.pm.shape[2] // 2]

    @property
    def pm_mem(self):
        return None if self.pm is None else self.pm[:, :, self.pm.shape[2] // 2:]

    def env(self, i):
        """Envs i (an index, a slice or a list) alone."""
        i = [i] if np.isscalar(i) else i
        return Series(self.rows[i], self.meta[i], self.stride, None if self.pm is None else self.pm[i])

    # ------------------------------------------------------------ files
    def save(self, path):
        d = dict(rows=self.rows, meta=self.meta, stride=np.int64(self.stride))
        if self.pm is not None:
            d["pm"] = self.pm
        with open(path, "wb") as f:
            np.savez(f, **d)

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            return cls(z["rows"], z["meta"], int(z["stride"]), z["pm"] if "pm" in z.files else None)

    CSV_HEADER = "Env,Window," + ",".join(FIELDS)

    def to_csv(self, path=None):
        """One line per written row of every env, floats in repr (they read
        back exactly); written to `path` if given, and returned."""
        lines = [self.CSV_HEADER]
        for i, n in enumerate(self.rows_written):
            for r in range(int(n)):
                lines.append("%d,%d,%s" % (i, r, ",".join(repr(float(x)) for x in self.rows[i, r])))
        text = "\n".join(lines) + "\n"
        if path is not None:
            with open(path, "w") as f:
                f.write(text)
        return text
