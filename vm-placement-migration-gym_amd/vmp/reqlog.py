"""The per-request outcome log (vmp_reqlog_* in include/vmp.h) on the host.

`BatchedVmEnv.request_log()` switches the device log on; `request_log_read()`
returns a `RequestLog`: for every env one row per request id (the request's
ordinal among the requests offered since the env's reset; on a traced env its
index in the trace), so request j can be compared across policies that replayed
the same trace.
"""
import numpy as np

FIELDS = ("slot", "arrived", "placed", "finished", "suspends", "wait_steps")  # VMP_RQ_*
NF = len(FIELDS)
FIRST, NEXT, LOST = 0, 1, 2
UNOBSERVED, DROPPED = -2, -1


class RequestLog:
    """rows int32 [N, C, 6], meta int64 [N, 3] (FIRST, NEXT, LOST) as
    vmp_reqlog_read gives them. Every field is an int32 [N, C] array:
      slot        -2 not observed, -1 dropped, >= 0 the slot the request took
      arrived     timestep of the step that offered it (dropped ones too)
      placed      timestep of its first valid placement, 0 = not yet
      finished    timestep of the step that finished it, 0 = not yet
      suspends    valid suspend actions on it
      wait_steps  steps that left it waiting, the arrival step included
    """

    def __init__(self, rows, meta):
        rows, meta = np.asarray(rows), np.asarray(meta)
        if rows.ndim != 3 or rows.shape[2] != NF or meta.shape != (rows.shape[0], 3):
            raise ValueError("rows must be [N, C, 6] and meta [N, 3]")
        self.rows = rows.astype(np.int32, copy=False)
        self.meta = meta.astype(np.int64, copy=False)
        for k, name in enumerate(FIELDS):
            setattr(self, name, self.rows[:, :, k])

    @property
    def n_envs(self):
        return self.rows.shape[0]

    @property
    def capacity(self):
        return self.rows.shape[1]

    @property
    def lost(self):
        """Requests per env whose id was >= capacity (not logged)."""
        return self.meta[:, LOST]

    def env(self, i):
        """Env i alone, trimmed to the ids it observed: [FIRST, min(NEXT, C))."""
        lo = int(min(self.meta[i, FIRST], self.capacity))
        hi = int(min(self.meta[i, NEXT], self.capacity))
        return RequestLog(self.rows[i:i + 1, lo:hi], self.meta[i:i + 1])

    # ---------------------------------------------------------------- masks
    @property
    def dropped(self):
        return self.slot == DROPPED

    @property
    def accepted(self):
        return self.slot >= 0

    @property
    def is_placed(self):
        return self.accepted & (self.placed > 0)

    @property
    def is_finished(self):
        return self.accepted & (self.finished > 0)

    # ------------------------------------------------------- derived columns
    @property
    def pending_steps(self):
        """Steps before the first placement, PLACED - ARRIVED (-1: not placed)."""
        return np.where(self.is_placed, self.placed - self.arrived, -1).astype(np.int32)

    @property
    def suspended_steps(self):
        """Steps spent suspended after the first placement,
        WAIT_STEPS - (PLACED - ARRIVED) (-1: not placed)."""
        return np.where(self.is_placed, self.wait_steps - (self.placed - self.arrived),
                        -1).astype(np.int32)

    @property
    def sojourn(self):
        """FINISHED - ARRIVED (-1: not finished)."""
        return np.where(self.is_finished, self.finished - self.arrived, -1).astype(np.int32)

    CSV_HEADER = "Env,Request," + ",".join(FIELDS)

    def to_csv(self, path=None):
        """One line per observed request of every env; written to `path` if
        given, and returned."""
        lines = [self.CSV_HEADER]
        for i in range(self.n_envs):
            lo = int(min(self.meta[i, FIRST], self.capacity))
            hi = int(min(self.meta[i, NEXT], self.capacity))
            for j in range(lo, hi):
                lines.append("%d,%d,%s" % (i, j, ",".join("%d" % x for x in self.rows[i, j])))
        text = "\n".join(lines) + "\n"
        if path is not None:
            with open(path, "w") as f:
                f.write(text)
        return text
