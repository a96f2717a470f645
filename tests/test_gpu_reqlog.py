"""The per-request outcome log (vmp_reqlog_*, BatchedVmEnv.request_log) on the
GPU against the ground truth of tests/reqlog_literal.LogEnv, a literal env that
knows which slot took which request. The GPU's own heuristic actions (or the
test's random ones) are fed to the literal; rows and meta must be equal, every
comparison exact. Shapes: P 12 / V 90 (tests/test_gpu_workload.BASE), N <= 8."""
import ctypes

import numpy as np
import pytest
import torch

from tests import reqlog_literal as RL
from tests.test_gpu_trace import _generated, _traces
from tests.test_gpu_workload import BASE, DEV, LAM, LEN, N, SEEDS, _config, _ref

pytestmark = pytest.mark.gpu

EINVAL, EOOM, ESTATE = -1, -3, -4
CFG = dict(BASE, reward_function="wr")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")


def _workload(kind):
    return RL.extra_traces(kind) if kind in ("churn", "burst200") else _generated(kind)


def _env(traces=None, m=None, n=None, cfg=None):
    from vmp.batched import BatchedVmEnv
    from vmp.config import Config
    n = n if n is not None else len(traces)
    b = BatchedVmEnv(Config(**(cfg or CFG)), n, seeds=np.arange(n, dtype=np.int64) * 4, device=DEV)
    if traces is not None:
        b.set_trace(traces, np.arange(n) if m is None else m)
    return b


def _lits(traces, capacity, m=None, cfg=None):
    return [RL.LogEnv(cfg or CFG, traces[j].offs, traces[j].cpu, traces[j].mem, traces[j].runtime,
                      capacity=capacity) for j in (range(len(traces)) if m is None else m)]


def _capacity(b):
    c = ctypes.c_int64()
    from vmp import _lib
    _lib.check(_lib.lib().vmp_reqlog_info(b._bind(), ctypes.byref(c)))
    return c.value


def _assert_log(b, lits, what=""):
    lg = b.request_log_read()
    for i, e in enumerate(lits):
        assert np.array_equal(lg.meta[i], e.meta), ("meta", what, i, lg.meta[i], e.meta)
        bad = np.flatnonzero(np.any(lg.rows[i] != e.rows, axis=1))
        assert bad.size == 0, ("rows", what, i, bad[:5], lg.rows[i][bad[:5]], e.rows[bad[:5]])
    return lg


def _heuristic_steps(b, lits, policy, steps):
    for _ in range(steps):
        _, _, _, valid, act = b.heuristic_step(policy, want_actions=True, want_valid=True)
        valid, act = valid.cpu().numpy(), act.cpu().numpy()
        for i, e in enumerate(lits):
            _, _, _, v = e.step(act[i])
            assert np.array_equal(v, valid[i]), ("valid", i)


# ------------------------------------------------- 1: generated traces, heuristics
@pytest.mark.parametrize("kind", ["drops", "burst", "short", "empty", "churn", "burst200"])
@pytest.mark.parametrize("policy", ["firstfit", "bestfit"])
def test_generated_traces_vs_literal(kind, policy):
    traces = _workload(kind)
    b = _env(traces)
    b.request_log()
    cap = _capacity(b)
    assert cap == max(1, max(t.requests for t in traces))
    lits = _lits(traces, cap)
    _assert_log(b, lits, "start")
    done = 0
    for upto in (1, 2, 75, 150):  # the mid-run reads also show that a read changes nothing
        _heuristic_steps(b, lits, policy, upto - done)
        done = upto
        lg = _assert_log(b, lits, upto)
    ctr = b.counters().cpu().numpy()
    for i, t in enumerate(traces):
        assert lg.meta[i, 1] == t.requests and lg.meta[i, 2] == 0
        assert RL.identities(lg.rows[i], ctr[i]), i
        assert np.array_equal(ctr[i], lits[i].counters()), i
    if kind == "burst":     # 80 arrivals in one step: ranks across the row boundary, V % 64 != 0
        assert np.array_equal(lg.slot[:, :80], np.broadcast_to(np.arange(80), (4, 80)))
    if kind == "burst200":  # 90 arrivals, then 110 dropped ids: more than one wave of them
        assert np.all(lg.slot[:, 90:200] == -1) and np.all(lg.arrived[:, :200] == 1)
    if kind == "churn":
        assert np.count_nonzero(lg.is_finished & (lg.finished == lg.placed)) > 100
    b.close()


# ------------------------------------------------------- 2: random external actions
@pytest.mark.parametrize("call", ["step", "step_mask"])
def test_random_external_actions(call):
    from vmp.config import Config
    from vmp.trace import Trace
    traces = [RL.extra_traces("churn")[0], RL.extra_traces("burst200")[0],
              Trace.synthetic(Config(**dict(CFG, arrival_rate=25.0, service_length=2.0)), 150, 0),
              Trace.synthetic(Config(**dict(CFG, arrival_rate=4.0, service_length=30.0)), 40, 1)]
    b = _env(traces)
    b.request_log()
    lits = _lits(traces, _capacity(b))
    g = np.random.default_rng(7)
    mask_out = torch.empty((4, b.V, b.W), dtype=torch.int32, device=DEV) if call == "step_mask" else None
    for s in range(150):
        a = np.stack([RL.random_actions(g, e) for e in lits])
        _, _, _, valid = b.step(torch.tensor(a, dtype=torch.int32, device=DEV), mask_out=mask_out)
        valid = valid.cpu().numpy()
        for i, e in enumerate(lits):
            _, _, _, v = e.step(a[i])
            assert np.array_equal(v, valid[i]), ("valid", s, i)
    lg = _assert_log(b, lits)
    ctr = b.counters().cpu().numpy()
    for i in range(4):
        assert RL.identities(lg.rows[i], ctr[i]), i
        assert lg.meta[i, 1] == ctr[i, 0] == traces[i].requests
    assert np.all(ctr[:, 2] > 20) and int(lg.suspends.sum()) == int(ctr[:, 2].sum())
    b.close()


# ---------------------------------------------------------------- 3: RNG workload
@pytest.mark.parametrize("policy", ["firstfit", "bestfit"])
def test_rng_workload(policy):
    from vmp.batched import BatchedVmEnv
    ref = _ref(policy, "wr")
    traces = _traces(policy, "wr")  # what every oracle env accepted, drops as fillers
    cap = max(1, max(t.requests for t in traces))
    b = BatchedVmEnv(_config("wr"), N, seeds=SEEDS, device=DEV)
    b.set_workload(LAM, LEN)
    with pytest.raises(ValueError):
        b.request_log()  # an RNG env must pass a capacity
    b.request_log(capacity=cap)
    lits = _lits(traces, cap)
    for t in range(200):
        _, _, _, _, act = b.heuristic_step(policy, want_actions=True)
        assert np.array_equal(act.cpu().numpy(), ref["act"][t]), t
        for i, e in enumerate(lits):
            e.step(ref["act"][t, i])
    lg = _assert_log(b, lits)
    ctr = b.counters().cpu().numpy()
    assert np.array_equal(ctr, ref["ctr"][199])
    for i in range(N):
        assert RL.identities(lg.rows[i], ctr[i]), i
    d = lg.dropped
    assert d.sum() > 1000 and not np.any(lg.rows[d][:, 2:])  # a dropped row: SLOT and ARRIVED only
    b.close()


# ------------------------------------------------------------- 4: fused rollout call
def test_rollout_call_and_recorder_side_by_side():
    traces = _workload("drops")
    out = {}
    for mode in ("log", "rec", "both", "single"):
        b = _env(traces)
        b.eval(True)
        b.reset()
        if mode in ("rec", "both"):
            b.record(True)
        if mode != "rec":
            b.request_log()
        if mode == "single":
            for _ in range(111):
                b.heuristic_step("bestfit")
        else:
            for _ in range(3):
                b.rollout("bestfit", 37)
        lg = b.request_log_read() if mode != "rec" else None
        out[mode] = (lg, b.record_summary() if mode in ("rec", "both") else None)
        b.close()
    for mode in ("log", "both"):
        assert np.array_equal(out[mode][0].rows, out["single"][0].rows), mode
        assert np.array_equal(out[mode][0].meta, out["single"][0].meta), mode
    np.testing.assert_equal(out["both"][1], out["rec"][1])
    assert np.all(out["single"][0].meta[:, 1] == [t.offs[111] for t in traces])


# ------------------------------------------------------------------ 5: block kernel
def test_block_kernel_forced(monkeypatch):
    traces = _workload("burst")
    monkeypatch.setenv("VMP_BIG_KERNEL", "1")
    b = _env(traces)
    monkeypatch.delenv("VMP_BIG_KERNEL")
    b.request_log()
    lits = _lits(traces, _capacity(b))
    _heuristic_steps(b, lits, "firstfit", 100)
    _assert_log(b, lits)
    b.close()


def test_block_kernel_large_v_burst():
    """A real V > 1024 handle whose first step carries 1 100 requests (the
    traces of tests/test_gpu_trace.test_block_kernel_large_v_burst): 18 rows of
    64 slots, the last one partial."""
    from vmp.config import Config
    from vmp.trace import Trace
    cfg = dict(BASE, pms=20, vms=1100, reward_function="wr", arrival_rate=8.0, service_length=6.0)
    rng = np.random.default_rng(3)
    traces = []
    for i in range(4):
        t = Trace.synthetic(Config(**cfg), 40, seed=i)
        n0 = 1100 if i < 2 else 700
        burst = (rng.integers(1, 101, n0), rng.integers(1, 101, n0), rng.integers(1, 9, n0))
        traces.append(Trace(np.r_[0, t.offs + n0], np.r_[burst[0], t.cpu], np.r_[burst[1], t.mem],
                            np.r_[burst[2], t.runtime]))
    b = _env(traces, cfg=cfg)
    b.request_log()
    lits = _lits(traces, _capacity(b), cfg=cfg)
    _heuristic_steps(b, lits, "firstfit", 30)
    lg = _assert_log(b, lits)
    assert np.array_equal(lg.slot[0, :1100], np.arange(1100))
    b.close()


# ---------------------------------------------------------------------- 6: capacity
def test_capacity_smaller_than_the_trace():
    from vmp import _lib
    traces = _workload("drops")
    assert all(t.requests > 300 for t in traces)
    b = _env(traces)
    b.request_log(capacity=100)
    lits = _lits(traces, 100)
    _heuristic_steps(b, lits, "firstfit", 150)
    lg = _assert_log(b, lits)
    assert np.array_equal(lg.lost, [t.requests - 100 for t in traces])
    # read into the prefix of a larger poisoned buffer: nothing lands past row 99 of the last env
    n = 4 * 100 * 6
    buf = torch.full((n + 4096,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    meta = torch.full((4 * 3 + 64,), -7, dtype=torch.int64, device=DEV)
    _lib.check(_lib.lib().vmp_reqlog_read(b._bind(), _lib.ptr(buf), _lib.ptr(meta)))
    buf, meta = buf.cpu().numpy(), meta.cpu().numpy()
    assert np.array_equal(buf[:n].reshape(4, 100, 6), lg.rows) and np.all(buf[n:] == 0x5A5A5A5A)
    assert np.array_equal(meta[:12].reshape(4, 3), lg.meta) and np.all(meta[12:] == -7)
    # the env itself is as an unlogged one
    twin = _env(traces)
    for _ in range(150):
        twin.heuristic_step("firstfit")
    assert torch.equal(twin.obs(), b.obs()) and torch.equal(twin.counters(), b.counters())
    twin.close()
    b.close()


# ------------------------------------------- 7: enable mid-run, masked reset, restore
def test_enable_mid_run_masked_reset_restore():
    traces = _workload("churn")
    b = _env(traces)
    cap = max(t.requests for t in traces)
    lits = _lits(traces, cap)
    _heuristic_steps(b, lits, "firstfit", 60)
    b.request_log()
    for e in lits:
        e.log_start()
    _heuristic_steps(b, lits, "firstfit", 30)
    lg = _assert_log(b, lits, "mid-run")
    first = [int(t.offs[60]) for t in traces]
    assert np.array_equal(lg.meta[:, 0], first) and min(first) > 0
    for i, f in enumerate(first):  # earlier ids unobserved, the VMs then present never logged
        assert np.all(lg.slot[i, :f] == -2) and np.all(lg.slot[i, f:traces[i].offs[90]] > -2)
    mask = torch.zeros(4, dtype=torch.uint8)
    mask[3] = 1
    b.reset(torch.full((4,), 99, dtype=torch.int64), mask=mask)
    lits[3].reset()
    _assert_log(b, lits, "after reset")
    _heuristic_steps(b, lits, "firstfit", 30)
    lg = _assert_log(b, lits, "reset env 3")  # lits[3] is a fresh run since its reset
    assert np.array_equal(lg.meta[3], [0, traces[3].offs[30], 0])
    assert np.array_equal(lg.rows[3, :traces[3].offs[30], RL.ARRIVED],
                          np.repeat(np.arange(30), traces[3].arrivals()[:30]) + 1)
    assert np.array_equal(lg.meta[:3, 0], first[:3])
    snap = b.snapshot()
    b.restore(snap)
    for e in lits:
        e.log_start()
    _assert_log(b, lits, "restored")
    _heuristic_steps(b, lits, "firstfit", 20)
    _assert_log(b, lits, "after restore")
    b.request_log(False)
    from vmp._lib import VmpError
    with pytest.raises(VmpError):
        b.request_log_read()
    b.close()


# ------------------------------------------------------------------ 8: failure paths
def test_failure_paths():
    from vmp import _lib
    L = _lib.lib()
    traces = _workload("churn")
    b, twin = _env(traces), _env(traces)
    h = b._bind()
    live = L.vmp_debug_live_allocs()
    assert L.vmp_reqlog_read(h, None, None) == ESTATE
    assert L.vmp_reqlog_enable(h, -1) == EINVAL
    assert L.vmp_reqlog_enable(h, 1 << 62) == EINVAL       # the byte size does not fit
    assert L.vmp_reqlog_enable(h, 1 << 31) == EINVAL       # ids are int32
    assert L.vmp_reqlog_enable(None, 10) == EINVAL
    assert L.vmp_reqlog_info(h, None) == EINVAL
    assert L.vmp_reqlog_enable(h, 0) == 0                  # off while off
    for recorder, n_alloc in ((False, 6), (True, 4)):      # rows, ids, prev, meta (, act, valid)
        if recorder:
            b.record(True)
        base = L.vmp_debug_live_allocs()
        for nth in range(1, n_alloc + 1):
            _lib.check(L.vmp_debug_fail_alloc(nth))
            rc = L.vmp_reqlog_enable(h, 500)
            _lib.check(L.vmp_debug_fail_alloc(0))
            assert rc == EOOM, (recorder, nth, rc)
            assert L.vmp_debug_live_allocs() == base and _capacity(b) == 0
            assert L.vmp_reqlog_read(h, None, None) == ESTATE
        _lib.check(L.vmp_debug_fail_alloc(n_alloc + 1))    # one more than it makes: succeeds
        assert L.vmp_reqlog_enable(h, 500) == 0
        _lib.check(L.vmp_debug_fail_alloc(0))
        assert L.vmp_debug_live_allocs() == base + n_alloc and _capacity(b) == 500
        # a failed re-enable leaves the log it had
        _lib.check(L.vmp_debug_fail_alloc(2))
        assert L.vmp_reqlog_enable(h, 700) == EOOM
        _lib.check(L.vmp_debug_fail_alloc(0))
        assert L.vmp_debug_live_allocs() == base + n_alloc and _capacity(b) == 500
        assert L.vmp_reqlog_enable(h, 700) == 0 and _capacity(b) == 700
        assert L.vmp_debug_live_allocs() == base + n_alloc
        b.request_log(False)
        assert L.vmp_debug_live_allocs() == base and _capacity(b) == 0
    b.record(False)
    assert L.vmp_debug_live_allocs() == live
    # after all of it the env steps as an untouched twin does
    for _ in range(40):
        o1, r1, _, _, _ = b.heuristic_step("bestfit")
        o2, r2, _, _, _ = twin.heuristic_step("bestfit")
        assert torch.equal(o1, o2) and torch.equal(r1, r2)
    assert torch.equal(b.counters(), twin.counters()) and int(b.counters()[:, 0].min()) > 0
    b.close()
    twin.close()


# ------------------------------------------------------------------------- 9: graph
def test_step_graph_captured_after_enable():
    traces = _workload("drops")
    b = _env(traces)
    b.request_log()
    b.heuristic_step("firstfit")  # a launch outside the capture first
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(10):
            b.heuristic_step("firstfit")
    b.reset(torch.tensor(np.arange(4) * 4))
    for _ in range(4):
        g.replay()
    got = b.request_log_read()
    del g
    e = _env(traces)
    e.request_log()
    lits = _lits(traces, _capacity(e))
    _heuristic_steps(e, lits, "firstfit", 40)
    want = _assert_log(e, lits)
    assert np.array_equal(got.rows, want.rows) and np.array_equal(got.meta, want.meta)
    assert np.all(got.meta[:, 1] == [t.offs[40] for t in traces])
    b.close()
    e.close()


# --------------------------------------------------------------------------- 10: CLI
def test_cli_paired_requests(tmp_path, capsys):
    from vmp import exp
    from vmp.config import Config
    from vmp.trace import Trace
    busy = Config(**dict(exp.ENV100, reward_function="wr", arrival_rate=6.0, service_length=20))
    traces = [Trace.synthetic(busy, 60, seed=s) for s in (1, 2)]
    paths = [str(tmp_path / ("t%d.npz" % i)) for i in range(2)]
    for t, p in zip(traces, paths):
        t.save(p)
    out = str(tmp_path / "req.csv")
    exp.main(["paired", "--trace", ",".join(paths)])
    plain = capsys.readouterr().out
    exp.main(["paired", "--trace", ",".join(paths), "--requests", out])
    flagged = capsys.readouterr().out
    agents = ("firstfit", "bestfit")
    assert flagged.startswith(plain) and plain.count("\n") == 1 + 2 * 2
    rest = flagged[len(plain):].splitlines()
    lines = open(out).read().splitlines()
    assert lines[0] == exp.paired_requests_header(agents)
    rows = exp.paired_requests(traces, agents, device=DEV)
    assert lines[1:] == rows and len(rows) == sum(t.requests for t in traces) > 500
    assert rest[0] == exp.PAIRED_DIFF_HEADER and len(rest) == 1 + 2
    assert [r.split(",")[:3] for r in rest[1:]] == [["0", "firstfit", "bestfit"],
                                                    ["1", "firstfit", "bestfit"]]
    assert all(int(r.split(",")[3]) > 100 for r in rest[1:])  # placed under both
