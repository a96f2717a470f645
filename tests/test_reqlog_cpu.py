"""The per-request outcome log without a device: the kernel's rule
(tests/reqlog_literal.RuleLog) against the ground truth of a literal env that
knows which slot took which request (tests/reqlog_literal.LogEnv), the host
classes on hand-made arrays, the binding, and csrc/vmp_reqlog.h under the host
sanitizers. Every comparison is exact integer equality."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import reqlog_literal as RL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "vm-placement-migration-gym_amd")
BASE = dict(pms=12, vms=90, allow_null_action=True, training_steps=10000, eval_steps=100000,
            seed=0, sequence="uniform", cap_target_util=True, beta=0.5, reward_function="wr")


def _workload(kind):
    """(trace, steps to run) of the four workloads."""
    from vmp.config import Config
    from vmp.trace import Trace
    if kind == "churn":       # runtimes 1..3 at 6 arrivals per step
        return RL.extra_traces("churn")[0], 150
    if kind == "burst200":    # a 200-request first step: > 64 arrivals, > 64 drops
        return RL.extra_traces("burst200")[0], 150
    if kind == "drops":       # lambda 25 / L 2
        return Trace.synthetic(Config(**dict(BASE, arrival_rate=25.0, service_length=2.0)), 150, 0), 150
    assert kind == "short"    # a 40-step trace run for 100 steps
    return Trace.synthetic(Config(**dict(BASE, arrival_rate=4.0, service_length=30.0)), 40, 1), 100


def _run(kind, actions, capacity=None, start=0):
    """The literal under `actions`, the rule fed what the kernel would see.
    start > 0: both logs are started after that many steps."""
    tr, steps = _workload(kind)
    env = RL.LogEnv(BASE, tr.offs, tr.cpu, tr.mem, tr.runtime, capacity=capacity)
    g = np.random.default_rng(7)
    rule = lazy = None
    for s in range(steps):
        if s == start:
            env.log_start()
            rule = RL.RuleLog(env.P, env.V, env.capacity, env.vm_placement, env.total_requests)
            lazy = RL.RuleLog(env.P, env.V, env.capacity, env.vm_placement, env.total_requests,
                              open_counts=True)
        a = RL.random_actions(g, env) if actions == "random" else RL.first_fit(env)
        t = env.timestep
        _, _, _, valid = env.step(a)
        if rule is not None:
            rule.update(t, a, valid, env.vm_placement, env.total_requests)
            lazy.update(t, a, valid, env.vm_placement, env.total_requests)
            # the kernel's event-only WAIT_STEPS, closed as a read closes it, at every step
            assert np.array_equal(lazy.read(t), env.rows), s
            assert np.array_equal(lazy.meta, env.meta), s
    return tr, env, rule


@pytest.mark.parametrize("actions", ["random", "firstfit"])
@pytest.mark.parametrize("kind", ["churn", "burst200", "drops", "short"])
def test_rule_equals_ground_truth_and_counter_identities(kind, actions):
    tr, env, rule = _run(kind, actions)
    assert np.array_equal(rule.rows, env.rows)
    assert np.array_equal(rule.meta, env.meta)
    assert np.array_equal(env.meta, [0, env.total_requests, 0])
    assert env.total_requests == tr.requests > 0
    assert RL.identities(env.rows, env.counters())
    assert RL.identities(rule.rows, env.counters())
    # the ground truth itself: an accepted request's sizes and runtime are its trace entry's
    acc = np.flatnonzero(env.rows[:, RL.SLOT] >= 0)
    step_of = np.repeat(np.arange(tr.steps), tr.arrivals())
    assert np.array_equal(env.rows[:tr.requests, RL.ARRIVED], step_of + 1)
    fin = acc[env.rows[acc, RL.FINISHED] > 0]
    assert np.all(env.rows[fin, RL.PLACED] > 0)
    # runtime r, placed at p, never suspended: finished at p + r - 1
    calm = fin[env.rows[fin, RL.SUSPENDS] == 0]
    assert np.array_equal(env.rows[calm, RL.FINISHED],
                          env.rows[calm, RL.PLACED] + tr.runtime[calm].astype(np.int64) - 1)
    if kind == "churn":  # placed and finished within one step, the slot refilled at once
        assert np.count_nonzero(env.rows[fin, RL.FINISHED] == env.rows[fin, RL.PLACED]) > 50
    if kind in ("burst200", "drops"):
        assert np.count_nonzero(env.rows[:, RL.SLOT] == -1) > 64
    if actions == "random":
        assert env.suspend_action > 20


@pytest.mark.parametrize("kind", ["churn", "drops"])
def test_rule_with_a_capacity_and_a_late_start(kind):
    tr, env, rule = _run(kind, "random", capacity=100, start=0)
    assert np.array_equal(rule.rows, env.rows) and np.array_equal(rule.meta, env.meta)
    assert env.meta[RL.LOST] == tr.requests - 100 > 0
    tr, env, rule = _run(kind, "random", start=40)
    assert np.array_equal(rule.rows, env.rows) and np.array_equal(rule.meta, env.meta)
    first = int(env.meta[RL.FIRST])
    assert first == tr.offs[40] > 0 and np.all(env.rows[:first, RL.SLOT] == -2)
    assert np.all(env.rows[first:tr.requests, RL.SLOT] > -2)


# ------------------------------------------------------------- host classes
def _hand_log():
    from vmp.reqlog import RequestLog
    #        slot arrived placed finished suspends wait
    rows = np.array([[[3, 1, 2, 5, 0, 1],      # placed in the next step, finished at 5
                      [-1, 1, 0, 0, 0, 0],     # dropped
                      [0, 2, 5, 9, 1, 6],      # waited 3, suspended once for 3 steps
                      [7, 3, 0, 0, 0, 4],      # still waiting
                      [2, 4, 5, 0, 0, 1],      # running
                      [-2, 0, 0, 0, 0, 0]]], np.int32)
    return RequestLog(rows, np.array([[0, 5, 0]], np.int64))


def test_request_log_columns():
    lg = _hand_log()
    assert lg.n_envs == 1 and lg.capacity == 6
    assert np.array_equal(lg.slot[0], [3, -1, 0, 7, 2, -2])
    assert np.array_equal(lg.dropped[0], [0, 1, 0, 0, 0, 0])
    assert np.array_equal(lg.accepted[0], [1, 0, 1, 1, 1, 0])
    assert np.array_equal(lg.is_placed[0], [1, 0, 1, 0, 1, 0])
    assert np.array_equal(lg.is_finished[0], [1, 0, 1, 0, 0, 0])
    assert np.array_equal(lg.pending_steps[0], [1, -1, 3, -1, 1, -1])
    assert np.array_equal(lg.suspended_steps[0], [0, -1, 3, -1, 0, -1])
    assert np.array_equal(lg.sojourn[0], [4, -1, 7, -1, -1, -1])
    e = lg.env(0)
    assert e.capacity == 5 and np.array_equal(e.rows[0], lg.rows[0, :5])
    text = lg.to_csv()
    lines = text.splitlines()
    assert lines[0] == "Env,Request,slot,arrived,placed,finished,suspends,wait_steps"
    assert lines[1:] == ["0,0,3,1,2,5,0,1", "0,1,-1,1,0,0,0,0", "0,2,0,2,5,9,1,6",
                         "0,3,7,3,0,0,0,4", "0,4,2,4,5,0,0,1"]
    late = type(lg)(lg.rows, np.array([[2, 4, 0]], np.int64)).env(0)
    assert np.array_equal(late.rows[0], lg.rows[0, 2:4])
    with pytest.raises(ValueError):
        type(lg)(np.zeros((1, 4, 5), np.int32), np.zeros((1, 3), np.int64))


def test_paired_requests_and_differences_on_hand_made_logs(tmp_path):
    import vmp.exp as exp
    from vmp.reqlog import RequestLog
    from vmp.trace import Trace
    tr = Trace([0, 2, 3, 4, 5], [10, 20, 30, 40, 50], [11, 21, 31, 41, 51], [3, 4, 5, 6, 7])
    a = _hand_log()
    rows_b = a.rows.copy()
    rows_b[0, 0] = [5, 1, 4, 7, 0, 3]      # placed two steps later, finished two later
    rows_b[0, 1] = [6, 1, 2, 0, 0, 1]      # not dropped under B
    rows_b[0, 2] = [0, 2, 4, 8, 0, 2]      # placed a step earlier, never suspended
    rows_b[0, 3] = [-1, 3, 0, 0, 0, 0]     # dropped under B only
    b = RequestLog(rows_b, a.meta)
    logs = {"firstfit": a, "bestfit": b}
    rows = exp.paired_requests([tr], ("firstfit", "bestfit"), logs=logs)
    assert rows == ["0,0,0,10,11,3,3,2,5,0,1,5,4,7,0,3",
                    "0,1,0,20,21,4,-1,0,0,0,0,6,2,0,0,1",
                    "0,2,1,30,31,5,0,5,9,1,6,0,4,8,0,2",
                    "0,3,2,40,41,6,7,0,0,0,4,-1,0,0,0,0",
                    "0,4,3,50,51,7,2,5,0,0,1,2,5,0,0,1"]
    hdr = exp.paired_requests_header(("firstfit", "bestfit"))
    assert len(hdr.split(",")) == len(rows[0].split(",")) == 16
    # placed under both: requests 0, 2, 4 with pending 1-3, 3-2, 1-1; finished under both:
    # 0 and 2 with sojourn 4-6 and 7-6
    diff = exp.paired_differences([tr], ("firstfit", "bestfit"), logs)
    assert diff == ["0,firstfit,bestfit,3,-0.333,0.000,1,1,2,-0.500"]
    assert len(exp.PAIRED_DIFF_HEADER.split(",")) == len(diff[0].split(","))
    one = exp.paired_differences([tr], ("firstfit",), logs)
    assert one == []
    none = RequestLog(np.array(RL.empty_rows(5))[None], np.array([[0, 0, 0]], np.int64))
    assert exp.paired_differences([tr], ("x", "y"), {"x": none, "y": a}) == \
        ["0,x,y,0,nan,nan,0,1,0,nan"]


# ------------------------------------------------------------------ binding
def test_header_declares_and_binding_types_the_calls():
    import ctypes
    from vmp import _lib
    hdr = open(os.path.join(ROOT, "include", "vmp.h")).read()
    assert re.search(r"#define VMP_ABI_VERSION 14\b", hdr)
    for name, decl in (("vmp_reqlog_enable", "int vmp_reqlog_enable(vmp_handle *h, int64_t capacity);"),
                       ("vmp_reqlog_info", "int vmp_reqlog_info(const vmp_handle *h, int64_t *capacity);"),
                       ("vmp_reqlog_read", "int vmp_reqlog_read(vmp_handle *h, int32_t *rows, int64_t *meta);")):
        assert name in _lib.EXPORTS and decl in hdr
    for k, name in enumerate(("SLOT", "ARRIVED", "PLACED", "FINISHED", "SUSPENDS", "WAIT_STEPS", "NF")):
        assert re.search(r"#define VMP_RQ_%s %d\b" % (name, k), hdr)
        assert getattr(RL, name) == k
    for k, name in enumerate(("FIRST", "NEXT", "LOST", "NMETA")):
        assert re.search(r"#define VMP_RQ_%s %d\b" % (name, k), hdr)
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libvmp.so is not built")
    L = _lib.lib()
    P = ctypes.c_void_p
    assert L.vmp_reqlog_enable.argtypes == [P, ctypes.c_int64]
    assert L.vmp_reqlog_info.argtypes == [P, P]
    assert L.vmp_reqlog_read.argtypes == [P, P, P]
    assert all(f.restype == ctypes.c_int for f in (L.vmp_reqlog_enable, L.vmp_reqlog_info,
                                                   L.vmp_reqlog_read))
    # no device is touched by a null handle
    assert L.vmp_reqlog_enable(None, 10) == -1 and L.vmp_reqlog_read(None, None, None) == -1


# --------------------------------------------- vmp_reqlog.h under sanitizers
def test_reqlog_sizes_under_asan_ubsan():
    e = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
             UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run(["make", "-s", "-C", PKG, "reqlog-sizes"], cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    p = subprocess.run([os.path.join(PKG, "build", "san", "reqlog_sizes")], cwd=ROOT, env=e,
                       capture_output=True, text=True, timeout=600)
    out = p.stdout + p.stderr
    assert p.returncode == 0, out[-4000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
    assert "0 violations" in out and "reqlog sizes ok" in out, out[-4000:]
