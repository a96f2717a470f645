"""The device recorder (vmp_record_*, csrc/vmp_record.hip) on the GPU against a
ground truth of its own, tests/record_truth.RecEnv: a literal env that knows
its arrivals from its own _accept and keeps the Record traces itself, so
nothing the device reads back enters the truth. The test's seeded actions
(suspension-heavy: reqlog_literal.random_actions) go to the device and to the
literal alike; validity flags are compared every step, state and counters at
the end, so a recorder mismatch cannot be an env mismatch. hist and the
integer-valued sums must be bit-exact, the floating sums within the derived
bound of record_truth.judge. Shapes: the smallest on
either side of each border in k_record (record_truth.CASES)."""
import warnings

import numpy as np
import pytest
import torch

from tests import record_truth as R
from tests.trace_literal import STATE_KEYS

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu_and_print_ratios():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    R.RATIOS.clear()
    yield
    print("\n| quantity | |device - truth| at the worst ratio | its bound | max error / bound |")
    print("|---|---|---|---|")
    for name in [R.NAMES[k] for k in R.BOUNDED]:
        err, bound, ratio = R.RATIOS.get(name, (0.0, 0.0, 0.0))
        print(f"| {name} | {err:.3e} | {bound:.3e} | {ratio:.3f} |")


def _handle(c, traces, record=True):
    from vmp.batched import BatchedVmEnv
    from vmp.config import Config
    n = c["N"]
    b = BatchedVmEnv(Config(**R.case_cfg(c)), n, seeds=np.arange(n, dtype=np.int64) * 4, device=DEV)
    b.set_trace(traces, np.arange(n))
    b.eval(True)
    b.reset()
    if record:
        b.record(True)
    return b


def _drive(b, r, lo, hi, want_valid=True, mask_out=None):
    """Steps lo .. hi - 1 of the run r on the device -> the device's rewards [hi - lo, N]."""
    rewards = []
    for s in range(lo, hi):
        a = torch.tensor(r.acts[s], dtype=torch.int32, device=DEV)
        _, rw, _, valid = b.step(a, want_valid=want_valid, mask_out=mask_out)
        if want_valid:
            assert np.array_equal(valid.cpu().numpy(), r.valids[s]), ("valid", s)
        rewards.append(rw.cpu().numpy())
    return rewards


def _same_env(b, envs):
    st = {k: v.cpu().numpy() for k, v in b.state().items()}
    ctr = b.counters().cpu().numpy()
    for i, e in enumerate(envs):
        assert np.array_equal(ctr[i], e.counters()), ("counters", i, ctr[i], e.counters())
        for k, x in zip(STATE_KEYS, e.state()):
            assert np.array_equal(st[k][i], x), (k, i)


def _read(b):
    hist, sums = b.record_read()
    return hist.cpu().numpy().view(np.uint32), sums.cpu().numpy()


def _judge(b, c, envs, rewards, what, **kw):
    hist, sums = _read(b)
    truth = R.handle_raw(envs, np.array(rewards).reshape(-1, c["N"]), **kw)
    bad = []
    for i in range(c["N"]):
        bad += R.judge(hist[i], sums[i], truth[i], c["P"], c["V"], c["N"], f"{what} env {i}")
    for line in bad:
        print(line)
    assert not bad, bad[:4]
    return hist, sums


def _bits(hist, sums):
    return hist.tobytes(), sums.tobytes()


# ------------------------------------------------------------------ the case table
@pytest.mark.parametrize("name", list(R.CASES))
def test_case_against_the_truth(name):
    r = R.run_case(name)
    c = r.case
    b = _handle(c, r.traces)
    rewards = _drive(b, r, 0, c["steps"])
    _same_env(b, r.envs)
    _, sums = _judge(b, c, r.envs, rewards, name)
    if name == "cross-N65":
        assert not sums[:, R.XMEM].any()
    if name == "cross-N64":
        assert sums[:, R.XMEM].all()
    dev = b.record_summary()
    for i, e in enumerate(r.envs):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)  # means of nothing: the empty trace
            lit = e.summary()
        assert not R.summary_mismatch(dev[i], lit, e.exact_means()), (name, i)
    b.close()


# ---------------------------------------------------- further tests: 12 / 90, N 5, mixed
READS = (1, 2, 60, 120)


@pytest.fixture(scope="module")
def baseline():
    """The FURTHER case recorded once and read once: (hist, sums) bits and the rewards."""
    r = R.run_case(R.FURTHER, READS)
    b = _handle(r.case, r.traces)
    rewards = _drive(b, r, 0, r.case["steps"])
    out = _bits(*_read(b)), rewards
    b.close()
    return out


def test_read_is_non_destructive(baseline):
    r = R.run_case(R.FURTHER, READS)
    c = r.case
    b = _handle(c, r.traces)
    rewards, done = [], 0
    for upto in READS:
        rewards += _drive(b, r, done, upto)
        done = upto
        for _ in range(2):  # and a second read of the same step sees the same
            got = _judge(b, c, r.snaps[upto], rewards, f"read after {upto}")
    assert _bits(*got) == baseline[0]
    b.close()


@pytest.mark.parametrize("how", ["scratch_valid", "step_mask"])
def test_caller_or_scratch_buffers(how, baseline):
    """want_valid=False: the recorder steps on the handle's scratch validity
    buffer; mask_out: the step goes through vmp_step_mask."""
    r = R.run_case(R.FURTHER, READS)
    b = _handle(r.case, r.traces)
    mask_out = None
    if how == "step_mask":
        mask_out = torch.empty((r.case["N"], b.V, b.W), dtype=torch.int32, device=DEV)
    _drive(b, r, 0, r.case["steps"], want_valid=how != "scratch_valid", mask_out=mask_out)
    assert _bits(*_read(b)) == baseline[0]
    b.close()


def test_heuristic_paths():
    """heuristic_step with actions and flags requested feeds the literal and is
    judged against the truth; heuristic_step with nothing requested (the
    recorder on its scratch buffers) and one rollout call give the same bits."""
    c = R.CASES[R.FURTHER]
    traces = R.case_traces(c)
    envs = R.make_envs(c, traces)
    b = _handle(c, traces)
    rewards = []
    for s in range(c["steps"]):
        _, rw, _, valid, act = b.heuristic_step("bestfit", want_actions=True, want_valid=True)
        valid, act = valid.cpu().numpy(), act.cpu().numpy()
        rewards.append(rw.cpu().numpy())
        for i, e in enumerate(envs):
            assert np.array_equal(e.step(act[i])[3], valid[i]), ("valid", s, i)
    _same_env(b, envs)
    want = _bits(*_judge(b, c, envs, rewards, "heuristic_step"))
    b.close()
    for how in ("nothing requested", "rollout"):
        b = _handle(c, traces)
        if how == "rollout":
            b.rollout("bestfit", c["steps"])
        else:
            for _ in range(c["steps"]):
                b.heuristic_step("bestfit")
        assert _bits(*_read(b)) == want, how
        b.close()


def test_recorder_beside_the_other_observers(baseline):
    r = R.run_case(R.FURTHER, READS)
    b = _handle(r.case, r.traces)
    b.request_log()
    b.series(capacity=r.case["steps"])
    _drive(b, r, 0, r.case["steps"])
    assert _bits(*_read(b)) == baseline[0]
    b.close()


# ------------------------------------------------------------- reset and restore
def test_masked_reset_restarts_the_recorder_of_the_envs_it_resets():
    """Envs 1 and 3 are reset by mask after 40 steps: their recorder restarts
    (prev from the reset state, no open lives, zero hist and sums) and equals a
    truth restarted there; envs 0, 2 and 4 equal their truth over all 100
    steps. tests/test_record_truth_cpu.py holds that some reset slot stood at
    WAIT and takes an arrival in the next step."""
    r = R.run_reset()
    c = r.case
    b = _handle(c, r.traces)
    rewards = _drive(b, r, 0, R.RESET_AT)
    mask = torch.zeros(c["N"], dtype=torch.uint8)
    mask[list(R.RESET_ENVS)] = 1
    b.reset(torch.arange(c["N"], dtype=torch.int64), mask=mask)
    rewards += _drive(b, r, R.RESET_AT, R.RESET_STEPS)
    _same_env(b, r.envs)
    _, sums = _judge(b, c, r.envs, rewards, "masked reset", mem=r.mem, first=r.first)
    assert np.array_equal(sums[:, R.STEPS], [R.RESET_STEPS - f for f in r.first])
    b.close()


def test_restore_restarts_every_recorder():
    """Snapshot before step 20, restore before step 50: every recorder starts
    again from the restored state. A VM present then has no arrival in the
    record; k_record_init documents that its life starts with length 0 and
    grows from the next step (RecEnv.record_start). The reference has no such
    case (it records from reset), so only hist and sums, as the kernel header
    defines them, are compared here, not the summary."""
    r = R.run_restore()
    c = r.case
    b = _handle(c, r.traces)
    _drive(b, r, 0, R.SNAP_AT)
    snap = b.snapshot()
    _drive(b, r, R.SNAP_AT, R.RESTORE_AT)
    b.restore(snap)
    rewards = _drive(b, r, R.RESTORE_AT, R.RESTORE_STEPS)
    _same_env(b, r.envs)
    _, sums = _judge(b, c, r.envs, rewards, "restore")
    assert np.all(sums[:, R.STEPS] == R.RESTORE_STEPS - R.RESTORE_AT)
    b.close()
