"""The call sequences of tests/seq_cases.py on the model alone (no GPU): they
are not vacuous. Every number below is a condition the generator was tuned to
meet, never the other way round; DESIGN.md §5.4 lists what each (case, seed)
reaches. tests/test_gpu_sequences.py walks the device through the same lists."""
import collections
import functools
import time

import numpy as np
import pytest

from tests import seq_cases as S

PAIRS = [(c, s) for c in S.CASES for s in S.SEQ_SEEDS]
IDS = ["%s-%d" % (c.name, s) for c, s in PAIRS]


@functools.lru_cache(maxsize=None)
def _run(case, seed):
    """-> (ops, model after the run, per-op record, seconds of the model run)."""
    ops = S.gen_ops(case, seed)
    t0 = time.perf_counter()
    m, rec = S.run_model(case, ops)
    return ops, m, rec, time.perf_counter() - t0


def _same(x, y):
    if isinstance(x, dict):
        return x.keys() == y.keys() and all(_same(x[k], y[k]) for k in x)
    if isinstance(x, (tuple, list)):
        return len(x) == len(y) and all(_same(a, b) for a, b in zip(x, y))
    x, y = np.asarray(x), np.asarray(y)
    if x.dtype.kind == "f":  # bit for bit, NaN included
        return x.shape == y.shape and np.array_equal(x.astype(np.float64).view(np.uint64),
                                                     y.astype(np.float64).view(np.uint64))
    return np.array_equal(x, y)


@pytest.mark.parametrize("case,seed", PAIRS, ids=IDS)
def test_every_sequence_goes_everywhere(case, seed):
    ops, m, _, secs = _run(case, seed)
    main = m.h[0]
    print("%s-%d: %d ops, %d env-steps per env, model run %.2f s, stats %s, counters moved (min "
          "over envs: place suspend served dropped) %s"
          % (case.name, seed, len(ops), main.stats["env_steps"] // main.n, secs,
             {k: int(v) for k, v in main.stats.items()}, main.moved[:, [3, 2, 1, 4]].min(axis=0)))
    count = collections.Counter(op["op"] for op in ops)
    for kind in case.kinds():
        assert count[kind] >= 3, (kind, count[kind])
    assert main.stats["env_steps"] // main.n <= 1500
    # every env's placement, suspension, served and dropped counters move under its steps
    assert np.all(main.moved[:, [3, 2, 1, 4]] > 0), main.moved
    assert main.stats["done_training"] >= 1
    assert main.stats["refused"] >= 3 and main.stats["imported"] >= 10, main.stats
    assert secs < 30.0, secs  # it has to stay in seconds
    if case.name in ("A", "D"):
        share = main.stats["bare_idle"] / main.stats["bare_steps"]
        assert share >= 0.10, share
    if case.name == "C":
        assert main.stats["last_row_accept"] >= 1 and main.stats["bestfit_tie"] >= 1, main.stats


@pytest.mark.parametrize("case", S.CASES, ids=[c.name for c in S.CASES])
def test_every_hand_over_occurs(case):
    """The three seeds of a case together: every mutator directly before every
    launch kind; every mutator while the series and the request log are on;
    cases A and D: the two hand-overs around the idle path."""
    follow, observed = set(), set()
    dangerous = opposite = 0
    for seed in S.SEQ_SEEDS:
        ops, m, _, _ = _run(case, seed)
        series = reqlog = False
        for k, op in enumerate(ops):
            kind = op["op"]
            if kind in ("series_on", "series_off"):
                series = kind == "series_on"
            if kind in ("reqlog_on", "reqlog_off"):
                reqlog = kind == "reqlog_on"
            if kind in case.mutators():
                if series and reqlog:
                    observed.add(kind)
                if k + 1 < len(ops):
                    follow.add((kind, ops[k + 1]["op"]))
        dangerous += m.h[0].stats["dangerous"]
        opposite += m.h[0].stats["opposite"]
    missing = [(mu, la) for mu in case.mutators() for la in S.LAUNCHES if (mu, la) not in follow]
    assert not missing, missing
    assert observed == set(case.mutators()), set(case.mutators()) - observed
    if case.name in ("A", "D"):
        # idle at its last per-step launch, written into a state where something can
        # happen, then a bare launch; and the other way round
        assert dangerous >= 10 and opposite >= 10, (dangerous, opposite)


@pytest.mark.parametrize("case,seed", PAIRS, ids=IDS)
def test_replay_gives_identical_model_outputs(case, seed):
    ops, m, rec, _ = _run(case, seed)
    ops2 = S.gen_ops(case, seed)
    assert len(ops) == len(ops2) and all(_same(a, b) for a, b in zip(ops, ops2))
    m2, rec2 = S.run_model(case, ops2)
    for k, (a, b) in enumerate(zip(rec, rec2)):
        assert _same(a, b), (k, ops[k]["op"])
    assert _same(m.final(), m2.final())


@pytest.mark.parametrize("case,seed", PAIRS, ids=IDS)
def test_model_restore_equals_never_having_run(case, seed):
    """After a restore the main handle's state, counters, stats and ranks are
    those right after the snapshot, whatever ran in between, and what it
    returns from there on is what a model returns that went from the snapshot
    straight to the ops after the restore."""
    ops, _, rec, _ = _run(case, seed)
    snaps = [k for k, op in enumerate(ops) if op["op"] == "snapshot"]
    checked = 0
    for j, op in enumerate(ops):
        if op["op"] != "restore":
            continue
        i = max(k for k in snaps if k < j)
        assert _same(rec[i][1], rec[j][1]), (i, j)
        checked += any(o["op"] in S.LAUNCHES for o in ops[i + 1:j])  # steps were taken back
    assert checked >= 1
    # the continuation: ops i+1 .. j left out, for the last pair that has no op between
    # them touching what a snapshot does not hold (eval mode, workload, start state,
    # the second handle, the observers)
    outside = ("eval", "set_workload", "set_start_state", "set_start_none", "branch_into_second",
               "h2_step") + S.OBSERVERS
    for j in reversed([k for k, op in enumerate(ops) if op["op"] == "restore"]):
        i = max(k for k in snaps if k < j)
        if any(o["op"] in outside for o in ops[i + 1:j]):
            continue
        m3 = S.Model(case)
        for op in ops[:i + 1]:
            m3.apply(op)
        for k in range(j + 1, min(j + 6, len(ops))):
            if ops[k]["op"] in ("series_read", "reqlog_read"):
                break  # the observers restarted at the restore: their rows differ
            assert _same(m3.apply(ops[k]), rec[k][0]), (i, j, k)
            assert _same(m3.h[0].observe(), rec[k][1]), (i, j, k)
        break


def test_cli_prints_the_op_list(capsys):
    assert S.main(["--case", "A", "--seed", "2", "--upto", "9", "--short"]) == 0
    lines = capsys.readouterr().out.splitlines()
    ops = S.gen_ops(S.BY_NAME["A"], 2)
    assert len(lines) == 10 and all(ln.split()[1].startswith(op["op"] + "(")
                                    for ln, op in zip(lines, ops))
