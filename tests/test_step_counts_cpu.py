"""The cases of tests/test_gpu_step_counts.py are not vacuous (oracle only).

The wave env kernels derive a step's VM counts from its events (DESIGN.md
§3.1, "Counts from events"). Every walk the GPU test compares with must
therefore hold, at least MIN_OCCURRENCES env-steps each:

  finisher / no_finisher   steps with and without a finishing VM
  placed_no_finisher       accepted placements, no finisher (no per-slot loop
                           in _run_vms, but words switch representation)
  leaves_null              a NULL slot is left (the hint's bit 32)
  fills_last_null          requests accepted and no NULL slot left (n_null == k)
  arrivals_over_nulls      arrivals > n_null > 0
  pad_rows_matter          V is no multiple of 64 and VMs wait: counting the
                           padded rows as VMs would change the waiting ratio
  carried_wait             VMs wait after the step (the carried n_w is not 0)
  suspension / rejected_placement   external walks only

The two P100 / V1000 cases cannot run out of NULL slots within 400 steps
(tests/step_counts_cases.py); they are held to every other class."""
import pytest

from tests import step_counts_cases as S


@pytest.mark.parametrize("mode", ("heur", "ext"))
@pytest.mark.parametrize("policy", S.POLICIES)
@pytest.mark.parametrize("case", S.CASES, ids=[c.name for c in S.CASES])
def test_walk_holds_every_class(case, policy, mode):
    assert case.steps <= 400
    assert case.steps >= 2 * sum(S.ROLLS)  # the fused drive passes each launch length twice
    cl = S.classes(S.walk(case, policy, "wr", mode))
    for name in S.required(case, mode):
        assert cl[name] >= S.MIN_OCCURRENCES, (case.name, policy, mode, name, cl)
    if mode == "heur":
        assert cl["suspension"] == 0  # heuristic launches suspend nothing


def test_cases_are_the_specified_ones():
    shapes = {(c.P, c.V) for c in S.CASES}
    assert shapes == {(10, 30), (20, 64), (20, 65), (100, 1000), (50, 1024)}
    lams = sorted(c.lam for c in S.CASES if (c.P, c.V) == (100, 1000))
    assert lams == [0.182, 1.8182]
    assert [c.exhausts for c in S.CASES if c.V == 1000] == [False, False]
    assert all(c.exhausts for c in S.CASES if c.V != 1000)
    assert any(s > 1 << 32 for s in S.SEEDS) and len(S.SEEDS) == S.N_ENV == 6


@pytest.mark.parametrize("name", S.TRACE_CASES)
def test_trace_variant_replays_what_the_walk_accepted(name):
    case = S.BY_NAME[name]
    w = S.walk(case, "firstfit", "wr", "heur", want_trace=True)
    for i, (offs, cpu, mem, rt) in enumerate(w.traces):
        assert len(offs) == case.steps + 1 and offs[-1] == w.ctr[-1, i, 0]
        assert len(cpu) == len(mem) == len(rt) == offs[-1]
