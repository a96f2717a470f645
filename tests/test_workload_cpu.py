"""Host logic of the per-env workload feature (no GPU): which sweep cells merge
into one handle (vmp.exp.merge_groups) and which refuse, the load ->
arrival-rate mapping and the seeded per-episode loads of the PPO trainer."""
import numpy as np
import pytest

from vmp import exp, ppo


def _cfgs(cells, make=exp.suspension_config):
    return [dict(c.cfg) if c.cfg is not None else make(c.load, c.service_length) for c in cells]


def test_merge_groups_one_handle_per_heuristic_agent():
    """The suspension grid: per agent, every (load, service length) cell lands in
    one group, in cell order; without merge every cell is alone."""
    cells = [exp.Cell(a, 1.0, sr, (0,)) for sr in (100, 300, 500) for a in ("firstfit", "bestfit")]
    cells += [exp.Cell(a, ld, 1000, (0, 1)) for ld in (0.2, 0.6) for a in ("firstfit", "bestfit")]
    cfgs = _cfgs(cells)
    assert exp.merge_groups(cells, cfgs, merge=False) == [[i] for i in range(len(cells))]
    groups = exp.merge_groups(cells, cfgs, merge=True)
    assert groups == [[0, 2, 4, 6, 8], [1, 3, 5, 7, 9]]
    for g in groups:
        assert len({cells[i].agent for i in g}) == 1


def test_merge_groups_keeps_other_differences_and_ppo_apart():
    base = exp.suspension_config(1.0, 100)
    other_reward = dict(base, reward_function="kl")
    other_size = dict(base, vms=200)
    other_seed = dict(base, seed=7, arrival_rate=0.5, service_length=40)
    cells = [exp.Cell("firstfit", 1.0, 100, (0,), cfg=base),          # 0
             exp.Cell("firstfit", 1.0, 100, (0,), cfg=other_reward),  # 1: reward differs
             exp.Cell("firstfit", 1.0, 100, (0,), cfg=other_size),    # 2: V differs
             exp.Cell("firstfit", 0.5, 40, (3,), cfg=other_seed),     # 3: workload + seed only
             exp.Cell("ppo", 1.0, 100, (0,), "w.pt", cfg=base),       # 4
             exp.Cell("ppo", 0.5, 40, (0,), "w.pt", cfg=other_seed),  # 5
             exp.Cell("bestfit", 1.0, 100, (0,), cfg=base)]           # 6: another agent
    groups = exp.merge_groups(cells, _cfgs(cells), merge=True)
    assert groups == [[0, 3], [1], [2], [4], [5], [6]]


def test_merge_groups_refuses_unknown_agent():
    cells = [exp.Cell("roundrobin", 1.0, 100, (0,))]
    for merge in (False, True):
        with pytest.raises(ValueError):
            exp.merge_groups(cells, _cfgs(cells), merge=merge)


def test_performance_sweep_refuses_merge():
    """Its Memory Variance column needs the recorder's cross-env sums over exactly
    one cell's seeds; refused before any device work."""
    cells = [exp.performance_cell("firstfit", "firstfit", 1.0)]
    with pytest.raises(ValueError):
        exp.performance_sweep(cells, merge=True)


def test_cli_has_merge_flag(monkeypatch):
    seen = {}
    monkeypatch.setattr(exp, "suspension_sweep", lambda **kw: seen.update(kw) or [])
    exp.main(["suspension", "--merge"])
    assert seen["merge"] is True
    exp.main(["suspension"])
    assert seen["merge"] is False


def test_load_to_arrival_rate_is_the_reference_definition():
    """exp_performance.py:20-33 / exp_suspension.py:13-19 before their rounding."""
    assert ppo.load_arrival_rate(100, 1000, 1.0) == 100 / 0.55 / 1000 * 1.0
    for load in (0.2, 0.6, 1.0):
        assert round(ppo.load_arrival_rate(100, 1000, load), 4) == \
            exp.performance_config(load)["arrival_rate"]
        assert round(ppo.load_arrival_rate(100, 300, load), 3) == \
            exp.suspension_config(load, 300)["arrival_rate"]
    loads = np.array([0.25, 0.5])
    assert np.array_equal(ppo.load_arrival_rate(10, 1000, loads), 10 / 0.55 / 1000 * loads)


def test_episode_loads_seeded_and_in_range():
    a = ppo.episode_loads(1, 0, 0, 16, (0.2, 1.0))
    assert a.shape == (16,) and a.dtype == np.float64
    assert np.all(a >= 0.2) and np.all(a <= 1.0) and len(set(a)) == 16
    assert np.array_equal(a, ppo.episode_loads(1, 0, 0, 16, (0.2, 1.0)))
    assert np.array_equal(a, np.random.default_rng([1, 0, 0]).uniform(0.2, 1.0, 16))
    for other in ((2, 0, 0), (1, 1, 0), (1, 0, 1)):  # config seed, episode, rank
        assert not np.array_equal(a, ppo.episode_loads(*other, 16, (0.2, 1.0)))
    assert np.all(ppo.episode_loads(1, 0, 0, 4, (0.5, 0.5)) == 0.5)
    with pytest.raises(ValueError):
        ppo.episode_loads(1, 0, 0, 4, (1.0, 0.2))
    assert ppo.PPOConfig().load_range is None
