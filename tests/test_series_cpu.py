"""The per-step time series without a device: the literal's windows
(tests/series_literal.LiteralSeries), the host class vmp.series.Series on its
rows, the experiment CSV, the binding, and csrc/vmp_series.h under the host
sanitizers. Sums are compared bit for bit with sequential adds."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import series_literal as SL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "vm-placement-migration-gym_amd")


def _rows(n, seed=3, t0=1):
    """n made-up step rows of one env with growing counters."""
    g = np.random.default_rng(seed)
    out = []
    ctr = np.zeros(5, np.int64)
    for s in range(n):
        r = np.zeros(SL.NF)
        r[SL.STEPS] = 1.0
        r[1:SL.N_SUMMED] = g.random(SL.N_SUMMED - 1) * g.integers(1, 50)
        ctr += g.integers(0, 4, 5)
        r[SL.TIMESTEP] = t0 + s + 1
        r[SL.TOTAL_REQUESTS:SL.DROPPED + 1] = ctr
        out.append(r)
    return out


def _fold(rows, capacity, stride, t0=1):
    lit = SL.LiteralSeries(capacity, stride, t0)
    for r in rows:
        lit.add(r)
    return lit


# ------------------------------------------------------------------ the literal
def test_stride_one_rows_are_the_steps():
    rows = _rows(20)
    lit = _fold(rows, 20, 1)
    assert np.array_equal(lit.rows, np.array(rows)) and np.array_equal(lit.meta, [1, 20, 0])
    assert lit.rows_written == 20


def test_windows_partial_last_row_and_counters_of_the_last_step():
    rows = _rows(60)
    lit = _fold(rows, 10, 7)
    assert np.array_equal(lit.meta, [1, 60, 0]) and lit.rows_written == 9
    assert np.array_equal(lit.rows[:, SL.STEPS], [7] * 8 + [4, 0])
    for w in range(9):
        steps = rows[7 * w:7 * w + 7]
        acc = steps[0][:SL.N_SUMMED].copy()
        for r in steps[1:]:
            acc = acc + r[:SL.N_SUMMED]  # left to right, as the kernel adds
        assert np.array_equal(lit.rows[w, :SL.N_SUMMED], acc), w
        assert np.array_equal(lit.rows[w, SL.N_SUMMED:], steps[-1][SL.N_SUMMED:]), w
    assert not lit.rows[9].any()
    # sequential adds are not numpy's pairwise sum: the rule is the order, not the value
    assert np.allclose(lit.rows[0, 1:SL.N_SUMMED], np.sum(rows[:7], axis=0)[1:SL.N_SUMMED], rtol=1e-14)


def test_capacity_overflow_counts_lost_steps_and_restart():
    rows = _rows(60)
    lit = _fold(rows, 5, 7)
    assert np.array_equal(lit.meta, [1, 60, 25]) and lit.rows_written == 5
    want = _fold(rows[:35], 5, 7)
    assert np.array_equal(lit.rows, want.rows)
    lit.restart(61)
    assert np.array_equal(lit.meta, [61, 0, 0]) and not lit.rows.any() and lit.rows_written == 0
    lit.add(rows[0])
    assert np.array_equal(lit.rows[0], rows[0]) and np.array_equal(lit.meta, [61, 1, 0])


def test_row_of_reads_state_counters_stats_rank():
    P = 4
    state = dict(vm_placement=np.array([0, 0, 4, 5, 3, 4, 5]), vm_cpu=np.array([.5, .25, .5, 0, .75, 1., 0]),
                 vm_memory=np.array([.1, .2, .3, 0, .4, .5, 0]),
                 cpu=np.array([.75, 0., 0., .75]), memory=np.array([.3, 0., 0., .4]))
    r = SL.row_of(state, [9, 3, 1, 6, 2, 12], [0.4, 0.75, 0.375, 0, 0], 2, -0.4, P)
    assert r.tolist() == [1, -0.4, 0.4, 1.5, 0.7, np.var(state["cpu"]), np.var(state["memory"]), 0.75,
                          0.375, 2, 2, 2, 3, 12, 9, 3, 1, 6, 2]
    assert SL.target_means(state, P, True) == [0.75, 0.375]
    assert SL.target_means(dict(state, vm_cpu=state["vm_cpu"] * 2), P, True)[0] == 1.0
    assert SL.target_means(dict(state, vm_cpu=state["vm_cpu"] * 2), P, False)[0] == 1.5


# --------------------------------------------------------------- the host class
def _series(capacity=10, stride=7, n_envs=3, steps=(60, 60, 60), pm=False):
    from vmp.series import Series
    lits = [_fold(_rows(steps[i], seed=i), capacity, stride) for i in range(n_envs)]
    rows = np.stack([l.rows for l in lits])
    meta = np.stack([l.meta for l in lits])
    pmr = None
    if pm:
        pmr = np.random.default_rng(0).random((n_envs, capacity, 8)).astype(np.float32)
    return Series(rows, meta, stride, pmr), lits


def test_series_fields_means_and_bands():
    from vmp import series as S
    assert len(S.FIELDS) == S.NF == SL.NF and S.N_SUMMED == SL.N_SUMMED
    for name, k in (("steps", SL.STEPS), ("reward", SL.REWARD), ("waiting_ratio", SL.WAITING_RATIO),
                    ("cpu_sum", SL.CPU_SUM), ("mem_var", SL.MEM_VAR),
                    ("target_mem_mean", SL.TARGET_MEM_MEAN), ("used_pm", SL.USED_PM),
                    ("empty_pm", SL.EMPTY_PM), ("running", SL.RUNNING), ("timestep", SL.TIMESTEP),
                    ("dropped", SL.DROPPED)):
        assert S.FIELDS[k] == name
    ser, lits = _series(steps=(60, 60, 46))
    assert ser.n_envs == 3 and ser.capacity == 10 and ser.stride == 7
    assert np.array_equal(ser.rows_written, [9, 9, 7])
    assert np.array_equal(ser.first, [1, 1, 1]) and np.array_equal(ser.count, [60, 60, 46])
    assert np.array_equal(ser.lost, [0, 0, 0])
    assert np.array_equal(ser.cpu_sum[1], lits[1].rows[:, SL.CPU_SUM])
    m = ser.mean("cpu_sum")
    assert np.array_equal(m[0, :8], lits[0].rows[:8, SL.CPU_SUM] / 7)
    assert m[0, 8] == lits[0].rows[8, SL.CPU_SUM] / 4 and np.isnan(m[0, 9]) and np.isnan(m[2, 7])
    assert np.array_equal(ser.mean("served"), ser.served) and np.array_equal(ser.mean("steps"), ser.steps)
    mean, std = ser.band("reward")   # the rows all three envs wrote
    assert mean.shape == std.shape == (7,)
    assert np.array_equal(mean, ser.mean("reward")[:, :7].mean(axis=0))
    assert np.array_equal(std, ser.mean("reward")[:, :7].std(axis=0))
    one = ser.env(2)
    assert one.n_envs == 1 and np.array_equal(one.rows[0], lits[2].rows)
    assert ser.pm_cpu is None and ser.pm_mem is None
    with pytest.raises(ValueError):
        S.Series(np.zeros((1, 4, 5)), np.zeros((1, 3), np.int64))
    with pytest.raises(ValueError):
        S.Series(ser.rows, ser.meta, 0)


def test_series_npz_and_csv_round_trip(tmp_path):
    from vmp.series import Series
    ser, lits = _series(capacity=5, pm=True)
    assert np.array_equal(ser.lost, [25, 25, 25]) and np.array_equal(ser.rows_written, [5, 5, 5])
    assert ser.pm_cpu.shape == ser.pm_mem.shape == (3, 5, 4)
    assert np.array_equal(np.concatenate([ser.pm_cpu, ser.pm_mem], axis=2), ser.pm)
    p = str(tmp_path / "s.npz")
    ser.save(p)
    back = Series.load(p)
    assert np.array_equal(back.rows, ser.rows) and np.array_equal(back.meta, ser.meta)
    assert back.stride == 7 and np.array_equal(back.pm, ser.pm) and back.pm.dtype == np.float32
    text = ser.to_csv(str(tmp_path / "s.csv"))
    assert open(str(tmp_path / "s.csv")).read() == text
    lines = text.splitlines()
    assert lines[0] == Series.CSV_HEADER == "Env,Window," + ",".join(__import__("vmp.series").series.FIELDS)
    assert len(lines) == 1 + 15
    for line in lines[1:]:
        c = line.split(",")
        i, r = int(c[0]), int(c[1])
        assert np.array_equal(np.array([float(x) for x in c[2:]]), lits[i].rows[r])  # repr reads back
    none, _ = _series(capacity=5)
    p2 = str(tmp_path / "n.npz")
    none.save(p2)
    assert Series.load(p2).pm is None


def test_experiment_csv_rows_are_numpy_over_the_envs():
    import vmp.exp as exp
    ser, _ = _series(steps=(60, 60, 60))
    rows = exp.series_rows(4, "bestfit", ser)
    hdr = exp.series_header().split(", ")
    assert hdr[:5] == ["Cell", "Agent", "Envs", "Window", "Timestep"] and len(rows) == 9
    assert len(hdr) == 5 + 2 * 17 and "timestep Mean" not in hdr
    for r, line in enumerate(rows):
        c = line.split(",")
        assert len(c) == len(hdr)
        assert c[:4] == ["4", "bestfit", "3", str(r)] and int(c[4]) == int(ser.timestep[0, r])
        for k in range(5, len(hdr), 2):
            name = hdr[k][:-len(" Mean")]
            assert hdr[k + 1] == name + " Std"
            m = ser.mean(name)[:, r]
            assert float(c[k]) == m.mean() and float(c[k + 1]) == m.std(), (r, name)


# ------------------------------------------------------------------ binding, CLI
def test_header_declares_and_binding_types_the_calls():
    import ctypes
    from vmp import _lib
    hdr = open(os.path.join(ROOT, "include", "vmp.h")).read()
    assert re.search(r"#define VMP_ABI_VERSION 14\b", hdr)
    for name, decl in (
            ("vmp_series_enable",
             "int vmp_series_enable(vmp_handle *h, int64_t capacity, int32_t stride, int32_t pm_rows);"),
            ("vmp_series_info",
             "int vmp_series_info(const vmp_handle *h, int64_t *capacity, int32_t *stride, int32_t *pm_rows);"),
            ("vmp_series_read", "int vmp_series_read(vmp_handle *h, double *rows, float *pm, int64_t *meta);")):
        assert name in _lib.EXPORTS and decl in hdr
    for k, name in enumerate(("STEPS", "REWARD", "WAITING_RATIO", "CPU_SUM", "MEM_SUM", "CPU_VAR", "MEM_VAR",
                              "TARGET_CPU_MEAN", "TARGET_MEM_MEAN", "USED_PM", "EMPTY_PM", "WAITING",
                              "RUNNING", "TIMESTEP", "TOTAL_REQUESTS", "SERVED", "SUSPEND", "PLACE",
                              "DROPPED", "NF")):
        assert re.search(r"#define VMP_SR_%s %d\b" % (name, k), hdr)
        assert getattr(SL, name) == k
    for k, name in enumerate(("FIRST", "COUNT", "LOST", "NMETA")):
        assert re.search(r"#define VMP_SR_%s %d\b" % (name, k), hdr)
        assert getattr(SL, name) == k
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libvmp.so is not built")
    L = _lib.lib()
    P = ctypes.c_void_p
    assert L.vmp_series_enable.argtypes == [P, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]
    assert L.vmp_series_info.argtypes == [P, P, P, P]
    assert L.vmp_series_read.argtypes == [P, P, P, P]
    assert all(f.restype == ctypes.c_int for f in (L.vmp_series_enable, L.vmp_series_info,
                                                   L.vmp_series_read))
    # no device is touched by a null handle
    assert L.vmp_series_enable(None, 10, 1, 0) == -1 and L.vmp_series_read(None, None, None, None) == -1
    assert L.vmp_series_info(None, None, None, None) == -1


def test_exp_cli_parses_series():
    import vmp.exp as exp
    ap = exp.arg_parser()
    for sub in ("suspension", "performance", "performance_small", "vm_size", "reward", "migration_ratio",
                "paired"):
        a = ap.parse_args([sub, "--series", "o.csv", "--series-stride", "25"])
        assert a.series == "o.csv" and a.series_stride == 25
        a = ap.parse_args([sub])
        assert a.series is None and a.series_stride == 1
    with pytest.raises(SystemExit):
        exp.main(["suspension", "--series", "o.csv", "--series-stride", "0"])
    with pytest.raises(ValueError):
        exp._series_request((0, "o.csv"))
    assert exp._series_request(None) is None and exp._series_request((3, "x")) == (3, "x")


# --------------------------------------------- vmp_series.h under sanitizers
def test_series_sizes_under_asan_ubsan():
    e = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
             UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run(["make", "-s", "-C", PKG, "series-sizes"], cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    p = subprocess.run([os.path.join(PKG, "build", "san", "series_sizes")], cwd=ROOT, env=e,
                       capture_output=True, text=True, timeout=600)
    out = p.stdout + p.stderr
    assert p.returncode == 0, out[-4000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
    assert "0 violations" in out and "series sizes ok" in out, out[-4000:]
