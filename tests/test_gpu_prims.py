"""The device's restatements of numpy, one by one (MI355X): PCG64 seeding,
stepping and jumping, random_poisson in its serial and its lane-parallel form,
the pairwise sum through every plan, and the scalar introsort in its three
forms, reached through the test-only library vmp/libvmp_prims.so
(csrc/vmp_prims.hip wraps the headers the env kernels include; it restates
nothing). Every comparison is exact: integers and f64 bit patterns.

Judges: the C oracle's entry points for the RNG and the sorts (pinned to numpy
on the CPU by tests/test_oracle.py and tests/golden/rng_kat.npz); np.sum of a
contiguous float64 array, and oracle_pw_sum, for the sums. np.argsort is no
judge: numpy's SIMD sorts order ties differently from the scalar introsort the
reference ran."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import prims_cases as C
from tests import test_sort_model_cpu as SM
from tests import traj as T

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KAT = np.load(os.path.join(T.GOLDEN, "rng_kat.npz"))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")


@functools.lru_cache(None)
def plib():
    import vmp
    path = os.path.join(os.path.dirname(os.path.abspath(vmp.__file__)), "libvmp_prims.so")
    assert os.path.exists(path), f"{path} is missing: make -C vm-placement-migration-gym_amd"
    L = ctypes.CDLL(path)
    P, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    sig = {
        "vmp_prims_last_error": (ctypes.c_char_p, []),
        "vmp_prims_pcg_seed": (ctypes.c_int, [i32, P, P]),
        "vmp_prims_pcg_draws": (ctypes.c_int, [i32, P, P, i32, P, P]),
        "vmp_prims_poisson": (ctypes.c_int, [i32, i32, P, P, P, P, i32, P, P, P]),
        "vmp_prims_pw_sum": (ctypes.c_int, [i32, i32, P, i64, P, P, i32, P]),
        "vmp_prims_sort": (ctypes.c_int, [i32, i32, P, P, i64, P, P, i64, P, i64, P]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
    return L


def ok(rc):
    assert rc == 0, plib().vmp_prims_last_error().decode()


def dev(a):
    """numpy array -> device tensor of the same bytes (unsigned types as signed)."""
    a = np.ascontiguousarray(a)
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint16): np.int16}.get(a.dtype)
    return torch.from_numpy(a.view(signed) if signed else a).to(DEV)


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


def u64(xs):
    return np.array([int(x) for x in xs], np.uint64)


# ------------------------------------------------------------------- RNG ----
def test_seed_matches_oracle():
    seeds = u64(list(KAT["seeds"]) + list(C.EXTRA_SEEDS))
    out = torch.zeros((len(seeds), 4), dtype=torch.int64, device=DEV)
    dseeds = dev(seeds)  # every device input stays referenced until its call returns
    ok(plib().vmp_prims_pcg_seed(len(seeds), ptr(dseeds), ptr(out)))
    got = host(out, np.uint64)
    exp = np.zeros(4, np.uint64)
    for i, s in enumerate(seeds):
        O.lib().oracle_pcg_seed(int(s), O._p(exp))
        assert np.array_equal(got[i], exp), int(s)
    assert np.array_equal(got[:len(KAT["seeds"])], KAT["state_inc"])

    z = torch.zeros(len(seeds), dtype=torch.int64, device=DEV)
    raw = torch.zeros((len(seeds), 8), dtype=torch.int64, device=DEV)
    dbl = torch.zeros((len(seeds), 8), dtype=torch.float64, device=DEV)
    ok(plib().vmp_prims_pcg_draws(len(seeds), ptr(dseeds), ptr(z), 8, ptr(raw), ptr(dbl)))
    raw, dbl = host(raw, np.uint64), host(dbl, np.uint64)
    er, ed = np.zeros(8, np.uint64), np.zeros(8)
    for i, s in enumerate(seeds):
        O.lib().oracle_pcg_raw(int(s), 8, O._p(er))
        O.lib().oracle_pcg_double(int(s), 8, O._p(ed))
        assert np.array_equal(raw[i], er), int(s)
        assert np.array_equal(dbl[i], ed.view(np.uint64)), int(s)


def test_advance_matches_oracle_and_stepping():
    seeds, deltas = [], []
    for s in (0, 7, 2**40 + 3, 2**63 - 1):
        for d in C.ADVANCE_DELTAS:
            seeds.append(s)
            deltas.append(d)
    n = len(seeds)
    raw = torch.zeros((n, 8), dtype=torch.int64, device=DEV)
    dbl = torch.zeros((n, 8), dtype=torch.float64, device=DEV)
    dseeds, ddeltas = dev(u64(seeds)), dev(u64(deltas))
    ok(plib().vmp_prims_pcg_draws(n, ptr(dseeds), ptr(ddeltas), 8, ptr(raw), ptr(dbl)))
    raw, dbl = host(raw, np.uint64), host(dbl, np.uint64)
    for i, (s, d) in enumerate(zip(seeds, deltas)):
        assert int(raw[i, 0]) == O.lib().oracle_pcg_advance_raw(s, d), (s, d)
        if d <= 1000:
            er, ed = np.zeros(d + 8, np.uint64), np.zeros(d + 8)
            O.lib().oracle_pcg_raw(s, d + 8, O._p(er))
            O.lib().oracle_pcg_double(s, d + 8, O._p(ed))
            assert np.array_equal(raw[i], er[d:]), (s, d)
            assert np.array_equal(dbl[i], ed[d:].view(np.uint64)), (s, d)


# --------------------------------------------------------------- Poisson ----
def _poisson_cases(force_tab):
    """(seed, offset, lam) of every case; force_tab: the PTRS rates only."""
    lams = [l for l in C.POISSON_LAMS if l >= 10] if force_tab else list(C.POISSON_LAMS)
    return [(s, o, l) for l in lams for s in C.POISSON_SEEDS for o in C.POISSON_OFFSETS]


@functools.lru_cache(None)
def _poisson_oracle(force_tab):
    """Per case: the oracle's draws i64 [nd], states u64 [nd][2], the raw draw after."""
    cases = _poisson_cases(force_tab)
    nd = C.POISSON_DRAWS
    draws = np.zeros((len(cases), nd), np.int64)
    states = np.zeros((len(cases), nd, 2), np.uint64)
    after = np.zeros(len(cases), np.uint64)
    for i, (s, o, l) in enumerate(cases):
        after[i] = O.lib().oracle_pcg_poisson_at(s, o, float(l), nd, O._p(draws[i]),
                                                 O._p(states[i]))
    # the offset-0 cases through the entry point the KATs pin
    for i, (s, o, l) in enumerate(cases):
        if o == 0:
            d0 = np.zeros(nd, np.int64)
            a0 = O.lib().oracle_pcg_poisson(s, float(l), nd, O._p(d0))
            assert np.array_equal(d0, draws[i]) and a0 == int(after[i])
    return draws, states, after


def _run_poisson(parallel, force_tab):
    cases = _poisson_cases(force_tab)
    n, nd = len(cases), C.POISSON_DRAWS
    seeds = dev(u64([c[0] for c in cases]))
    offs = dev(u64([c[1] for c in cases]))
    lams = dev(np.array([c[2] for c in cases], np.float64))
    tabn = dev(np.full(n, 1 if force_tab else 0, np.int32))
    draws = torch.zeros((n, nd), dtype=torch.int64, device=DEV)
    states = torch.zeros((n, nd, 2), dtype=torch.int64, device=DEV)
    after = torch.zeros(n, dtype=torch.int64, device=DEV)
    ok(plib().vmp_prims_poisson(int(parallel), n, ptr(seeds), ptr(offs), ptr(lams), ptr(tabn), nd,
                                ptr(draws), ptr(states), ptr(after)))
    return host(draws, np.int64), host(states, np.uint64), host(after, np.uint64)


def _first_bad(cases, got, exp):
    bad = np.flatnonzero((got != exp).reshape(len(cases), -1).any(axis=1))
    if len(bad) == 0:
        return None
    i = int(bad[0])
    j = int(np.flatnonzero((got[i] != exp[i]).reshape(got.shape[1], -1).any(axis=1))[0])
    return len(bad), cases[i], "draw", j, got[i, j].tolist(), exp[i, j].tolist()


@pytest.mark.parametrize("force_tab", [False, True], ids=["table", "loggam_far"])
def test_poisson_serial_matches_oracle(force_tab):
    """poisson() from every offset: draws, the state after every draw and the
    raw draw that follows equal the oracle's. loggam_far: the table length is
    forced to 1, so every k that reaches the log test takes the device's own
    loggam."""
    cases = _poisson_cases(force_tab)
    ed, es, ea = _poisson_oracle(force_tab)
    gd, gs, ga = _run_poisson(False, force_tab)
    assert _first_bad(cases, gd, ed) is None, _first_bad(cases, gd, ed)
    assert _first_bad(cases, gs, es) is None, _first_bad(cases, gs, es)
    assert np.array_equal(ga, ea)


@pytest.mark.parametrize("force_tab", [False, True], ids=["table", "loggam_far"])
def test_poisson_parallel_matches_serial(force_tab):
    """ParRng / par_fill / par_poisson / par_state started 0, 1, 2, 31, 62, 63,
    64, 65 and 127 raw draws into the stream (so the chunk borders fall at
    every phase of a draw): draw by draw and state by state the serial form's,
    and the oracle's."""
    cases = _poisson_cases(force_tab)
    ed, es, _ = _poisson_oracle(force_tab)
    sd, ss, _ = _run_poisson(False, force_tab)
    gd, gs, _ = _run_poisson(True, force_tab)
    assert _first_bad(cases, gd, sd) is None, _first_bad(cases, gd, sd)
    assert _first_bad(cases, gs, ss) is None, _first_bad(cases, gs, ss)
    assert np.array_equal(gd, ed) and np.array_equal(gs, es)


def test_poisson_ptrs_cases_reach_the_log_test():
    """Not vacuous: in every PTRS case some (U, V) pair among the first
    POISSON_DRAWS pairs (each draw consumes at least one) passes neither
    squeeze and reaches the log test, i.e. the loggam table or loggam_far."""
    npairs = C.POISSON_DRAWS
    for s, o, l in _poisson_cases(True):
        if o != 0:
            continue
        u = np.zeros(2 * npairs)
        O.lib().oracle_pcg_double(s, 2 * npairs, O._p(u))
        U, V = u[0::2] - 0.5, u[1::2]
        slam = np.sqrt(l)
        b = 0.931 + 2.53 * slam
        a = -0.059 + 0.02483 * b
        vr = 0.9277 - 3.6224 / (b - 2)
        us = 0.5 - np.abs(U)
        k = np.floor((2 * a / us + b) * U + l + 0.43)
        fast = (us >= 0.07) & (V <= vr)
        reject = (k < 0) | ((us < 0.013) & (V > us))
        assert int((~fast & ~reject).sum()) > 0, (s, l)


# ---------------------------------------------------------- pairwise sum ----
@functools.lru_cache(None)
def _pw_expected(family):
    pool = C.pw_values(family)
    cases = C.pw_cases()
    exp = np.zeros(len(cases))
    for i, (off, n) in enumerate(cases):
        a = np.ascontiguousarray(pool[off:off + n])
        exp[i] = np.sum(a)
        o = O.lib().oracle_pw_sum(O._p(a), n)
        assert np.float64(o).view(np.uint64) == exp[i:i + 1].view(np.uint64)[0], (family, off, n)
    return pool, cases, exp


@pytest.mark.parametrize("cap", [10240, 24577])
@pytest.mark.parametrize("family", C.PW_FAMILIES)
@pytest.mark.parametrize("rd", [4, 6])
def test_pairwise_sum_matches_numpy(rd, family, cap):
    """wave_pw_sum<rd> equals np.sum bit for bit at the direct loop, one leaf,
    around both register plans' caps (1928, 7688), in the LDS plan and across
    numpy's buffers of 8192 elements, at non-zero offsets. cap: the size the
    LDS plan's arrays are carved for (10240: the largest V a handle takes)."""
    pool, cases, exp = _pw_expected(family)
    keep = [i for i, (_, n) in enumerate(cases) if n <= cap]
    off = np.array([cases[i][0] for i in keep], np.int32)
    n = np.array([cases[i][1] for i in keep], np.int32)
    out = torch.zeros(len(keep), dtype=torch.float64, device=DEV)
    dpool, doff, dn = dev(pool), dev(off), dev(n)
    ok(plib().vmp_prims_pw_sum(rd, len(keep), ptr(dpool), len(pool), ptr(doff), ptr(dn), cap,
                               ptr(out)))
    got = host(out, np.uint64)
    want = exp[keep].view(np.uint64)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, [(int(n[i]), int(off[i]), got[i:i + 1].view(np.float64)[0],
                            want[i:i + 1].view(np.float64)[0]) for i in bad[:8]]


def test_mixed_summands_show_a_wrong_order():
    """The mixed family tells addition orders apart: a plain left-to-right
    sum differs from np.sum at most sizes above the direct loop."""
    pool, cases, exp = _pw_expected("mixed")
    differs = 0
    big = [(i, c) for i, c in enumerate(cases) if c[1] >= 120]
    for i, (off, n) in big:
        acc = 0.0
        for x in pool[off:off + n].tolist():
            acc += x
        differs += acc != exp[i]
    assert differs >= len(big) // 2, (differs, len(big))


# ------------------------------------------------------------------ sort ----
def _oracle_order(keys):
    out = np.zeros(len(keys), np.int64)
    O.lib().oracle_argsort_f32(O._p(np.ascontiguousarray(keys, np.float32)), len(keys), O._p(out))
    return out


@functools.lru_cache(None)
def _sort_cases():
    """Every (n, pattern) of the sort tests: name, key offset into the pool,
    keys, the oracle's order, the (lo, hi) ranges. -> (pool f32, list)."""
    sets, pool, off = [], [], 0
    for n in C.SORT_N:
        pats = C.sort_patterns(n)
        if n >= 129:
            pats["adversary"] = SM.adversary_keys(n)
        for name, keys in pats.items():
            order = _oracle_order(keys)
            sets.append((f"{name}-{n}", off, keys, order, C.sort_ranges(keys[order])))
            pool.append(keys)
            off += n
    return np.concatenate(pool), sets


def _run_sort(form, ka, kb, rows, fit=None):
    """rows: (key_off, n, lo, hi, fit_off) -> order slices (forms 0, 1; list of
    arrays) or sel i32 [cases][2] (form 2)."""
    cs = np.zeros((len(rows), 6), np.int32)
    out_off = 0
    for i, (ko, n, lo, hi, fo) in enumerate(rows):
        cs[i] = (ko, n, lo, hi, fo, out_off)
        out_off += hi - lo + 1
    assert out_off < 2**31
    dka, dkb, dcs = dev(ka), (None if kb is None else dev(kb)), dev(cs)
    if form == 2:
        sel = torch.full((len(rows), 2), -7, dtype=torch.int32, device=DEV)
        dfit = dev(fit)
        ok(plib().vmp_prims_sort(2, len(rows), ptr(dka), ptr(dkb), len(ka), ptr(dcs), ptr(dfit),
                                 len(fit), None, 0, ptr(sel)))
        return sel.cpu().numpy()
    out = torch.full((out_off,), -1, dtype=torch.int16, device=DEV)
    ok(plib().vmp_prims_sort(form, len(rows), ptr(dka), ptr(dkb), len(ka), ptr(dcs), None, 0,
                             ptr(out), out_off, None))
    return host(out, np.uint16), cs[:, 5]


def _check_orders(form, ka, kb, sets):
    rows, exp, tags = [], [], []
    for name, off, keys, order, ranges in sets:
        for lo, hi in ranges:
            rows.append((off, len(keys), lo, hi, 0))
            exp.append(order[lo:hi + 1])
            tags.append((name, lo, hi))
    got, out_off = _run_sort(form, ka, kb, rows)
    want = np.concatenate(exp).astype(np.uint16)
    if not np.array_equal(got, want):
        first = int(np.flatnonzero(got != want)[0])
        i = int(np.searchsorted(out_off, first, side="right") - 1)
        seg = slice(int(out_off[i]), int(out_off[i]) + len(exp[i]))
        raise AssertionError((form, tags[i], got[seg][:16].tolist(), want[seg][:16].tolist()))


@pytest.mark.parametrize("form", [0, 1], ids=["aquicksort_lds", "wave_aquicksort"])
def test_sort_ranges_match_oracle(form):
    """Positions lo..hi of the device's order equal the oracle's full order
    there: the full range (where the forms thereby agree with each other),
    single positions, every tie block and random ranges, for few distinct
    values, all equal, ascending, descending, organ pipe, random keys and the
    adversary's order that ends in the depth limit's heapsort."""
    pool, sets = _sort_cases()
    _check_orders(form, pool, None, sets)


def test_select_top_matches_oracle():
    """wave_aqselect_top: the highest position in [lo, hi] whose element fits,
    read from the oracle's order, for fit bitmaps of density 0 (-> -1), only
    the lowest member of the range, only the highest, and random ones."""
    pool, sets = _sort_cases()
    rng = np.random.default_rng(5)
    rows, exp, tags, fits, foff = [], [], [], [], 0

    def add_fit(f):
        nonlocal foff
        fits.append(f)
        foff += len(f)
        return foff - len(f)

    for name, off, keys, order, ranges in sets:
        n = len(keys)
        shared = [add_fit(np.zeros(n, np.uint8)),
                  add_fit((rng.random(n) < 0.3).astype(np.uint8)),
                  add_fit((rng.random(n) < 2.0 / n).astype(np.uint8))]
        for lo, hi in ranges:
            own = []
            for pos in (lo, hi):
                f = np.zeros(n, np.uint8)
                f[order[pos]] = 1
                own.append(add_fit(f))
            for kind, fo in zip(("none", "random", "sparse", "lowest", "highest"), shared + own):
                rows.append((off, n, lo, hi, fo))
                tags.append((name, lo, hi, kind))
    fit = np.concatenate(fits)
    assert len(fit) < 2**31
    # expected, from the oracle's order
    by_off = {off: order for _, off, _, order, _ in sets}
    for off, n, lo, hi, fo in rows:
        order = by_off[off]
        hit = np.flatnonzero(fit[fo:fo + n][order[lo:hi + 1]])
        exp.append((lo + int(hit[-1]), int(order[lo + int(hit[-1])])) if len(hit) else (-1, -1))
    sel = _run_sort(2, pool, None, rows, fit)
    want = np.array(exp, np.int32)
    bad = np.flatnonzero((sel != want).any(axis=1))
    assert len(bad) == 0, (len(bad), [(tags[i], sel[i].tolist(), want[i].tolist()) for i in bad[:8]])
    assert (want[:, 0] == -1).any() and (want[:, 0] >= 0).any()


def test_keysum_sort_matches_oracle():
    """wave_aquicksort over KeySum (the f32 sum of two rows formed at each
    read, BestFit's keys): the judge sorts the f32 sum formed in numpy."""
    rng = np.random.default_rng(9)
    sets, pa, pb, off = [], [], [], 0
    for n in C.SORT_N:
        for name, hi in (("loads", 101), ("coarse", 4)):
            a = (rng.integers(0, hi, n) / np.float64(hi - 1)).astype(np.float32)
            b = (rng.integers(0, hi, n) / np.float64(hi - 1)).astype(np.float32)
            keys = a + b  # f32 + f32, rounded to f32
            assert keys.dtype == np.float32
            order = _oracle_order(keys)
            sets.append((f"{name}-{n}", off, keys, order, C.sort_ranges(keys[order])))
            pa.append(a)
            pb.append(b)
            off += n
    _check_orders(1, np.concatenate(pa), np.concatenate(pb), sets)
