"""Cases shared by the tests of the numpy primitives (the oracle's on the CPU,
tests/test_oracle.py; the device's, tests/test_gpu_prims.py): the sizes at
which the pairwise sum changes plan, two families of summands, the seeds,
jumps and rates of the RNG tests, and the key patterns of the sort tests."""
import numpy as np

# ---- pairwise sum -----------------------------------------------------------
# the direct loop (< 8), one leaf (<= 128), the first splits, the register
# plans' caps (1928 for depth 4, 3848, 7688 for depth 6), numpy's buffer of
# 8192 elements, and sizes of two, three and four buffers
PW_N = (list(range(0, 41)) + list(range(120, 138)) + list(range(248, 265)) +
        list(range(1016, 1033)) + list(range(1920, 1937)) + list(range(3840, 3857)) +
        list(range(7680, 7697)) + list(range(8184, 8201)) +
        [10000, 10239, 10240, 16384, 16385, 24577])
PW_FAMILIES = ("hundredths", "mixed")
PW_POOL = 24577 + 64  # summands per family: every case is a slice of one array


def pw_values(family, n=PW_POOL, seed=11):
    """n float64 summands. hundredths: k/100, k in 1..100 (what the envs add);
    mixed: magnitudes from 1e-8 to 1e8 and both signs, so that the order of
    the additions shows in the last bits."""
    rng = np.random.default_rng(seed)
    if family == "hundredths":
        return rng.integers(1, 101, n) / 100.0
    return rng.uniform(-1, 1, n) * 10.0 ** rng.integers(-8, 9, n)


def pw_cases():
    """(offset, n) into a PW_POOL array: every n of PW_N once, at an offset
    that is non-zero and no multiple of 8 except for a few at 0."""
    cases = []
    for i, n in enumerate(PW_N):
        cases.append((0 if i % 7 == 0 else 1 + (i * 5) % 61, n))
    assert all(o + n <= PW_POOL for o, n in cases)
    return cases


# ---- RNG ----------------------------------------------------------------------
EXTRA_SEEDS = (0, 1, 2**32 - 1, 2**32, 2**32 + 3, 2**40 + 11, 2**63 - 1)
ADVANCE_DELTAS = (0, 1, 2, 63, 64, 65, 1000, 2**32 - 1, 2**32, 2**63, 2**64 - 1)
POISSON_LAMS = (0, 1e-3, 0.0182, 0.3, 1.8182, 4, 9.99, 10.0, 10.000001, 12, 25, 100, 1000,
                2000, 9500)
POISSON_SEEDS = (0, 7, 2**40 + 11)
POISSON_OFFSETS = (0, 1, 2, 31, 62, 63, 64, 65, 127)
POISSON_DRAWS = 2048

# ---- sort -----------------------------------------------------------------------
SORT_N = (1, 2, 15, 16, 17, 18, 63, 64, 65, 127, 128, 129, 130, 200, 1000, 1024, 4000)


def sort_patterns(n, seed=0):
    """name -> float32 keys [n] (the adversarial order comes from
    tests/test_sort_model_cpu.py: adversary_keys)."""
    rng = np.random.default_rng(1000 + 17 * n + seed)
    i = np.arange(n)
    pipe = np.minimum(i, n - 1 - i)
    return {
        "few3": (rng.integers(0, 3, n) / 4).astype(np.float32),
        "few6": (rng.integers(0, 6, n) / 8).astype(np.float32),
        "equal": np.full(n, 0.75, np.float32),
        "asc": (i / 8).astype(np.float32),
        "desc": ((n - 1 - i) / 8).astype(np.float32),
        "pipe": (pipe / 8).astype(np.float32),
        "random": rng.random(n, dtype=np.float32),
    }


def tie_blocks(sorted_keys):
    """(lo, hi) of every maximal run of equal keys in an ascending key array."""
    n = len(sorted_keys)
    if n == 0:
        return []
    cut = np.flatnonzero(np.diff(sorted_keys) != 0) + 1
    lo = np.concatenate([[0], cut])
    hi = np.concatenate([cut - 1, [n - 1]])
    return list(zip(lo.tolist(), hi.tolist()))


def sort_ranges(sorted_keys, seed=0, n_random=6):
    """The (lo, hi) ranges of one sort case: the full range, single positions
    at both ends and the middle, every tie block, and random ranges."""
    n = len(sorted_keys)
    rng = np.random.default_rng(77 + n + seed)
    r = [(0, n - 1), (0, 0), (n - 1, n - 1), (n // 2, n // 2)]
    r += [b for b in tie_blocks(sorted_keys) if b[1] > b[0]]
    for _ in range(n_random):
        lo = int(rng.integers(0, n))
        r.append((lo, int(rng.integers(lo, n))))
    return list(dict.fromkeys(r))
