"""Cases, exact operands and the launch plan of the bf16 fused actor head
(csrc/vmp_headgemm_bf16.hip, k_hg16<TS, BWD, 8, SMP>) for
tests/test_hg16_cases_cpu.py and tests/test_gpu_hg16_instances.py (test
infrastructure: numpy and CPU torch, importable without a GPU).

1. plan(B, V, A): csrc/vmp_hg16_plan.h in Python (held against the native
   program tests/native/hg16_plan.cpp by the CPU test).

2. Exact operands. The bf16 kernels have no logits_out, so the reference must
   know the logits the kernel forms exactly, or MFMA summation order would
   decide SAMPLE boundaries and eat the 4 e_ref rule. h, W and the bias are
   built so that every partial sum of b + h W^T is a multiple of 2^-7 below
   2^9 — exact in f32 in any order:
     dense block  K0 columns, h in {-1, -1/2, 0, 1/2, 1}, W in {k/64, |k| <= 8}
                  (products: multiples of 2^-7, their absolute sum <= K0 / 8);
     one-hot      h[b, K0 + b] = 1, W[n, K0 + b] = the target logit of sample b
                  rounded to a multiple of 2^-7 and then to bf16 (|.| < 256);
     bias         multiples of 2^-7, |b| <= 1/2;
     K            K0 + B rounded up to a multiple of 64.
   The targets are head_cases' given_case / sample_case / wait_case (reused
   unchanged), SAMPLE rows with an argmax_case-style duplicated maximum whose
   two columns share their dense W rows and bias, so the tie is exact in the
   final logits too.

3. CASES, each naming what it selects (Case.selects()).
"""
import functools
from dataclasses import dataclass

import numpy as np
import torch

from tests import head_cases as C
from tests import head_ref as R

BM, MAX_NT, TEAM = 256, 14, 8   # kHg16BM, kHg16MaxNT, kHg16Team
GRAIN = 2.0 ** -7               # every operand product and partial sum is a multiple of it
LIMIT = 2.0 ** 9                # ... and below this: 16 bits, exact in f32
PEAK_MARGIN, WAIT_MARGIN = 50.0, 10.0


# ---------------------------------------------------------------------- plan
def pick_ts(A):
    return (A + 15) // 16


def _fullest(n_units, unit_wg, limit, pad8):
    """The r in 1..limit (at most 64) whose grid has the fullest last round of
    256 workgroups; the first one past 0.97 ends the search."""
    best, best_eff = 1, -1.0
    for r in range(1, min(limit, 64) + 1):
        units = n_units * r
        wg = (units + 7) // 8 * 8 * unit_wg if pad8 else units * unit_wg
        eff = (units * unit_wg) / (((wg + 255) // 256) * 256.0)
        if eff > best_eff + 1e-9:
            best, best_eff = r, eff
        if eff > 0.97:
            break
    return best


def tile_of(p, b):
    """hg16_tile: block indices b -> (column tile, first M block, live)."""
    b = np.asarray(b, np.int64)
    if p["team"] > 0:
        i = b >> 3
        T = (i // p["team"]) * 8 + (b & 7)
        live = T < p["teams"]
        n_tile, g = T % p["n_tiles"], (T // p["n_tiles"]) * p["team"] + i % p["team"]
    else:
        live = np.ones(b.shape, bool)
        n_tile, g = b % p["n_tiles"], b // p["n_tiles"]
    return n_tile, g, live & (g < p["m_blocks"])


def plan(B, V, A):
    """hg16_plan + hg16_bwd_workspace of csrc/vmp_hg16_plan.h, and the number of
    padding blocks of the grid (blocks hg16_tile sends home)."""
    TS = pick_ts(A)
    S = MAX_NT // TS
    p = dict(B=B, V=V, A=A, TS=TS, S=S, n_tiles=(V + S - 1) // S, m_blocks=(B + BM - 1) // BM, team=0, teams=0)
    if p["m_blocks"] >= TEAM:
        r = _fullest(p["n_tiles"], TEAM, p["m_blocks"] // TEAM, True)
        p.update(team=TEAM, teams=p["n_tiles"] * r, m_groups=TEAM * r)
        p["grid"] = (p["teams"] + 7) // 8 * 8 * TEAM
    else:
        p["m_groups"] = _fullest(p["n_tiles"], 1, p["m_blocks"], False)
        p["grid"] = p["n_tiles"] * p["m_groups"]
    p["padding"] = int((~tile_of(p, np.arange(p["grid"]))[2]).sum())
    p["workspace"] = max(1, min(p["m_blocks"], 512)) * V * A
    return p


PLAN_FIELDS = ("B", "V", "A", "TS", "S", "n_tiles", "m_blocks", "team", "teams", "m_groups", "padding", "grid",
               "workspace")


def plan_line(p):
    """The line tests/native/hg16_plan.cpp prints for this plan."""
    return "plan " + " ".join(f"{k} {p[k]}" for k in PLAN_FIELDS)


# --------------------------------------------------------------------- cases
@dataclass(frozen=True)
class Case:
    name: str
    B: int
    V: int
    A: int
    K0: int = 64
    shift: float = 0.0
    ld_extra: int = 0             # backward: ld = V A + ld_extra
    bits: bool = True             # False: bits = None in every mode (no WAIT coin then)
    modes: tuple = ("given", "bwd", "sample", "wait")
    grads: tuple = ("both", "lp", "ent")  # backward runs: (g_lp, g_ent), (g_lp, None), (None, g_ent)
    counter: bool = False         # SAMPLE once more through HeadRng.graph_counter, values 0 and 1
    dense: bool = False           # ordinary random operands at K = 512 instead of exact ones
    note: str = ""

    @property
    def plan(self):
        return plan(self.B, self.V, self.A)

    @property
    def ld(self):
        return self.V * self.A + self.ld_extra

    @property
    def pair_store(self):
        """store_dl_tile's dwordx2 / dword path: A and ld both even."""
        return self.A % 2 == 0 and self.ld % 2 == 0

    def selects(self):
        """What the case launches and reaches: ("k_hg16", TS, mode) with mode
        fwd / bwd / smp, ("plan", feature), ("edge", feature)."""
        p, s = self.plan, set()
        kern = {"given": "fwd", "bwd": "bwd", "sample": "smp", "wait": "smp"}
        for m in self.modes:
            s.add(("k_hg16", p["TS"], kern[m]))
            s.add(("plan", "team" if p["team"] else "groups", kern[m]))
            if p["team"] and p["TS"] != 1:
                s.add(("plan", "team at TS > 1", kern[m]))
            if p["padding"]:
                s.add(("plan", "padding blocks", kern[m]))
            if p["m_groups"] < p["m_blocks"]:
                s.add(("plan", "walked M block", kern[m]))
            if not self.bits:
                s.add(("edge", "bits None", kern[m]))
            if self.dense:
                s.add(("edge", "dense GEMM", kern[m]))
            if self.B < 16:
                s.add(("edge", "B < 16", kern[m]))
            if self.B == 1:
                s.add(("edge", "B = 1", kern[m]))
        if "bwd" in self.modes:
            s.add("k_dsum")
            s.add(("edge", "pair store" if self.pair_store else "2-byte store"))
            if self.ld_extra:
                s.add(("edge", "ld > V A", "pair store" if self.pair_store else "2-byte store"))
            for g in self.grads:
                s.add(("edge", "grads", g))
        if p["n_tiles"] > 1 and self.V % p["S"]:
            s.add(("plan", "last tile with missing segments"))
        if self.B % BM:
            s.add(("plan", "ragged M block"))
        for name, hit in (("A = 1", self.A == 1), ("A % 16 = 0", self.A % 16 == 0), ("A % 16 = 1", self.A % 16 == 1)):
            if hit:
                s.add(("edge", name))
        if self.counter:
            s.add(("edge", "graph counter"))
        return s


# both ends of every TS's A range, an odd A, the configs' A = 12 and A = 102
TS_A = (1, 16, 17, 32, 33, 48, 49, 64, 65, 80, 81, 96, 97, 112, 113, 128, 39, 12, 102)
# A -> ld - V A of the backward: pair path with padding columns (16, 128), odd
# ld at even A (32), odd A at even ld (17, 65), odd A and odd ld (33)
_LD_EXTRA = {16: 6, 128: 6, 32: 1, 17: 6, 65: 1, 33: 6}


def _cases():
    out = []
    for i, A in enumerate(TS_A):
        TS = pick_ts(A)
        out.append(Case(f"ts{TS}-A{A}", 135, MAX_NT // TS + 1, A, K0=(64, 128)[i % 2], shift=(0.0, 20.0, -20.0)[i % 3],
                        ld_extra=_LD_EXTRA.get(A, 0), counter=A == 39,
                        note="M groups, one ragged M block, two column tiles (the second with missing segments)"))
    out += [
        Case("small-B13", 13, 5, 39, note="B < 16: h rows clamped to B - 1"),
        Case("small-B1", 1, 5, 39, ld_extra=1, note="B = 1"),
        Case("team-ts5", 2049, 3, 77, shift=20.0, note="XCD teams: 9 M blocks, m_groups 8, 6 padding teams"),
        Case("team-ts3", 4200, 9, 33, grads=("both",), ld_extra=1,
             note="XCD teams: 17 M blocks, m_groups 16, 2 padding teams"),
        Case("team-ts8", 1793, 1, 128, shift=-20.0, ld_extra=6, note="XCD teams: exactly 8 M blocks, 7 padding teams"),
        Case("groups-walk", 257, 200, 128, modes=("given", "bwd"), grads=("both",),
             note="M groups: 200 tiles, 2 M blocks, m_groups 1"),
        Case("nobits", 135, 3, 77, bits=False, modes=("given", "bwd", "sample"), note="bits = None"),
        Case("dense", 300, 5, 44, dense=True, modes=("given", "bwd", "sample"), grads=("both",),
             note="tanh(randn) h, randn 2 / sqrt(K) W at K = 512: the accumulation itself"),
    ]
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
DENSE_K = 512


# ---------------------------------------------------------------- operands
def to_bf16(x):
    """f32 / f64 array -> the nearest bf16 values as f32 (round to nearest even)."""
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.bfloat16).float().numpy()


def bf16_rne(x):
    """f64 array -> the nearest bf16 value (ties to even) as f64, rounded ONCE from
    f64: 8 significand bits, exponent floor -126 (subnormals in steps of 2^-133)."""
    x = np.asarray(x, np.float64)
    _, e = np.frexp(x)
    ulp = np.ldexp(1.0, np.maximum(e, -125) - 8)
    return np.rint(x / ulp) * ulp


def bf16_cell(s):
    """bf16 values s (as f64) -> (lo, hi): the reals that round to s lie in [lo, hi]
    (the midpoints to the neighbouring bf16 values). For measuring only: how far
    outside its stored value's cell a reference d lies is the least error the
    kernel's f32 value had before it was rounded."""
    s = np.asarray(s, np.float64)
    m, e = np.frexp(np.abs(s))
    e = np.where(s == 0, -125, np.maximum(e, -125))
    out = np.ldexp(1.0, e - 9)                                 # half a step away from 0
    inn = np.where((m == 0.5) & (e > -125), out / 2, out)       # ... towards 0 (a power of two: half of it)
    inn = np.where(s == 0, out, inn)
    return np.where(s >= 0, s - inn, s - out), np.where(s > 0, s + out, s + inn)


def exact_operands(target, V, A, seed, K0, tie=None):
    """target f32 [B, V*A] -> dict(h f32 [B, K], w f32 [V*A, K], bias f32 [V*A],
    logits f32 [B, V*A]) with bf16-exact h and w and logits = bias + h w^T
    exactly, in any summation order. tie = (j1, j2): columns j1 and j2 of every
    VM row get the same dense W row and bias."""
    B, N = target.shape
    assert N == V * A and K0 in (64, 128)
    rs = np.random.RandomState(seed)
    h0 = rs.randint(-2, 3, size=(B, K0)).astype(np.float32) / 2
    w0 = rs.randint(-8, 9, size=(N, K0)).astype(np.float32) / 64
    bias = rs.randint(-64, 65, size=N).astype(np.float32) / 128
    if tie is not None:
        j1, j2 = tie
        w0.reshape(V, A, K0)[:, j2] = w0.reshape(V, A, K0)[:, j1]
        bias.reshape(V, A)[:, j2] = bias.reshape(V, A)[:, j1]
    t = to_bf16(np.rint(target.astype(np.float64) / GRAIN) * GRAIN)
    K = (K0 + B + 63) // 64 * 64
    h = np.zeros((B, K), np.float32)
    w = np.zeros((N, K), np.float32)
    h[:, :K0] = h0
    h[np.arange(B), K0 + np.arange(B)] = 1
    w[:, :K0] = w0
    w[:, K0:K0 + B] = t.T
    x = bias.astype(np.float64) + h0.astype(np.float64) @ w0.astype(np.float64).T + t
    worst = float(np.abs(bias).max() + (np.abs(h0).astype(np.float64) @ np.abs(w0).astype(np.float64).T
                                        + np.abs(t)).max())
    assert worst < LIMIT, worst  # every partial sum, in any order, stays below 2^9
    assert np.array_equal(x, x.astype(np.float32))
    return dict(h=h, w=w, bias=bias, logits=x.astype(np.float32), K=K, K0=K0)


def _given_targets(c):
    """head_cases.given_case; below its 5 samples: random logits, 40 % masked, valid actions."""
    if c.B >= 5:
        g = C.given_case(c.B, c.V, c.A, seed=c.A * 100 + c.V, shift=c.shift)
        return g["logits"], g["invalid"], g["action"]
    rs = np.random.RandomState(c.A * 100 + c.V)
    x = (rs.randn(c.B, c.V, c.A) * 3 + c.shift).astype(np.float32)
    inv = rs.rand(c.B, c.V, c.A) < 0.4
    act = np.array([[C._valid_action(rs, inv[b, v]) for v in range(c.V)] for b in range(c.B)], np.int64)
    return x.reshape(c.B, -1), inv, act


def _seed(c, k):
    return 7919 * CASES.index(c) + k


@functools.lru_cache(maxsize=None)
def given_inputs(name):
    """GIVEN forward and backward: dict(h, w, bias, logits, invalid, action, g_lp, g_ent, dbias0)."""
    c = BY_NAME[name]
    x, inv, act = _given_targets(c)
    if not c.bits:
        inv = np.zeros_like(inv)
    rs = np.random.RandomState(_seed(c, 1))
    if c.dense:
        d = dense_operands(c, x)
    else:
        d = exact_operands(x, c.V, c.A, _seed(c, 0), c.K0)
    d.update(invalid=inv, action=act, g_lp=rs.randn(c.B).astype(np.float32), g_ent=rs.randn(c.B).astype(np.float32),
             dbias0=(rs.randn(c.V * c.A) / 16).astype(np.float32))
    return d


def sample_seed(c):
    return 1000 + c.A, 7 * c.V


@functools.lru_cache(maxsize=None)
def sample_inputs(name):
    """SAMPLE: head_cases.sample_case, every third row with its maximum duplicated
    at columns 0 and A - 1 (both always valid).
    -> dict(h, w, bias, logits, invalid, skip, seed, offset, tie_rows)"""
    c = BY_NAME[name]
    x, inv, skip = C.sample_case(c.B, c.V, c.A, seed=c.A * 100 + c.V)
    x = x.reshape(c.B, c.V, c.A).copy()
    tie_rows = (np.arange(c.B * c.V) % 3 == 0).reshape(c.B, c.V)
    top = x.max(-1) + np.float32(8.0)  # above the dense block's spread: still the row's maximum (CPU test)
    x[tie_rows, 0] = top[tie_rows]
    x[tie_rows, c.A - 1] = top[tie_rows]
    x = x.reshape(c.B, -1)
    if not c.bits:
        inv, skip = np.zeros_like(inv), np.zeros_like(skip)
    d = dense_operands(c, x) if c.dense else exact_operands(x, c.V, c.A, _seed(c, 2), c.K0, tie=(0, c.A - 1))
    seed, off = sample_seed(c)
    d.update(invalid=inv, skip=skip, seed=seed, offset=off, tie_rows=tie_rows)
    return d


WAIT_RATIOS = (0.0, 0.3, 1.0)


def wait_seed(c, i):
    return 7 + c.A, 1000 * i + c.V


@functools.lru_cache(maxsize=None)
def wait_inputs(name):
    """The WAIT coin: head_cases.wait_case -> dict(h, w, bias, logits, invalid, P, kind)."""
    c = BY_NAME[name]
    x, inv, P, kind = C.wait_case(c.B, c.V, c.A, seed=c.A * 100 + c.V + 1)
    d = exact_operands(x, c.V, c.A, _seed(c, 3), c.K0)
    d.update(invalid=inv, P=P, kind=kind)
    return d


def dense_operands(c, x):
    """Ordinary operands (the dense-GEMM case): tanh(randn) h, randn 2 / sqrt(K) W
    at K = 512 and a bias of 0.1 randn, h and W rounded to bf16; logits64 is the
    f64 product of the rounded operands, logits its f32 rounding (head_ref reads
    f32 logits; that rounding, at most 2^-24 |x|, is inside the GEMM term of the
    case's floor), logits_f32 torch's f32 addmm, abs_sum max_n sum_k |h_k w_nk|."""
    B, N, K = c.B, c.V * c.A, DENSE_K
    rs = np.random.RandomState(_seed(c, 4))
    h = to_bf16(np.tanh(rs.randn(B, K)))
    w = to_bf16(rs.randn(N, K) * (2.0 / K ** 0.5))
    bias = (rs.randn(N) * 0.1).astype(np.float32)
    x64 = h.astype(np.float64) @ w.astype(np.float64).T + bias.astype(np.float64)
    tor = torch.addmm(torch.from_numpy(bias), torch.from_numpy(h), torch.from_numpy(w).t()).numpy()
    abs_sum = float((np.abs(h).astype(np.float64) @ np.abs(w).astype(np.float64).T).max())
    return dict(h=h, w=w, bias=bias, logits=x64.astype(np.float32), logits64=x64, logits_f32=tor, abs_sum=abs_sum,
                K=K, K0=0)


def dense_floor_gain(c, d):
    """What every floor of the dense case gains (logprob, entropy, the gradient
    and dbias alike): V roundings at the size of a logit's absolute sum, the
    accumulation's own error scale."""
    return c.V * C.EPS * d["abs_sum"]


# ------------------------------------------------------- edges, re-derived
def given_edges(c, d):
    """The edge rows of head_cases.given_case, read from the FINAL logits:
    -> dict of what holds (the CPU test asserts every entry)."""
    x = d["logits"].reshape(c.B, c.V, c.A).astype(np.float64)
    inv, act = d["invalid"], d["action"]
    out = {}
    if c.B >= 5 and c.bits:
        out["all masked"] = bool(inv[0, 0].all())
        out["one valid"] = int((~inv[1, 1 % c.V]).sum()) == 1 and not inv[1, 1 % c.V, act[1, 1 % c.V]]
        out["masked GIVEN action"] = bool(inv[2, 2 % c.V, act[2, 2 % c.V]])
    if c.B >= 5:
        out["GIVEN out of range"] = act[3, 3 % c.V] == c.A or act[3, 4 % c.V] == -1
        if c.A > 1:
            for k, b in enumerate((4, 5 if c.B > 5 else 4)):
                row = np.sort(x[b, (4 + k) % c.V])
                out[f"peak {k} by {PEAK_MARGIN}"] = bool(row[-1] - row[-2] >= PEAK_MARGIN)
    out["shift"] = bool(abs(float(np.median(x)) - c.shift) < 3.0)
    return out


def wait_margin(c, d):
    """min over rows of logit[WAIT] - the largest other logit, in the final logits."""
    if c.A == 1:
        return np.inf
    x = d["logits"].reshape(c.B, c.V, c.A).astype(np.float64)
    others = np.delete(x, d["P"], axis=-1).max(-1)
    return float((x[..., d["P"]] - others).min())


# ------------------------------------------------------ references, once
def draw_reference(logits, V, A, invalid, seed, offset, counter=None):
    """The inverse-CDF draw in action order j = 0..A-1 (the order k_hg16's SAMPLE
    block documents: tile totals, then the tile's lanes in q order, then r).
    -> (u, action, dist, lo, hi)"""
    B = logits.shape[0]
    u = R.sample_uniforms(seed, offset, B * V, counter)
    return (u,) + R.sample(logits, V, A, invalid, u, np.arange(A))


COUNTER_SEED, COUNTER_RATIO = 77, 0.5  # the HeadRng.graph_counter run (on the WAIT inputs)


def coin_reference(c, w, ratio, seed, offset, counter=None):
    """The coin, then the draw on the rows it left: -> (invalid with the forbidden
    WAITs, all-masked rows [B, V], reference action, dist, lo, hi)."""
    forbid = R.coin_forbids(w["invalid"], w["P"], ratio, seed, offset, counter)
    inv2 = R.with_forbidden(w["invalid"], forbid, w["P"])
    _, act, dist, lo, hi = draw_reference(w["logits"], c.V, c.A, inv2, seed, offset, counter)
    return inv2, inv2.all(-1), act, dist, lo, hi, forbid


def grad_reference(c, d, which):
    """-> (g_lp, g_ent, ref f64 [B, V, A], torch f32 grad as f64, judged rows [B, V, 1])."""
    g_lp = d["g_lp"] if which in ("both", "lp") else None
    g_ent = d["g_ent"] if which in ("both", "ent") else None
    ref = R.head_grad(d["logits"], c.V, c.A, d["invalid"], d["action"], g_lp, g_ent)
    _, _, tor = C.torch_f32(d["logits_f32"] if c.dense else d["logits"], c.V, c.A, d["invalid"], d["action"], g_lp,
                            g_ent)
    ok = ((d["action"] >= 0) & (d["action"] < c.A))[..., None]
    return g_lp, g_ent, ref, tor, ok
