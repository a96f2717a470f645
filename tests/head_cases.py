"""Inputs and the tolerance rule shared by tests/test_head_ref_cpu.py and
tests/test_gpu_head_instances.py (test infrastructure, numpy / CPU torch only).

Tolerance rule (no fixed numbers): per case and quantity, e_ref is the largest
|torch_head (f32, CPU) - head_ref (f64)|; a kernel must stay within
4 e_ref + floor of head_ref, where floor is one f32 rounding of the largest
term of the quantity's formula:
  logprob, entropy   V 2^-23 (1 + max|x_valid|)           (a sum of V rows of x - lse)
  gradient           2^-23 (max|g_lp| + max|g_ent| (1 + max|x_valid|))
                     (g_lp (1[j=a] - q_j) - g_ent q_j (x_j - lse + H) with q_j <= 1:
                     the x_j - lse difference is rounded at the size of x)
  GAE                2^-23 max(1, max|adv|, max|ret|)
The factor 4 is a margin over the f32 reference's own error for __expf and
another summation order; it is not taken from any kernel.
A sample whose GIVEN action is masked has logprob ~ -1e7: the largest term of
its sum is the masked fill itself, not a valid logit, and every one of the V
f32 additions rounds at that size (ulp(1e7) = 1). Such samples are judged by
the same rule in a group of their own with the floor of their own largest
term, V 2^-23 (1 + 1e7), so that they do not loosen the bound of the ordinary
samples (which of two neighbouring integers the f32 sum lands on depends on
the summation order: torch's 0.06 against a kernel's 0.94 from -10000008.1
is one rounding either way).
"""
import numpy as np
import torch

from tests import head_ref as R
from tests.torch_ref import torch_gae, torch_head

EPS = 2.0 ** -23


def pack_bits(invalid):
    """bool [B, V, A] -> int32 bits [B, V, W] (bit a of word a // 32 set = invalid)."""
    inv = np.asarray(invalid, bool)
    B, V, A = inv.shape
    W = (A + 31) // 32
    pad = np.zeros((B, V, W * 32), np.uint64)
    pad[..., :A] = inv
    w = (pad.reshape(B, V, W, 32) << np.arange(32, dtype=np.uint64)).sum(-1)
    return w.astype(np.uint32).view(np.int32)


def _valid_action(rs, invalid_row):
    ok = np.nonzero(~invalid_row)[0]
    if len(ok) == 0:
        ok = np.arange(len(invalid_row))
    return int(ok[rs.randint(len(ok))])


def given_case(B, V, A, seed, shift=0.0):
    """GIVEN-mode inputs with every edge row the suite asks for (B >= 5):
    an all-masked row, a one-valid row, a masked GIVEN action, out-of-range
    GIVEN actions (A and -1: NaN on both sides), a row with one logit 60 (and,
    further, 120: f32 exp underflows to exactly 0) above the rest, an unmasked
    row (B >= 7); then `shift` added to every logit.
    -> dict(logits f32 [B, V*A], invalid bool [B, V, A], action i64 [B, V])"""
    assert B >= 5
    rs = np.random.RandomState(seed)
    x = (rs.randn(B, V, A) * 3).astype(np.float32)
    inv = rs.rand(B, V, A) < 0.4
    act = np.zeros((B, V), np.int64)
    for b in range(B):
        for v in range(V):
            act[b, v] = _valid_action(rs, inv[b, v])
    inv[0, 0] = True                                       # all masked
    act[0, 0] = rs.randint(A)
    j = rs.randint(A)                                      # one valid action
    inv[1, 1 % V] = True
    inv[1, 1 % V, j] = False
    act[1, 1 % V] = j
    j = rs.randint(A)                                      # GIVEN action masked
    inv[2, 2 % V] = False
    inv[2, 2 % V, j] = True
    act[2, 2 % V] = j
    act[3, 3 % V] = A                                      # GIVEN out of range
    act[3, 4 % V] = -1
    for k, (b, up) in enumerate(((4, 60.0), (5 if B > 5 else 4, 120.0))):
        v = (4 + k) % V
        j = rs.randint(A)
        inv[b, v] = rs.rand(A) < 0.3
        inv[b, v, j] = False
        inv[b, v, (j + 1) % A] = False
        x[b, v, j] = np.delete(x[b, v], j).max(initial=-9.0) + up
        act[b, v] = (j + 1) % A if (k == 0 and A > 1) else j  # the underflowing neighbour / the peak
    if B >= 7:
        inv[6, 6 % V] = False
        act[6, 6 % V] = rs.randint(A)
    x = (x + np.float32(shift)).astype(np.float32)
    return dict(logits=x.reshape(B, V * A), invalid=inv, action=act)


def argmax_case(B, V, A, seed):
    """Rows whose maximum is duplicated on purpose: at positions 5, 17 and 65
    apart (different lanes and different e of every group width), and at
    random triples. -> (logits f32 [B, V*A], invalid)"""
    rs = np.random.RandomState(seed)
    x = (rs.randn(B, V, A) * 3).astype(np.float32)
    top = x.max(-1) + np.float32(1.0)
    for r in range(B * V):
        b, v = divmod(r, V)
        kind = r % 5
        if kind == 0:
            pos = rs.choice(A, size=min(3, A), replace=False)
        elif kind == 4:
            pos = []  # no forced tie
        else:
            pos = [A - 1, max(0, A - 1 - (5, 17, 65)[kind - 1])]
        for j in pos:
            x[b, v, j] = top[b, v]
    return x.reshape(B, V * A), rs.rand(B, V, A) < 0.4


def sample_case(B, V, A, seed):
    """SAMPLE-mode inputs: logits randn * 3, at most 10 valid categories per row
    (8 random positions and the forced positions 0 and A - 1); row (0, 0) is
    all masked (range-checked only). -> (logits, invalid, skip bool [B, V])"""
    rs = np.random.RandomState(seed)
    x = (rs.randn(B, V, A) * 3).astype(np.float32)
    inv = np.ones((B, V, A), bool)
    pos = rs.randint(0, A, size=(B, V, 8))
    np.put_along_axis(inv, pos, False, -1)
    inv[..., 0] = False
    inv[..., A - 1] = False
    inv[0, 0] = True
    skip = np.zeros((B, V), bool)
    skip[0, 0] = True
    return x.reshape(B, V * A), inv, skip


def wait_case(B, V, A, seed):
    """WAIT-coin inputs (the row mix of test_wait_coin_flips): WAIT = column
    max(A - 2, 0) with logit +30 and valid; rows cycle through: qualifies (more
    than one invalid, WAIT and 1-3 others valid), nothing invalid, WAIT already
    invalid (one other valid), only WAIT valid.
    -> (logits, invalid, wait_index, kind [B, V])"""
    rs = np.random.RandomState(seed)
    P = max(A - 2, 0)
    x = (rs.randn(B, V, A) * 3).astype(np.float32)
    x[..., P] = 30.0
    inv = np.zeros((B, V, A), bool)
    kind = (np.arange(B * V) % 4).reshape(B, V)
    for b in range(B):
        for v in range(V):
            k = kind[b, v]
            if k == 0:
                inv[b, v] = True
                inv[b, v, rs.randint(0, A, size=rs.randint(1, 4))] = False
                inv[b, v, P] = False
            elif k == 2:
                inv[b, v] = True
                inv[b, v, (P + 1 + rs.randint(max(A - 1, 1))) % A] = False
                inv[b, v, P] = True
            elif k == 3:
                inv[b, v] = True
                inv[b, v, P] = False
    return x.reshape(B, V * A), inv, P, kind


# ------------------------------------------------------------ tolerance rule
def torch_f32(logits, V, A, invalid, action, g_lp=None, g_ent=None):
    """tests.torch_ref.torch_head in f32 on the CPU (the rule's f32 side):
    -> (logprob [B], entropy [B], grad [B, V, A] or None) as f64 arrays.
    Out-of-range actions are replaced by 0 for torch's gather; their samples
    are NaN in the reference and excluded from e_ref."""
    B = logits.shape[0]
    x = torch.from_numpy(np.ascontiguousarray(logits, np.float32)).clone().requires_grad_(True)
    bits = torch.from_numpy(pack_bits(invalid))
    a = np.where((action >= 0) & (action < A), action, 0)
    _, lp, ent = torch_head(x, V, A, bits=bits, action=torch.from_numpy(a))
    grad = None
    if g_lp is not None or g_ent is not None:
        loss = 0
        if g_lp is not None:
            loss = loss + (torch.from_numpy(np.asarray(g_lp, np.float32)) * lp).sum()
        if g_ent is not None:
            loss = loss + (torch.from_numpy(np.asarray(g_ent, np.float32)) * ent).sum()
        loss.backward()
        grad = x.grad.double().numpy().reshape(B, V, A)
    return lp.detach().double().numpy(), ent.detach().double().numpy(), grad


def x_valid_max(logits, invalid):
    x = np.abs(np.asarray(logits, np.float64).reshape(invalid.shape))
    return float(np.where(invalid, 0.0, x).max(initial=0.0))


def floor_sum(V, logits, invalid):
    return V * EPS * (1.0 + x_valid_max(logits, invalid))


def floor_grad(logits, invalid, g_lp, g_ent):
    a = 0.0 if g_lp is None else float(np.abs(g_lp).max())
    b = 0.0 if g_ent is None else float(np.abs(g_ent).max())
    return EPS * (a + b * (1.0 + x_valid_max(logits, invalid)))


# ------------------------------------------------- vmp_policy_head's matrix
# family -> the A values that reach it. Tile kernels: A <= 128 on 16-byte
# aligned logits (mask-word edges W = 1..4, tiles that are no multiple of 4
# floats). Group kernels k_head_fwd/bwd<G, E>: A > 128 on ordinary tensors,
# A <= 128 through logits (and dlogits) that start 4 bytes past alignment;
# every (G, E) the dispatch can pick, at both ends of its A range.
FAMILY_A = {
    "tile": (1, 2, 3, 4, 5, 16, 17, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128),
    "group_misaligned": (1, 2, 16, 17, 32, 33, 64, 65, 128),
    "group": (129, 256, 257, 512, 513, 1024),
}
HEAD_PARAMS = [(f, A) for f, As in FAMILY_A.items() for A in As]


def group_width(A):
    """pick_g of csrc/vmp_policy.hip."""
    return 4 if A <= 64 else (16 if A <= 256 else 64)


def lanes(family, A):
    return 4 if family == "tile" else group_width(A)


def shapes(family, A):
    """(B, V) of a family's cases. Tiles: 135 rows = two full tiles of 64 and one
    of 7. Groups (one block per sample, 64 / 128 / 256 threads by V G, a group
    of G lanes per row): V = 1, a V with 65 <= V G <= 128, and a V with more
    rows than the block has groups."""
    if family == "tile":
        return [(5, 27)]
    return [(8, V) for V in {4: (1, 20, 70), 16: (1, 7, 19), 64: (1, 2, 9)}[group_width(A)]]


def sample_seed(A, V):
    return 1000 + A, 7 * V


def sample_inputs():
    """Every SAMPLE input of test_gpu_head_instances' vmp_policy_head matrix:
    (name, (logits, invalid, skip, V, A, G, seed, offset))."""
    for fam, A in HEAD_PARAMS:
        for B, V in shapes(fam, A):
            x, inv, skip = sample_case(B, V, A, seed=A * 100 + V)
            seed, off = sample_seed(A, V)
            yield f"{fam}-A{A}-V{V}", (x, inv, skip, V, A, lanes(fam, A), seed, off)


RATIOS = {}  # (family, mode, quantity) -> [max kernel err, max e_ref, max err / bound]


def judge(key, kern, ref, tor, floor, groups=None):
    """Assert |kern - ref| <= 4 e_ref + floor per group [(label, leading
    indices, the group's floor)] (default: one group of everything); NaN exactly where the
    reference is NaN. Prints the figures before asserting and records them in
    RATIOS[key] (a labelled group under its own quantity name)."""
    kern, ref, tor = (np.asarray(t, np.float64) for t in (kern, ref, tor))
    assert kern.shape == ref.shape == tor.shape, (kern.shape, ref.shape, tor.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(kern), nan), (key, "NaN pattern", np.isnan(kern), nan)
    if groups is None:
        groups = [("", np.arange(ref.shape[0]), floor)]
    worst = None
    for label, g, floor in groups:
        ok = ~nan[g]
        if len(g) == 0 or not ok.any():
            continue
        e_ref = float(np.abs(tor[g] - ref[g])[ok].max())
        err = float(np.abs(kern[g] - ref[g])[ok].max())
        bound = 4.0 * e_ref + floor
        k = key if not label else key[:-1] + (key[-1] + label,)
        rec = RATIOS.setdefault(k, [0.0, 0.0, 0.0])
        rec[0], rec[1], rec[2] = max(rec[0], err), max(rec[1], e_ref), max(rec[2], err / bound)
        print(f"HEADERR {k} err {err:.3e} e_ref {e_ref:.3e} floor {floor:.3e} used {err / bound:.3f}")
        if err > bound and worst is None:
            worst = (k, err, e_ref, floor)
    assert worst is None, ("key, err, e_ref, floor", worst)


def lp_groups(ref_lp, floor, V):
    """Ordinary samples / samples with a masked GIVEN action (|logprob| ~ 1e7),
    each with its floor."""
    big = np.abs(np.nan_to_num(ref_lp)) > 1e6
    return [("", np.nonzero(~big)[0], floor),
            (" (masked action)", np.nonzero(big)[0], V * EPS * (1.0 - R.MASKED))]


def gae_case(T, N, pattern, seed):
    rs = np.random.RandomState(seed)
    r = rs.randn(T, N).astype(np.float32)
    v = rs.randn(T, N).astype(np.float32)
    nv = rs.randn(T, N).astype(np.float32)
    d = np.zeros((T, N), np.float32)
    if pattern == "all":
        d[:] = 1
    elif pattern == "last":
        d[-1] = 1
    elif pattern == "random":
        d[rs.rand(T, N) < 0.05] = 1
    return r, d, v, nv


def gae_torch_f32(r, d, v, nv, gamma, lam):
    adv, ret = torch_gae(*(torch.from_numpy(t) for t in (r, d, v, nv)), gamma, lam)
    return adv.double().numpy(), ret.double().numpy()
