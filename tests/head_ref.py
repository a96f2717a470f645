"""float64 reference of the masked multi-categorical head (test infrastructure).

Restates Network.get_action / get_det_action (src/agents/ppo.py:115-131) and the
PPOAgent.act WAIT coin (ppo.py:154-156) in numpy float64 and calls no kernel.
Every HIP head (vmp_policy_head's tile and group kernels, vmp_actor_head,
vmp_actor_mlp_head_f32) is judged against this one file.

Conventions (the behaviour torch and every kernel share):
  * masked entries are filled with -1e7;
  * lse = max + log(sum exp(x - max)) is formed in f64 and rounded to f32 ONCE
    (at |m| = 1e7 that rounding is the reference's behaviour: an all-masked
    row of 12 has logprob -2, not -2.48); everything after stays in f64:
    logprob = x_a - lse32, entropy = -sum_{q_j > 0} q_j (x_j - lse32);
  * per-sample values are sums over the V rows of the sample;
  * an action outside [0, A) gives NaN.

The sampling stream is a Python-integer port of csrc/vmp_head_dev.h's
mix64 / uniform_at / eff_seed, so the reference predicts, row by row, the WAIT
coin's decision and the uniform of the inverse-CDF draw, and with the order in
which a kernel walks the categories, the drawn action itself.
"""
import numpy as np

MASKED = -1e7
_M = (1 << 64) - 1
COIN_STREAM = 0xC0FFEE5EED
_CTR_SALT = 0x5851F42D4C957F2D


# ------------------------------------------------------------------ stream
def mix64(x):
    """splitmix64's output function of the state x + golden ratio (hd::mix64)."""
    x = (int(x) + 0x9E3779B97F4A7C15) & _M
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M
    return x ^ (x >> 31)


def uniform_at(seed, ctr):
    """hd::uniform_at: 24 random bits of stream (seed, ctr) -> k / 2^24 (exact in f32 and f64)."""
    return (mix64((int(seed) & _M) ^ mix64(int(ctr) & _M)) >> 40) / 16777216.0


def eff_seed(seed, counter=None):
    """hd::eff_seed: HeadRng's device-counter mode mixes the counter's value into the seed."""
    seed = int(seed) & _M
    return seed if counter is None else seed ^ mix64((int(counter) + _CTR_SALT) & _M)


def _mix64_v(x):
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def uniforms(seed, offset, n, counter=None):
    """uniform_at(eff_seed(seed, counter), offset + r) for r in range(n), as f64 [n]."""
    with np.errstate(over="ignore"):
        ctr = np.uint64(int(offset) & _M) + np.arange(n, dtype=np.uint64)
    h = _mix64_v(np.uint64(eff_seed(seed, counter)) ^ _mix64_v(ctr))
    return (h >> np.uint64(40)).astype(np.float64) / 16777216.0


def sample_uniforms(seed, offset, rows, counter=None):
    """The inverse-CDF uniform of each (sample, VM) row: stream seed, counter offset + row."""
    return uniforms(seed, offset, rows, counter)


def coin_forbids(invalid, wait_index, wait_ratio, seed, offset, counter=None):
    """PPOAgent.act's WAIT coin per row of invalid [..., A]: True where WAIT gets
    forbidden (more than one invalid action, WAIT valid, rand() > ratio).
    Stream: seed ^ 0xC0FFEE5EED, counter offset + row; ratio compared as f32."""
    inv = np.asarray(invalid, bool)
    flat = inv.reshape(-1, inv.shape[-1])
    if wait_ratio < 0:
        return np.zeros(inv.shape[:-1], bool)
    u = uniforms(eff_seed(seed, counter) ^ COIN_STREAM, offset, flat.shape[0])
    f = (flat.sum(-1) > 1) & ~flat[:, wait_index] & (u > float(np.float32(wait_ratio)))
    return f.reshape(inv.shape[:-1])


def with_forbidden(invalid, forbid, wait_index):
    out = np.array(invalid, bool, copy=True)
    out[..., wait_index] |= forbid
    return out


# ---------------------------------------------------------- masked statistics
def _rows(logits, V, A):
    x32 = np.asarray(logits, np.float32)
    return x32.reshape(-1, V, A)


def masked(logits, V, A, invalid=None):
    """f32 logits [B, V*A] -> f64 [B, V, A] with -1e7 at invalid entries."""
    x = _rows(logits, V, A).astype(np.float64)
    if invalid is not None:
        x = np.where(np.asarray(invalid, bool).reshape(x.shape), MASKED, x)
    return x


def row_stats(x):
    """x f64 masked [..., A] -> (q softmax, l = x - lse32, lse32, H) per row."""
    m = x.max(-1, keepdims=True)
    p = np.exp(x - m)
    S = p.sum(-1, keepdims=True)
    lse32 = (m + np.log(S)).astype(np.float32).astype(np.float64)  # the one f32 rounding
    q = p / S
    l = x - lse32
    H = -np.where(q > 0, q * l, 0.0).sum(-1)
    return q, l, lse32[..., 0], H


def head_given(logits, V, A, invalid, action):
    """-> (logprob [B], entropy [B], row logprob [B, V], row entropy [B, V]), f64."""
    x = masked(logits, V, A, invalid)
    _, l, _, H = row_stats(x)
    a = np.asarray(action).reshape(x.shape[0], V).astype(np.int64)
    ok = (a >= 0) & (a < A)
    la = np.take_along_axis(l, np.clip(a, 0, A - 1)[..., None], -1)[..., 0]
    row_lp = np.where(ok, la, np.nan)
    return row_lp.sum(-1), H.sum(-1), row_lp, H


def head_grad(logits, V, A, invalid, action, g_lp=None, g_ent=None):
    """d/dlogits of sum_b g_lp[b] logprob[b] + g_ent[b] entropy[b] w.r.t. the
    pre-mask logits -> f64 [B, V, A]: exactly 0 at masked entries, elsewhere
    g_lp (1[j = a] - q_j) - g_ent q_j (l_j + H)."""
    x = masked(logits, V, A, invalid)
    q, l, _, H = row_stats(x)
    B = x.shape[0]
    a = np.asarray(action).reshape(B, V).astype(np.int64)
    one = np.arange(A)[None, None, :] == a[..., None]
    glp = np.zeros(B) if g_lp is None else np.asarray(g_lp, np.float64)
    gen = np.zeros(B) if g_ent is None else np.asarray(g_ent, np.float64)
    g = glp[:, None, None] * (one - q) - gen[:, None, None] * np.where(q > 0, q * (l + H[..., None]), 0.0)
    if invalid is not None:
        g = np.where(np.asarray(invalid, bool).reshape(g.shape), 0.0, g)
    return g


def argmax(logits, V, A):
    """get_det_action: first maximum of the UNMASKED f32 row -> int64 [B, V]. Exact."""
    return _rows(logits, V, A).argmax(-1)


# ----------------------------------------------------------------- sampling
def lane_major_order(A, G):
    """The order in which a kernel whose G lanes hold categories j = g + G e walks
    them: lane-major, sorted by (g, e). Group kernels: their G; the tile kernels,
    k_head_gemm and lane_row: a quad, G = 4."""
    return np.array(sorted(range(A), key=lambda j: (j % G, j // G)), dtype=np.int64)


def sample(logits, V, A, invalid, u, order):
    """Inverse-CDF draw of every row with its uniform u [B*V] over the masked
    softmax, categories taken in `order`.
    -> (action [B, V], dist [B, V], lo [B, V], hi [B, V]): dist is the distance
    from u * total to the nearest CDF boundary relative to total; lo / hi are
    the neighbouring positive categories in the order (-1: none), which a row
    inside the rounding band may take instead."""
    x = masked(logits, V, A, invalid).reshape(-1, A)
    R = x.shape[0]
    p = np.exp(x - x.max(-1, keepdims=True))[:, order]
    c = np.cumsum(p, -1)
    total = c[:, -1]
    t = np.asarray(u, np.float64).reshape(R) * total
    k = np.minimum((c <= t[:, None]).sum(-1), A - 1)
    bounds = np.concatenate([np.zeros((R, 1)), c], -1)
    dist = np.abs(bounds - t[:, None]).min(-1) / total
    pos = p > 0
    idx = np.arange(A)[None, :]
    lo_i = np.where(pos & (idx < k[:, None]), idx, -1).max(-1)
    hi_i = np.where(pos & (idx > k[:, None]), idx, A).min(-1)
    lo = np.where(lo_i >= 0, order[np.clip(lo_i, 0, A - 1)], -1)
    hi = np.where(hi_i < A, order[np.clip(hi_i, 0, A - 1)], -1)
    sh = (-1, V)
    return order[k].reshape(sh), dist.reshape(sh), lo.reshape(sh), hi.reshape(sh)


BAND = 64 * 2.0 ** -24  # rows nearer than this to a boundary may take a neighbour


def judge_draw(act, ref_act, dist, lo, hi, skip=None):
    """The SAMPLE rule: outside the band the action is the reference's; inside
    it the reference's or a neighbouring positive category.
    -> (ok [B, V] bool, near-row fraction)."""
    act = np.asarray(act).astype(np.int64).reshape(ref_act.shape)
    near = dist <= BAND
    ok = (act == ref_act) | (near & ((act == lo) | (act == hi)))
    if skip is not None:
        ok = ok | skip
        near = near & ~skip
    return ok, float(near.mean())


# ------------------------------------------------------------------ GAE
def gae(rew, done, values, next_values, gamma, lam):
    """PPOAgent.update's reverse scan (ppo.py:232-243) as an f64 loop over f32 inputs."""
    r, d, v, nv = (np.asarray(t, np.float32).astype(np.float64) for t in (rew, done, values, next_values))
    gamma, lam = float(np.float32(gamma)), float(np.float32(lam))
    adv = np.zeros_like(r)
    g = np.zeros_like(r[0]) if r.shape[0] else None
    for t in reversed(range(r.shape[0])):
        nd = 1.0 - d[t]
        g = r[t] + nd * gamma * nv[t] - v[t] + nd * gamma * lam * g
        adv[t] = g
    return adv, adv + v
