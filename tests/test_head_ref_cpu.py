"""tests/head_ref.py (the float64 reference every HIP head is judged against)
checked on the CPU: against tests.torch_ref.torch_head and
torch.distributions.Categorical run in f64, the public splitmix64 vector for
its port of the sampling stream, its inverse-CDF draw against a direct
per-row loop, and the near-boundary share of the SAMPLE inputs the GPU tests
use (tests/head_cases.py), which must stay within the 0.5 % those tests allow."""
import numpy as np
import pytest
import torch

from tests import head_cases as C
from tests import head_ref as R
from tests.torch_ref import torch_gae, torch_head


def test_splitmix64_vector_and_stream_port():
    assert R.mix64(0) == 0xE220A8397B1DCDAF  # first output of splitmix64 seeded with 0
    # the next outputs of the same generator: state advances by the golden ratio
    assert R.mix64(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4
    assert R.mix64(2 * 0x9E3779B97F4A7C15) == 0x06C45D188009454F
    for seed, off, ctr in ((0, 0, None), (123, 77, None), (2**64 - 1, 2**63, 5), (9, 0, 0)):
        u = R.uniforms(seed, off, 50, ctr)
        es = R.eff_seed(seed, ctr)
        assert [R.uniform_at(es, off + r) for r in range(50)] == list(u)
        assert ((u >= 0) & (u < 1)).all() and (u * 2**24 == np.round(u * 2**24)).all()
    assert R.eff_seed(5, None) == 5
    assert R.eff_seed(5, 0) == 5 ^ R.mix64(0x5851F42D4C957F2D)
    assert R.eff_seed(5, 0) != R.eff_seed(5, 1)


@pytest.mark.parametrize("V,A", [(1, 1), (3, 2), (4, 12), (2, 129), (1, 1024)])
def test_given_matches_torch_f64(V, A):
    """logprob, entropy and gradient against torch_head and Categorical in f64.
    The only difference allowed is the reference's single f32 rounding of lse
    (relative 2^-24 per row) - except on all-masked rows, where that rounding is
    the behaviour under test and is checked by value below."""
    B = 8
    c = C.given_case(B, V, A, seed=V * 1000 + A)
    inv, act = c["invalid"], c["action"]
    g_lp, g_ent = np.linspace(-1, 1, B), np.linspace(0.5, -2, B)
    lp, ent, row_lp, row_ent = R.head_given(c["logits"], V, A, inv, act)
    grad = R.head_grad(c["logits"], V, A, inv, act, g_lp, g_ent)
    x = torch.from_numpy(c["logits"]).double().requires_grad_(True)
    a0 = np.where((act >= 0) & (act < A), act, 0)
    _, lp_t, ent_t = torch_head(x, V, A, bits=torch.from_numpy(C.pack_bits(inv)),
                                action=torch.from_numpy(a0))
    (torch.from_numpy(g_lp) * lp_t + torch.from_numpy(g_ent) * ent_t).sum().backward()
    xm = torch.from_numpy(R.masked(c["logits"], V, A, inv))
    cat = torch.distributions.Categorical(logits=xm)
    cat_lp = cat.log_prob(torch.from_numpy(a0)).numpy()
    cat_ent = cat.entropy().numpy()
    allm = inv.all(-1)
    oor = (act < 0) | (act >= A)
    assert np.isnan(row_lp[oor]).all() and not np.isnan(row_lp[~oor]).any()
    assert np.isnan(lp[3]) and np.isfinite(np.delete(lp, 3)).all()
    scale = np.abs(R.masked(c["logits"], V, A, inv)).max(-1) + 8.0  # |lse| <= max|x| + log A
    tol = 2.0 ** -24 * scale * 1.01 + 1e-12
    ok = ~allm & ~oor
    assert (np.abs(row_lp - cat_lp)[ok] <= tol[ok]).all()
    assert (np.abs(row_ent - cat_ent)[~allm] <= tol[~allm]).all()
    # all-masked rows: -1e7 + log A rounds to an integer in f32
    want = -1e7 - float(np.float32(-1e7 + np.log(A)))
    assert (row_lp[allm & ~oor] == want).all() and (np.abs(row_ent[allm] + want) < 1e-12).all()
    if A == 12:
        assert want == -2.0
    keep = np.ones(B, bool)
    keep[3] = False
    keep &= ~allm.any(-1)
    assert np.abs(lp - lp_t.detach().numpy())[keep].max() <= V * tol.max()
    assert np.abs(ent - ent_t.detach().numpy())[keep].max() <= V * tol.max()
    gt = x.grad.numpy().reshape(B, V, A)
    assert (grad[inv] == 0).all() and (gt[inv] == 0).all()
    rows = ~allm & ~oor
    gscale = 2.0 ** -24 * scale.max() * 4 * 1.01 + 1e-12  # |g_ent| <= 2, |g_lp| <= 1 on the lse shift
    assert np.abs(grad - gt)[rows].max() <= gscale


def test_argmax_is_first_maximum_unmasked():
    for A in (1, 5, 130):
        x, inv = C.argmax_case(4, 6, A, seed=A)
        ref = R.argmax(x, 6, A)
        tor = torch.from_numpy(x).reshape(4, 6, A).argmax(-1).numpy()
        assert np.array_equal(ref, tor)
        xs = x.reshape(4, 6, A)
        for b in range(4):
            for v in range(6):
                j = ref[b, v]
                assert xs[b, v, j] == xs[b, v].max() and (xs[b, v, :j] < xs[b, v, j]).all()
    x, _ = C.argmax_case(4, 6, 130, seed=1)  # the forced ties really are ties
    xs = x.reshape(24, 130)
    assert ((xs == xs.max(-1, keepdims=True)).sum(-1) >= 2).sum() >= 18


def test_lane_major_order():
    assert list(R.lane_major_order(6, 4)) == [0, 4, 1, 5, 2, 3]
    assert list(R.lane_major_order(3, 16)) == [0, 1, 2]
    o = R.lane_major_order(1000, 64)
    assert sorted(o) == list(range(1000)) and list(o[:3]) == [0, 64, 128]


def test_draw_matches_a_plain_loop_and_the_law():
    """The vectorised inverse-CDF draw equals a per-row Python loop over the
    ordered categories, and over many uniforms follows Categorical's probs."""
    V, A = 3, 23
    x, inv, _ = C.sample_case(4, V, A, seed=2)
    order = R.lane_major_order(A, 4)
    u = R.sample_uniforms(77, 5, 4 * V)
    act, dist, lo, hi = R.sample(x, V, A, inv, u, order)
    xm = R.masked(x, V, A, inv).reshape(-1, A)
    for r in range(4 * V):
        p = np.exp(xm[r] - xm[r].max())
        t, c, pick, prev = u[r] * p.sum(), 0.0, None, -1
        bounds = [0.0]
        for j in order:
            if p[j] > 0:
                c += p[j]
                bounds.append(c)
                if pick is None and t < c:
                    pick = j
                    assert lo.reshape(-1)[r] == prev
                if pick is None:
                    prev = j
        assert pick == act.reshape(-1)[r]
        assert abs(min(abs(b - t) for b in bounds) / p.sum() - dist.reshape(-1)[r]) < 1e-12
    # the law: one row, 200 000 uniforms of the stream
    row = np.repeat(x.reshape(-1, A)[5:6], 200000, 0)
    rinv = np.repeat(inv.reshape(-1, 1, A)[5:6], 200000, 0)
    a, _, _, _ = R.sample(row, 1, A, rinv, R.sample_uniforms(3, 0, 200000), order)
    q = torch.distributions.Categorical(logits=torch.from_numpy(xm[5])).probs.numpy()
    cnt = np.bincount(a.reshape(-1), minlength=A)
    sd = np.sqrt(200000 * q * (1 - q)) + 1e-9
    assert (np.abs(cnt - 200000 * q) <= 5 * sd + 1).all()


def test_coin_forbids():
    x, inv, P, kind = C.wait_case(8, 9, 12, seed=4)
    for ratio in (0.0, 0.3, 1.0):
        f = R.coin_forbids(inv, P, ratio, seed=11, offset=3)
        u = R.uniforms(11 ^ R.COIN_STREAM, 3, 72).reshape(8, 9)
        assert not f[(kind == 1) | (kind == 2)].any()
        q = (kind == 0) | (kind == 3)
        assert np.array_equal(f[q], (u > float(np.float32(ratio)))[q])
    assert not R.coin_forbids(inv, P, 1.0, 11, 3).any()
    assert R.coin_forbids(inv, P, 0.0, 11, 3)[(kind == 0) | (kind == 3)].mean() > 0.9
    assert not R.coin_forbids(inv, P, -1.0, 11, 3).any()
    g = R.with_forbidden(inv, R.coin_forbids(inv, P, 0.0, 11, 3), P)
    assert g[kind == 3].all(-1).mean() > 0.9 and not inv[kind == 3][:, P].any()


def test_near_boundary_share_of_the_sampling_inputs():
    """The SAMPLE inputs of the GPU tests: the share of rows whose u * total
    lies within 64 * 2^-24 * total of a CDF boundary is at most 0.5 % (the GPU
    tests allow such rows a neighbouring category), per input and overall."""
    tot = near = 0
    for name, (x, inv, skip, V, A, G, seed, off) in C.sample_inputs():
        rows = x.shape[0] * V
        u = R.sample_uniforms(seed, off, rows)
        _, dist, _, _ = R.sample(x, V, A, inv, u, R.lane_major_order(A, G))
        n = int(((dist <= R.BAND) & ~skip).sum())
        assert n <= 0.005 * rows, (name, n, rows)
        tot, near = tot + rows, near + n
    print(f"near rows: {near} of {tot}")
    assert near <= 0.005 * tot and tot > 5000


def test_gae_loop_matches_torch_f64():
    r, d, v, nv = C.gae_case(17, 33, "random", seed=1)
    adv, ret = R.gae(r, d, v, nv, 0.99, 0.95)
    g, l = float(np.float32(0.99)), float(np.float32(0.95))
    a_t, r_t = torch_gae(*(torch.from_numpy(t).double() for t in (r, d, v, nv)), g, l)
    assert np.abs(adv - a_t.numpy()).max() < 1e-12 and np.abs(ret - r_t.numpy()).max() < 1e-12
