"""Every instantiation of the masked head kernels against the float64
reference tests/head_ref.py (inputs and the tolerance rule: tests/head_cases.py).

vmp_policy_head / vmp_policy_head_backward (csrc/vmp_policy.hip):
  tile      k_head_fwd_tile / k_head_bwd_tile: A <= 128, 16-byte aligned tensors
  group     k_head_fwd/bwd<G, E>: A > 128
  group_misaligned  the same kernels at A <= 128, reached through logits and
            dlogits that start 4 bytes past alignment (a contiguous view)
so all seven (G, E) of pick_g / pick_e run forward and backward, in GIVEN,
ARGMAX, SAMPLE and with the WAIT coin. vmp_actor_head (every row_task<KQ>
bucket, NT 4 / 8 / 13, NW 4 / 8, one and two epilogue stages) and
vmp_actor_mlp_head_f32 (lane_row<16> / <0>, TPW3 1..4) are judged through
their logits_out, so GEMM rounding cannot move a CDF boundary; vmp_gae
against an f64 loop.

SAMPLE is checked deterministically: the reference predicts each row's
uniform and walks the categories in the kernel's documented order; outside
64 * 2^-24 * total of a CDF boundary the action must be the reference's.
"""
import numpy as np
import pytest
import torch

from tests import head_cases as C
from tests import head_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SAMPLE, GIVEN, ARGMAX = 0, 1, 2


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    yield
    print("\n| family | mode | quantity | max kernel err | max e_ref | err / e_ref | bound used |")
    print("|---|---|---|---|---|---|---|")
    for (fam, mode, q), (err, e_ref, used) in sorted(C.RATIOS.items()):
        ratio = f"{err / e_ref:.2f}" if e_ref > 0 else "-"
        print(f"| {fam} | {mode} | {q} | {err:.2e} | {e_ref:.2e} | {ratio} | {used:.2f} |")


# ------------------------------------------------------------------ plumbing
def _dev(x, misaligned=False):
    """numpy -> device tensor of the same shape; misaligned: a contiguous view
    that starts at element 1 of a buffer one element longer."""
    t = torch.from_numpy(np.ascontiguousarray(x))
    if not misaligned:
        out = t.to(DEV)
        assert out.data_ptr() % 16 == 0
        return out
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    return view


def _bits(inv):
    return torch.from_numpy(C.pack_bits(inv)).to(DEV)


def _head(lg, bits, V, A, mode, action=None, seed=0, off=0, ctr=None, ratio=-1.0, P=-1):
    """vmp_policy_head on the tensors as they are (no copies: alignment decides the kernel)."""
    from vmp._lib import check, lib, ptr
    from vmp.head import _stream
    B = lg.shape[0]
    if mode == GIVEN:
        act = torch.from_numpy(np.asarray(action, np.int32).reshape(B, V)).to(DEV)
    else:
        act = torch.full((B, V), -7, dtype=torch.int32, device=DEV)
    lp = ent = ws = None
    if mode != ARGMAX:
        lp = torch.full((B,), 777.0, dtype=torch.float32, device=DEV)
        ent = torch.full((B,), 777.0, dtype=torch.float32, device=DEV)
        ws = torch.empty((2 * B * V,), dtype=torch.float32, device=DEV)
    check(lib().vmp_policy_head(B, V, A, mode, ptr(lg), ptr(bits), float(ratio), int(P), seed, off,
                                ptr(ctr), ptr(act), ptr(lp), ptr(ent), ptr(ws), _stream(lg)))
    torch.cuda.synchronize()
    f = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
    return f(act), f(lp), f(ent)


def _backward(lg, bits, V, A, action, g_lp, g_ent, misaligned):
    from vmp._lib import check, lib, ptr
    from vmp.head import _stream
    B = lg.shape[0]
    act = torch.from_numpy(np.asarray(action, np.int32).reshape(B, V)).to(DEV)
    d = _dev(np.full((B, V * A), np.nan, np.float32), misaligned)
    glp = None if g_lp is None else _dev(np.asarray(g_lp, np.float32))
    gen = None if g_ent is None else _dev(np.asarray(g_ent, np.float32))
    check(lib().vmp_policy_head_backward(B, V, A, ptr(lg), ptr(bits), ptr(act), ptr(glp), ptr(gen),
                                         ptr(d), _stream(lg)))
    torch.cuda.synchronize()
    return d.cpu().numpy().reshape(B, V, A)


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.int32), np.asarray(b, np.float32).view(np.int32))


def _judge_given(fam, lp, ent, logits, V, A, inv, act, mode="given"):
    ref_lp, ref_ent, _, _ = R.head_given(logits, V, A, inv, act)
    tor_lp, tor_ent, _ = C.torch_f32(logits, V, A, inv, act)
    fl = C.floor_sum(V, logits, inv)
    C.judge((fam, mode, "logprob"), lp, ref_lp, tor_lp, fl, C.lp_groups(ref_lp, fl, V))
    C.judge((fam, mode, "entropy"), ent, ref_ent, tor_ent, fl)


def _judge_draw(act, logits, V, A, inv, u, G, skip, what):
    ref_act, dist, lo, hi = R.sample(logits, V, A, inv, u, R.lane_major_order(A, G))
    assert ((act >= 0) & (act < A)).all(), what
    ok, near = R.judge_draw(act, ref_act, dist, lo, hi, skip)
    bad = np.argwhere(~ok)
    assert len(bad) == 0, (what, "rows", bad[:5].tolist(), "got", act[~ok][:5], "want", ref_act[~ok][:5],
                           "dist", dist[~ok][:5])
    assert near <= 0.005, (what, near)
    taken = np.take_along_axis(inv, act.astype(np.int64)[..., None], -1)[..., 0]
    assert not (taken & ~skip).any(), what
    return ref_act


# --------------------------------------------------- vmp_policy_head's matrix
@pytest.mark.parametrize("fam,A", C.HEAD_PARAMS)
def test_policy_head_given_forward_backward(fam, A):
    """GIVEN forward and the backward with (g_lp, g_ent), (g_lp, None) and
    (None, g_ent), at a common logit offset of 0, +20 and -20. Gradient floor:
    2^-23 (max|g_lp| + max|g_ent| (1 + max|x_valid|)), see tests/head_cases.py."""
    mis = fam == "group_misaligned"
    for B, V in C.shapes(fam, A):
        rs = np.random.RandomState(A + V)
        g1, g2 = rs.randn(B).astype(np.float32), rs.randn(B).astype(np.float32)
        for shift in (0.0, 20.0, -20.0):
            c = C.given_case(B, V, A, seed=A * 100 + V, shift=shift)
            logits, inv, act = c["logits"], c["invalid"], c["action"]
            lg, bits = _dev(logits, mis), _bits(inv)
            a, lp, ent = _head(lg, bits, V, A, GIVEN, action=act)
            assert np.array_equal(a, act)
            _judge_given(fam, lp, ent, logits, V, A, inv, act)
            oor = ((act < 0) | (act >= A))[..., None]  # no gradient is defined for a NaN logprob
            for glp, gen in ((g1, g2), (g1, None), (None, g2)):
                d = _backward(lg, bits, V, A, act, glp, gen, mis)
                assert np.isfinite(d).all() and (d[inv] == 0).all()
                ref = R.head_grad(logits, V, A, inv, act, glp, gen)
                _, _, tor = C.torch_f32(logits, V, A, inv, act, glp, gen)
                z = lambda t: np.where(oor, 0.0, t)  # noqa: E731
                C.judge((fam, "given", "grad"), z(d), z(ref), z(tor), C.floor_grad(logits, inv, glp, gen))


@pytest.mark.parametrize("fam,A", C.HEAD_PARAMS)
def test_policy_head_argmax_exact(fam, A):
    """get_det_action: the first maximum of the unmasked row, ties built on
    purpose across lanes and elements; the mask (passed on odd A) is ignored."""
    for B, V in C.shapes(fam, A):
        logits, inv = C.argmax_case(B, V, A, seed=A * 10 + V)
        lg = _dev(logits, fam == "group_misaligned")
        a, _, _ = _head(lg, _bits(inv) if A % 2 else None, V, A, ARGMAX)
        assert np.array_equal(a, R.argmax(logits, V, A)), (V, np.argwhere(a != R.argmax(logits, V, A))[:5])


@pytest.mark.parametrize("fam,A", C.HEAD_PARAMS)
def test_policy_head_sample_deterministic(fam, A):
    """SAMPLE against the reference's prediction of every row's draw; the
    returned logprob / entropy equal GIVEN mode on the returned actions bit for bit."""
    G = C.lanes(fam, A)
    for B, V in C.shapes(fam, A):
        logits, inv, skip = C.sample_case(B, V, A, seed=A * 100 + V)
        seed, off = C.sample_seed(A, V)
        lg, bits = _dev(logits, fam == "group_misaligned"), _bits(inv)
        act, lp, ent = _head(lg, bits, V, A, SAMPLE, seed=seed, off=off)
        _judge_draw(act, logits, V, A, inv, R.sample_uniforms(seed, off, B * V), G, skip, (fam, A, V))
        _, lp2, ent2 = _head(lg, bits, V, A, GIVEN, action=act)
        assert _same_bits(lp, lp2) and _same_bits(ent, ent2), (V, lp, lp2)
        _judge_given(fam, lp, ent, logits, V, A, inv, act, "sample")


@pytest.mark.parametrize("fam,A", C.HEAD_PARAMS)
def test_policy_head_wait_coin_deterministic(fam, A):
    """PPOAgent.act's coin per row: the kernel forbids WAIT exactly on the rows
    the reference's coin stream forbids it (ratios 0.0, 0.3, 1.0). WAIT has
    logit +30, so outside the rounding band the action is WAIT exactly when
    WAIT is valid and not forbidden; a flipped only-WAIT row is all masked and
    may give any index."""
    G = C.lanes(fam, A)
    for B, V in C.shapes(fam, A):
        logits, inv, P, kind = C.wait_case(B, V, A, seed=A * 100 + V + 1)
        lg, bits = _dev(logits, fam == "group_misaligned"), _bits(inv)
        for i, ratio in enumerate((0.0, 0.3, 1.0)):
            seed, off = 7 + A, 1000 * i + V
            act, lp, ent = _head(lg, bits, V, A, SAMPLE, seed=seed, off=off, ratio=ratio, P=P)
            forbid = R.coin_forbids(inv, P, ratio, seed, off)
            inv2 = R.with_forbidden(inv, forbid, P)
            skip = inv2.all(-1)
            u = R.sample_uniforms(seed, off, B * V)
            _, dist, _, _ = R.sample(logits, V, A, inv2, u, R.lane_major_order(A, G))
            _judge_draw(act, logits, V, A, inv2, u, G, skip, (fam, A, V, ratio))
            clear = ~skip & (dist > R.BAND)
            assert np.array_equal((act == P)[clear], (~inv2[..., P])[clear]), (V, ratio)
            if ratio == 1.0:
                assert not forbid.any()
            # GIVEN with the same coin sees the same rows forbidden
            _, lp2, ent2 = _head(lg, bits, V, A, GIVEN, action=act, seed=seed, off=off, ratio=ratio, P=P)
            assert _same_bits(lp, lp2) and _same_bits(ent, ent2), (V, ratio)
            _judge_given(fam, lp, ent, logits, V, A, inv2, act, "wait")


@pytest.mark.parametrize("V,A", [(27, 33), (7, 129)])
def test_policy_head_sample_graph_counter(V, A):
    """HeadRng.graph_counter: the device counter's value (0, then 1) is mixed
    into the seed of both the sampling and the coin stream."""
    from vmp.head import HeadRng, policy_head
    B, G = 8, (4 if A <= 128 else C.group_width(A))
    logits, inv, P, _ = C.wait_case(B, V, A, seed=3)
    lg, bits = _dev(logits), _bits(inv)
    rng = HeadRng(77).graph_counter(DEV)
    for counter in (0, 1):
        assert int(rng.counter[0]) == counter
        with torch.no_grad():
            act, _, _ = policy_head(lg, V, A, bits=bits, rng=rng, wait_ratio=0.5, wait_index=P)
        act = act.cpu().numpy()
        forbid = R.coin_forbids(inv, P, 0.5, 77, 0, counter)
        inv2 = R.with_forbidden(inv, forbid, P)
        u = R.sample_uniforms(77, 0, B * V, counter)
        _judge_draw(act, logits, V, A, inv2, u, G, inv2.all(-1), (A, counter))
    assert not np.array_equal(R.sample_uniforms(77, 0, 8, 0), R.sample_uniforms(77, 0, 8, 1))


def test_group_head_sampling_law_and_validity():
    """test_head_sampling_law_and_validity on the group kernels (A = 129):
    per-category frequencies within 5 sigma, never a masked action."""
    from vmp.head import HeadRng, pack_mask, policy_head
    V, A, B = 2, 129, 20000
    g = torch.Generator().manual_seed(7)
    row = torch.randn((V, A), generator=g)
    mask = torch.rand((V, A), generator=g) < 0.4
    mask[:, 10] = False
    logits = row.reshape(1, -1).repeat(B, 1).to(DEV)
    bits = pack_mask(mask.to(DEV).expand(B, V, A), V, A)
    rng = HeadRng(123)
    with torch.no_grad():
        act, lp, _ = policy_head(logits, V, A, bits=bits, rng=rng)
        act2, _, _ = policy_head(logits, V, A, bits=bits, rng=rng)
    act = act.cpu().long()
    assert not torch.equal(act, act2.cpu().long())  # the stream advances
    assert not mask.gather(1, act.T).any()
    p = torch.softmax(row.masked_fill(mask, -1e7).double(), -1)
    for v in range(V):
        cnt = torch.bincount(act[:, v], minlength=A).double()
        sd = torch.sqrt(B * p[v] * (1 - p[v])) + 1e-9
        assert torch.all((cnt - B * p[v]).abs() <= 5 * sd + 1), v
    ref_lp = torch.log_softmax(row.masked_fill(mask, -1e7), -1).gather(1, act.T).sum(0)
    torch.testing.assert_close(lp.cpu(), ref_lp, rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------ the fused paths
def _fused_masks(B, V, A, seed):
    """(GIVEN invalid, GIVEN action, SAMPLE invalid, SAMPLE skip, WAIT invalid, P) for a fused shape."""
    c = C.given_case(B, V, A, seed)
    _, s_inv, s_skip = C.sample_case(B, V, A, seed + 1)
    _, w_inv, P, _ = C.wait_case(B, V, A, seed + 2)
    return c["invalid"], c["action"], s_inv, s_skip, w_inv, P


def _fused_modes(fam, run, B, V, A, seed, set_wait_bias):
    """The four modes of a fused head. run(mode, bits, action, rng, ratio, P)
    -> (action, logprob, entropy, logits) as numpy; the reference is fed the
    launch's own f32 logits."""
    from vmp.head import HeadRng
    g_inv, g_act, s_inv, s_skip, w_inv, P = _fused_masks(B, V, A, seed)
    a, lp, ent, lg = run(GIVEN, g_inv, g_act, None, -1.0, -1)
    assert np.array_equal(a, g_act)
    _judge_given(fam, lp, ent, lg, V, A, g_inv, g_act)
    a, _, _, lg = run(ARGMAX, g_inv, None, None, -1.0, -1)
    assert np.array_equal(a, R.argmax(lg, V, A)), "argmax"
    rng = HeadRng(31 + A)
    rng.offset = 5 * V
    a, lp, ent, lg = run(SAMPLE, s_inv, None, rng, -1.0, -1)
    _judge_draw(a, lg, V, A, s_inv, R.sample_uniforms(31 + A, 5 * V, B * V), 4, s_skip, (fam, "sample"))
    _, lp2, ent2, _ = run(GIVEN, s_inv, a, None, -1.0, -1)
    assert _same_bits(lp, lp2) and _same_bits(ent, ent2), "sample vs given"
    _judge_given(fam, lp, ent, lg, V, A, s_inv, a, "sample")
    set_wait_bias(P)
    for i, ratio in enumerate((0.0, 0.3, 1.0)):
        rng = HeadRng(9 + A)
        rng.offset = 100 * i + 3
        a, lp, ent, lg = run(SAMPLE, w_inv, None, rng, ratio, P)
        forbid = R.coin_forbids(w_inv, P, ratio, 9 + A, 100 * i + 3)
        inv2 = R.with_forbidden(w_inv, forbid, P)
        skip = inv2.all(-1)
        u = R.sample_uniforms(9 + A, 100 * i + 3, B * V)
        _, dist, _, _ = R.sample(lg, V, A, inv2, u, R.lane_major_order(A, 4))
        _judge_draw(a, lg, V, A, inv2, u, 4, skip, (fam, "wait", ratio))
        clear = ~skip & (dist > R.BAND)
        assert np.array_equal((a == P)[clear], (~inv2[..., P])[clear]), ratio
        _judge_given(fam, lp, ent, lg, V, A, inv2, a, "wait")


# (B, K, V, A): row_task<8> A 20, 32; <16> A 49, 64; <24> A 81, 96; k_head_gemm<NT, NW>
ACTOR_HEAD_SHAPES = [
    (7, 32, 3, 20),       # <4, 4>
    (9, 64, 5, 32),       # <4, 4>
    (70, 32, 4, 49),      # <4, 4>, two row blocks, the second ragged
    (5, 96, 6, 64),       # <4, 4>
    (66, 64, 3, 81),      # <8, 4>
    (8, 32, 7, 96),       # <8, 4>
    (129, 32, 128, 20),   # <4, 8>
    (130, 32, 256, 128),  # <8, 8>, the whole C tile in one epilogue stage
    (65, 32, 512, 81),    # <13, 8>: two segments per tile (BN 176), two epilogue stages
]


@pytest.mark.parametrize("B,K,V,A", ACTOR_HEAD_SHAPES)
def test_actor_head_modes(B, K, V, A):
    from vmp.head import actor_head
    rs = np.random.RandomState(B + K + V + A)
    h = np.tanh(rs.randn(B, K)).astype(np.float32)
    w = (rs.randn(V, A, K) * (2.0 / K ** 0.5)).astype(np.float32)
    b = (rs.randn(V, A) * 0.1).astype(np.float32)
    j1, j2 = A - 1, max(0, A - 6)           # an exact tie of the two largest logits per row
    w[:, j2], b[:, j2] = w[:, j1], b[:, j1]
    b[1:, j1] += 4.0
    b[1:, j2] += 4.0
    b_wait = b.copy()                       # the WAIT phase: nothing may outweigh WAIT's +30
    b[0, rs.randint(A)] += 60.0             # VM row 0: one logit ~60 above the rest
    ht, wt = _dev(h), _dev(w.reshape(V * A, K))
    bias = {"t": _dev(b.reshape(-1))}
    fam = "actor_head"

    def run(mode, inv, action, rng, ratio, P):
        out = torch.full((B, V * A), float("nan"), device=DEV)
        act = None if action is None else torch.from_numpy(np.asarray(action, np.int32)).to(DEV)
        a, lp, ent = actor_head(ht, wt, bias["t"], V, A, bits=_bits(inv), action=act, rng=rng, mode=mode,
                                wait_ratio=ratio, wait_index=P, logits_out=out)
        torch.cuda.synchronize()
        lg = out.cpu().numpy()
        ref = h.astype(np.float64) @ w.reshape(V * A, K).astype(np.float64).T + bias["np"].astype(np.float64)
        tor = torch.addmm(torch.from_numpy(bias["np"]), torch.from_numpy(h),
                          torch.from_numpy(w.reshape(V * A, K)).t()).numpy()
        C.judge((fam, "gemm", "logits"), lg, ref, tor, C.EPS * float(np.abs(ref).max()))
        f = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
        return f(a), f(lp), f(ent), lg

    def set_wait_bias(P):
        nb = b_wait.copy()
        nb[:, P] = 30.0
        bias["np"], bias["t"] = nb.reshape(-1), _dev(nb.reshape(-1))

    bias["np"] = b.reshape(-1)
    shifts = (0.0, 20.0) if B * V < 2000 else (0.0,)
    for shift in shifts:
        nb = (b + np.float32(shift)).astype(np.float32).reshape(-1)
        bias["np"], bias["t"] = nb, _dev(nb)
        _fused_modes(fam, run, B, V, A, seed=B + V + A, set_wait_bias=set_wait_bias)


# (B, D, H, V, A): lane_row<16> at A 16, lane_row<0> at A 17; V A in each TPW3 range
MLP_HEAD_SHAPES = [(37, 20, 32, 8, 16), (20, 33, 64, 15, 17), (18, 16, 32, 24, 16), (33, 24, 64, 30, 17)]


@pytest.mark.parametrize("B,D,H,V,A", MLP_HEAD_SHAPES)
def test_actor_mlp_head_modes(B, D, H, V, A):
    from torch import nn

    from vmp.head import actor_mlp_head
    N = V * A
    assert (N + 127) // 128 == MLP_HEAD_SHAPES.index((B, D, H, V, A)) + 1  # TPW3 1..4
    g = torch.Generator().manual_seed(B + D + H + N)
    seq = nn.Sequential(nn.Linear(D, H), nn.Tanh(), nn.Linear(H, H), nn.Tanh(), nn.Linear(H, N))
    with torch.no_grad():
        for m in seq:
            if isinstance(m, nn.Linear):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (1.5 / m.in_features ** 0.5))
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
        w3, b3 = seq[4].weight.view(V, A, H), seq[4].bias.view(V, A)
        j1, j2 = A - 1, A - 6                # an exact tie of the two largest logits per row
        w3[:, j2], b3[:, j2] = w3[:, j1], b3[:, j1]
        b3[1:, j1] += 4.0
        b3[1:, j2] += 4.0
        b3[0, 3] += 60.0                     # VM row 0: one logit ~60 above the rest
    cpu = seq
    dev = nn.Sequential(*[nn.Linear(m.in_features, m.out_features) if isinstance(m, nn.Linear) else nn.Tanh()
                          for m in seq]).to(DEV)
    dev.load_state_dict(cpu.state_dict())
    x = torch.rand((B, D), generator=g)
    xt = x.to(DEV)
    fam = "actor_mlp_head"

    def run(mode, inv, action, rng, ratio, P):
        out = torch.full((B, N), float("nan"), device=DEV)
        act = None if action is None else torch.from_numpy(np.asarray(action, np.int32)).to(DEV)
        a, lp, ent = actor_mlp_head(xt, dev[0], dev[2], dev[4], V, A, bits=_bits(inv), action=act, rng=rng,
                                    mode=mode, wait_ratio=ratio, wait_index=P, logits_out=out)
        torch.cuda.synchronize()
        lg = out.cpu().numpy()
        with torch.no_grad():
            tor = cpu(x).numpy()
            hh = x.double()
            for m in cpu:
                hh = (hh @ m.weight.double().t() + m.bias.double()) if isinstance(m, nn.Linear) else torch.tanh(hh)
        ref = hh.numpy()
        # k_actor_mlp starts its accumulators at the bias, so each of the last
        # layer's Hp / 4 MFMA steps (Hp: H padded to 128) rounds at the logit's
        # size, where torch adds the bias once at the end: the floor is
        # Hp / 4 + 1 roundings of the largest logit, not one (measured: 2.1e-5
        # at |logit| 60, 10 x torch's error, 6 roundings)
        steps = (H + 127) // 128 * 128 // 4 + 1
        C.judge((fam, "mlp", "logits"), lg, ref, tor, steps * 0.5 * C.EPS * float(np.abs(ref).max()))
        f = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
        return f(a), f(lp), f(ent), lg

    def set_wait_bias(P):
        with torch.no_grad():
            cpu[4].bias.view(V, A)[0, 3] -= 60.0  # nothing may outweigh WAIT's +30
            cpu[4].bias.view(V, A)[:, P] = 30.0
            dev[4].bias.copy_(cpu[4].bias)

    _fused_modes(fam, run, B, V, A, seed=B + N, set_wait_bias=set_wait_bias)


# ------------------------------------------------------------------------ GAE
@pytest.mark.parametrize("T,N", [(1, 1), (3, 257), (17, 600), (100, 37)])
def test_gae_vs_float64_loop(T, N):
    """vmp_gae (one lane per column, 256 per block: one block, a block and one
    lane, two full blocks and a tail) against an f64 loop; done patterns none,
    all, only the last step, random 5 %. Floor: 2^-23 max(1, max|adv|, max|ret|)."""
    from vmp.head import gae
    for k, pattern in enumerate(("none", "all", "last", "random")):
        r, d, v, nv = C.gae_case(T, N, pattern, seed=T * 7 + N + k)
        adv, ret = gae(*(_dev(t) for t in (r, d, v, nv)), 0.99, 0.95)
        torch.cuda.synchronize()
        ref_a, ref_r = R.gae(r, d, v, nv, 0.99, 0.95)
        tor_a, tor_r = C.gae_torch_f32(r, d, v, nv, 0.99, 0.95)
        fl = C.EPS * max(1.0, float(np.abs(ref_a).max()), float(np.abs(ref_r).max()))
        C.judge(("gae", pattern, "advantage"), adv.cpu().numpy(), ref_a, tor_a, fl)
        C.judge(("gae", pattern, "return"), ret.cpu().numpy(), ref_r, tor_r, fl)
