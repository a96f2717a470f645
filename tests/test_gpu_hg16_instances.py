"""Every instantiation and launch plan of the bf16 fused actor head
(csrc/vmp_headgemm_bf16.hip: k_hg16<TS, BWD, 8, SMP> for TS = 1..8 in forward
GIVEN, backward and SAMPLE, and k_dsum) against the float64 reference
tests/head_ref.py, one test per case of tests/hg16_cases.py.

The kernels have no logits_out, so the operands are built to make the logits
exact (tests/hg16_cases.py: every partial sum of b + h W^T is a multiple of
2^-7 below 2^9): the reference knows the logits the kernel forms bit for bit,
and what is judged is the epilogue, the lane mapping and the plan, not MFMA
summation order. One case with ordinary operands judges the accumulation.

  forward GIVEN  |kernel - head_ref| <= 4 e_ref + floor (tests/head_cases.py),
                 NaN exactly where the reference has NaN;
  SAMPLE, coin   row by row against the reference's inverse-CDF draw in
                 action order with the kernel's own uniforms (head_ref.BAND);
                 logprob / entropy bit-identical to GIVEN on the drawn actions;
  backward       with e = 4 e_ref + floor_grad every stored bf16 lies in
                 [bf16_rne(d - e), bf16_rne(d + e)] (round to nearest even of
                 a value within e of d: a derived bound, not a measured one),
                 exactly 0 at masked j, sentinel kept outside [B] x [V A];
                 dbias against its start + sum_b d in f64;
  dense case     every floor (logprob, entropy, gradient, dbias) gains the one
                 term V 2^-23 max_n sum_k |h_k w_nk|; SAMPLE: validity and
                 the GIVEN identity only.
"""
import numpy as np
import pytest
import torch

from tests import head_cases as C
from tests import head_ref as R
from tests import hg16_cases as H

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -7.75  # bf16-exact; dlogits outside the written block keep its bits
SEEN = set()  # what the cases that ran launched (Case.selects())
RAN = set()   # their names


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    yield
    print("\n| family | mode | quantity | max kernel err | max e_ref | err / e_ref | bound used |")
    print("|---|---|---|---|---|---|---|")
    for (fam, mode, q), (err, e_ref, used) in sorted(C.RATIOS.items()):
        if not fam.startswith("k_hg16"):  # the dictionary is shared with test_gpu_head_instances.py
            continue
        ratio = f"{err / e_ref:.2f}" if e_ref > 0 else "-"
        print(f"| {fam} | {mode} | {q} | {err:.2e} | {e_ref:.2e} | {ratio} | {used:.3f} |")
    print("instantiations run:", sorted(str(s) for s in SEEN if s == "k_dsum" or s[0] == "k_hg16"))
    if RAN >= {c.name for c in H.CASES}:  # every case ran (not a -k selection): all 24 kernels and k_dsum did
        want = {("k_hg16", ts, m) for ts in range(1, 9) for m in ("fwd", "bwd", "smp")} | {"k_dsum"}
        assert want <= SEEN, sorted(str(s) for s in want - SEEN)


# ------------------------------------------------------------------ plumbing
class Ops:
    """A case's operands on the device: bf16 h [B, K] and W [V A, K], f32 bias."""

    def __init__(self, d):
        self.h = torch.from_numpy(d["h"]).to(DEV).to(torch.bfloat16)
        self.w = torch.from_numpy(d["w"]).to(DEV).to(torch.bfloat16)
        self.bias = torch.from_numpy(d["bias"]).to(DEV)


def _bits(c, inv):
    return torch.from_numpy(C.pack_bits(inv)).to(DEV) if c.bits else None


def _np(t):
    return t.cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.int32), np.asarray(b, np.float32).view(np.int32))


def _fam(c):
    return "k_hg16 dense" if c.dense else "k_hg16"


def _forward(o, c, bits, action):
    from vmp.head import actor_head_bf16_fwd
    act = torch.from_numpy(np.asarray(action, np.int32).reshape(c.B, c.V)).to(DEV)
    _, lp, ent = actor_head_bf16_fwd(o.h, o.w, o.bias, c.V, c.A, bits, act)
    torch.cuda.synchronize()
    return _np(lp), _np(ent)


def _sample(o, c, bits, rng, ratio=-1.0, P=-1):
    from vmp.head import actor_head_bf16_sample
    act, lp, ent = actor_head_bf16_sample(o.h, o.w, o.bias, c.V, c.A, bits, rng, wait_ratio=ratio, wait_index=P)
    torch.cuda.synchronize()
    return _np(act), _np(lp), _np(ent)


def _judge_given(c, d, lp, ent, inv, act, mode):
    """logprob / entropy by the 4 e_ref + floor rule; the dense case: reference on
    the f64 product, f32 side on torch's addmm, floor + V roundings of a logit's
    absolute sum."""
    ref_lp, ref_ent, _, _ = R.head_given(d["logits"], c.V, c.A, inv, act)
    tor_lp, tor_ent, _ = C.torch_f32(d["logits_f32"] if c.dense else d["logits"], c.V, c.A, inv, act)
    fl = C.floor_sum(c.V, d["logits"], inv) + (H.dense_floor_gain(c, d) if c.dense else 0.0)
    C.judge((_fam(c), mode, "logprob"), lp, ref_lp, tor_lp, fl, C.lp_groups(ref_lp, fl, c.V))
    C.judge((_fam(c), mode, "entropy"), ent, ref_ent, tor_ent, fl)


def _judge_draw(act, ref_act, dist, lo, hi, inv, skip, A, what):
    assert ((act >= 0) & (act < A)).all(), what
    ok, near = R.judge_draw(act, ref_act, dist, lo, hi, skip)
    bad = np.argwhere(~ok)
    assert len(bad) == 0, (what, "rows", bad[:5].tolist(), "got", act[~ok][:5], "want", ref_act[~ok][:5],
                           "dist", dist[~ok][:5])
    assert near <= 0.005, (what, near)
    taken = np.take_along_axis(inv, act.astype(np.int64)[..., None], -1)[..., 0]
    assert not (taken & ~skip).any(), what


def _record(key, err, e_ref, used):
    rec = C.RATIOS.setdefault(key, [0.0, 0.0, 0.0])
    rec[0], rec[1], rec[2] = max(rec[0], err), max(rec[1], e_ref), max(rec[2], used)
    print(f"HEADERR {key} err {err:.3e} e_ref {e_ref:.3e} used {used:.3f}")


# --------------------------------------------------------------------- modes
def run_given(c, d, o):
    bits = _bits(c, d["invalid"])
    lp, ent = _forward(o, c, bits, d["action"])
    _judge_given(c, d, lp, ent, d["invalid"], d["action"], "given")
    lp2, ent2 = _forward(o, c, bits, d["action"])
    assert _same_bits(lp, lp2) and _same_bits(ent, ent2)


def _backward(o, c, d, bits, g_lp, g_ent, workspace):
    from vmp.head import actor_head_bf16_bwd, bf16_bwd_workspace
    act = torch.from_numpy(np.asarray(d["action"], np.int32)).to(DEV)
    out = torch.full((c.B + 3, c.ld), SENTINEL, dtype=torch.bfloat16, device=DEV)
    db = torch.from_numpy(d["dbias0"]).to(DEV).clone()
    ws = None
    if workspace:  # NaN: a partial read before it is written would show
        ws = torch.full((bf16_bwd_workspace(c.B, c.V, c.A),), float("nan"), dtype=torch.float32, device=DEV)
    t = lambda g: None if g is None else torch.from_numpy(g).to(DEV)  # noqa: E731
    actor_head_bf16_bwd(o.h, o.w, o.bias, c.V, c.A, bits, act, t(g_lp), t(g_ent), out, dbias=db, workspace=ws)
    torch.cuda.synchronize()
    return _np(out.view(torch.int16)), _np(out.float()).astype(np.float64), _np(db)


def run_bwd(c, d, o):
    bits = _bits(c, d["invalid"])
    inv, N = d["invalid"], c.V * c.A
    sent = _np(torch.tensor([SENTINEL], dtype=torch.bfloat16).view(torch.int16))[0]
    for i, which in enumerate(c.grads):
        g_lp, g_ent, ref, tor, ok = H.grad_reference(c, d, which)
        raw, val, db = _backward(o, c, d, bits, g_lp, g_ent, workspace=i == 0)
        assert (raw[c.B:] == sent).all() and (raw[:, N:] == sent).all(), "wrote outside [B] x [V A]"
        got = val[:c.B, :N].reshape(c.B, c.V, c.A)
        assert np.isfinite(got).all() and (got[inv] == 0).all()
        # dlogits: an interval of bf16 values around d
        e_ref = float(np.abs(np.where(ok, tor - ref, 0.0)).max())
        e = 4.0 * e_ref + C.floor_grad(d["logits"], inv, g_lp, g_ent)
        if c.dense:
            e += H.dense_floor_gain(c, d)
        lo, hi = H.bf16_rne(ref - e), H.bf16_rne(ref + e)
        # measured: the least error of the kernel's f32 value before its rounding
        # (how far d lies outside the cell of reals that round to the stored value)
        c_lo, c_hi = H.bf16_cell(got)
        need = float(np.where(ok, np.maximum(0.0, np.maximum(c_lo - ref, ref - c_hi)), 0.0).max())
        _record((_fam(c), "bwd", "dlogits (before bf16)"), need, e_ref, need / e if e > 0 else float(need > 0))
        bad = ok & ((got < lo) | (got > hi))
        assert not bad.any(), (which, np.argwhere(bad)[:5].tolist(), got[bad][:5], ref[bad][:5], e)
        # dbias = its start + sum_b d (out-of-range actions contribute -q (...), as in the reference)
        z = lambda t: np.where(ok, t, 0.0)  # noqa: E731
        ref_db = d["dbias0"].astype(np.float64) + ref.sum(0).reshape(-1)
        tor_db = torch.from_numpy(z(tor).astype(np.float32)).sum(0).double().numpy().reshape(-1)
        e_db = float(np.abs(tor_db - z(ref).sum(0).reshape(-1)).max())
        fl = C.EPS * float(np.abs(ref).sum(0).max())
        if c.dense:
            fl += H.dense_floor_gain(c, d)
        err = float(np.abs(db - ref_db).max())
        bound = 4.0 * e_db + fl  # 0 at A = 1, where every d is 0
        _record((_fam(c), "bwd", "dbias"), err, e_db, err / bound if bound > 0 else float(err > 0))
        assert err <= bound, (which, "dbias", err, e_db, fl)
        if i == 0:  # again without a workspace: the same bits
            raw2, _, db2 = _backward(o, c, d, bits, g_lp, g_ent, workspace=False)
            assert np.array_equal(raw, raw2) and _same_bits(db, db2)


def run_sample(c, s, o):
    from vmp.head import HeadRng
    bits = _bits(c, s["invalid"])
    rng = HeadRng(s["seed"])
    rng.offset = s["offset"]
    act, lp, ent = _sample(o, c, bits, rng)
    assert ((act >= 0) & (act < c.A)).all()
    taken = np.take_along_axis(s["invalid"], act.astype(np.int64)[..., None], -1)[..., 0]
    assert not (taken & ~s["skip"]).any()
    if not c.dense:  # exact logits: the draw itself, row by row
        _, ref_act, dist, lo, hi = H.draw_reference(s["logits"], c.V, c.A, s["invalid"], s["seed"], s["offset"])
        _judge_draw(act, ref_act, dist, lo, hi, s["invalid"], s["skip"], c.A, (c.name, "sample"))
    lp2, ent2 = _forward(o, c, bits, act)
    assert _same_bits(lp, lp2) and _same_bits(ent, ent2), "sample vs given"
    _judge_given(c, s, lp, ent, s["invalid"], act, "sample")


def run_wait(c, w, o):
    from vmp.head import HeadRng
    bits, P = _bits(c, w["invalid"]), w["P"]
    runs = [(ratio,) + H.wait_seed(c, i) + (None,) for i, ratio in enumerate(H.WAIT_RATIOS)]
    if c.counter:
        runs += [(H.COUNTER_RATIO, H.COUNTER_SEED, 0, counter) for counter in (0, 1)]
        crng = HeadRng(H.COUNTER_SEED).graph_counter(DEV)
    for ratio, seed, off, counter in runs:
        if counter is None:
            rng = HeadRng(seed)
            rng.offset = off
        else:
            rng = crng
            assert int(rng.counter[0]) == counter
        act, lp, ent = _sample(o, c, bits, rng, ratio, P)
        inv2, skip, ref_act, dist, lo, hi, forbid = H.coin_reference(c, w, ratio, seed, off, counter)
        _judge_draw(act, ref_act, dist, lo, hi, inv2, skip, c.A, (c.name, "wait", ratio, counter))
        clear = ~skip & (dist > R.BAND)
        assert np.array_equal((act == P)[clear], (~inv2[..., P])[clear]), (c.name, ratio)
        if ratio == 1.0:
            assert not forbid.any()
        # GIVEN on the drawn actions, with the forbidden WAITs in its mask
        lp2, ent2 = _forward(o, c, _bits(c, inv2), act)
        assert _same_bits(lp, lp2) and _same_bits(ent, ent2), (c.name, ratio)
        _judge_given(c, w, lp, ent, inv2, act, "wait")
    if c.counter:
        assert not np.array_equal(R.sample_uniforms(H.COUNTER_SEED, 0, 8, 0), R.sample_uniforms(H.COUNTER_SEED, 0, 8, 1))


@pytest.mark.parametrize("c", H.CASES, ids=lambda c: c.name)
def test_hg16_case(c):
    from vmp.head import actor_head_bf16_supported, bf16_bwd_workspace
    assert bf16_bwd_workspace(c.B, c.V, c.A) == c.plan["workspace"]
    if "given" in c.modes or "bwd" in c.modes:
        d = H.given_inputs(c.name)
        assert actor_head_bf16_supported(d["K"], c.A)
        o = Ops(d)
        if "given" in c.modes:
            run_given(c, d, o)
        if "bwd" in c.modes:
            run_bwd(c, d, o)
    if "sample" in c.modes:
        s = H.sample_inputs(c.name)
        run_sample(c, s, Ops(s))
    if "wait" in c.modes:
        w = H.wait_inputs(c.name)
        run_wait(c, w, Ops(w))
    SEEN.update(c.selects())
    RAN.add(c.name)
