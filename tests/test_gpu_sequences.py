"""Device handles driven through random call sequences against the model of
tests/seq_cases.py: one test per (case, seed) walks two
BatchedVmEnv handles and the model through the same op list.

After every launch every returned value is compared with the model's: obs,
done, valid, actions, mask bits and done_count bit for bit, the reward bit for
bit under wr / ut and within tests.traj.kl_close under kl. After EVERY op,
mutators and readers included, counters(), stats(), the six state() arrays and
rank() of both handles equal the model's. The series and the request log are
compared at every read op and at the end. The per-step launches write into the
test's own buffers, poisoned before every launch (NaN obs and reward, done
0xFF): an idle step's unwritten output cannot pass for the previous step's.

A failing assertion names the case, the seed and the op index;
`python -m tests.seq_cases --case A --seed 2 --upto K` prints the ops up to it."""
import numpy as np
import pytest
import torch

from tests import seq_cases as S
from tests import series_literal as SR
from tests import traj as T

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAIRS = [(c, s) for c in S.CASES for s in S.SEQ_SEEDS]
IDS = ["%s-%d" % (c.name, s) for c, s in PAIRS]
EXACT = [f for f in range(SR.NF) if f not in SR.VAR_FIELDS]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")


def _np(x):
    return None if x is None else x.cpu().numpy()


def _unpack(bits, A):
    """int32 [N, V, W] -> bool [N, V, A] (bit a of word a // 32 set = invalid)."""
    w = bits.cpu().numpy().view(np.uint32)
    a = np.arange(A)
    return ((w[:, :, a // 32] >> (a % 32).astype(np.uint32)) & 1).astype(bool)


class _Handle:
    """A BatchedVmEnv and the poisoned output buffers of its per-step launches."""

    def __init__(self, case, which):
        from vmp.batched import BatchedVmEnv
        from vmp.config import Config
        from vmp.trace import Trace
        n = (S.N_MAIN, S.N_SECOND)[which]
        seeds = np.asarray((S.SEEDS_MAIN, S.SEEDS_SECOND)[which], dtype=np.int64)
        kw = {}
        if case.source == "workload":
            wl = case.workload(which)
            kw = dict(arrival_rate=np.array([w[0] for w in wl]),
                      service_length=np.array([w[1] for w in wl]))
        self.b = b = BatchedVmEnv(Config(**case.cfg()), n, seeds=seeds, device=DEV, **kw)
        if case.source == "trace":
            b.set_trace([Trace(*t) for t in case.traces()], np.asarray(S.TRACE_MAP[which]))
        self.obs = torch.empty((n, b.D), dtype=torch.float32, device=DEV)
        self.rew = torch.empty((n,), dtype=torch.float64, device=DEV)
        self.done = torch.empty((n,), dtype=torch.uint8, device=DEV)

    def poison(self):
        self.obs.fill_(float("nan"))
        self.rew.fill_(float("nan"))
        self.done.fill_(0xFF)
        return dict(obs=self.obs, reward=self.rew, done=self.done)

    def outputs(self):
        return dict(obs=_np(self.obs), reward=_np(self.rew), done=_np(self.done))

    def observe(self):
        b = self.b
        out = dict(counters=_np(b.counters()), stats=_np(b.stats()), rank=_np(b.rank()))
        out.update({k: _np(v) for k, v in b.state().items()})
        return out


def _device_op(case, main, second, op, snap):
    """Run `op` on the device -> dict of what it returned, as numpy."""
    from vmp.state import State
    k = op["op"]
    b = main.b
    if k == "step_ext":
        a = torch.tensor(op["actions"], dtype=torch.int32, device=DEV)
        mo = torch.full((b.n_envs, b.V, b.W), -1, dtype=torch.int32, device=DEV) \
            if op["mask_out"] else None
        _, _, _, valid = b.step(a, bool_done=False, mask_out=mo, **main.poison())
        out = dict(main.outputs(), valid=_np(valid))
        if mo is not None:
            out["mask_out"] = _unpack(mo, b.A)
        return out
    if k in ("hstep_full", "h2_step"):
        h = second if k == "h2_step" else main
        _, _, _, valid, act = h.b.heuristic_step(case.policy, want_actions=True, want_valid=True,
                                                 **h.poison())
        return dict(h.outputs(), valid=_np(valid), actions=_np(act).astype(np.int64))
    if k == "hstep_bare":
        _, _, _, valid, act = b.heuristic_step(case.policy, **main.poison())
        assert valid is None and act is None
        return main.outputs()
    if k == "rollout":
        rs, dc = b.rollout(case.policy, op["K"])
        return dict(rewards=_np(rs), done_count=_np(dc))
    if k == "mask":
        return dict(mask=_np(b.mask()))
    if k == "mask_bits":
        return dict(mask_bits=_unpack(b.mask_bits(), b.A))
    if k == "obs":
        return dict(obs=_np(b.obs()))
    if k == "heuristic_act":
        return dict(actions=_np(b.heuristic_act(case.policy)).astype(np.int64))
    if k == "getters":
        return {}
    if k in ("reset_seeds", "reset_none"):
        return dict(obs=_np(b.reset(seeds=op.get("seeds"), mask=op["mask"])))
    if k == "eval":
        b.eval(op["mode"])
    elif k == "snapshot":
        snap[0] = b.snapshot()
    elif k == "restore":
        b.restore(snap[0])
    elif k == "branch_self":
        b.branch(b, op["index"], op["seeds"])
    elif k == "branch_from_second":
        b.branch(second.b, op["index"], op["seeds"])
    elif k == "branch_into_second":
        second.b.branch(b, op["index"], op["seeds"])
    elif k in ("set_state_identity", "set_state_random", "set_state_invalid"):
        status = b.set_state(op["state"], mask=op["mask"], counters=op["counters"],
                             totals=op["totals"], seeds=op["seeds"], check=False)
        return dict(status=_np(status))
    elif k == "set_start_state":
        b.set_start_state(State(b.P, counters=op["counters"], totals=op["totals"], **op["state"]))
    elif k == "set_start_none":
        b.set_start_state(None)
    elif k == "set_workload":
        b.set_workload(op["arrival_rate"], op["service_length"])
    elif k == "series_on":
        b.series(True, capacity=op["capacity"], stride=op["stride"])
    elif k == "series_off":
        b.series(False)
    elif k == "series_read":
        return _read_series(b)
    elif k == "reqlog_on":
        b.request_log(True, capacity=op["capacity"])
    elif k == "reqlog_off":
        b.request_log(False)
    elif k == "reqlog_read":
        return _read_reqlog(b)
    elif k == "record_on":
        b.record(True)
    elif k == "record_off":
        b.record(False)
    else:
        raise ValueError(k)
    return {}


def _read_series(b):
    s = b.series_read()
    return dict(series_rows=s.rows, series_meta=s.meta)


def _read_reqlog(b):
    q = b.request_log_read()
    return dict(reqlog_rows=q.rows, reqlog_meta=q.meta)


def _compare(got, want, kl, where, op):
    assert got.keys() == want.keys(), where + (sorted(got), sorted(want))
    for name in sorted(want):
        g, w = np.asarray(got[name]), np.asarray(want[name])
        if name == "done":
            w = w.astype(np.uint8)  # a written 0 / 1: the 0xFF of the fill equals neither
        if name == "obs" and op["op"].startswith("reset") and op["mask"] is not None:
            sel = np.asarray(op["mask"], bool)  # a masked reset returns the reset envs' rows
            g, w = g[sel], w[sel]
        assert g.shape == w.shape, where + (name, g.shape, w.shape)
        if name in ("reward", "rewards") and kl:
            ok = all(T.kl_close(x, y) for x, y in zip(g.ravel(), w.ravel()))
            assert ok, where + (name, g, w)
        elif name == "series_rows":
            for f in SR.VAR_FIELDS:  # tests/test_gpu_series.py's rule
                err = np.abs(g[..., f] - w[..., f])
                assert np.all(err <= 1e-12 * np.abs(w[..., f])), where + (name, f, float(err.max()))
            bad = np.argwhere(g[..., EXACT] != w[..., EXACT])
            assert bad.size == 0, where + (name, [(tuple(x[:-1]), EXACT[x[-1]]) for x in bad[:6]])
        else:
            assert g.dtype.kind == w.dtype.kind or {g.dtype.kind, w.dtype.kind} <= set("iub"), \
                where + (name, g.dtype, w.dtype)
            if not np.array_equal(g, w):  # NaN never equals: a poisoned element fails here
                bad = np.argwhere(g != w)
                assert False, where + (name, bad[:6].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


def _walk(case, seed, upto=None):
    ops = S.gen_ops(case, seed)
    model = S.Model(case)
    main, second = _Handle(case, 0), _Handle(case, 1)
    kl = case.reward == "kl"
    snap = [None]
    try:
        for k, op in enumerate(ops if upto is None else ops[:upto + 1]):
            where = ("case %s seed %d op %d %s" % (case.name, seed, k, S.describe(op, short=True)),)
            got = _device_op(case, main, second, op, snap)
            rew = None
            if kl and ("reward" in got or "rewards" in got) and op["op"] != "h2_step":
                # the series row takes the step's own reward (tests/test_gpu_series.py)
                rew = got["rewards"] if "rewards" in got else got["reward"][None]
            want = model.apply(op, rew=rew)
            _compare(got, want, kl, where, op)
            for h, mh, name in ((main, model.h[0], "main"), (second, model.h[1], "second")):
                _compare(h.observe(), mh.observe(), False, where + (name, "after the op"), op)
        got = {}
        if model.h[0].series:
            got.update(_read_series(main.b))
        if model.h[0].reqlog:
            got.update(_read_reqlog(main.b))
        _compare(got, model.final(), kl, ("case %s seed %d at the end" % (case.name, seed),), {"op": ""})
    finally:
        main.b.close()
        second.b.close()


@pytest.mark.parametrize("case,seed", PAIRS, ids=IDS)
def test_sequence_vs_model(case, seed):
    _walk(case, seed)
