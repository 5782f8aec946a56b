"""
GPU tests of call SEQUENCES on one context (tests/sequence_cases.py): what a call computes must not depend on the entry point that used the
context before it.  Every expected value is the oracle's, computed once per call kind; every comparison is byte for byte.

  walks on host arrays      every ordered pair of a group's kinds at consecutive positions, each call compared when it returns
  walks on device tensors   the same walks with nothing but stream order between the calls (no synchronisation; a side stream for the middle
                            third), every result compared after one final synchronise
  jobs in flight            one cycle through all 32 kinds with three device-pointer jj_msm_begin jobs in flight on lanes 1 .. 3
  the ring of eight         more than eight 64-byte results bound for device memory queued behind a busy launch stream

Default options throughout (include/jubjub_hip.h: options are set before the first batch call); one Engine per test.
"""
import collections
import ctypes as C
import time

import numpy as np
import pytest

import sequence_cases as SC
from oracle import c_oracle as O
from util import rand_scalars

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    """both groups with the oracle's answer to every kind (the only slow part: about 15 s of CPU)"""
    t0 = time.time()
    K = SC.source_constants()
    km, kw = SC.kinds_m(K), SC.kinds_w(K)
    for k in km + kw:
        k.want()
    print("sequence cases: %d + %d kinds, oracle precompute %.1f s" % (len(km), len(kw), time.time() - t0))
    return {"K": K, "M": km, "W": kw}


@pytest.fixture()
def eng():
    from jubjub_amd import Engine

    e = Engine(0)
    yield e
    e.close()


def host_args(kind):
    return dict(kind.args)


def dev_args(kind):
    import torch

    return {name: v if name in kind.host_args else torch.tensor(v, device="cuda") for name, v in kind.args.items()}


def resources(eng, kinds, args):
    """the bases and tables the kinds use, made before the walk"""
    res = {}
    for k, a in zip(kinds, args):
        if k.setup:
            name, obj = k.setup(eng, a)
            res[name] = obj
    return res


def release(res):
    for obj in res.values():
        obj.close()


def to_np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def difference(kind, got):
    """None, or what differs between a call's results and the oracle's"""
    got = got if isinstance(got, tuple) else (got,)
    want = kind.want()
    if len(got) != len(want):
        return "%d results, %d expected" % (len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        g = to_np(g)
        if g.shape != w.shape:
            return "result %d has shape %r, expected %r" % (k, g.shape, w.shape)
        if not (g == w).all():
            rows = np.flatnonzero((g != w).reshape(g.shape[0], -1).any(axis=1)) if g.ndim > 1 else np.flatnonzero(g != w)
            return "result %d: %d of %d %s differ from the oracle, first %s" % (k, rows.size, g.shape[0], "rows" if g.ndim > 1 else "bytes", rows[:8].tolist())
    return None


class Walker:
    """makes the calls of a walk on one Engine.  check_now: every result is compared when it is there (host arrays); otherwise results are kept
    and compared by finish() after one synchronise.  A Deferred result (a job begun by the call) is finished after the NEXT call returned."""

    def __init__(self, eng, kinds, args, res, order, check_now):
        self.eng, self.kinds, self.args, self.res, self.order, self.check_now = eng, kinds, args, res, order, check_now
        self.pending, self.kept = [], []

    def where(self, pos):
        before = [self.kinds[i].name for i in self.order[max(0, pos - 4):pos - 1]] if pos > 1 else []
        prev = self.kinds[self.order[pos - 1]].name if pos else "(a fresh context)"
        return "position %d of %d: %s AFTER %s; the calls before that pair: %s" % (pos, len(self.order), self.kinds[self.order[pos]].name, prev, before or "none")

    def record(self, pos, got, note=""):
        if self.check_now:
            d = difference(self.kinds[self.order[pos]], got)
            if d:
                pytest.fail("%s%s: %s" % (self.where(pos), note, d), pytrace=False)
        else:
            self.kept.append((pos, got, note))

    def step(self, pos):
        r = self.kinds[self.order[pos]].call(self.eng, self.args[self.order[pos]], self.res)
        after = self.kinds[self.order[pos]].name
        for ppos, d in self.pending:
            self.record(ppos, d.finish(), " (finished after %s)" % after)
        self.pending = []
        if isinstance(r, SC.Deferred):
            self.pending.append((pos, r))
        else:
            self.record(pos, r)

    def run(self, lo=0, hi=None):
        for pos in range(lo, len(self.order) if hi is None else hi):
            self.step(pos)

    def finish(self):
        """the jobs still in flight; then, for a walk without checks on the way, every kept result against the oracle (the caller has synchronised)"""
        for ppos, d in self.pending:
            self.record(ppos, d.finish(), " (finished at the end of the walk)")
        self.pending = []
        bad = []
        for pos, got, note in self.kept:
            d = difference(self.kinds[self.order[pos]], got)
            if d:
                bad.append("%s%s: %s" % (self.where(pos), note, d))
        if bad:
            pytest.fail("%d of %d calls differ from the oracle:\n%s" % (len(bad), len(self.kept), "\n".join(bad[:12])), pytrace=False)


@pytest.mark.parametrize("group", ["M", "W"])
def test_walk_on_host_arrays(eng, cases, group):
    kinds = cases[group]
    args = [host_args(k) for k in kinds]
    res = resources(eng, kinds, args)
    w = Walker(eng, kinds, args, res, SC.euler_walk(len(kinds)), check_now=True)
    assert len(w.order) == len(kinds) ** 2 + 1
    w.run()
    w.finish()
    release(res)


@pytest.mark.parametrize("group", ["M", "W"])
def test_walk_on_device_tensors(eng, cases, group):
    """nothing but stream order between the calls: msm_basis_mul, msm_batch, msm_ragged, msm_dev and the elementwise calls only queue work on
    device pointers.  The middle third of the walk runs on a side stream."""
    import torch

    kinds = cases[group]
    args = [dev_args(k) for k in kinds]
    res = resources(eng, kinds, args)
    torch.cuda.synchronize()
    w = Walker(eng, kinds, args, res, SC.euler_walk(len(kinds)), check_now=False)
    a, b = len(w.order) // 3, 2 * len(w.order) // 3
    side = torch.cuda.Stream()
    w.run(0, a)
    with torch.cuda.stream(side):
        w.run(a, b)
    w.run(b)
    torch.cuda.synchronize()
    w.finish()
    assert len(w.kept) == len(w.order)
    release(res)


def test_jobs_in_flight_across_both_groups(eng, cases):
    """one cycle through all 32 kinds (host arrays, each compared when it returns) while three device-pointer jj_msm_begin jobs -- the small path,
    23 windows, 17 windows -- are in flight on lanes 1 .. 3: one is begun before each call, the oldest finished after it"""
    import torch

    kinds = cases["M"] + cases["W"]
    args = [host_args(k) for k in kinds]
    res = resources(eng, kinds, args)
    job_kinds = cases["M"][:3]
    assert [len(k.args["s"]) for k in job_kinds] == [700, 20000, cases["K"]["MSM_LARGE_MIN"] + 5]
    job_args = [dev_args(k) for k in job_kinds]
    torch.cuda.synchronize()
    w = Walker(eng, kinds, args, res, SC.one_cycle(len(kinds)), check_now=True)
    flying = collections.deque()
    begun = 0

    def begin():
        nonlocal begun
        j = begun % 3
        flying.append((begun, j, eng.msm_begin(job_args[j]["s"], job_args[j]["p"])))
        begun += 1

    def finish_oldest(where):
        seq, j, job = flying.popleft()
        got = eng.msm_finish(job)
        assert (got == job_kinds[j].want()[0]).all(), "job %d (%s, begun before call %d) differs from the oracle when finished %s" % (seq, job_kinds[j].name, seq - 2, where)

    begin()
    begin()
    for pos in range(len(w.order)):
        begin()
        assert len(flying) == 3
        w.step(pos)
        finish_oldest("after " + w.where(pos))
    w.finish()
    while flying:
        finish_oldest("after the cycle")
    release(res)


def _busy_stream(eng, n_log2=18):
    """one long asynchronous call on the context's stream (torch's current one): varbase_mul on device tensors; -> (result, scalars, points)"""
    import torch

    n = 1 << n_log2
    s, p = rand_scalars(0x52494E47, n, full_width=True), SC.points_for(n, offset=31)
    ds, dp = torch.tensor(s, device="cuda"), torch.tensor(p, device="cuda")
    torch.cuda.synchronize()
    return ds, dp, s, p


def _check_long_call(out, s, p):
    rows = np.linspace(0, len(s) - 1, 64).astype(np.int64)
    got = out.cpu().numpy()
    assert (got[rows] == O.varbase_mul(s[rows], p[rows])).all(), "the long call itself differs from the oracle"


def test_ring_of_eight_job_results(eng, cases):
    """twelve jobs finished INTO DEVICE MEMORY while the launch stream is busy: twelve 64-byte copies out of the context's ring of eight host
    slots are queued behind the long call; every row must still be its own job's sum"""
    import torch

    assert cases["K"]["HOST_OUT_SLOTS"] < 12
    ds, dp, s, p = _busy_stream(eng)
    terms = [(40 + 13 * i, 300 + i) for i in range(12)]
    ins = [(rand_scalars(seed, n, full_width=True), SC.points_for(n, offset=seed)) for n, seed in terms]
    want = np.stack([O.msm(a, b) for a, b in ins])
    assert len({bytes(r) for r in want}) == 12
    dins = [(torch.tensor(a, device="cuda"), torch.tensor(b, device="cuda")) for a, b in ins]
    out = torch.zeros((12, 64), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    jobs = [eng.msm_begin(a, b) for a, b in dins]
    long_out = eng.varbase_mul(ds, dp)
    for i, job in enumerate(jobs):
        rc = eng._lib.jj_msm_finish(job._h, C.c_void_p(out[i].data_ptr()))
        job._h = None
        assert rc == 0, (i, rc)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    bad = [i for i in range(12) if not (got[i] == want[i]).all()]
    assert not bad, "rows %s of 12 are not their job's sum; they hold the sums of jobs %s" % (
        bad, [[j for j in range(12) if (got[i] == want[j]).all()] for i in bad])
    _check_long_call(long_out, s, p)


def test_ring_of_eight_empty_records(eng, cases):
    """the same with the empty record of jj_msm_partial written to device memory: twelve calls with n = 0 (the issue's case: identical headers),
    then twelve parts beyond the last window of 1 .. 12 terms, whose headers differ in their term count"""
    import torch

    ds, dp, s, p = _busy_stream(eng)
    none_s, none_p = torch.zeros((0, 32), dtype=torch.uint8, device="cuda"), torch.zeros((0, 64), dtype=torch.uint8, device="cuda")
    few_s, few_p = torch.tensor(rand_scalars(7, 12), device="cuda"), torch.tensor(SC.points_for(12), device="cuda")
    torch.cuda.synchronize()
    long_out = eng.varbase_mul(ds, dp)
    recs0 = [eng.msm_partial(none_s, none_p) for _ in range(12)]
    recs1 = [eng.msm_partial(few_s[:i + 1], few_p[:i + 1], SC.SM_W, SC.SM_W + 1) for i in range(12)]
    torch.cuda.synchronize()
    for i in range(12):
        assert (recs0[i].cpu().numpy() == SC.empty_record(0)).all(), i
        got = recs1[i].cpu().numpy()
        assert (got == SC.empty_record(i + 1)).all(), "record %d: header %s" % (i, got[:32].view("<u4").tolist())
    assert (eng.msm_combine(torch.stack(recs0 + recs1)) == SC.IDENTITY).all()
    _check_long_call(long_out, s, p)
