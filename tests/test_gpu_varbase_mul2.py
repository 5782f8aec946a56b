"""
GPU tests of the two-term variable-base multiplication (jj_varbase_mul2_vartime, _compressed, jj_varbase_mul2_scalars; Engine.varbase_mul2_*):
every unit of every batch byte for byte against the oracle (its ladder twice and its addition), against the composed GPU calls and against
jj_msm_batch on two-term rows; the edge matrix of tests/test_emu_straus.py through the C ABI; every kind of pointer; both window widths.
No unit is sampled away or tolerated.
"""
import threading

import numpy as np
import pytest

from oracle import c_oracle as O
from tests.straus_cases import edge_matrix, want
from tests.util import rand_scalars

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1000, 70001, (1 << 20) + 3]     # the last one: above the persistent grid (several cursor draws per wave, ragged last wave)


@pytest.fixture(scope="module")
def eng():
    from jubjub_amd import Engine

    e = Engine(0)
    yield e
    e.close()


def inputs(eng, n, seed):
    """full-width scalars (bits above 251 set in most) and points of the whole group"""
    a, b = rand_scalars(seed, n, full_width=True), rand_scalars(seed + 1, n, full_width=True)
    if n == 0:
        return a, np.zeros((0, 64), np.uint8), b, np.zeros((0, 64), np.uint8)
    p = eng.random_points(n, seed=seed + 2, subgroup=False).reshape(n, 64)
    q = eng.random_points(n, seed=seed + 3, subgroup=(seed % 2 == 0)).reshape(n, 64)
    return a, p, b, q


def composed(eng, a, p, b, q):
    return eng.point_add(eng.varbase_mul(a, p), eng.varbase_mul(b, q))


@pytest.mark.parametrize("n", SIZES)
def test_random_units_match_the_oracle_and_the_composed_calls(eng, n):
    a, p, b, q = inputs(eng, n, seed=900 + n % 1000)
    got = eng.varbase_mul2_vartime(a, p, b, q)
    assert got.shape == (n, 64)
    assert np.array_equal(got, want(a, p, b, q).reshape(n, 64))           # all units
    assert np.array_equal(got, composed(eng, a, p, b, q).reshape(n, 64))


def test_edge_matrix_interleaved_with_ordinary_units(eng, golden):
    ea, ep, eb, eq = edge_matrix(golden)
    m = len(ea)
    ra, rp, rb, rq = inputs(eng, m, seed=31)
    a, p, b, q = (np.stack([x, y], axis=1).reshape(2 * m, -1) for x, y in ((ea, ra), (ep, rp), (eb, rb), (eq, rq)))
    got = eng.varbase_mul2_vartime(a, p, b, q)
    exp = want(a, p, b, q)
    bad = [i for i in range(2 * m) if not np.array_equal(got[i], exp[i])]
    assert not bad, "%d of %d units differ, first: unit %d" % (len(bad), 2 * m, bad[0])
    assert np.array_equal(eng.varbase_mul2_vartime_compressed(a, p, b, q), O.compress(exp))


def test_entry_points_agree(eng):
    n = 257
    a, p, b, q = inputs(eng, n, seed=77)
    got = eng.varbase_mul2_vartime(a, p, b, q)
    assert np.array_equal(got, want(a, p, b, q))
    assert np.array_equal(eng.varbase_mul2_vartime_compressed(a, p, b, q), eng.compress(got))
    assert np.array_equal(got, composed(eng, a, p, b, q))
    assert np.array_equal(got, eng.point_add(eng.varbase_mul_vartime(a, p), eng.varbase_mul_vartime(b, q)))
    rows = eng.msm_batch(np.stack([a, b], axis=1), np.stack([p, q], axis=1))              # B = 257 rows of two terms
    assert np.array_equal(got, rows)
    # one pair of scalars for the whole batch = the general call on broadcast scalars
    ab = np.concatenate([a[3], b[5]])
    one = eng.varbase_mul2_scalars(ab, p, q)
    ba, bb = np.tile(a[3], (n, 1)), np.tile(b[5], (n, 1))
    assert np.array_equal(one, eng.varbase_mul2_vartime(ba, p, bb, q))
    assert np.array_equal(one, want(ba, p, bb, q))
    assert np.array_equal(one, eng.msm_batch(np.stack([ba, bb], axis=1), np.stack([p, q], axis=1)))
    for m in (1, 64, 70001):
        a2, p2, b2, q2 = inputs(eng, m, seed=78 + m % 100)
        assert np.array_equal(eng.varbase_mul2_scalars(ab.reshape(2, 32), p2, q2), want(np.tile(ab[:32], (m, 1)), p2, np.tile(ab[32:], (m, 1)), q2))
    assert eng.varbase_mul2_scalars(ab, p[:0], q[:0]).shape == (0, 64)


def test_group_mirror(eng):
    from jubjub_amd.group import Points

    a, p, b, q = inputs(eng, 100, seed=55)
    r = Points(eng, p).mul2_vartime(a, Points(eng, q), b)
    assert np.array_equal(r.data, want(a, p, b, q))


def test_pointer_kinds(eng):
    import torch

    n = 3000
    a, p, b, q = inputs(eng, n, seed=11)
    exp = want(a, p, b, q)
    dev = [torch.from_numpy(x).cuda() for x in (a, p, b, q)]
    got_dev = eng.varbase_mul2_vartime(*dev)                               # device-resident: the reference for the other kinds
    assert got_dev.is_cuda and np.array_equal(got_dev.cpu().numpy(), exp)
    assert np.array_equal(eng.varbase_mul2_vartime_compressed(*dev).cpu().numpy(), O.compress(exp))
    assert np.array_equal(eng.varbase_mul2_scalars(torch.cat([dev[0][7], dev[2][7]]), dev[1], dev[3]).cpu().numpy(),
                          want(np.tile(a[7], (n, 1)), p, np.tile(b[7], (n, 1)), q))
    assert np.array_equal(eng.varbase_mul2_vartime(a, p, b, q), exp)       # pageable numpy
    pinned = []
    for x in (a, p, b, q):
        h = eng.host_alloc(x.shape)
        h[...] = x
        pinned.append(h)
    out = eng.host_alloc((n, 64))
    assert eng.varbase_mul2_vartime(*pinned, out=out) is out and np.array_equal(out, exp)
    pooled = eng.result_acquire((n, 32))
    assert eng.varbase_mul2_vartime_compressed(pinned[0], p, pinned[2], q, out=pooled) is pooled and np.array_equal(pooled, O.compress(exp))
    eng.result_release(pooled)
    # mixed through the C ABI: device scalars and P, host b and Q, host result
    res = np.zeros((n, 64), np.uint8)
    lib, ctx = eng._lib, eng._ctx
    eng._lib.jj_ctx_use_own_stream(ctx)
    torch.cuda.synchronize()
    rc = lib.jj_varbase_mul2_vartime(ctx, n, dev[0].data_ptr(), dev[1].data_ptr(), b.ctypes.data, pinned[3].ctypes.data, res.ctypes.data)
    assert rc == 0 and np.array_equal(res, exp)
    rc = lib.jj_varbase_mul2_scalars(ctx, n, dev[0].data_ptr(), p.ctypes.data, dev[3].data_ptr(), res.ctypes.data)     # ab64 on the device: a[0] then a[1]
    assert rc == 0 and np.array_equal(res, want(np.tile(a[0], (n, 1)), p, np.tile(a[1], (n, 1)), q))


def test_argument_checks_with_a_context(eng):
    from jubjub_amd import _lib

    lib, ctx = eng._lib, eng._ctx
    buf = np.zeros(64, np.uint8)
    ptr = buf.ctypes.data
    assert lib.jj_varbase_mul2_scalars(ctx, 1, None, ptr, ptr, ptr) == _lib.JJ_ERR_INVALID          # NULL ab64
    assert lib.jj_varbase_mul2_scalars(ctx, 0, None, None, None, None) == _lib.JJ_ERR_INVALID
    assert lib.jj_varbase_mul2_vartime(ctx, 1, ptr, ptr, None, ptr, ptr) == _lib.JJ_ERR_INVALID      # a NULL array with n > 0
    assert lib.jj_varbase_mul2_vartime(ctx, 1, ptr, ptr, ptr, ptr, None) == _lib.JJ_ERR_INVALID
    buf[:] = 0xEE
    assert lib.jj_varbase_mul2_vartime(ctx, 0, None, None, None, None, None) == 0                    # n = 0 succeeds
    assert lib.jj_varbase_mul2_vartime_compressed(ctx, 0, ptr, ptr, ptr, ptr, ptr) == 0 and (buf == 0xEE).all()   # ... and touches nothing
    assert lib.jj_varbase_mul2_scalars(ctx, 0, ptr, ptr, ptr, ptr) == 0 and (buf == 0xEE).all()


def test_host_pipeline_chunks(eng):
    """pipe_chunk_log2 = 10: host batches cut into chunks of 1024 with a ragged last chunk (pageable and page-locked), equal to the
    device-resident call"""
    import torch

    from jubjub_amd import Engine

    n = 5 * 1024 + 77
    a, p, b, q = inputs(eng, n, seed=21)
    ref = eng.varbase_mul2_vartime(*[torch.from_numpy(x).cuda() for x in (a, p, b, q)]).cpu().numpy()
    assert np.array_equal(ref, want(a, p, b, q))
    ep = Engine(0, options={"pipe_chunk_log2": 10})
    try:
        assert np.array_equal(ep.varbase_mul2_vartime(a, p, b, q), ref)
        assert np.array_equal(ep.varbase_mul2_vartime_compressed(a, p, b, q), O.compress(ref))
        pinned = []
        for x in (a, p, b, q):
            h = ep.host_alloc(x.shape)
            h[...] = x
            pinned.append(h)
        out = ep.host_alloc((n, 64))
        ep.varbase_mul2_vartime(*pinned, out=out)
        assert np.array_equal(out, ref)
        ab = np.concatenate([a[1], b[2]])
        assert np.array_equal(ep.varbase_mul2_scalars(ab, p, pinned[3]), eng.varbase_mul2_scalars(ab, p, q))
        assert np.array_equal(ep.varbase_mul2_scalars(ab, p, q), want(np.tile(a[1], (n, 1)), p, np.tile(b[2], (n, 1)), q))
    finally:
        ep.close()


def test_both_window_widths_give_identical_bytes(eng, golden):
    from jubjub_amd import Engine

    assert eng.get_option("vb_mul2_window") in (4, 5)
    ea, ep_, eb, eq = edge_matrix(golden)
    ra, rp, rb, rq = inputs(eng, 70001, seed=61)
    a, p, b, q = np.concatenate([ea, ra]), np.concatenate([ep_, rp]), np.concatenate([eb, rb]), np.concatenate([eq, rq])
    exp = want(a, p, b, q)
    ab = np.concatenate([a[9], b[4]])
    exp_s = want(np.tile(a[9], (len(a), 1)), p, np.tile(b[4], (len(a), 1)), q)
    for w in (4, 5):
        e = Engine(0, options={"vb_mul2_window": w})
        try:
            assert e.get_option("vb_mul2_window") == w
            assert np.array_equal(e.varbase_mul2_vartime(a, p, b, q), exp), w
            assert np.array_equal(e.varbase_mul2_scalars(ab, p, q), exp_s), w
        finally:
            e.close()
    with pytest.raises(Exception):
        Engine(0, options={"vb_mul2_window": 6})


def test_two_host_threads_on_one_context(eng):
    sets = [inputs(eng, 4000 + 13 * t, seed=300 + 10 * t) for t in range(2)]
    exps = [want(*s) for s in sets]
    errs = []

    def work(t):
        try:
            for _ in range(4):
                if not np.array_equal(eng.varbase_mul2_vartime(*sets[t]), exps[t]):
                    errs.append("thread %d: wrong result" % t)
                if not np.array_equal(eng.varbase_mul_vartime(sets[t][0], sets[t][1]), O.varbase_mul(sets[t][0], sets[t][1])):
                    errs.append("thread %d: wrong one-term result" % t)
        except Exception as e:  # noqa: BLE001
            errs.append(repr(e))

    ths = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    assert not errs, errs


def test_caller_stream_and_back(eng):
    """a call on a caller's stream (jj_ctx_set_stream through torch's current stream), then on the context's own stream again"""
    import torch

    n = 2000
    a, p, b, q = inputs(eng, n, seed=41)
    exp = want(a, p, b, q)
    dev = [torch.from_numpy(x).cuda() for x in (a, p, b, q)]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        r1 = eng.varbase_mul2_vartime(*dev)
        r1c = eng.varbase_mul2_vartime_compressed(*dev)
    s.synchronize()
    assert np.array_equal(r1.cpu().numpy(), exp) and np.array_equal(r1c.cpu().numpy(), O.compress(exp))
    assert np.array_equal(eng.varbase_mul2_vartime(a, p, b, q), exp)                     # numpy: back on the context's own stream
    assert np.array_equal(eng.varbase_mul2_vartime(*dev).cpu().numpy(), exp)             # torch's default stream
