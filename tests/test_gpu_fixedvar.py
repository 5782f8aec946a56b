"""
GPU tests of the fused fixed + variable multiplication (jj_fixedvar_mul_vartime, _compressed; Engine.fixedvar_mul_vartime*,
Points.mul_add_fixed_vartime): every unit of every batch byte for byte against the oracle (its ladder twice and its addition) and against the
composed GPU calls, on every kind of table -- the two LDS layouts (7, 6), the smallest gathered table (8), the full top window (11) and an odd
width (13) -- and on both sides of vb_quad_max: the default (the quad ladder, then the table's own kernel) and vb_quad_max = 1 (k_varbase_fixed for
the gathered tables, k_varbase<true> and the LDS kernel for the others).  The edge matrix of tests/fixedvar_cases.py through the C ABI on every
base kind; every kind of pointer; the host pipeline; argument checks; threads and streams.  No unit is sampled away or tolerated.
"""
import os
import re
import threading

import numpy as np
import pytest

from oracle import c_oracle as O
from tests.fixedvar_cases import bases, edge_matrix, want
from tests.util import rand_scalars

pytestmark = pytest.mark.gpu

KINDS = [7, 6, 8, 11, 13]
SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1000]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eng():
    from jubjub_amd import Engine

    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def lane_eng():
    """every batch of two units and more on the lane routes"""
    from jubjub_amd import Engine

    e = Engine(0, options={"vb_quad_max": 1})
    yield e
    e.close()


@pytest.fixture(scope="module")
def gens(golden):
    return bases(golden)


@pytest.fixture(scope="module")
def tabs(eng, gens):
    """one table of every kind on the generator, built once; a table serves every context of its device"""
    t = {wb: eng.fixedbase_table(gens["G"], wb) for wb in KINDS}
    yield t
    for x in t.values():
        x.close()


def inputs(eng, n, seed):
    """full-width scalars (bits above 251 set in most) and points of the whole group"""
    a, b = rand_scalars(seed, n, full_width=True), rand_scalars(seed + 1, n, full_width=True)
    if n == 0:
        return a, b, np.zeros((0, 64), np.uint8)
    return a, b, eng.random_points(n, seed=seed + 3, subgroup=(seed % 2 == 0)).reshape(n, 64)


@pytest.fixture(scope="module")
def sized(eng, gens):
    """inputs and oracle values of every size, computed once for all table kinds and both routes"""
    out = {}
    for n in SIZES:
        a, b, q = inputs(eng, n, seed=500 + n)
        out[n] = (a, b, q, want(gens["G"], a, b, q).reshape(n, 64))
    return out


def composed(eng, tab, a, b, q):
    return eng.point_add(eng.fixedbase_mul(tab, a), eng.varbase_mul(b, q))


@pytest.mark.parametrize("route", ["quad", "lane"])
@pytest.mark.parametrize("wb", KINDS)
def test_sizes_match_the_oracle_and_the_composed_calls(eng, lane_eng, tabs, sized, wb, route):
    e = eng if route == "quad" else lane_eng
    for n in SIZES:
        a, b, q, exp = sized[n]
        got = e.fixedvar_mul_vartime(tabs[wb], a, b, q)
        assert got.shape == (n, 64)
        assert np.array_equal(got, exp), (wb, route, n)                     # all units
        assert np.array_equal(got, composed(e, tabs[wb], a, b, q).reshape(n, 64)), (wb, route, n)


def _vb_blocks_per_cu():
    env = os.environ.get("JJ_VB_BLOCKS_PER_CU")
    if env and 1 <= int(env) <= 8:
        return int(env)
    with open(os.path.join(ROOT, "jubjub_amd", "csrc", "jj_engine.h")) as f:
        return int(re.search(r"int\s+vb_blocks_per_cu\s*=\s*(\d+)\s*;", f.read()).group(1))


def test_batch_above_the_persistent_grid(eng, tabs, gens):
    """several cursor draws per wave and a ragged last wave"""
    n = eng.device_info()["cus"] * 256 * _vb_blocks_per_cu() + 67
    assert n > eng.get_option("vb_quad_max")
    a, b, q = inputs(eng, n, seed=71)
    assert np.array_equal(eng.fixedvar_mul_vartime(tabs[8], a, b, q), want(gens["G"], a, b, q))


@pytest.fixture(scope="module")
def matrix(eng, golden):
    """name -> (G, a, b, Q, oracle value): the edge matrix interleaved with ordinary units"""
    out = {}
    for k, (name, (g, ea, eb, eq)) in enumerate(edge_matrix(golden).items()):
        m = len(ea)
        ra, rb, rq = inputs(eng, m, seed=31 + 2 * k)
        a, b, q = (np.stack([x, y], axis=1).reshape(2 * m, -1) for x, y in ((ea, ra), (eb, rb), (eq, rq)))
        out[name] = (g, a, b, q, want(g, a, b, q))
    return out


@pytest.mark.parametrize("route", ["quad", "lane"])
@pytest.mark.parametrize("wb", KINDS)
def test_edge_matrix_interleaved_with_ordinary_units(eng, lane_eng, tabs, matrix, wb, route):
    """every base kind on table kinds 8 and 7, the generator on all five"""
    e = eng if route == "quad" else lane_eng
    for name, (g, a, b, q, exp) in matrix.items():
        if name != "G" and wb not in (8, 7):
            continue
        tab = tabs[wb] if name == "G" else eng.fixedbase_table(g, wb)
        try:
            got = e.fixedvar_mul_vartime(tab, a, b, q)
            bad = [i for i in range(len(a)) if not np.array_equal(got[i], exp[i])]
            assert not bad, "base %s, table %d, %s: %d of %d units differ, first: unit %d" % (name, wb, route, len(bad), len(a), bad[0])
            assert np.array_equal(e.fixedvar_mul_vartime_compressed(tab, a, b, q), O.compress(exp)), (name, wb, route)
        finally:
            if name != "G":
                tab.close()


def test_entry_points_agree(eng, lane_eng, tabs, gens):
    from jubjub_amd.group import Points

    n = 257
    a, b, q = inputs(eng, n, seed=77)
    g = np.tile(gens["G"], (n, 1))
    exp = want(gens["G"], a, b, q)
    rows = eng.msm_batch(np.stack([a, b], axis=1), np.stack([g, q], axis=1))                  # 257 rows of two terms
    for e in (eng, lane_eng):
        for wb in (8, 7):
            got = e.fixedvar_mul_vartime(tabs[wb], a, b, q)
            assert np.array_equal(got, exp)
            assert np.array_equal(got, e.varbase_mul2_vartime(a, g, b, q))
            assert np.array_equal(got, rows)
            assert np.array_equal(e.fixedvar_mul_vartime_compressed(tabs[wb], a, b, q), e.compress(got))
            assert np.array_equal(Points(e, q).mul_add_fixed_vartime(b, tabs[wb], a).data, exp)


@pytest.mark.parametrize("wb", [8, 7])
def test_pointer_kinds(lane_eng, tabs, gens, wb):
    import torch

    e, tab, n = lane_eng, tabs[wb], 3000
    a, b, q = inputs(e, n, seed=11)
    exp = want(gens["G"], a, b, q)
    dev = [torch.from_numpy(x).cuda() for x in (a, b, q)]
    got_dev = e.fixedvar_mul_vartime(tab, *dev)                            # device-resident
    assert got_dev.is_cuda and np.array_equal(got_dev.cpu().numpy(), exp)
    assert np.array_equal(e.fixedvar_mul_vartime_compressed(tab, *dev).cpu().numpy(), O.compress(exp))
    assert np.array_equal(e.fixedvar_mul_vartime(tab, a, b, q), exp)       # pageable numpy
    pinned = []
    for x in (a, b, q):
        h = e.host_alloc(x.shape)
        h[...] = x
        pinned.append(h)
    out = e.host_alloc((n, 64))
    assert e.fixedvar_mul_vartime(tab, *pinned, out=out) is out and np.array_equal(out, exp)
    pooled = e.result_acquire((n, 32))
    assert e.fixedvar_mul_vartime_compressed(tab, pinned[0], b, pinned[2], out=pooled) is pooled and np.array_equal(pooled, O.compress(exp))
    e.result_release(pooled)
    # mixed through the C ABI: device a, host b, page-locked Q, host result
    res = np.zeros((n, 64), np.uint8)
    lib, ctx = e._lib, e._ctx
    lib.jj_ctx_use_own_stream(ctx)
    torch.cuda.synchronize()
    rc = lib.jj_fixedvar_mul_vartime(ctx, tab._h, n, dev[0].data_ptr(), b.ctypes.data, pinned[2].ctypes.data, res.ctypes.data)
    assert rc == 0 and np.array_equal(res, exp)


def test_host_pipeline_chunks(eng, tabs, gens):
    """pipe_chunk_log2 = 10: host batches cut into chunks of 1024 with a ragged last chunk (pageable and page-locked), equal to the
    device-resident call; chunks of 1024 with vb_quad_max = 1 run the lane routes, with the default the quad route"""
    import torch

    from jubjub_amd import Engine

    n = 5 * 1024 + 77
    a, b, q = inputs(eng, n, seed=21)
    exp = want(gens["G"], a, b, q)
    for opts in ({"pipe_chunk_log2": 10, "vb_quad_max": 1}, {"pipe_chunk_log2": 10}):
        ep = Engine(0, options=opts)
        try:
            for wb in (8, 7):
                ref = ep.fixedvar_mul_vartime(tabs[wb], *[torch.from_numpy(x).cuda() for x in (a, b, q)]).cpu().numpy()
                assert np.array_equal(ref, exp)
                assert np.array_equal(ep.fixedvar_mul_vartime(tabs[wb], a, b, q), ref)
                assert np.array_equal(ep.fixedvar_mul_vartime_compressed(tabs[wb], a, b, q), O.compress(ref))
                pinned = []
                for x in (a, b, q):
                    h = ep.host_alloc(x.shape)
                    h[...] = x
                    pinned.append(h)
                out = ep.host_alloc((n, 64))
                ep.fixedvar_mul_vartime(tabs[wb], *pinned, out=out)
                assert np.array_equal(out, ref)
        finally:
            ep.close()


def test_argument_checks_with_a_context(eng, tabs, gens):
    from jubjub_amd import _lib

    lib, ctx, tab = eng._lib, eng._ctx, tabs[8]._h
    buf = np.zeros(64, np.uint8)
    ptr = buf.ctypes.data
    for fn in (lib.jj_fixedvar_mul_vartime, lib.jj_fixedvar_mul_vartime_compressed):
        assert fn(ctx, None, 1, ptr, ptr, ptr, ptr) == _lib.JJ_ERR_INVALID          # a NULL table
        assert fn(ctx, None, 0, ptr, ptr, ptr, ptr) == _lib.JJ_ERR_INVALID
        for hole in range(4):                                                      # a NULL array with n > 0
            args = [ptr] * 4
            args[hole] = None
            assert fn(ctx, tab, 1, *args) == _lib.JJ_ERR_INVALID
    comp = eng.fixedbase_composite_table(np.stack([gens["G"], gens["P"]]), [64, 64])
    try:
        assert lib.jj_fixedvar_mul_vartime(ctx, comp._h, 1, ptr, ptr, ptr, ptr) == _lib.JJ_ERR_INVALID
        assert b"composite" in lib.jj_last_error(ctx)
        assert lib.jj_fixedvar_mul_vartime(ctx, comp._h, 0, None, None, None, None) == _lib.JJ_ERR_INVALID
    finally:
        comp.close()
    buf[:] = 0xEE
    assert lib.jj_fixedvar_mul_vartime(ctx, tab, 0, None, None, None, None) == 0                     # n = 0 succeeds
    assert lib.jj_fixedvar_mul_vartime_compressed(ctx, tab, 0, ptr, ptr, ptr, ptr) == 0 and (buf == 0xEE).all()   # ... and touches nothing
    assert lib.jj_fixedvar_mul_vartime(ctx, tabs[7]._h, 0, ptr, ptr, ptr, ptr) == 0 and (buf == 0xEE).all()


def test_two_host_threads_on_one_context(lane_eng, tabs, gens):
    """the fused call and jj_fixedbase_mul on the same table from two threads"""
    e = lane_eng
    sets = [inputs(e, 4000 + 13 * t, seed=300 + 10 * t) for t in range(2)]
    exps = [want(gens["G"], *s) for s in sets]
    fixed = [O.fixedbase_mul(s[0], gens["G"]) for s in sets]
    errs = []

    def work(t):
        try:
            for _ in range(3):
                for wb in (8, 7):
                    if not np.array_equal(e.fixedvar_mul_vartime(tabs[wb], *sets[t]), exps[t]):
                        errs.append("thread %d, table %d: wrong result" % (t, wb))
                    if not np.array_equal(e.fixedbase_mul(tabs[wb], sets[t][0]), fixed[t]):
                        errs.append("thread %d, table %d: wrong fixed-base result" % (t, wb))
        except Exception as x:  # noqa: BLE001
            errs.append(repr(x))

    ths = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    assert not errs, errs


def test_caller_stream_and_back(lane_eng, tabs, gens):
    """a call on a caller's stream (jj_ctx_set_stream through torch's current stream), then on the context's own stream again"""
    import torch

    e, n = lane_eng, 2000
    a, b, q = inputs(e, n, seed=41)
    exp = want(gens["G"], a, b, q)
    dev = [torch.from_numpy(x).cuda() for x in (a, b, q)]
    for wb in (8, 7):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            r1 = e.fixedvar_mul_vartime(tabs[wb], *dev)
            r1c = e.fixedvar_mul_vartime_compressed(tabs[wb], *dev)
        s.synchronize()
        assert np.array_equal(r1.cpu().numpy(), exp) and np.array_equal(r1c.cpu().numpy(), O.compress(exp))
        assert np.array_equal(e.fixedvar_mul_vartime(tabs[wb], a, b, q), exp)                  # numpy: back on the context's own stream
        assert np.array_equal(e.fixedvar_mul_vartime(tabs[wb], *dev).cpu().numpy(), exp)       # torch's default stream
