"""
GPU tests of jj_sigverify_each (one Schnorr verdict per signature; Engine.sigverify_each, Engine.sig_locate): every planted case of
tests/sig_each_cases.py byte for byte in both modes (tests/test_sig_each_cases_cpu.py holds the expected bytes to the oracle) behind every
ladder of fixedvar_to_ext -- the quad ladder and the table's kernel (the default engine: n <= vb_quad_max), k_varbase<true> and an LDS table's
kernel above it, and k_varbase_fixed (vb_quad_max = 0 with tables of width 10 and 13: the persistent grid) --, k_sig_each_tail after each, at the
sizes around a wave and a workgroup and at the sizes derived from the persistent grid and the internal chunk; the routes against each other;
the call against the family (sigbatch_verify, sig_locate, sigbatch_locate) and against the four-call composed route;
every kind of pointer; the empty and the invalid calls; one sequence on a single context with a signature job in flight; and the entry point's
buffer-discipline row (tests/sig_each_buffer_row.py) through the guarded arenas of tests/buffer_cases.py.  No unit is sampled away or tolerated.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import sig_batch_cases as SC
from tests import sig_each_buffer_row as BR
from tests import sig_each_cases as EC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 2, 63, 64, 65, 255, 256, 257]


def chunk_units():
    """units per internal chunk of jj_sigverify_each, read from the source"""
    src = open(os.path.join(ROOT, "jubjub_amd", "csrc", "jj_abi.hip")).read()
    m = re.search(r"constexpr size_t SIG_EACH_CHUNK = \(size_t\)1 << (\d+);", src)
    assert m, "SIG_EACH_CHUNK not found in jj_abi.hip"
    return 1 << int(m.group(1))


def _vb_blocks_per_cu():
    with open(os.path.join(ROOT, "jubjub_amd", "csrc", "jj_engine.h")) as f:
        return int(re.search(r"int\s+vb_blocks_per_cu\s*=\s*(\d+)\s*;", f.read()).group(1))


@pytest.fixture(scope="module")
def eng():
    from jubjub_amd import Engine

    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def fused_eng():
    """every batch on a gathered table takes k_varbase_fixed, the ladder with both terms in one accumulator"""
    from jubjub_amd import Engine

    e = Engine(0, options={"vb_quad_max": 0})
    yield e
    e.close()


@pytest.fixture(scope="module")
def tabs(eng):
    """(base name, window_bits) -> table, built once; 0: the default LDS table.  A table serves every context of its device."""
    t = {(name, wb): eng.fixedbase_table(SC.bases()[name], wb) for name in ("prime", "order8r") for wb in (0, 10, 13)}
    yield t
    for x in t.values():
        x.close()


def grid_lanes(e):
    return e.device_info()["cus"] * 256 * _vb_blocks_per_cu()


def cuda(x):
    import torch

    return torch.from_numpy(np.array(x)).cuda()


def host(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


def check(e, tab, b, arrays=None, what=""):
    for cofactored in (True, False):
        got = host(e.sigverify_each(tab, *(arrays or b.arrays()), zip216=bool(b.flags), cofactored=cofactored))
        assert got.shape == (b.n,) and got.dtype == np.uint8
        bad = np.nonzero(got != b.expect[cofactored])[0]
        assert not len(bad), "%s%s, %s: %d of %d units differ, first: unit %d got %d want %d (planted %r)" % (
            b.name, what, "cofactored" if cofactored else "cofactorless", len(bad), b.n, bad[0], got[bad[0]], b.expect[cofactored][bad[0]], b.planted[:8])


CONFIGS = {"quad-w13": ("eng", 13), "quad-lds": ("eng", 0), "fused-ladder-w10": ("fused", 10), "fused-ladder-w13": ("fused", 13)}


@pytest.mark.parametrize("config", list(CONFIGS))
def test_every_planted_case_in_both_modes(eng, fused_eng, tabs, config):
    which, wb = CONFIGS[config]
    e = eng if which == "eng" else fused_eng
    assert e.get_option("vb_quad_max") == (0 if which == "fused" else eng.get_option("vb_quad_max")) and max(SIZES) <= eng.get_option("vb_quad_max")
    for n in SIZES:
        for b in EC.batches(n):
            check(e, tabs[b.base_name, wb], b, what=" (%s)" % config)


@pytest.fixture(scope="module")
def large(eng):
    """the closed-form batches of the sizes that exercise the persistent grid, the LDS tables' threshold and the chunk, on the device"""
    cache = {}

    def get(n):
        if n not in cache:
            b = EC.large_batch(n)
            cache[n] = (b, [cuda(x) for x in b.arrays()])
        return cache[n]
    return get


@pytest.mark.parametrize("wb", [10, 13])
def test_fused_ladder_around_the_persistent_grid(fused_eng, tabs, large, wb):
    """one wave short of the grid; the grid + 65: the cursor loop takes a second trip with a ragged last wave"""
    g = grid_lanes(fused_eng)
    for n in (g - 64, g + 65):
        b, dev = large(n)
        check(fused_eng, tabs["prime", wb], b, dev, " (fused ladder, table %d)" % wb)


def test_across_the_chunk_boundary(eng, tabs, large):
    n = chunk_units() + 65
    assert n > eng.get_option("vb_quad_max")
    b, dev = large(n)
    check(eng, tabs["prime", 13], b, dev, " (two chunks)")
    for d, h in zip(dev, b.arrays()):
        assert np.array_equal(d[:4096].cpu().numpy(), h[:4096]) and np.array_equal(d[-4096:].cpu().numpy(), h[-4096:])      # inputs as they were


def test_lds_table_above_vb_quad_max_and_the_routes_agree(eng, tabs, large):
    """vb_quad_max + 1 units: the LDS table runs k_varbase<true>, its own kernel and k_sig_each_tail; the gathered tables run k_varbase_fixed and
    k_sig_each_tail; below the threshold all run the quad ladder.  The same bytes from all of them."""
    n = eng.get_option("vb_quad_max") + 1
    b, dev = large(n)
    check(eng, tabs["prime", 0], b, dev, " (LDS table, lanes)")
    check(eng, tabs["prime", 13], b, dev, " (gathered table, fused ladder)")
    for cofactored in (True, False):
        v = [host(eng.sigverify_each(tabs["prime", wb], *dev, zip216=True, cofactored=cofactored)) for wb in (0, 10, 13)]
        assert np.array_equal(v[0], v[1]) and np.array_equal(v[0], v[2])


def test_routes_agree_on_the_planted_batches(eng, fused_eng, tabs):
    for b in EC.batches(300):
        for cofactored in (True, False):
            v = [host(e.sigverify_each(tabs[b.base_name, wb], *b.arrays(), zip216=bool(b.flags), cofactored=cofactored))
                 for e, wb in ((eng, 13), (eng, 0), (fused_eng, 13), (fused_eng, 10), (fused_eng, 0))]
            for x in v[1:]:
                assert np.array_equal(v[0], x), b.name


def test_agreement_with_the_batch_family(eng, tabs):
    """all OK iff the batch job says "ok"; any MALFORMED iff it says "malformed"; sig_locate returns exactly the units that fail"""
    for n in (1, 65):
        for b in EC.batches(n):
            v = host(eng.sigverify_each(tabs[b.base_name, 13], *b.arrays(), zip216=bool(b.flags)))
            batch = eng.sigbatch_verify(b.base, *b.arrays(), zip216=bool(b.flags))
            assert (batch == "ok") == bool((v == EC.OK).all()), (b.name, batch)
            assert (batch == "malformed") == bool((v == EC.MALFORMED).any()), (b.name, batch)
            assert eng.sig_locate(b.base, tabs[b.base_name, 13], *b.arrays(), zip216=bool(b.flags)) == b.failing(), b.name


def test_sig_locate_equals_sigbatch_locate(eng, fused_eng, tabs):
    b = EC.planted_batch(300, ["bad_s", "off_curve_r", "bad_r"])
    assert len(b.failing()) == 3
    want = eng.sigbatch_locate(b.base, *b.arrays())
    assert want == b.failing()
    for e in (eng, fused_eng):
        assert e.sig_locate(b.base, tabs["prime", 13], *b.arrays()) == want
        assert e.sig_locate(cuda(b.base), tabs["prime", 10], *[cuda(x) for x in b.arrays()]) == want
    valid = EC.batches(300)[0]
    assert eng.sig_locate(valid.base, tabs["prime", 13], *valid.arrays()) == []


def test_cofactorless_mode_equals_the_composed_route(eng, fused_eng, tabs):
    """jj_decompress x 2, jj_point_neg, jj_fixedvar_mul_vartime_compressed and a byte compare in the caller, with c reduced and s range-checked on
    the host: the route the call replaces checks the cofactorless equation"""
    for b in EC.batches(300):
        tab = tabs[b.base_name, 13]
        rp, rok = eng.decompress(b.r, b.flags)
        ap, aok = eng.decompress(b.a, b.flags)
        cred = np.stack([SC.b32(SC.to_int(x) % SC.R) for x in b.c])
        s_ok = np.array([SC.to_int(x) < SC.R for x in b.s])
        enc = eng.fixedvar_mul_vartime_compressed(tab, b.s, cred, eng.point_neg(ap))
        same = (enc == b.r).all(axis=1)
        want = np.where((rok.reshape(-1) != 0) & (aok.reshape(-1) != 0) & s_ok, np.where(same, EC.OK, EC.REJECT), EC.MALFORMED).astype(np.uint8)
        for e in (eng, fused_eng):
            got = e.sigverify_each(tab, *b.arrays(), zip216=bool(b.flags), cofactored=False)
            assert np.array_equal(got, want), b.name


def test_pointer_kinds(eng, fused_eng, tabs):
    import torch

    b = EC.planted_batch(300, ["torsion_r", "bad_s", "s_plus_r", "off_curve_r", "c_all_ones"])
    for e in (eng, fused_eng):
        tab = tabs["prime", 13]
        check(e, tab, b, what=" (host)")
        dev = [cuda(x) for x in b.arrays()]
        out = e.sigverify_each(tab, *dev)
        assert out.is_cuda and tuple(out.shape) == (b.n,) and np.array_equal(out.cpu().numpy(), b.expect[True])
        for d, h in zip(dev, b.arrays()):
            assert np.array_equal(d.cpu().numpy(), h)
        pinned = e.host_alloc(b.c.shape)
        pinned[...] = b.c
        for k, arrays in enumerate([(dev[0], b.a, b.s, pinned), (b.r, dev[1], dev[2], b.c), (dev[0], dev[1], b.s, pinned)]):
            check(e, tab, b, arrays, " (mix %d)" % k)
        # through the C ABI: device R, host A, device s, page-locked c, and a result in each kind of memory with its neighbours watched
        lib, ctx = e._lib, e._ctx
        lib.jj_ctx_use_own_stream(ctx)
        torch.cuda.synchronize()
        a_host = np.ascontiguousarray(b.a)
        for flags, cofactored in ((0, True), (EC.COFACTORLESS, False)):
            res = np.full(b.n + 64, 0xAB, np.uint8)
            rc = lib.jj_sigverify_each(ctx, tab._h, b.n, dev[0].data_ptr(), a_host.ctypes.data, dev[2].data_ptr(), pinned.ctypes.data, flags, C.c_void_p(res.ctypes.data))
            assert rc == 0 and np.array_equal(res[:b.n], b.expect[cofactored]) and (res[b.n:] == 0xAB).all()
            dres = torch.full((b.n + 64,), 0xAB, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            rc = lib.jj_sigverify_each(ctx, tab._h, b.n, dev[0].data_ptr(), a_host.ctypes.data, dev[2].data_ptr(), pinned.ctypes.data, flags, C.c_void_p(dres.data_ptr()))
            assert rc == 0 and lib.jj_ctx_sync(ctx) == 0
            assert np.array_equal(dres[:b.n].cpu().numpy(), b.expect[cofactored]) and bool((dres[b.n:] == 0xAB).all())
        out = np.zeros(b.n, np.uint8)
        assert e.sigverify_each(tab, *b.arrays(), out=out) is out and np.array_equal(out, b.expect[True])


def test_empty_and_invalid_calls(eng, tabs):
    from jubjub_amd import _lib

    lib, ctx, tab = eng._lib, eng._ctx, tabs["prime", 13]._h
    buf = np.full(64, 0xEE, np.uint8)
    ptr = C.c_void_p(buf.ctypes.data)
    for t in (tab, tabs["prime", 0]._h):
        assert lib.jj_sigverify_each(ctx, t, 0, None, None, None, None, 0, None) == 0                     # n = 0 succeeds with NULL arrays
        assert lib.jj_sigverify_each(ctx, t, 0, ptr, ptr, ptr, ptr, EC.ZIP216 | EC.COFACTORLESS, ptr) == 0 and (buf == 0xEE).all()      # ... and touches nothing
    assert eng.sigverify_each(tabs["prime", 13], *[np.zeros((0, 32), np.uint8)] * 4).shape == (0,)
    for flags in (2, 4, 8, 32, 17 | 2, 1 << 31):                                                          # anything but ZIP-216 and cofactorless
        assert lib.jj_sigverify_each(ctx, tab, 1, ptr, ptr, ptr, ptr, flags, ptr) == _lib.JJ_ERR_INVALID
        assert lib.jj_sigverify_each(ctx, tab, 0, None, None, None, None, flags, None) == _lib.JJ_ERR_INVALID
    assert b"flags" in lib.jj_last_error(ctx)
    assert lib.jj_sigverify_each(None, tab, 1, ptr, ptr, ptr, ptr, 0, ptr) == _lib.JJ_ERR_INVALID         # a NULL context
    assert lib.jj_sigverify_each(ctx, None, 1, ptr, ptr, ptr, ptr, 0, ptr) == _lib.JJ_ERR_INVALID         # a NULL table
    assert lib.jj_sigverify_each(ctx, None, 0, None, None, None, None, 0, None) == _lib.JJ_ERR_INVALID
    for hole in range(5):                                                                                 # a NULL array with n > 0
        args = [ptr] * 5
        args[hole] = None
        assert lib.jj_sigverify_each(ctx, tab, 1, *args[:4], 0, args[4]) == _lib.JJ_ERR_INVALID
    comp = eng.fixedbase_composite_table(np.stack([SC.bases()["prime"], SC.bases()["order8r"]]), [64, 64])
    try:
        assert lib.jj_sigverify_each(ctx, comp._h, 1, ptr, ptr, ptr, ptr, 0, ptr) == _lib.JJ_ERR_INVALID
        assert b"composite" in lib.jj_last_error(ctx)
    finally:
        comp.close()
    assert (buf == 0xEE).all()
    b = EC.batches(65)[0]
    check(eng, tabs["prime", 13], b, what=" (after the refused calls)")


def test_one_sequence_on_a_single_context(fused_eng, tabs):
    """fixedvar_mul_vartime, sigverify_each, a sigbatch_begin job in flight, sigverify_each, then the finish: the ladders share the lane tables and
    the work cursor, the stream orders them"""
    from oracle import c_oracle as O
    from tests.fixedvar_cases import want
    from tests.util import rand_points, rand_scalars

    e, tab = fused_eng, tabs["prime", 13]
    n = 3000
    fa, fb, fq = rand_scalars(91, n, full_width=True), rand_scalars(92, n, full_width=True), rand_points(93, n)
    b1 = EC.planted_batch(n, ["bad_s", "torsion_r", "off_curve_r", "r_order2", "c_plus_r"])
    b2 = EC.planted_batch(257, ["both_undecodable", "a_is_neg_b", "bad_r", "torsion_a_odd_c", "s_r_minus_1"])
    job_batch = EC.batches(300)[0]
    r0 = e.fixedvar_mul_vartime(tab, fa, fb, fq)
    v1 = e.sigverify_each(tab, *b1.arrays())
    job = e.sigbatch_begin(job_batch.base, *job_batch.arrays())
    v2 = e.sigverify_each(tab, *b2.arrays(), cofactored=False)
    v3 = e.sigverify_each(tab, *b1.arrays(), cofactored=False)
    r1 = e.fixedvar_mul_vartime(tab, fa, fb, fq)
    done = e.msm_finish(job)
    assert np.array_equal(r0, want(SC.bases()["prime"], fa, fb, fq)) and np.array_equal(r1, r0)
    assert np.array_equal(v1, b1.expect[True]) and np.array_equal(v2, b2.expect[False]) and np.array_equal(v3, b1.expect[False])
    assert bytes(done) == bytes(SC.IDENTITY)
    assert O.predicate("is_identity", np.asarray(done).reshape(1, 64))[0]


def test_buffer_discipline_row():
    """the row of tests/sig_each_buffer_row.py through the runner of tests/test_gpu_buffers.py (its Env, checked_call, placements and skews): every
    size of the table x every skew (0, 16, 496 and the mixed one) in one device arena, the host arenas and the mixed placements at the host sizes,
    n = 0 -- on both routes: return code 0, the n verdict bytes equal to the oracle, guards and inputs untouched"""
    import test_gpu_buffers as TB

    case, env = BR.ROW, TB.Env()
    try:
        for options in case.options:
            for n in TB.SIZES:
                for skew in TB.SKEW_SETS:
                    TB.checked_call(env, case, options, n, TB.placement(case, "dev", "dev"), skew)
            for n in TB.HOST_SIZES:
                for ins, outs in (("host", "host"), ("pinned", "pinned"), ("dev", "host"), ("host", "dev"), ("dev", "pinned")):
                    TB.checked_call(env, case, options, n, TB.placement(case, ins, outs), TB.MIXED_SKEW)
            for where in ("dev", "host"):
                for skew in (TB.SKEW_SETS[1], TB.MIXED_SKEW):
                    TB.checked_call(env, case, options, 0, TB.placement(case, where, where), skew)
    finally:
        env.close()
