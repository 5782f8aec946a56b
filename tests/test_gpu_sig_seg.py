"""
GPU tests of jj_sigbatch_ragged (one batch Schnorr verdict per segment of one signature array): every case of tests/sig_seg_cases.py byte for byte
(tests/test_sig_seg_cases_cpu.py holds the expected rows to the oracle) on host arrays, on device tensors and on mixes of both (every case on each); every segment's row
against jj_sigbatch_begin + jj_msm_finish on the segment alone; inputs unchanged, rows beyond S untouched; the argument checks on a live context;
one sequence of calls on a single context with a signature job in flight across it; the verdict strings; and Engine.sigbatch_locate, which must
return exactly the planted signatures within its budget of calls; and the entry point's buffer-discipline row (tests/sig_seg_buffer_row.py) through the
guarded arenas of tests/buffer_cases.py.
"""
import ctypes as C
import math

import numpy as np
import pytest

from tests import sig_batch_cases as SC
from tests import sig_seg_buffer_row as BR
from tests import sig_seg_cases as GC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from jubjub_amd import Engine

    e = Engine(0)
    yield e
    e.close()


def cuda(x):
    import torch

    return torch.from_numpy(np.array(x)).cuda()


def rows_of(out):
    a = out.cpu().numpy() if hasattr(out, "cpu") else np.asarray(out)
    return [bytes(r) for r in a.reshape(-1, 64)]


def check(c, out, what=""):
    got, want = rows_of(out), [bytes(r) for r in c.expected]
    assert len(got) == len(want), c.name
    for g, (x, y) in enumerate(zip(got, want)):
        assert x == y, "%s%s, segment %d of sizes %r: got %s, want %s" % (c.name, what, g, c.sizes()[:8], x.hex(), y.hex())


def test_every_case_on_host_arrays(eng):
    for c in GC.all_cases():
        check(c, eng.sigbatch_ragged(c.base, c.offsets, *c.arrays(), zip216=bool(c.flags)))


def test_every_case_on_device_tensors_and_the_inputs_stay_as_they_were(eng):
    import torch

    for c in GC.all_cases():
        dev = [cuda(c.base)] + [cuda(x) for x in c.arrays()]
        out = eng.sigbatch_ragged(dev[0], c.offsets, *dev[1:], zip216=bool(c.flags))
        assert out.is_cuda and tuple(out.shape) == (c.S, 64)
        check(c, out, " (device)")
        for d, h in zip(dev, (c.base,) + c.arrays()):
            assert np.array_equal(d.cpu().numpy(), h), c.name
    torch.cuda.synchronize()


def test_every_case_on_mixed_pointer_kinds(eng):
    """every case with its five arrays, the base and the result in mixes of device, pageable host and page-locked host memory: four mixes, two per
    side of the base"""
    import torch

    for c in GC.all_cases():
        r, a, s, ch, z = c.arrays()
        dr, da, ds, dc, dz = [cuda(x) for x in c.arrays()]
        pinned = eng.host_alloc(ch.shape)
        pinned[...] = ch
        mixes = [(c.base, (dr, a, s, pinned, dz)), (cuda(c.base), (r, da, ds, ch, z)), (cuda(c.base), (dr, da, s, ch, dz)), (c.base, (r, a, ds, dc, z))]
        for i, (base, arrays) in enumerate(mixes):
            check(c, eng.sigbatch_ragged(base, c.offsets, *arrays, zip216=bool(c.flags)), " (mix %d)" % i)
        host_out = np.full((c.S, 64), 0xAB, np.uint8)
        assert eng.sigbatch_ragged(c.base, c.offsets, dr, da, ds, dc, dz, zip216=bool(c.flags), out=None).is_cuda
        assert eng.sigbatch_ragged(c.base, c.offsets, r, a, s, ch, z, zip216=bool(c.flags), out=host_out) is host_out
        check(c, host_out, " (caller's host rows)")
    torch.cuda.synchronize()


def test_rows_beyond_s_stay_as_they_were(eng):
    """a device result tensor longer than S keeps its other rows"""
    import torch

    by_name = {c.name: c for c in GC.all_cases()}
    picks = [by_name["valid [63, 1, 64, 65]"], by_name["two failures in two segments"], by_name["a malformed and a reject unit in one segment"],
             by_name["[3, 4096, 2], malformed in the job, bad s behind it"], by_name["geometric, S = 64, ZIP-216, a non-canonical key in segment 40"]]
    lib, ctx = eng._lib, eng._ctx
    for c in picks:
        dr, da, ds, dc, dz = [cuda(x) for x in c.arrays()]
        big = torch.full((c.S + 3, 64), 0xAB, dtype=torch.uint8, device="cuda")
        ptrs = [C.c_void_p(t.data_ptr()) for t in (dr, da, ds, dc, dz)]
        offs = np.ascontiguousarray(c.offsets)
        base = np.ascontiguousarray(c.base)
        assert lib.jj_sigbatch_ragged(ctx, C.c_void_p(base.ctypes.data), c.S, C.c_void_p(offs.ctypes.data), *ptrs, c.flags, C.c_void_p(big.data_ptr() + 64)) == 0
        eng.sync()
        torch.cuda.synchronize()
        got = big.cpu().numpy()
        check(c, got[1:c.S + 1], " (rows 1 .. S of a longer tensor)")
        assert (got[0] == 0xAB).all() and (got[c.S + 1:] == 0xAB).all(), c.name


def test_every_row_equals_sigbatch_begin_on_the_segment_alone(eng):
    ran = 0
    for c in GC.all_cases():
        if c.n > 600:
            continue
        got = rows_of(eng.sigbatch_ragged(c.base, c.offsets, *c.arrays(), zip216=bool(c.flags)))
        for g in range(c.S):
            b = c.slice(g)
            alone = bytes(eng.msm_finish(eng.sigbatch_begin(b.base, *b.arrays(), zip216=bool(c.flags))))
            assert got[g] == alone == bytes(c.expected[g]), "%s, segment %d" % (c.name, g)
            ran += 1
    assert ran > 500


def test_empty_calls(eng):
    """S = 0 touches nothing; n = 0 with S > 0 writes S identities and reads no array"""
    import torch

    lib, ctx = eng._lib, eng._ctx
    base = (C.c_uint8 * 64).from_buffer_copy(bytes(SC.bases()["prime"]))
    out = np.full((4, 64), 0xAB, np.uint8)
    assert lib.jj_sigbatch_ragged(ctx, base, 0, None, None, None, None, None, None, 0, None) == 0
    assert lib.jj_sigbatch_ragged(ctx, base, 0, None, None, None, None, None, None, 1, C.c_void_p(out.ctypes.data)) == 0 and (out == 0xAB).all()
    offs = np.zeros(4, np.uint64)
    for flags in (0, 1):
        out[...] = 0xAB
        assert lib.jj_sigbatch_ragged(ctx, base, 3, C.c_void_p(offs.ctypes.data), None, None, None, None, None, flags, C.c_void_p(out.ctypes.data)) == 0
        assert rows_of(out[:3]) == [bytes(SC.IDENTITY)] * 3 and (out[3] == 0xAB).all()
        dev = torch.full((4, 64), 0xAB, dtype=torch.uint8, device="cuda")
        assert lib.jj_sigbatch_ragged(ctx, base, 3, C.c_void_p(offs.ctypes.data), None, None, None, None, None, flags, C.c_void_p(dev.data_ptr())) == 0
        eng.sync()
        torch.cuda.synchronize()
        assert rows_of(dev[:3]) == [bytes(SC.IDENTITY)] * 3 and (dev[3].cpu().numpy() == 0xAB).all()
    c = GC.layout("all empty", [0, 0, 0])
    check(c, eng.sigbatch_ragged(c.base, c.offsets, *c.arrays()))


def test_argument_checks_on_a_live_context(eng):
    """every JJ_ERR_INVALID row.  What is observed: the return code, the result rows staying as they were, and the same context giving right
    rows in the next call; that nothing was queued is read in the source (the checks stand before the first launch), not seen here"""
    import torch

    from jubjub_amd import _lib

    lib, ctx = eng._lib, eng._ctx
    c = GC.layout("checks", [3, 4], {1: ("bad_s", 2)})
    good = np.array([0, 3, 7], np.uint64)
    host = [np.ascontiguousarray(x) for x in (c.base, *c.arrays())]
    base, r, a, s, ch, z = [C.c_void_p(x.ctypes.data) for x in host]
    out = np.full((2, 64), 0xAB, np.uint8)
    po = lambda x: C.c_void_p(x.ctypes.data)      # noqa: E731

    def works():
        res = np.zeros((2, 64), np.uint8)
        return lib.jj_sigbatch_ragged(ctx, base, 2, po(good), r, a, s, ch, z, 0, po(res)) == 0 and rows_of(res) == [bytes(x) for x in c.expected]

    assert works()
    dev_offsets = torch.from_numpy(good.view(np.uint8).copy()).cuda()
    big = 1 << 24
    rows = {
        "NULL context": (None, base, 2, po(good), r, a, s, ch, z, 0, po(out)),
        "NULL base": (ctx, None, 2, po(good), r, a, s, ch, z, 0, po(out)),
        "NULL base, S = 0": (ctx, None, 0, None, None, None, None, None, None, 0, None),
        "NULL offsets, S > 0": (ctx, base, 2, None, r, a, s, ch, z, 0, po(out)),
        "NULL out, S > 0": (ctx, base, 2, po(good), r, a, s, ch, z, 0, None),
        "NULL r": (ctx, base, 2, po(good), None, a, s, ch, z, 0, po(out)),
        "NULL a": (ctx, base, 2, po(good), r, None, s, ch, z, 0, po(out)),
        "NULL s": (ctx, base, 2, po(good), r, a, None, ch, z, 0, po(out)),
        "NULL c": (ctx, base, 2, po(good), r, a, s, None, z, 0, po(out)),
        "NULL z": (ctx, base, 2, po(good), r, a, s, ch, None, 0, po(out)),
        "offsets[0] != 0": (ctx, base, 2, po(np.array([1, 3, 7], np.uint64)), r, a, s, ch, z, 0, po(out)),
        "a decreasing pair": (ctx, base, 2, po(np.array([0, 8, 7], np.uint64)), r, a, s, ch, z, 0, po(out)),
        "offsets in device memory": (ctx, base, 2, C.c_void_p(dev_offsets.data_ptr()), r, a, s, ch, z, 0, po(out)),
        "flags 2": (ctx, base, 2, po(good), r, a, s, ch, z, 2, po(out)),
        "flags 8 (the cofactor flag is the call's own)": (ctx, base, 2, po(good), r, a, s, ch, z, 8, po(out)),
        "flags 0x80000001": (ctx, base, 2, po(good), r, a, s, ch, z, 0x80000001, po(out)),
        "2n + S = 2^24 + 1": (ctx, base, 1, po(np.array([0, big // 2], np.uint64)), r, a, s, ch, z, 0, po(out)),
        "2n + S = 2^24 + 2": (ctx, base, 2, po(np.array([0, 3, big // 2], np.uint64)), r, a, s, ch, z, 0, po(out)),
        "offsets[S] = 2^63": (ctx, base, 2, po(np.array([0, 3, 1 << 63], np.uint64)), r, a, s, ch, z, 0, po(out)),
    }
    for name, args in rows.items():
        assert lib.jj_sigbatch_ragged(*args) == _lib.JJ_ERR_INVALID, name
        assert (out == 0xAB).all(), name
        assert works(), "after " + name
    # a misaligned device pointer: each array, the result and the base in turn
    for which in range(7):
        keep, ptrs = [], []
        for i, x in enumerate(host[1:] + [out, host[0]]):
            if i == which:
                t = torch.full((x.size + 16,), 0xAB, dtype=torch.uint8, device="cuda")
                t[8:8 + x.size] = torch.from_numpy(x.reshape(-1).copy()).cuda()
                keep.append(t)
                ptrs.append(C.c_void_p(t.data_ptr() + 8))
            else:
                ptrs.append(C.c_void_p(x.ctypes.data))
        torch.cuda.synchronize()
        assert lib.jj_sigbatch_ragged(ctx, ptrs[6], 2, po(good), *ptrs[:5], 0, ptrs[5]) == _lib.JJ_ERR_INVALID, which
        assert "device pointers must be 16-byte aligned" in lib.jj_last_error(ctx).decode(), which
        eng.sync()
        if which == 5:
            assert (keep[0].cpu().numpy() == 0xAB).all()
        assert (out == 0xAB).all() and works(), which
    with pytest.raises(ValueError):
        eng.sigbatch_ragged(c.base, [0, 3, 6], *c.arrays())
    with pytest.raises(ValueError):
        eng.sigbatch_ragged(c.base, c.offsets, *c.arrays(), out=np.zeros((3, 64), np.uint8))


def test_one_sequence_on_a_single_context(eng):
    """sigbatch_ragged, msm_ragged, msm, decompress with the cofactor flag, sigbatch_ragged with other offsets -- the workspaces the calls share are
    ordered by the stream -- with a sigbatch_begin job in flight across all of them and finished last"""
    from oracle import c_oracle as O
    from tests.util import rand_points, rand_scalars

    by_name = {c.name: c for c in GC.all_cases()}
    first, second = by_name["[3, 4096, 2], malformed in the job, bad s behind it"], by_name["300 x [1], failures at segments 0, 63, 64, 255, 256, 299"]
    plain = SC.batch(257, "bad_r", 64)
    job = eng.sigbatch_begin(cuda(plain.base), *[cuda(x) for x in plain.arrays()])
    check(first, eng.sigbatch_ragged(first.base, first.offsets, *first.arrays()))
    sc, pt = rand_scalars(11, 700), rand_points(11, 700)
    offs = [0, 5, 5, 300, 700]
    want = np.stack([O.msm(sc[lo:hi], pt[lo:hi]) if hi > lo else SC.IDENTITY for lo, hi in zip(offs[:-1], offs[1:])])
    assert rows_of(eng.msm_ragged(sc, pt, offs)) == rows_of(want)
    assert bytes(eng.msm(sc, pt)) == bytes(O.msm(sc, pt))
    enc = np.concatenate([first.r[:300], SC.off_curve_encoding()[None], SC.NONCANONICAL_IDENTITY[None]])
    for flags in (8, 9):
        got, ok = eng.decompress(enc, flags=flags)
        wpts, wok = O.decompress(enc, flags)
        assert np.array_equal(np.asarray(ok), wok) and np.array_equal(np.asarray(got)[wok != 0], wpts[wok != 0])
    check(second, eng.sigbatch_ragged(cuda(second.base), second.offsets, *[cuda(x) for x in second.arrays()]))
    check(first, eng.sigbatch_ragged(first.base, first.offsets, *first.arrays()), " (again)")
    assert bytes(eng.msm_finish(job)) == bytes(plain.expected)


def test_verdict_strings(eng):
    c = {x.name: x for x in GC.all_cases()}["300 x [1], failures at segments 0, 63, 64, 255, 256, 299"]
    want = ["ok"] * 300
    for g, v in {0: "reject", 63: "malformed", 64: "reject", 255: "malformed", 256: "reject", 299: "reject"}.items():
        want[g] = v
    assert [GC.verdict(r) for r in c.expected] == want
    assert eng.sigbatch_ragged_verify(c.base, c.offsets, *c.arrays()) == want
    assert eng.sigbatch_ragged_verify(c.base, c.offsets, c.r, c.a, c.s, c.c) == want, "z drawn"
    assert eng.sigbatch_ragged_verify(cuda(c.base), c.offsets, *[cuda(x) for x in c.arrays()]) == want
    z = GC.layout("zip", [63, 1, 64, 65], {2: ("noncanonical_a_zip216", 63)})
    assert eng.sigbatch_ragged_verify(z.base, z.offsets, *z.arrays(), zip216=True) == ["ok", "ok", "malformed", "ok"]
    assert eng.sigbatch_ragged_verify(z.base, z.offsets, *z.arrays(), zip216=False) == ["ok"] * 4


def test_locate_returns_exactly_the_planted_signatures(eng, monkeypatch):
    """the number of jj_sigbatch_ragged calls: one for a valid batch, at most 1 + ceil(log_fanout(n)) with failures"""
    bound = eng._lib.jj_sigbatch_ragged
    calls = []

    def counted(*args):
        calls.append(args[2])
        return bound(*args)

    monkeypatch.setattr(eng._lib, "jj_sigbatch_ragged", counted)
    base, r, a, s, c, z, want = GC.locate_batch()
    vbase, vr, va, vs, vc, vz, none = GC.locate_batch(valid=True)
    assert none == [] and len(want) == 5
    for fanout in (2, 16):
        budget = 1 + math.ceil(math.log(GC.LOCATE_N, fanout))
        for dev in (False, True):
            f = cuda if dev else (lambda x: x)
            del calls[:]
            assert eng.sigbatch_locate(f(base), f(r), f(a), f(s), f(c), f(z), fanout=fanout) == want, (fanout, dev)
            assert 2 <= len(calls) <= budget, (fanout, len(calls))
            del calls[:]
            assert eng.sigbatch_locate(f(vbase), f(vr), f(va), f(vs), f(vc), f(vz), fanout=fanout) == [] and len(calls) == 1
        del calls[:]
        assert eng.sigbatch_locate(base, r, a, s, c, fanout=fanout) == want and len(calls) <= budget, "z drawn"


def test_buffer_discipline_row():
    """the row of tests/sig_seg_buffer_row.py through the runner of tests/test_gpu_buffers.py (its Env, checked_call, placements and skews): every size
    of the table x every skew in one device arena, the host arenas and the mixed placements at the host sizes, S = 0 -- return code 0, result rows
    equal to the oracle, guards and inputs untouched"""
    import test_gpu_buffers as TB

    case, env = BR.ROW, TB.Env()
    try:
        for n in TB.SIZES:
            for skew in TB.SKEW_SETS:
                TB.checked_call(env, case, {}, n, TB.placement(case, "dev", "dev"), skew)
        for n in TB.HOST_SIZES:
            for ins, outs in (("host", "host"), ("pinned", "pinned"), ("dev", "host"), ("host", "dev"), ("dev", "pinned")):
                TB.checked_call(env, case, {}, n, TB.placement(case, ins, outs), TB.MIXED_SKEW)
        for where in ("dev", "host"):
            for skew in (TB.SKEW_SETS[1], TB.MIXED_SKEW):
                TB.checked_call(env, case, {}, 0, TB.placement(case, where, where), skew)
    finally:
        env.close()
