"""jj_pedersen_commit_vartime, Engine.pedersen_commit / note_commit / note_check on the GPU against the restatement of tests/commit_cases.py (the
formula on the oracle's point arithmetic), byte for byte.

Commitment bytes: every case of the table x every n around a wave and a workgroup x every window_chunks x R's table at window_bits 8, 13 (the
fused walk), the default and 6 (the LDS kernels on the accumulator the message left), both output forms, numpy arrays and CUDA tensors, no
unit sampled away.  The composed route on packed rows gives the same bytes.  The buffer-discipline row through the guarded arenas.  Every
refused call with the output watched.  note_check over 96 rows whose plaintexts, cmu and epk come from hashlib and the oracle, with one row
planted for every verdict the check can give."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from oracle import jubjub_ref as J
from tests import commit_buffer_row as BR
from tests import commit_cases as CC
from tests import group_hash_cases as GC
from tests import pedersen_cases as PC

pytestmark = pytest.mark.gpu

RBASE_BITS = (8, 13, 0, 6)


@pytest.fixture(scope="module")
def eng():
    from jubjub_amd import Engine

    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def tables(eng):
    made = {}

    def get(kind, *key):
        if (kind,) + key not in made:
            if kind == "ped":
                gens, seg_chunks, w = key
                made[(kind,) + key] = eng.pedersen_table(CC.gens_bytes(gens), seg_chunks, w)
            else:
                base, bits = key
                made[(kind,) + key] = eng.fixedbase_table(PC.point_bytes(CC.bases()[base]).copy(), bits)
        return made[(kind,) + key]

    yield get
    for t in made.values():
        t.close()


def cuda(x):
    import torch

    return torch.from_numpy(np.array(x)).cuda()


def host(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


def same(got, want, what):
    got = host(got)
    assert got.shape == want.shape and got.dtype == np.uint8, (what, got.shape, want.shape)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert not len(bad), "%s: %d of %d units differ from the restatement, the first is unit %d" % (what, len(bad), len(want), bad[0])


def inputs(c, n):
    return [np.ascontiguousarray(a[:n]) for a in c.sources], np.ascontiguousarray(c.r[:n])


@pytest.mark.parametrize("w", CC.WINDOWS)
@pytest.mark.parametrize("cid", [c.id for c in CC.CASES])
def test_commit_bytes_every_case_size_window_and_table(eng, tables, cid, w):
    c = CC.BY_ID[cid]
    ped = tables("ped", c.gens, c.seg_chunks, w)
    for n in c.sizes:
        want = CC.expected_points(c, n)
        want_u = np.ascontiguousarray(want[:, :32])
        srcs, r = inputs(c, n)
        dsrcs, dr = [cuda(a) for a in srcs], cuda(r)
        for bits in (RBASE_BITS if c.rbase else (None,)):
            rt = tables("fb", c.rbase, bits) if c.rbase else None
            what = "%s, n %d, window_chunks %d, rbase %s" % (cid, n, w, bits)
            hr, ddr = (r, dr) if c.rbase else (None, None)
            same(eng.pedersen_commit(ped, rt, srcs, c.fields, hr, c.prefix, c.prefix_bits), want_u, what + ", host, u")
            same(eng.pedersen_commit(ped, rt, srcs, c.fields, hr, c.prefix, c.prefix_bits, point=True), want, what + ", host, point")
            got = eng.pedersen_commit(ped, rt, dsrcs, c.fields, ddr, c.prefix, c.prefix_bits)
            assert hasattr(got, "cpu")
            same(got, want_u, what + ", device, u")
            same(eng.pedersen_commit(ped, rt, dsrcs, c.fields, ddr, c.prefix, c.prefix_bits, point=True), want, what + ", device, point")


def test_planted_rows_views_and_out(eng, tables):
    c = CC.BY_ID["twin"]
    ped = tables("ped", c.gens, c.seg_chunks, 0)
    srcs, r = inputs(c, 8)
    for bits in RBASE_BITS:
        got = eng.pedersen_commit(ped, tables("fb", "P0", bits), srcs, c.fields, r, point=True)
        row = got[CC.TWIN_CANCEL_ROW]
        assert not row[:32].any() and row[32] == 1 and not row[33:].any(), bits           # the identity (0, 1): u = 0 in the u-only form
        same(got, CC.expected_points(c, 8), "twin, rbase %d" % bits)
    # row-strided views are read where they are: the note shape's three sources as columns of one wider array, on the host and on the device
    c = CC.BY_ID["note"]
    ped, rt = tables("ped", c.gens, c.seg_chunks, 0), tables("fb", "R", 13)
    n = 65
    wide = np.full((n, 52 + 32 + 32 + 7), 0xA5, np.uint8)
    wide[:, 0:52], wide[:, 52:84], wide[:, 84:116] = c.sources[0][:n], c.sources[1][:n], c.sources[2][:n]
    want = np.ascontiguousarray(CC.expected_points(c, n)[:, :32])
    for arr in (wide, cuda(wide)):
        views = [arr[:, 0:52], arr[:, 52:84], arr[:, 84:116]]
        same(eng.pedersen_commit(ped, rt, views, c.fields, c.r[:n] if arr is wide else cuda(c.r[:n]), c.prefix, c.prefix_bits), want, "note, views")
    same(eng.note_commit(ped, rt, c.sources[0][:n], 12, c.sources[1][:n], c.sources[2][:n], c.r[:n]), want, "note_commit")
    out = np.full((n + 1, 32), 0xEE, np.uint8)
    res = eng.pedersen_commit(ped, rt, [a[:n] for a in c.sources], c.fields, c.r[:n], c.prefix, c.prefix_bits, out=out[:n])
    assert np.shares_memory(res, out)
    same(out[:n], want, "out=")
    assert (out[n] == 0xEE).all()


@pytest.mark.parametrize("cid", [c.id for c in CC.CASES])
def test_composed_route_on_packed_rows(eng, tables, cid):
    c = CC.BY_ID[cid]
    n = min(65, c.nrows)
    ped = tables("ped", c.gens, c.seg_chunks, 0)
    rows, pairs = c.packed(n)
    srcs, r = inputs(c, n)
    hashed = eng.pedersen_hash(ped, cuda(rows), pairs, c.prefix, c.prefix_bits, point=True)
    dsrcs = [cuda(a) for a in srcs]
    if c.rbase is None:
        fused = eng.pedersen_commit(ped, None, dsrcs, c.fields, None, c.prefix, c.prefix_bits, point=True)
        same(fused, host(hashed), cid + ": hash-only against jj_pedersen_hash_vartime on packed rows")
        same(fused, CC.expected_points(c, n), cid + ": hash-only against the restatement")
        if len(c.strides) == 1:                                # one source: the same call layout, byte for byte, in both output forms
            own = tuple((off, nb) for _, off, nb in c.fields)
            for point in (False, True):
                same(eng.pedersen_commit(ped, None, dsrcs, c.fields, None, c.prefix, c.prefix_bits, point=point),
                     host(eng.pedersen_hash(ped, dsrcs[0], own, c.prefix, c.prefix_bits, point=point)), cid + ": one source, point=%s" % point)
        return
    for bits in RBASE_BITS:
        rt = tables("fb", c.rbase, bits)
        composed = eng.point_add(hashed, eng.fixedbase_mul(rt, cuda(r)))
        fused = eng.pedersen_commit(ped, rt, dsrcs, c.fields, cuda(r), c.prefix, c.prefix_bits, point=True)
        same(fused, host(composed), "%s, rbase %d: fused against composed" % (cid, bits))
        same(fused, CC.expected_points(c, n), "%s, rbase %d: fused against the restatement" % (cid, bits))


def test_buffer_discipline_row():
    """the row of tests/commit_buffer_row.py through the runner of tests/test_gpu_buffers.py (its Env, checked_call, placements and skews): every
    size of the table x every skew in one device arena, the host arenas and the mixed placements at the host sizes, n = 0"""
    import test_gpu_buffers as TB

    env = TB.Env()
    try:
        case = BR.ROW
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


def test_refused_calls_leave_the_output_untouched(eng, tables):
    import torch

    from jubjub_amd import _lib

    lib, ctx = eng._lib, eng._ctx
    lib.jj_ctx_use_own_stream(ctx)
    INVALID = _lib.JJ_ERR_INVALID
    c = CC.BY_ID["tiny3_two"]                                                     # exactly at capacity: 27 bits in three segments of 3
    ped, rt = tables("ped", c.gens, c.seg_chunks, 0), tables("fb", "R", 8)
    n = 4
    srcs, r = inputs(c, n)
    out = np.full((n + 1, 64), 0xEE, np.uint8)
    dout = torch.full((n + 1, 64), 0xEE, dtype=torch.uint8, device="cuda")
    dany = torch.zeros(256, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    o, rp = out.ctypes.data, r.ctypes.data
    F = lib.jj_pedersen_commit_vartime

    def u32(*v):
        return (C.c_uint32 * max(len(v), 1))(*v)

    def ptrs(*v):
        return (C.c_void_p * max(len(v), 1))(*v)

    def sizes(*v):
        return (C.c_size_t * max(len(v), 1))(*v)

    S, ST = ptrs(*[a.ctypes.data for a in srcs]), sizes(*c.strides)
    good = u32(*[v for f in c.fields for v in f])

    def call(outp, ped_h=ped._h, rbase=rt._h, n=n, prefix=0, prefix_bits=0, nsrc=3, S=S, ST=ST, nfields=3, fields=good, r=rp, flags=0, ctx=ctx):
        return F(ctx, ped_h, rbase, n, prefix, prefix_bits, nsrc, S, ST, nfields, fields, r, flags, outp)

    assert F(ctx, ped._h, None, 0, 0, 0, 0, None, None, 0, None, None, 0, None) == 0                     # n = 0 succeeds with NULL arrays
    assert call(o, n=0) == 0                                                                              # ... and touches nothing
    for outp in (o, dout.data_ptr()):
        assert call(outp, ctx=None) == INVALID                                                            # a NULL context
        assert call(outp, ped_h=None) == INVALID                                                          # a NULL table
        assert call(outp, ped_h=rt._h) == INVALID                                                         # a fixed-base table as `ped`
        assert call(outp, rbase=ped._h) == INVALID and b"Pedersen" in lib.jj_last_error(ctx)              # a Pedersen table as `rbase`
        assert call(outp, rbase=None) == INVALID and call(outp, r=None) == INVALID                        # exactly one of rbase, r32 NULL
        assert b"both" in lib.jj_last_error(ctx)
        assert call(outp, fields=u32(0, 1, 7, 1, 0, 5, 2, 2, 16)) == INVALID                              # one bit over capacity
        assert b"longer" in lib.jj_last_error(ctx)
        assert call(outp, prefix=1, prefix_bits=1) == INVALID                                             # ... by the prefix
        assert call(outp, fields=u32(0, 1, 7, 1, 1, 17, 2, 2, 3)) == INVALID                              # a field past its source's stride: 1 + 3 bytes of 3
        assert b"stride" in lib.jj_last_error(ctx)
        assert call(outp, fields=u32(0, 1, 7, 1, 0, 0, 2, 2, 15)) == INVALID                              # an empty field
        assert call(outp, fields=u32(0, 1, 7, 3, 0, 5, 2, 2, 15)) == INVALID                              # src = nsrc
        assert b"source" in lib.jj_last_error(ctx)
        assert call(outp, nsrc=2) == INVALID                                                              # ... a field of source 2 with two sources
        assert call(outp, nfields=5, fields=u32(*([0, 0, 1] * 5))) == INVALID                             # nfields = 5
        assert call(outp, nsrc=5) == INVALID and call(outp, nsrc=-1) == INVALID                           # nsrc outside 0..4
        assert call(outp, nsrc=0) == INVALID                                                              # nsrc = 0 with fields
        assert call(outp, prefix_bits=33, nfields=0) == INVALID and call(outp, prefix_bits=-1, nfields=0) == INVALID
        assert call(outp, flags=2) == INVALID and call(outp, flags=3) == INVALID                          # an unknown flag
        assert call(outp, S=None) == INVALID and call(outp, ST=None) == INVALID and call(outp, fields=None) == INVALID      # NULL host arrays
        assert call(outp, S=ptrs(srcs[0].ctypes.data, None, srcs[2].ctypes.data)) == INVALID               # a NULL source
        assert call(outp, S=ptrs(srcs[0].ctypes.data, dany.data_ptr() + 8, srcs[2].ctypes.data)) == INVALID           # a misaligned device source
        assert call(outp, r=dany.data_ptr() + 8) == INVALID                                                # ... r
        assert call(outp, ST=sizes(5, (1 << 32) + 1, 9)) == INVALID and b"2^32" in lib.jj_last_error(ctx)  # a stride over 2^32
        assert call(outp, n=1 << 30) == INVALID and b"2^32" in lib.jj_last_error(ctx)                      # n * stride over 2^32
    assert call(dout.data_ptr() + 4) == INVALID and call(None) == INVALID
    comp = eng.fixedbase_composite_table(np.stack([PC.point_bytes(CC.bases()["R"])]).copy(), [64])
    try:
        assert call(o, rbase=comp._h) == INVALID and b"composite" in lib.jj_last_error(ctx)               # a composite table as `rbase`
    finally:
        comp.close()
    assert lib.jj_ctx_sync(ctx) == 0
    assert (out == 0xEE).all() and bool((dout == 0xEE).all())                                             # untouched by every refused call
    assert all(np.array_equal(a, b) for a, b in zip(srcs, inputs(c, n)[0])) and np.array_equal(r, c.r[:n])
    assert call(o, flags=1) == 0                                                                          # the context is as good as before
    same(out[:n], CC.expected_points(c, n), "after the refused calls")
    assert (out[n] == 0xEE).all()
    # nsrc = 0 without fields: the prefix alone, blinded
    assert call(o, nsrc=0, S=None, ST=None, nfields=0, fields=None, prefix=0b101, prefix_bits=3, flags=1) == 0
    h = J.affine_to_extended(PC.expected(CC.gens_of(c.gens), c.seg_chunks, [1, 0, 1]))
    want = np.stack([PC.point_bytes(J.ext_to_affine(J.ext_add(h, J.affine_to_extended(J.scalar_mul_fast(CC.bases()["R"], c.r_int(i)))))) for i in range(n)])
    same(out[:n], want, "prefix only")
    with pytest.raises(ValueError):
        eng.pedersen_commit(ped, rt, srcs, c.fields, None)
    with pytest.raises(ValueError):
        eng.pedersen_commit(ped, rt, srcs, ((0, 1, 7), (1, 0, 5), (2, 8, 9)), r)
    with pytest.raises(ValueError):
        eng.pedersen_commit(ped, rt, srcs + srcs, c.fields, r)


# ---------------------------------------------------------------------------------------------------- note_check
GD_PERSONAL, GD_PREFIX, EXPAND_PERSONAL = b"JJ_gd_t1", bytes(range(64)), b"JJ_ExpandSeed_t1"
NOTE_ROWS, PLAIN_LEN = 96, 60


def to_scalar(personal, data):
    return int.from_bytes(hashlib.blake2b(data, digest_size=64, person=personal).digest(), "little") % J.R_MOD


def le32(v):
    return np.frombuffer(v.to_bytes(32, "little"), dtype=np.uint8)


def bits_of(b, count):
    return [(b[k >> 3] >> (k & 7)) & 1 for k in range(count)]


def build_notes():
    """(ivk, plaintexts, cmu, epk, verdicts) of 96 rows by hashlib and the oracle; the planted rows are named in the returned dict"""
    from jubjub_amd import engine as E

    rng = np.random.default_rng(31337)
    gens, rpt = CC.gens_of("four"), CC.bases()["R"]
    ivk = int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") % J.R_MOD
    # diversifiers: about half have a point; the rows take those that do, one planted row takes one that does not
    cand = rng.integers(0, 256, size=(4 * NOTE_ROWS, 11), dtype=np.uint8)
    pts, ok = GC.expected(GD_PERSONAL, GD_PREFIX, cand, E.GROUP_HASH_FLAGS)
    with_point, without = np.nonzero(ok)[0], np.nonzero(ok == 0)[0]
    assert len(with_point) >= NOTE_ROWS and len(without)
    plain = rng.integers(0, 256, size=(NOTE_ROWS, PLAIN_LEN), dtype=np.uint8)
    plant = {"lead": 5, "no_point": 9, "cmu": 17, "epk": 23, "value": 31, "lead1_big": 40, "lead1": 41}
    plain[:, 0] = 2
    plain[plant["lead"], 0] = 3
    plain[plant["lead1"], 0] = plain[plant["lead1_big"], 0] = 1
    plain[plant["lead1"], 51] &= 0x07                                             # rseed below 2^251: a canonical Fr
    plain[plant["lead1_big"], 20:52] = le32(J.R_MOD)                              # rseed = r: not canonical
    cmu, epk, verdict = np.zeros((NOTE_ROWS, 32), np.uint8), np.zeros((NOTE_ROWS, 32), np.uint8), np.ones(NOTE_ROWS, np.uint8)
    for i in range(NOTE_ROWS):
        k = without[0] if i == plant["no_point"] else with_point[i]
        plain[i, 1:12] = cand[k]
        row = plain[i].tobytes()
        if i == plant["no_point"]:
            continue
        gd = (int.from_bytes(pts[k][:32].tobytes(), "little"), int.from_bytes(pts[k][32:].tobytes(), "little"))
        pkd = J.scalar_mul_fast(gd, ivk)
        rseed = row[20:52]
        rcm = int.from_bytes(rseed, "little") if row[0] == 1 else to_scalar(EXPAND_PERSONAL, rseed + b"\x04")
        bits = [1] * 6 + bits_of(row[12:20], 64) + bits_of(J.affine_to_bytes(gd), 256) + bits_of(J.affine_to_bytes(pkd), 256)
        h = J.affine_to_extended(PC.expected(gens, 63, bits))
        cm = J.ext_to_affine(J.ext_add(h, J.affine_to_extended(J.scalar_mul_fast(rpt, rcm & ((1 << 252) - 1)))))
        cmu[i] = le32(cm[0])
        epk[i] = np.frombuffer(J.affine_to_bytes(J.scalar_mul_fast(gd, to_scalar(EXPAND_PERSONAL, rseed + b"\x05"))), dtype=np.uint8)
    cmu[plant["cmu"], 7] ^= 0x10
    epk[plant["epk"], 30] ^= 0x01
    plain[plant["value"], 15] ^= 0x40                                             # after cmu was made: v differs from the committed one
    epk[plant["lead1"]] = 0xA5                                                    # lead 1 has no epk check: any bytes pass
    for name in ("lead", "no_point", "lead1_big"):
        verdict[plant[name]] = 2
    for name in ("cmu", "epk", "value"):
        verdict[plant[name]] = 0
    return le32(ivk).copy(), plain, cmu, epk, verdict, plant


def test_note_check_verdicts_are_exact(eng, tables):
    ivk, plain, cmu, epk, want, plant = build_notes()
    ped = tables("ped", "four", 63, 0)
    for bits in (0, 13):
        rt = tables("fb", "R", bits)
        for conv in (lambda x: x, cuda):
            got = eng.note_check(conv(ivk), conv(plain), conv(cmu), ped, rt, GD_PERSONAL, GD_PREFIX, EXPAND_PERSONAL, epk=conv(epk), leads=(1, 2))
            assert hasattr(got, "cpu") == (conv is cuda)
            got = host(got)
            assert got.dtype == np.uint8 and got.shape == (NOTE_ROWS,)
            assert got.tolist() == want.tolist(), (bits, np.nonzero(got != want)[0].tolist())
    rt = tables("fb", "R", 0)
    # leads = (2,), the default: both lead-1 rows are malformed
    w2 = want.copy()
    w2[plant["lead1"]] = 2
    assert host(eng.note_check(ivk, cuda(plain), cuda(cmu), ped, rt, GD_PERSONAL, GD_PREFIX, EXPAND_PERSONAL, epk=cuda(epk))).tolist() == w2.tolist()
    # without epk the flipped epk bit is not looked at
    w3 = want.copy()
    w3[plant["epk"]] = 1
    assert host(eng.note_check(ivk, plain, cmu, ped, rt, GD_PERSONAL, GD_PREFIX, EXPAND_PERSONAL, leads=(1, 2))).tolist() == w3.tolist()
    # another ivk: no row is a note, the malformed ones stay malformed
    other = ivk.copy()
    other[0] ^= 1
    got = host(eng.note_check(other, plain, cmu, ped, rt, GD_PERSONAL, GD_PREFIX, EXPAND_PERSONAL, epk=epk, leads=(1, 2)))
    assert got.tolist() == np.where(want == 2, 2, 0).tolist()
