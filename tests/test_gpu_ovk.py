"""
GPU tests of jj_blake2b and jj_ka_kdf_each (raw BLAKE2b digests over rows gathered from several arrays: k_blake2b<32|64>; the key agreement with
one secret scalar per row: k_varbase_mont_ka_each<cofactor>) and of what the Python package builds on them (Engine.blake2b, ka_kdf_each,
note_encrypt, ovk_open).  Every check demands byte equality with the restatements of tests/ovk_cases.py -- hashlib.blake2b over the concatenated
rows, tests/ka_cases.py's decoder, integer ladder and doublings, tests/aead_cases.py's pure-Python AEAD --; no row is sampled or tolerated
except in the one call of 2^20 + 1 rows, whose rows are compared with their 1025-row tile on the device.  Every BLAKE2b case at both digest
lengths with host and device pointers mixed, a last row that begins at 2^32 - stride, every scalar-point pair under every flag combination at
every size with and without h32, the composed route, one scalar repeated against jj_ka_kdf, the chunk seam, every refusal of the contract
with the outputs watched, and the round trip note_encrypt -> ovk_open -> ka_open_aead -> note_check.
"""
import ctypes as C
import hashlib

import numpy as np
import pytest

from tests import ka_cases as KC
from tests import ovk_cases as OC

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


def host(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


def same(got, want, what):
    got = host(got)
    assert got.shape == want.shape and got.dtype == np.uint8, (what, got.shape, want.shape)
    if got.ndim == 1:
        got, want = got.reshape(-1, 1), want.reshape(-1, 1)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert not len(bad), "%s: %d of %d rows differ from the restatement, the first is row %d" % (what, len(bad), len(want), bad[0])


# ---------------------------------------------------------------------------------------------------- jj_blake2b
def run_b2b_case(eng, case, n, digest_len, personal, kind, seed=0):
    """kind 0: host arrays, 1: device tensors, 2: sources alternately device and host with a host result, 3: device sources, host `out`"""
    from jubjub_amd.engine import _Rows

    arrays = case.arrays(n, seed)
    prefix = case.prefix()
    want = case.want(arrays, n, digest_len, personal, prefix)
    placed = [cuda(a) if kind in (1, 3) or (kind == 2 and k % 2 == 0) else a for k, a in enumerate(arrays)]
    views = case.views(placed)
    for v, (a, _, _) in zip(views, case.parts):                    # the views are read where they are: no copy stands in for the stride
        assert n <= 1 or _Rows(v).stride == case.strides[a], case.name
    out = None
    if kind in (2, 3) or (kind == 0 and not views):                # without a source the row count is `out`'s
        out = np.full((n, digest_len), 0xEE, np.uint8)
    elif not views:
        out = cuda(np.full((n, digest_len), 0xEE, np.uint8))
    got = eng.blake2b(views, personal, prefix, digest_len, out=out)
    what = "%s, digest %d, n %d, kind %d" % (case.name, digest_len, n, kind)
    assert (got is out) if out is not None else (hasattr(got, "is_cuda") and got.is_cuda) == (kind == 1), what
    same(got, want, what)
    for p, a in zip(placed, arrays):
        assert np.array_equal(host(p), a), what                    # inputs as they were


def test_blake2b_every_case_digest_length_and_size(eng):
    personals = list(OC.PERSONALS.values())
    sizes, calls, seen = [n for n in OC.SIZES if n], 0, set()
    for k, case in enumerate(OC.B2B_SMALL):
        for digest_len in OC.DIGESTS:
            n = sizes[(k + digest_len // 32) % len(sizes)]
            run_b2b_case(eng, case, n, digest_len, personals[(k + calls) % 3], calls % 4, seed=k)
            seen.add(n)
            calls += 1
    assert seen == set(sizes) and calls == 2 * len(OC.B2B_SMALL)
    for case in OC.B2B_CASES:                                      # the longest prefix and the longest source, at their own row counts
        if case.nrows is not None:
            for digest_len in OC.DIGESTS:
                run_b2b_case(eng, case, case.nrows, digest_len, OC.SAPLING_OCK_PERSONAL, digest_len // 32)


def test_blake2b_ock_shape_at_every_size(eng):
    case = OC.B2B_BY_NAME["ock"]
    for j, n in enumerate(OC.SIZES):
        if n:
            run_b2b_case(eng, case, n, 32, OC.SAPLING_OCK_PERSONAL, j % 4, seed=j)
    got = eng.blake2b([np.zeros((0, 32), np.uint8)] * 3, OC.SAPLING_OCK_PERSONAL, bytes(32))
    assert got.shape == (0, 32)
    # no source: the digest of the prefix alone, one row by default; RFC 7693's "abc" (padded: the prefix is a multiple of 4) stays hashlib's
    assert bytes(eng.blake2b([], None, b"abcd", 64)[0]) == hashlib.blake2b(b"abcd").digest()
    out = cuda(np.zeros((5, 32), np.uint8))
    assert eng.blake2b([], OC.SAPLING_OCK_PERSONAL, b"", 32, out=out) is out
    same(out, OC.digests([], 5, 32, OC.SAPLING_OCK_PERSONAL, b""), "the empty string, five rows")


def test_blake2b_last_row_begins_at_two_to_the_32_minus_stride(eng):
    """four rows at a stride of 2^30 in one device array (a sparse layout, as tests/high_offset_cases.py makes them): n * stride = 2^32, rows 2
    and 3 begin at 2^31 and at 2^32 - stride, where a row offset needs bit 31; two sources in the one array, the second at a skew of 16"""
    import torch

    from tests import high_offset_cases as HC

    stride, n = 1 << 30, 4
    assert n * stride == HC.T32 and (n - 1) * stride == HC.T32 - stride
    try:
        buf = torch.empty((n - 1) * stride + 4096, dtype=torch.uint8, device="cuda")
    except RuntimeError as e:
        pytest.fail("this test needs 3 GiB of device memory: %s" % e)
    assert buf.data_ptr() % 16 == 0
    rows = KC.rng_bytes(7900, n, 112)
    for i in range(n):
        buf[i * stride:i * stride + 112] = cuda(rows[i])
    view = torch.as_strided(buf, (n, 112), (stride, 1))
    prefix = KC.rng_bytes(7901, 32).tobytes()
    for digest_len in OC.DIGESTS:
        got = eng.blake2b([view[:, :64], view[:, 16:112]], OC.SAPLING_OCK_PERSONAL, prefix, digest_len)
        same(got, OC.digests([rows[:, :64], rows[:, 16:112]], n, digest_len, OC.SAPLING_OCK_PERSONAL, prefix), "stride 2^30, digest %d" % digest_len)
    # one row more is one stride too many
    lib, ctx = eng._lib, eng._ctx
    out = torch.full((n + 1, 32), 0xEE, dtype=torch.uint8, device="cuda")
    srcs, lens, strides = (C.c_void_p * 1)(buf.data_ptr()), (C.c_size_t * 1)(64), (C.c_size_t * 1)(stride)
    assert lib.jj_blake2b(ctx, n + 1, 32, None, None, 0, 1, srcs, lens, strides, out.data_ptr()) == -1
    assert lib.jj_ctx_sync(ctx) == 0 and bool((out == 0xEE).all())
    del buf, view


# ---------------------------------------------------------------------------------------------------- jj_ka_kdf_each
def test_ka_kdf_each_every_pair_flag_combination_and_size(eng):
    personals = list(KC.PERSONALS.values())
    seen, calls = set(), 0
    for ci, flags in enumerate(KC.FLAGS):
        for si, n in enumerate(KC.SIZES):
            if (ci + si) % 3 and n not in (0, 1025):               # every flag set at 0 and 1025 rows (all pairs), a third of the other sizes each
                continue
            sks, encs = OC.ka_grid(n, shift=ci + si)
            with_h = bool(flags & KC.KA_HASH_INPUT) and calls % 2 == 0
            h = OC.hash_rows(n, seed=calls) if with_h else None
            personal = personals[(ci + 2 * si) % 3]
            want_keys, want_ok = OC.ka_each(sks, encs, flags, personal, h)
            kind = calls % 4                                       # all host, all device, device scalars + host points, host scalars + device points
            s = cuda(sks) if kind in (1, 2) else sks
            p = cuda(encs) if kind in (1, 3) else encs
            hh = None if h is None else cuda(h) if kind in (1, 2) else h
            keys, ok = eng.ka_kdf_each(s, p, personal, flags, hash_input=hh)
            what = "flags %d, n %d, kind %d, h %s" % (flags, n, kind, with_h)
            assert (hasattr(keys, "is_cuda") and keys.is_cuda) == (kind in (1, 3)) and (hasattr(ok, "is_cuda") and ok.is_cuda) == (kind in (1, 3)), what
            same(keys, want_keys, what + " (keys)")
            same(ok, want_ok, what + " (ok)")
            assert np.array_equal(host(s), sks) and np.array_equal(host(p), encs), what
            seen.add((ci, n))
            calls += 1
    assert {(ci, n) for ci in range(len(KC.FLAGS)) for n in (0, 1025)} <= seen and {n for _, n in seen} == set(KC.SIZES)
    assert 1025 >= OC.GRID                                         # a call of 1025 rows holds every scalar with every point


def test_ka_kdf_each_equals_the_composed_route_and_jj_ka_kdf(eng):
    """jj_decompress, jj_varbase_mul, jj_point_mul_by_cofactor, jj_compress, jj_blake2b on the same inputs; and one scalar repeated is jj_ka_kdf"""
    n = 257
    sks, encs = OC.ka_grid(n, shift=7)
    h = OC.hash_rows(n, seed=3)
    pts, ok = eng.decompress(encs, KC.ZIP216)
    pts = pts.copy()
    pts[ok == 0] = np.frombuffer(bytes(32) + (1).to_bytes(32, "little"), dtype=np.uint8)      # the identity where nothing decoded: any on-curve point
    prod = eng.varbase_mul(sks, pts)
    for cof in (0, KC.KA_COFACTOR):
        share = eng.compress(eng.mul_by_cofactor(prod) if cof else prod)
        for second in (None, encs, h):
            flags = KC.ZIP216 | cof | (0 if second is None else KC.KA_HASH_INPUT)
            composed = eng.blake2b([share] if second is None else [share, second], KC.SAPLING_PERSONAL)
            composed[ok == 0] = 0
            keys, got_ok = eng.ka_kdf_each(sks, encs, KC.SAPLING_PERSONAL, flags, hash_input=h if second is h else None)
            assert np.array_equal(keys, composed) and np.array_equal(got_ok, ok), flags
    assert 0 < int(ok.sum()) < n
    for sk in (KC.SCALARS[3], KC.SCALARS[-1]):
        encs = KC.tiled(n, shift=5)
        rep = np.repeat(np.frombuffer(sk, dtype=np.uint8).reshape(1, 32), n, axis=0)
        for flags in (KC.SAPLING_FLAGS, KC.TORSION_FREE | KC.KA_COFACTOR, KC.NOT_SMALL_ORDER):
            one = eng.ka_kdf(sk, encs, KC.SAPLING_PERSONAL, flags)
            each = eng.ka_kdf_each(cuda(rep), encs, KC.SAPLING_PERSONAL, flags)
            assert np.array_equal(one[0], each[0]) and np.array_equal(one[1], each[1]), flags


def test_ka_kdf_each_across_the_chunk_seam(eng):
    """2^20 + 1 rows: the 1025 restated rows repeated; every row must equal its tile's key on both sides of the seam between two chunks"""
    import torch

    sks, encs = OC.ka_grid(1025, shift=2)
    h = OC.hash_rows(1025, seed=9)
    want_keys, want_ok = OC.ka_each(sks, encs, KC.SAPLING_FLAGS, KC.SAPLING_PERSONAL, h)
    N = (1 << 20) + 1
    idx = torch.arange(N, device="cuda") % 1025
    S, P, H = cuda(sks)[idx].contiguous(), cuda(encs)[idx].contiguous(), cuda(h)[idx].contiguous()
    keys, ok = eng.ka_kdf_each(S, P, KC.SAPLING_PERSONAL, KC.SAPLING_FLAGS, hash_input=H)
    assert keys.is_cuda and tuple(keys.shape) == (N, 32) and tuple(ok.shape) == (N,)
    bad = (keys != cuda(want_keys)[idx]).any(dim=1) | (ok != cuda(want_ok)[idx])
    assert not bool(bad.any()), "%d rows differ, the first is row %d" % (int(bad.sum()), int(bad.nonzero()[0]))
    assert bool((S == cuda(sks)[idx]).all()) and bool((P == cuda(encs)[idx]).all())
    for i in (0, 1024, 1025, (1 << 20) - 1, 1 << 20):              # the strided sample by its own bytes, the seam's two rows among them
        assert bytes(host(keys[i])) == bytes(want_keys[i % 1025]) and int(ok[i]) == int(want_ok[i % 1025]), i


# ---------------------------------------------------------------------------------------------------- refusals
def test_empty_and_invalid_calls(eng):
    import torch

    from jubjub_amd import _lib

    lib, ctx = eng._lib, eng._ctx
    lib.jj_ctx_use_own_stream(ctx)
    INVALID = _lib.JJ_ERR_INVALID
    n = 4
    a = KC.rng_bytes(7950, n + 1, 48)
    out = np.full((n + 1, 64), 0xEE, np.uint8)
    dout = torch.full((n + 1, 64), 0xEE, dtype=torch.uint8, device="cuda")
    dany = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    prefix = bytes(range(32))
    b2b = lib.jj_blake2b
    one = lambda p: (C.c_void_p * 1)(p)                 # noqa: E731
    sz = lambda *v: (C.c_size_t * len(v))(*v)           # noqa: E731
    A, O = a.ctypes.data, out.ctypes.data

    def call(nn=n, digest=32, personal=None, pre=prefix, plen=32, nsrc=1, srcs=one(A), lens=sz(32), strides=sz(48), o=O):
        return b2b(ctx, nn, digest, personal, pre, plen, nsrc, srcs, lens, strides, o)

    assert b2b(ctx, 0, 32, None, None, 0, 0, None, None, None, None) == 0 and call(nn=0) == 0 and call(nn=0, o=None) == 0      # n = 0 succeeds and touches nothing
    assert b2b(None, n, 32, None, prefix, 32, 1, one(A), sz(32), sz(48), O) == INVALID                   # a NULL context
    for digest in (0, 1, 16, 31, 33, 48, 63, 65, 128, -32):
        assert call(digest=digest) == INVALID and call(nn=0, digest=digest) == INVALID, digest
    for plen in (1, 2, 3, 30, 4097, 4100, 1 << 20):
        assert call(pre=bytes(max(plen, 1)), plen=plen) == INVALID, plen
    assert call(pre=None, plen=32) == INVALID and call(nn=0, pre=None, plen=0) == 0                       # a NULL prefix only with length 0
    for nsrc in (-1, 5, 100):
        assert call(nsrc=nsrc) == INVALID, nsrc
    assert call(srcs=None) == INVALID and call(lens=None) == INVALID and call(strides=None) == INVALID
    for length, stride in ((0, 48), (2, 48), (6, 48), (30, 48), (65540, 65540), (1 << 20, 1 << 20), (32, 28), (32, 34), (32, 0), (48, 44)):
        assert call(lens=sz(length), strides=sz(stride)) == INVALID, (length, stride)
        assert call(nn=0, lens=sz(length), strides=sz(stride)) == INVALID, (length, stride)
    assert call(nn=(1 << 24) + 1, lens=sz(4), strides=sz(4)) == INVALID                                   # n > 2^24
    assert call(nn=(1 << 20) + 1, lens=sz(4096), strides=sz(4096)) == INVALID                            # n * stride > 2^32, before anything is read
    assert call(o=None) == INVALID and call(srcs=one(None)) == INVALID                                   # a NULL out or source with n > 0
    assert b2b(ctx, n, 32, None, None, 0, 2, (C.c_void_p * 2)(A, None), sz(32, 32), sz(48, 48), O) == INVALID
    assert call(srcs=one(dany.data_ptr() + 8)) == INVALID and b"16-byte aligned" in lib.jj_last_error(ctx)      # a misaligned device pointer
    assert call(o=dout.data_ptr() + 4) == INVALID and call(srcs=one(dany.data_ptr() + 4), o=dout.data_ptr()) == INVALID
    # srcs, lens, strides, prefix and personal16 are HOST memory
    dtab = torch.zeros(64, dtype=torch.int64, device="cuda")
    dp = C.cast(dtab.data_ptr(), C.POINTER(C.c_void_p))
    ds = C.cast(dtab.data_ptr(), C.POINTER(C.c_size_t))
    assert call(srcs=dp) == INVALID and call(lens=ds) == INVALID and call(strides=ds) == INVALID
    assert call(pre=C.c_void_p(dany.data_ptr())) == INVALID and call(personal=C.c_void_p(dany.data_ptr())) == INVALID
    # out must not overlap a source
    assert call(o=A) == INVALID and b"overlap" in lib.jj_last_error(ctx)
    assert call(o=A + 3 * 48 + 28) == INVALID and call(srcs=one(O + 32 * n - 4)) == INVALID
    assert call(srcs=one(dany.data_ptr()), o=dany.data_ptr() + 48 * 3 + 16) == INVALID
    assert b2b(ctx, n, 64, None, None, 0, 2, (C.c_void_p * 2)(A, O + 64), sz(32, 32), sz(48, 64), O) == INVALID       # the second source lies in out
    # jj_ka_kdf_each
    sks, encs = OC.ka_grid(n, shift=2)
    encs = KC.tiled(n, shift=18)                                                                       # four prime-order points
    h = OC.hash_rows(n)
    keys, ok = np.full((n + 1, 32), 0xEE, np.uint8), np.full(n + 1, 0xEE, np.uint8)
    dkeys = torch.full((n + 1, 32), 0xEE, dtype=torch.uint8, device="cuda")
    dok = torch.full((64,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s, p, hp, k, o = sks.ctypes.data, encs.ctypes.data, h.ctypes.data, keys.ctypes.data, ok.ctypes.data
    each = lib.jj_ka_kdf_each
    HI = KC.KA_HASH_INPUT
    assert each(ctx, 0, None, None, None, 0, None, None, None) == 0 and each(ctx, 0, s, p, hp, KC.SAPLING_FLAGS, KC.SAPLING_PERSONAL, k, o) == 0
    assert each(None, n, s, p, None, 0, None, k, o) == INVALID
    for flags in (KC.CLEAR_COFACTOR, KC.SAPLING_FLAGS | KC.CLEAR_COFACTOR, 16, 128, 1 << 31):
        assert each(ctx, n, s, p, None, flags, None, k, o) == INVALID and each(ctx, 0, s, p, None, flags, None, k, o) == INVALID, flags
    for flags in (0, KC.KA_COFACTOR, KC.ZIP216):                                                       # h32 without JJ_KA_HASH_INPUT
        assert each(ctx, n, s, p, hp, flags, None, k, o) == INVALID and each(ctx, 0, s, p, hp, flags, None, k, o) == INVALID, flags
    for a4 in ((None, p, k, o), (s, None, k, o), (s, p, None, o), (s, p, k, None)):
        assert each(ctx, n, a4[0], a4[1], None, HI, None, a4[2], a4[3]) == INVALID
    for j in range(5):                                                                                 # a misaligned device pointer, in every place
        a5 = [s, p, hp, k, o]
        a5[j] = dany.data_ptr() + 8
        assert each(ctx, n, a5[0], a5[1], a5[2], HI, None, a5[3], a5[4]) == INVALID, j
        assert b"16-byte aligned" in lib.jj_last_error(ctx)
    assert each(ctx, n, s, p, None, 0, None, dkeys.data_ptr() + 4, dok.data_ptr()) == INVALID
    assert lib.jj_ctx_sync(ctx) == 0
    assert (out == 0xEE).all() and (keys == 0xEE).all() and (ok == 0xEE).all()                         # the outputs untouched by every refused call
    assert bool((dout == 0xEE).all()) and bool((dkeys == 0xEE).all()) and bool((dok == 0xEE).all())
    assert np.array_equal(a, KC.rng_bytes(7950, n + 1, 48)) and np.array_equal(encs, KC.tiled(n, shift=18))
    # the context is as good as before, and writes no row beyond n
    assert call() == 0 and each(ctx, n, s, p, hp, KC.SAPLING_FLAGS, KC.SAPLING_PERSONAL, k, o) == 0
    flat = out.reshape(-1)                                                                             # n x 32 bytes, dense, at the array's start
    same(flat[:32 * n].reshape(n, 32), OC.digests([a[:n, :32]], n, 32, None, prefix), "after the refused calls")
    assert (flat[32 * n:] == 0xEE).all()
    want_keys, want_ok = OC.ka_each(sks, encs, KC.SAPLING_FLAGS, KC.SAPLING_PERSONAL, h)
    same(keys[:n], want_keys, "ka_kdf_each after the refused calls")
    assert (ok[:n] == want_ok).all() and want_ok.all() and ok[n] == 0xEE and (keys[n] == 0xEE).all()
    with pytest.raises(ValueError):
        eng.blake2b([a[:, :30]])
    with pytest.raises(ValueError):
        eng.blake2b([a[:, :32]], digest_len=48)
    with pytest.raises(ValueError):
        eng.blake2b([a[:, :32]], prefix=b"abc")
    with pytest.raises(ValueError):
        eng.blake2b([a[:, :32]] * 5)
    with pytest.raises(ValueError):
        eng.blake2b([a[:, :32], a[:2, :32]])
    with pytest.raises(ValueError):
        eng.ka_kdf_each(sks[:2], encs)
    with pytest.raises(ValueError):
        eng.ka_kdf_each(sks, encs, flags=KC.ZIP216, hash_input=h)
    # a row stride that is no multiple of 4 is copied, not refused
    odd = KC.rng_bytes(7951, 9, 38)
    same(eng.blake2b([odd[:, 2:34]]), OC.digests([odd[:, 2:34]], 9, 32, None, b""), "a stride of 38")


# ---------------------------------------------------------------------------------------------------- note_encrypt, ovk_open
@pytest.mark.parametrize("where", ["device", "numpy"])
def test_note_encrypt_then_ovk_open_over_the_planted_rows(eng, where):
    from jubjub_amd.engine import KA_SAPLING_FLAGS, SAPLING_KDF_PERSONAL, SAPLING_OCK_PERSONAL

    b = OC.planted_batch()
    put = cuda if where == "device" else (lambda x: np.array(x))
    n = OC.PLANTED_ROWS
    want_epk, want_enc, want_out = OC.note_encrypt(b["esk"], b["gd64"], b["pkd"], b["plain"], b["ovk"], b["cv"], b["cmu"], KC.SAPLING_PERSONAL, OC.SAPLING_OCK_PERSONAL)
    cv, cmu = put(b["cv"]), put(b["cmu"])
    epk, c_enc, c_out = eng.note_encrypt(put(b["esk"]), put(b["gd64"]), put(b["pkd"]), put(b["plain"]), b["ovk"], cv, cmu, SAPLING_KDF_PERSONAL, SAPLING_OCK_PERSONAL)
    assert all((hasattr(x, "is_cuda") and x.is_cuda) == (where == "device") for x in (epk, c_enc, c_out))
    same(epk, want_epk, "epk")
    same(c_enc, want_enc, "c_enc")
    same(c_out, want_out, "c_out")
    t_enc, t_out = OC.tamper(want_enc, want_out)
    want_plain, want_op, want_ok, verdicts = OC.ovk_open(b["ovk"], b["cv"], b["cmu"], want_epk, t_out, t_enc, KC.SAPLING_PERSONAL, OC.SAPLING_OCK_PERSONAL, OC.OPEN_FLAGS)
    assert want_ok.sum() == n - len(OC.PLANT) and sorted(np.nonzero(want_ok == 0)[0]) == sorted(OC.PLANT)
    plain, op, ok = eng.ovk_open(b["ovk"], cv, cmu, epk, put(t_out), put(t_enc), SAPLING_KDF_PERSONAL, SAPLING_OCK_PERSONAL, flags=OC.OPEN_FLAGS)
    assert all((hasattr(x, "is_cuda") and x.is_cuda) == (where == "device") for x in (plain, op, ok))
    same(ok, want_ok, "ovk_open ok")
    same(plain, want_plain, "ovk_open plaintext")
    same(op, want_op, "ovk_open pk_d || esk")
    for i in OC.PLANT:                                             # every row that is not ok is zeros
        assert not host(plain)[i].any() and not host(op)[i].any(), (i, OC.PLANT[i])
    clean = [i for i in range(n) if i not in OC.PLANT]
    assert np.array_equal(host(plain)[clean], b["plain"][clean])
    # another ovk finds nothing, and no second stage runs
    other = np.array(b["ovk"]) ^ 0x80
    p2, o2, k2 = eng.ovk_open(other, cv, cmu, epk, c_out, c_enc, SAPLING_KDF_PERSONAL, SAPLING_OCK_PERSONAL)
    assert not host(k2).any() and not host(p2).any() and not host(o2).any()
    # the recipient: ka_open_aead with the matching ivk opens the same c_enc
    got, rok = eng.ka_open_aead(b["ivk"], epk, c_enc, SAPLING_KDF_PERSONAL, KA_SAPLING_FLAGS)
    assert host(rok)[clean].all() and np.array_equal(host(got)[clean], b["plain"][clean])


def test_recovered_plaintexts_pass_note_check(eng):
    """real notes (tests/test_gpu_commit.py's build_notes: hashlib and the oracle): g_d, pk_d and esk made by the existing calls, sealed by
    note_encrypt -- whose epk must be the oracle's --, recovered by ovk_open, and handed to note_check, which accepts them"""
    from jubjub_amd.engine import SAPLING_KDF_PERSONAL, SAPLING_OCK_PERSONAL
    from tests import commit_cases as CC
    from tests import pedersen_cases as PC
    from tests.test_gpu_commit import EXPAND_PERSONAL, GD_PERSONAL, GD_PREFIX, build_notes

    ivk, plain, cmu, want_epk, want, _ = build_notes()
    rows = np.nonzero((want == 1) & (plain[:, 0] == 2))[0]
    plain, cmu, want_epk = np.ascontiguousarray(plain[rows]), np.ascontiguousarray(cmu[rows]), want_epk[rows]
    n = len(rows)
    assert n >= 80
    gd, gd_ok = eng.group_hash(plain[:, 1:12], GD_PERSONAL, GD_PREFIX)
    assert gd_ok.all()
    pkd = eng.compress(eng.varbase_mul(np.repeat(ivk.reshape(1, 32), n, axis=0), gd))
    esk = eng.sig_challenge(None, None, np.concatenate([plain[:, 20:52], np.full((n, 1), 5, np.uint8)], axis=1), EXPAND_PERSONAL)
    ovk, cv = KC.rng_bytes(7960, 32), KC.rng_bytes(7961, n, 32)
    epk, c_enc, c_out = eng.note_encrypt(esk, gd, pkd, plain, ovk, cv, cmu, SAPLING_KDF_PERSONAL, SAPLING_OCK_PERSONAL)
    same(epk, want_epk, "epk against the oracle's")
    got, op, ok = eng.ovk_open(ovk, cv, cmu, epk, c_out, c_enc, SAPLING_KDF_PERSONAL, SAPLING_OCK_PERSONAL)
    assert ok.all() and np.array_equal(got, plain) and np.array_equal(op[:, :32], pkd) and np.array_equal(op[:, 32:], esk)
    ped = eng.pedersen_table(CC.gens_bytes("four"), 63, 0)
    rt = eng.fixedbase_table(PC.point_bytes(CC.bases()["R"]).copy(), 0)
    try:
        assert eng.note_check(ivk, got, cmu, ped, rt, GD_PERSONAL, GD_PREFIX, EXPAND_PERSONAL, epk=epk).tolist() == [1] * n
    finally:
        ped.close()
        rt.close()
