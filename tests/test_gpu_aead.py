"""
GPU tests of jj_poly1305, jj_aead_seal and jj_aead_open (k_poly1305, k_aead<true>, k_aead<false>; Engine.poly1305, Engine.aead_seal,
Engine.aead_open, Engine.ka_open_aead).  Every check demands byte equality with the restatement of tests/aead_cases.py -- Poly1305 on Python
integers and the RFC 8439 AEAD on tests/ka_cases.py's ChaCha20, pinned by the RFC's vectors and against libcrypto --; no row is sampled or
tolerated.  The planted accumulator cases; every length, stride and aad length of the case lists at sizes that cycle through the wave edges,
the workgroup edges and the tail block of the grid; host arrays, device tensors and mixed; tampered rows among valid neighbours (both verdicts,
zero rows, neighbours untouched); another nonce and another aad across whole calls; ka_open_aead against the two calls made separately; the
three buffer-discipline rows through the guarded arenas; every refused call with the outputs watched; and jj_chacha20_xor and jj_ka_kdf on
the same context before and after.
"""
import ctypes as C

import numpy as np
import pytest

from tests import aead_buffer_row as BR
from tests import aead_cases as AC
from tests import ka_cases as KC

pytestmark = pytest.mark.gpu
AAD64 = KC.rng_bytes(14000, 64).tobytes()


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


def is_dev(v):
    return bool(hasattr(v, "is_cuda") and v.is_cuda)


def same(got, want, what):
    got = host(got)
    assert got.shape == want.shape and got.dtype == np.uint8, (what, got.shape, want.shape)
    if got.ndim == 1:
        got, want = got.reshape(-1, 1), want.reshape(-1, 1)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert not len(bad), "%s: %d of %d rows differ from the restatement, the first is row %d" % (what, len(bad), len(want), bad[0])


def nkeys_for(length):
    return 67 if length <= 128 else 9          # 67 keys: more than a wave, no period a lane count shares; fewer where a key's stream is long


def test_poly1305_planted_cases(eng):
    """every planted key and message, each alone (n = 1) and all rows of one length together, on host and device arrays"""
    cases = AC.planted()
    by_len = {}
    for name, key, msg, tag in cases:
        by_len.setdefault(len(msg), []).append((name, key, msg, tag))
    assert len(by_len) >= 10
    for length, group in by_len.items():
        keys = np.frombuffer(b"".join(g[1] for g in group), np.uint8).reshape(-1, 32)
        rows = np.frombuffer(b"".join(g[2] for g in group), np.uint8).reshape(-1, length)
        want = np.frombuffer(b"".join(g[3] for g in group), np.uint8).reshape(-1, 16)
        for put in (lambda x: x, cuda):
            got = eng.poly1305(put(keys), put(rows))
            for j, g in enumerate(group):
                assert host(got)[j].tobytes() == g[3], (g[0], host(got)[j].tobytes().hex(), g[3].hex())
        for j, g in enumerate(group):
            assert eng.poly1305(keys[j:j + 1], rows[j:j + 1])[0].tobytes() == g[3], g[0]
        same(eng.poly1305(keys, rows), want, "planted, len %d" % length)


def test_poly1305_every_length_stride_and_size(eng):
    calls, sizes = 0, set()
    for length in AC.MAC_LENS:
        for stride in (length, length + 4, length + 28):
            n = AC.SIZES[calls % len(AC.SIZES)]
            keys, data = AC.pool_keys(n, 67, 14100 + calls), KC.rng_bytes(14200 + calls, n, stride)
            want = AC.mac_rows(keys, data, length)
            kind = calls % 3
            k = cuda(keys) if kind in (1, 2) else keys
            d = cuda(data) if kind == 1 else data
            got = eng.poly1305(k, d, length)
            what = "len %d, stride %d, n %d, kind %d" % (length, stride, n, kind)
            assert is_dev(got) == (kind == 1) and tuple(got.shape) == (n, 16), what
            same(got, want, what)
            if kind == 1:
                assert np.array_equal(host(d), data) and np.array_equal(host(k), keys), what
            sizes.add(n)
            calls += 1
    assert calls == 30 and sizes == set(AC.SIZES)


@pytest.fixture(scope="module")
def sealed_cases():
    """[(length, aad, nonce, n, keys, plain, sealed)]: every length with every aad length, the nonce alternating, sizes cycling; the restatement's
    ciphertexts, made once and shared by the seal and the open test"""
    out, calls = [], 0
    for length in AC.SEAL_LENS:
        for aad_len in AC.AAD_LENS:
            n = AC.SIZES[calls % len(AC.SIZES)]
            if length > 128 and n > 257:
                n = 257 if calls % 2 else 65                                   # the restatement's Poly1305 is per row: long rows at fewer of them
            nonce = None if calls % 2 else AC.NONCE
            aad = AAD64[:aad_len]
            keys, plain = AC.pool_keys(n, nkeys_for(length), 14300 + calls), KC.rng_bytes(14400 + calls, n, length + 4 * (calls % 3))
            out.append((length, aad, nonce, n, keys, plain, AC.seal_rows(keys, plain, length, nonce, aad)))
            calls += 1
    assert calls == 77 and {c[3] for c in out} == set(AC.SIZES) and {c[2] for c in out} == {None, AC.NONCE}
    return out


def test_aead_seal_every_length_aad_and_nonce(eng, sealed_cases):
    for j, (length, aad, nonce, n, keys, plain, sealed) in enumerate(sealed_cases):
        kind = j % 3
        k = cuda(keys) if kind in (1, 2) else keys
        d = cuda(plain) if kind == 1 else plain
        got = eng.aead_seal(k, d, nonce, aad, length)
        what = "seal: len %d, stride %d, aad %d, nonce %s, n %d, kind %d" % (length, plain.shape[1], len(aad), "given" if nonce else "NULL", n, kind)
        assert is_dev(got) == (kind == 1) and tuple(got.shape) == (n, length + 16), what
        same(got, sealed, what)
        if kind == 1:
            assert np.array_equal(host(d), plain), what


def test_aead_open_valid_and_tampered_rows(eng, sealed_cases):
    """the restatement's ciphertexts at strides len + 16, len + 20 and len + 44: every valid row opens to its plaintext with ok = 1; with the
    tamper list applied to every third row, each tampered row gives ok = 0 and a zero row and every other row is as before"""
    seen = set()
    for j, (length, aad, nonce, n, keys, plain, sealed) in enumerate(sealed_cases):
        stride = length + (16, 20, 44)[j % 3]
        rows = KC.rng_bytes(14500 + j, n, stride)
        rows[:, :length + 16] = sealed
        kind = (j // 3) % 3
        put_k = cuda if kind in (1, 2) else (lambda x: x)
        put_d = cuda if kind == 1 else (lambda x: x)
        what = "open: len %d, stride %d, aad %d, n %d, kind %d" % (length, stride, len(aad), n, kind)
        got, ok = eng.aead_open(put_k(keys), put_d(rows), nonce, aad, length)
        assert is_dev(got) == (kind == 1) and is_dev(ok) == (kind == 1) and tuple(got.shape) == (n, length) and tuple(ok.shape) == (n,), what
        same(got, plain[:, :length], what)
        same(ok, np.ones(n, np.uint8), what + " (ok)")
        victims = list(range(j % 3, n, 3))
        tk, tr, names = AC.tamper(keys, rows, length, victims)
        got, ok = eng.aead_open(put_k(tk), put_d(tr), nonce, aad, length)
        got, ok = host(got), host(ok)
        for i in range(n):
            if i in names:
                assert ok[i] == 0 and not got[i].any(), (what, i, names[i])
                seen.add(names[i])
            else:
                assert ok[i] == 1 and np.array_equal(got[i], plain[i, :length]), (what, i)
        want_plain, want_ok = AC.open_rows(tk, tr, length, nonce, aad) if length <= 128 else (None, None)
        if want_ok is not None:
            same(got, want_plain, what + " (restated)")
            same(ok, want_ok, what + " (restated ok)")
    assert seen == {name for name, _ in AC.tamper_list(64)}


def test_aead_open_another_nonce_and_another_aad_fail_every_row(eng, sealed_cases):
    for j in (3, 18, 40, 76):
        length, aad, nonce, n, keys, plain, sealed = sealed_cases[j]
        other_nonce = bytes(11) + b"\x01" if nonce is None else None
        for nc, ad in ((other_nonce, aad), (nonce, aad + b"\x00" if len(aad) < 64 else aad[:-1]), (nonce, bytes(len(aad)) if any(aad) else b"\x01")):
            got, ok = eng.aead_open(keys, sealed, nc, ad, length)
            assert not ok.any() and not got.any(), (j, nc, len(ad))
        got, ok = eng.aead_open(cuda(keys), cuda(sealed), nonce, aad, length)
        assert bool(ok.all()) and np.array_equal(host(got), plain[:, :length])


@pytest.mark.parametrize("where", ["device", "numpy"])
def test_ka_open_aead_equals_the_two_calls(eng, where):
    from jubjub_amd.engine import KA_SAPLING_FLAGS, SAPLING_KDF_PERSONAL

    n, length = 257, 52
    sk, encs = KC.SCALARS[-1], KC.tiled(n, shift=11)
    want_keys, want_ok = KC.expected(sk, encs, KC.SAPLING_FLAGS, KC.SAPLING_PERSONAL)
    assert 0 < int(want_ok.sum()) < n                                            # points that do not decode among them
    plain = KC.rng_bytes(14600, n, length)
    rows = AC.seal_rows(want_keys, plain, length, None, b"")                      # a sender with these keys; the zero key where nothing decoded
    rows[5::7, length + 3] ^= 0x40                                               # some tags broken
    put = cuda if where == "device" else (lambda x: x)
    P, c = put(encs), put(rows)
    got, ok = eng.ka_open_aead(sk, P, c, SAPLING_KDF_PERSONAL, KA_SAPLING_FLAGS)
    assert is_dev(got) == (where == "device") and is_dev(ok) == (where == "device")
    tag_ok = np.ones(n, np.uint8)
    tag_ok[5::7] = 0
    want = plain * (want_ok & tag_ok)[:, None]
    same(ok, want_ok & tag_ok, "ka_open_aead ok")
    same(got, want, "ka_open_aead plaintext")                                     # rows whose P did not decode are zero rows, sealed under the zero key or not
    keys, ok1 = eng.ka_kdf(sk, P, SAPLING_KDF_PERSONAL, KA_SAPLING_FLAGS)
    two, ok2 = eng.aead_open(keys, c, None, b"", length)
    assert np.array_equal(host(ok1) & host(ok2), host(ok))
    assert np.array_equal(host(two) * host(ok1)[:, None], host(got))
    # another wallet's key: only the rows whose share does not depend on the key verify
    other_keys, other_ok = KC.expected(KC.SCALARS[-2], encs, KC.SAPLING_FLAGS, KC.SAPLING_PERSONAL)
    got2, ok2 = eng.ka_open_aead(KC.SCALARS[-2], P, c, SAPLING_KDF_PERSONAL, KA_SAPLING_FLAGS)
    same_key = (other_keys == want_keys).all(axis=1)
    same(ok2, want_ok & tag_ok & same_key.astype(np.uint8), "ka_open_aead with another key")
    assert not host(got2)[~same_key].any() and (~same_key).sum() >= n // 4


def test_buffer_discipline_rows():
    """the rows of tests/aead_buffer_row.py through the runner of tests/test_gpu_buffers.py (its Env, checked_call, placements and skews): every
    size of the table x every skew in one device arena, the host arenas and the mixed placements at the host sizes, n = 0: return code 0, the
    output bytes equal to the restatement -- both verdicts and the zero rows among them --, guards and inputs untouched, the bytes between two
    rows included"""
    import test_gpu_buffers as TB

    env = TB.Env()
    try:
        for case in (BR.ROW_MAC, BR.ROW_SEAL, BR.ROW_OPEN):
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


def test_empty_and_invalid_calls(eng):
    import torch

    from jubjub_amd import _lib

    lib, ctx = eng._lib, eng._ctx
    lib.jj_ctx_use_own_stream(ctx)
    INVALID = _lib.JJ_ERR_INVALID
    n = 4
    keys = KC.rng_bytes(14700, n, 32)
    data = KC.rng_bytes(14701, n, 72)
    aad = b"0123456789ab"
    out = np.full((n + 1, 68), 0xEE, np.uint8)
    ok = np.full(16, 0xEE, np.uint8)
    tag = np.full((n + 1, 16), 0xEE, np.uint8)
    dout = torch.full((n + 1, 68), 0xEE, dtype=torch.uint8, device="cuda")
    dok = torch.full((64,), 0xEE, dtype=torch.uint8, device="cuda")
    dany = torch.zeros(512, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    k, d, o, v, t = keys.ctypes.data, data.ctypes.data, out.ctypes.data, ok.ctypes.data, tag.ctypes.data
    mac = lambda cx, nn, kk, ii, ln, st, tt: lib.jj_poly1305(cx, C.c_size_t(nn), C.c_void_p(kk), C.c_void_p(ii), C.c_size_t(ln), C.c_size_t(st), C.c_void_p(tt))      # noqa: E731
    opn = lambda cx, nn, kk, nc, ad, al, ii, ln, st, oo, vv: lib.jj_aead_open(cx, C.c_size_t(nn), C.c_void_p(kk), nc, ad, C.c_size_t(al), C.c_void_p(ii), C.c_size_t(ln),      # noqa: E731
                                                                             C.c_size_t(st), C.c_void_p(oo), C.c_void_p(vv))
    seal = lambda cx, nn, kk, nc, ad, al, ii, ln, st, oo: lib.jj_aead_seal(cx, C.c_size_t(nn), C.c_void_p(kk), nc, ad, C.c_size_t(al), C.c_void_p(ii), C.c_size_t(ln),      # noqa: E731
                                                                          C.c_size_t(st), C.c_void_p(oo))
    # n = 0 succeeds and touches nothing, with NULL arrays too
    assert mac(ctx, 0, None, None, 52, 56, None) == 0 and mac(ctx, 0, k, d, 52, 72, t) == 0
    assert opn(ctx, 0, None, None, None, 0, None, 52, 68, None, None) == 0 and opn(ctx, 0, k, None, aad, 12, d, 52, 72, o, v) == 0
    assert seal(ctx, 0, None, None, None, 0, None, 52, 52, None) == 0 and seal(ctx, 0, k, None, aad, 12, d, 52, 72, dout.data_ptr()) == 0
    # a NULL context
    assert mac(None, n, k, d, 52, 72, t) == INVALID and opn(None, n, k, None, None, 0, d, 52, 72, o, v) == INVALID and seal(None, n, k, None, None, 0, d, 52, 72, o) == INVALID
    # len and in_stride (with n = 0 as well: the shape is checked first)
    for length, stride in ((0, 72), (2, 72), (6, 72), (50, 72), (1028, 1044), (2048, 2064), (52, 48), (52, 70), (52, 0)):
        for nn in (n, 0):
            assert mac(ctx, nn, k, d, length, stride, t) == INVALID, (length, stride)
            assert opn(ctx, nn, k, None, None, 0, d, length, stride, o, v) == INVALID, (length, stride)
            assert seal(ctx, nn, k, None, None, 0, d, length, stride, o) == INVALID, (length, stride)
    for stride in (52, 56, 64):                                                   # open needs room for the tag: in_stride >= len + 16
        assert opn(ctx, n, k, None, None, 0, d, 52, stride, o, v) == INVALID, stride
        assert seal(ctx, 0, k, None, None, 0, d, 52, stride, o) == 0 and mac(ctx, 0, k, d, 52, stride, t) == 0
    # n * in_stride > 2^32, before anything is read
    assert mac(ctx, (1 << 30) + 1, k, d, 4, 4, t) == INVALID and seal(ctx, (1 << 22) + 1, k, None, None, 0, d, 1024, 1024, o) == INVALID
    assert opn(ctx, (1 << 32) // 20 + 1, k, None, None, 0, d, 4, 20, o, v) == INVALID
    # the aad
    assert opn(ctx, n, k, None, aad, 65, d, 52, 72, o, v) == INVALID and seal(ctx, n, k, None, aad, 65, d, 52, 72, o) == INVALID
    assert opn(ctx, n, k, None, None, 1, d, 52, 72, o, v) == INVALID and seal(ctx, n, k, None, None, 12, d, 52, 72, o) == INVALID
    assert opn(ctx, 0, k, None, None, 1, d, 52, 72, o, v) == INVALID
    # a NULL array with n > 0
    for a in ((None, d, t), (k, None, t), (k, d, None)):
        assert mac(ctx, n, a[0], a[1], 52, 72, a[2]) == INVALID
        assert seal(ctx, n, a[0], None, None, 0, a[1], 52, 72, o if a[2] else None) == INVALID
        assert opn(ctx, n, a[0], None, None, 0, a[1], 52, 72, o if a[2] else None, v) == INVALID
    assert opn(ctx, n, k, None, None, 0, d, 52, 72, o, None) == INVALID
    # in and out overlap
    assert seal(ctx, n, k, None, None, 0, d, 52, 72, d) == INVALID and b"overlap" in lib.jj_last_error(ctx)
    assert opn(ctx, n, k, None, None, 0, d, 52, 72, d + 4 * 72 - 8, v) == INVALID and b"overlap" in lib.jj_last_error(ctx)
    assert opn(ctx, n, k, None, None, 0, o + 52, 52, 68, o, v) == INVALID
    assert mac(ctx, n, k, d, 52, 72, d + 64) == INVALID and b"overlap" in lib.jj_last_error(ctx)
    # a misaligned device pointer, in every place
    for j in range(3):
        a = [k, d, t]
        a[j] = dany.data_ptr() + 8
        assert mac(ctx, n, a[0], a[1], 52, 72, a[2]) == INVALID, j
        assert b"16-byte aligned" in lib.jj_last_error(ctx)
    for j in range(4):
        a = [k, d, o, v]
        a[j] = dany.data_ptr() + 8
        assert opn(ctx, n, a[0], None, None, 0, a[1], 52, 72, a[2], a[3]) == INVALID, j
        if j < 3:
            assert seal(ctx, n, a[0], None, None, 0, a[1], 52, 72, a[2]) == INVALID, j
    assert seal(ctx, n, k, None, None, 0, d, 52, 72, dout.data_ptr() + 4) == INVALID and opn(ctx, n, k, None, None, 0, d, 52, 72, dout.data_ptr(), dok.data_ptr() + 1) == INVALID
    assert lib.jj_ctx_sync(ctx) == 0
    assert (out == 0xEE).all() and (ok == 0xEE).all() and (tag == 0xEE).all()    # the outputs untouched by every refused call
    assert bool((dout == 0xEE).all()) and bool((dok == 0xEE).all())
    assert np.array_equal(keys, KC.rng_bytes(14700, n, 32)) and np.array_equal(data, KC.rng_bytes(14701, n, 72))
    # the context is as good as before
    assert seal(ctx, n, k, None, aad, 12, d, 52, 72, o) == 0
    same(out[:n], AC.seal_rows(keys, data, 52, None, aad), "seal after the refused calls")
    assert (out[n] == 0xEE).all()
    plain = np.full((n + 1, 52), 0xEE, np.uint8)
    assert opn(ctx, n, k, None, aad, 12, o, 52, 68, plain.ctypes.data, v) == 0
    same(plain[:n], data[:, :52], "open after the refused calls")
    assert (ok[:n] == 1).all() and (ok[n:] == 0xEE).all() and (plain[n] == 0xEE).all()
    assert mac(ctx, n, k, d, 52, 72, t) == 0
    same(tag[:n], AC.mac_rows(keys, data, 52), "poly1305 after the refused calls")
    assert (tag[n] == 0xEE).all()
    for bad in (lambda: eng.aead_open(keys, data, length=50), lambda: eng.aead_open(keys, data, length=60), lambda: eng.aead_seal(keys[:2], data),
                lambda: eng.aead_seal(keys, data, aad=bytes(65)), lambda: eng.poly1305(keys, data, length=76), lambda: eng.aead_open(keys, data, nonce=b"short")):
        with pytest.raises(ValueError):
            bad()


def test_neighbours_on_the_same_context_are_unchanged(eng):
    """a jj_chacha20_xor and a jj_ka_kdf call before and after the new calls give the same bytes, and those are the restatement's"""
    n = 65
    keys, data = AC.pool_keys(n, 67, 14800), KC.rng_bytes(14801, n, 56)
    encs = KC.tiled(n, shift=7)
    before = (eng.chacha20_xor(keys, data, KC.NONCE, 1, 52).copy(), [x.copy() for x in eng.ka_kdf(KC.SCALARS[-1], encs, KC.SAPLING_PERSONAL, KC.SAPLING_FLAGS)])
    rows = KC.rng_bytes(14802, 1025, 580)
    eng.aead_open(AC.pool_keys(1025, 9, 14803), rows, None, b"", 564)
    sealed = eng.aead_seal(cuda(AC.pool_keys(1025, 9, 14804)), cuda(rows), AC.NONCE, AAD64[:17], 564)
    eng.aead_open(cuda(AC.pool_keys(1025, 9, 14804)), sealed, AC.NONCE, AAD64[:17])
    eng.poly1305(keys, data, 52)
    after = (eng.chacha20_xor(keys, data, KC.NONCE, 1, 52), eng.ka_kdf(KC.SCALARS[-1], encs, KC.SAPLING_PERSONAL, KC.SAPLING_FLAGS))
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1][0], after[1][0]) and np.array_equal(before[1][1], after[1][1])
    same(after[0], KC.chacha20_xor(keys, data, 52, KC.NONCE, 1), "chacha20_xor after the new calls")
    want_keys, want_ok = KC.expected(KC.SCALARS[-1], encs, KC.SAPLING_FLAGS, KC.SAPLING_PERSONAL)
    same(after[1][0], want_keys, "ka_kdf after the new calls")
    same(after[1][1], want_ok, "ka_kdf ok after the new calls")
