"""
GPU tests of jj_ka_kdf and jj_chacha20_xor (key agreement with one secret scalar and its KDF, one ChaCha20 key per row: k_varbase_mont_ka,
k_ka_kdf, k_chacha20_xor; Engine.ka_kdf, Engine.chacha20_xor, Engine.ka_open).  Every check demands byte equality with the restatement of
tests/ka_cases.py -- oracle.jubjub_ref's decoder, integer ladder and to_bytes, hashlib.blake2b(digest_size=32), a pure-Python ChaCha20 pinned
by RFC 8439's block --; no unit is sampled or tolerated.  Every planted scalar with every combination of the decoder bits and the two KA flags,
every size of the list with every such combination (the wave edges, the workgroup edges, the 16 x 64-unit group of k_varbase_mont_x1), on
host arrays, on device tensors and mixed; the composed route through the existing entry points; the seam between two chunks of 2^20 units; the
cipher at every length, stride, counter and nonce of the case list; ka_open; the two buffer-discipline rows through the guarded arenas; every
refused call with the outputs watched; and the neighbours on the same context before and after.
"""
import ctypes as C
import hashlib

import numpy as np
import pytest

from tests import ka_buffer_row as BR
from tests import ka_cases as KC

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
    assert not len(bad), "%s: %d of %d units differ from the restatement, the first is unit %d" % (what, len(bad), len(want), bad[0])


def sk_array(sk):
    return np.frombuffer(sk, dtype=np.uint8).copy()


def test_ka_kdf_every_scalar_flag_combination_and_size(eng):
    personals = list(KC.PERSONALS.values())
    seen_sizes, calls = set(), 0
    for si, sk in enumerate(KC.SCALARS):
        for ci, flags in enumerate(KC.FLAGS):
            n = KC.SIZES[(si + ci) % len(KC.SIZES)]
            personal = personals[(si + 2 * ci) % len(personals)]
            encs = KC.tiled(n, shift=3 * si + ci)
            want_keys, want_ok = KC.expected(sk, encs, flags, personal)
            kind = calls % 4                                   # all host (bytes scalar), all device, host scalar + device points, device scalar + host points
            s = sk if kind == 0 else cuda(sk_array(sk)) if kind in (1, 3) else sk_array(sk)
            p = cuda(encs) if kind in (1, 2) else encs
            keys, ok = eng.ka_kdf(s, p, personal, flags)
            what = "scalar %d, flags %d, n %d, kind %d" % (si, flags, n, kind)
            assert (hasattr(keys, "is_cuda") and keys.is_cuda) == (kind in (1, 2)) and (hasattr(ok, "is_cuda") and ok.is_cuda) == (kind in (1, 2)), what
            same(keys, want_keys, what + " (keys)")
            same(ok, want_ok, what + " (ok)")
            if kind in (1, 2):
                assert np.array_equal(host(p), encs), what                       # inputs as they were
            seen_sizes.add((ci, n))
            calls += 1
    assert seen_sizes == {(ci, n) for ci in range(len(KC.FLAGS)) for n in KC.SIZES}      # every flag combination at every size
    assert calls == len(KC.SCALARS) * len(KC.FLAGS)


def test_ka_kdf_equals_the_composed_route(eng):
    """jj_decompress, jj_varbase_mul with the scalar repeated, jj_point_mul_by_cofactor, jj_compress, then hashlib -- on the same inputs"""
    n = 257
    sk, encs = KC.SCALARS[-1], KC.tiled(n, shift=5)
    pts, ok = eng.decompress(encs, KC.ZIP216)
    pts = pts.copy()
    pts[ok == 0] = np.frombuffer(bytes(32) + (1).to_bytes(32, "little"), dtype=np.uint8)      # the identity where nothing decoded: any on-curve point
    prod = eng.varbase_mul(np.repeat(sk_array(sk).reshape(1, 32), n, axis=0), pts)
    for cof in (0, KC.KA_COFACTOR):
        share = eng.compress(eng.mul_by_cofactor(prod) if cof else prod)
        for inp in (0, KC.KA_HASH_INPUT):
            want = np.zeros((n, 32), np.uint8)
            for i in range(n):
                if ok[i]:
                    want[i] = np.frombuffer(hashlib.blake2b(bytes(share[i]) + (bytes(encs[i]) if inp else b""), digest_size=32, person=KC.SAPLING_PERSONAL).digest(), dtype=np.uint8)
            keys, got_ok = eng.ka_kdf(sk, encs, KC.SAPLING_PERSONAL, KC.ZIP216 | cof | inp)
            same(keys, want, "composed route, flags %d" % (KC.ZIP216 | cof | inp))
            same(got_ok, ok, "composed route, ok")
    assert 0 < int(ok.sum()) < n


def test_ka_kdf_across_the_chunk_seam(eng):
    """2^20 + 65 units: the 1025 restated units repeated; every row must equal its tile's key on both sides of the seam between two chunks"""
    import torch

    sk, base = KC.SCALARS[-2], KC.tiled(1025)
    want_keys, want_ok = KC.expected(sk, base, KC.SAPLING_FLAGS, KC.SAPLING_PERSONAL)
    N = (1 << 20) + 65
    idx = torch.arange(N, device="cuda") % 1025
    P = cuda(base)[idx].contiguous()
    keys, ok = eng.ka_kdf(sk, P, KC.SAPLING_PERSONAL, KC.SAPLING_FLAGS)
    assert keys.is_cuda and tuple(keys.shape) == (N, 32) and tuple(ok.shape) == (N,)
    bad = (keys != cuda(want_keys)[idx]).any(dim=1) | (ok != cuda(want_ok)[idx])
    assert not bool(bad.any()), "%d units differ, the first is unit %d" % (int(bad.sum()), int(bad.nonzero()[0]))
    assert bool((P == cuda(base)[idx]).all())


def cipher_inputs(n, stride, nkeys, seed):
    pool = KC.rng_bytes(seed, nkeys, 32)
    return np.ascontiguousarray(pool[np.arange(n) % nkeys]), KC.rng_bytes(seed + 1, n, stride)


def test_chacha20_xor_every_length_stride_counter_and_nonce(eng):
    calls = 0
    for li, length in enumerate(KC.CIPHER_LENS):
        for stride in (length, length + 4):
            for counter in KC.CIPHER_COUNTERS:
                for nonce in (None, KC.NONCE):
                    n = KC.SIZES[calls % len(KC.SIZES)]
                    keys, data = cipher_inputs(n, stride, 67 if length <= 128 else 9, 8600 + calls)      # 67 keys: more than a wave, no period a lane count shares
                    want = KC.chacha20_xor(keys, data, length, nonce, counter)
                    kind = calls % 3
                    k = cuda(keys) if kind in (1, 2) else keys
                    d = cuda(data) if kind == 1 else data
                    out = eng.chacha20_xor(k, d, nonce, counter, length)
                    what = "len %d, stride %d, counter %d, nonce %s, n %d, kind %d" % (length, stride, counter, "given" if nonce else "NULL", n, kind)
                    assert (hasattr(out, "is_cuda") and out.is_cuda) == (kind == 1), what
                    same(out, want, what)
                    if kind == 1:
                        assert np.array_equal(host(d), data) and np.array_equal(host(k), keys), what
                    calls += 1
    assert calls == 96
    # the RFC's own block through the device: key 00..1f, its nonce, counter 1, a row of zeros
    out = eng.chacha20_xor(np.arange(32, dtype=np.uint8).reshape(1, 32), np.zeros((1, 64), np.uint8), KC.NONCE, 1)
    assert out[0].tobytes().hex() == ("10f1e7e4d13b5915500fdd1fa32071c4c7d1f4c733c068030422aa9ac3d46c4ed2826446079faa0914c2d705d98b02a2"
                                      "b5129cd1de164eb9cbd083e8a2503c4e")


@pytest.mark.parametrize("where", ["device", "numpy"])
def test_ka_open_equals_the_two_calls_and_recovers_planted_plaintext(eng, where):
    from jubjub_amd.engine import KA_SAPLING_FLAGS, SAPLING_KDF_PERSONAL

    n, length = 257, 52
    sk, encs = KC.SCALARS[-1], KC.tiled(n, shift=11)
    want_keys, want_ok = KC.expected(sk, encs, KC.SAPLING_FLAGS, KC.SAPLING_PERSONAL)
    plain = KC.rng_bytes(8800, n, length)
    ct = KC.chacha20_xor(want_keys, plain, length, None, 1)                       # what a sender with these keys would have written
    put = cuda if where == "device" else (lambda x: x)
    P, c = put(encs), put(ct)
    got, ok = eng.ka_open(sk, P, c, SAPLING_KDF_PERSONAL, KA_SAPLING_FLAGS)
    assert (hasattr(got, "is_cuda") and got.is_cuda) == (where == "device")
    same(ok, want_ok, "ka_open ok")
    same(got, plain, "ka_open plaintext")                                         # (a row that did not decode has the zero key on both sides)
    keys, ok2 = eng.ka_kdf(sk, P, SAPLING_KDF_PERSONAL, KA_SAPLING_FLAGS)
    two = eng.chacha20_xor(keys, c, None, 1, length)
    assert np.array_equal(host(two), host(got)) and np.array_equal(host(ok2), host(ok))
    # another wallet's key opens only the rows whose share does not depend on the key: the small-order points, whose [8]([sk]P) is the identity
    other_keys, _ = KC.expected(KC.SCALARS[-2], encs, KC.SAPLING_FLAGS, KC.SAPLING_PERSONAL)
    other, _ = eng.ka_open(KC.SCALARS[-2], P, c, SAPLING_KDF_PERSONAL, KA_SAPLING_FLAGS)
    same(other, KC.chacha20_xor(other_keys, ct, length, None, 1), "ka_open with another key")
    differ = (other_keys != want_keys).any(axis=1)
    assert differ.sum() >= n // 4 and not (host(other)[differ] == plain[differ]).all(axis=1).any()


def test_buffer_discipline_rows():
    """the rows of tests/ka_buffer_row.py through the runner of tests/test_gpu_buffers.py (its Env, checked_call, placements and skews): every
    size of the table x every skew (0, 16, 496 and the mixed one) in one device arena, the host arenas and the mixed placements at the host
    sizes, n = 0: return code 0, the output bytes equal to the restatement, guards and inputs untouched -- the four bytes between two cipher
    rows among them"""
    import test_gpu_buffers as TB

    env = TB.Env()
    try:
        for case in (BR.ROW_KDF, BR.ROW_CIPHER):
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
    sk, encs = sk_array(KC.SCALARS[-1]), KC.tiled(n, shift=18)                     # four prime-order points
    keys = np.full((n + 1, 32), 0xEE, np.uint8)
    ok = np.full(n + 1, 0xEE, np.uint8)
    dkeys = torch.full((n + 1, 32), 0xEE, dtype=torch.uint8, device="cuda")
    dok = torch.full((64,), 0xEE, dtype=torch.uint8, device="cuda")
    dany = torch.zeros(256, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s, p, k, o = sk.ctypes.data, encs.ctypes.data, keys.ctypes.data, ok.ctypes.data
    kdf = lib.jj_ka_kdf
    assert kdf(ctx, 0, None, None, 0, None, None, None) == 0                                          # n = 0 succeeds with NULL arrays
    assert kdf(ctx, 0, s, p, KC.SAPLING_FLAGS, KC.SAPLING_PERSONAL, k, o) == 0 and kdf(ctx, 0, s, p, 0, None, dkeys.data_ptr(), dok.data_ptr()) == 0
    assert kdf(None, n, s, p, 0, None, k, o) == INVALID                                               # a NULL context
    for flags in (KC.CLEAR_COFACTOR, KC.SAPLING_FLAGS | KC.CLEAR_COFACTOR, 16, 128, 1 << 31):          # the cofactor-clearing decoder bit and unknown bits
        assert kdf(ctx, n, s, p, flags, None, k, o) == INVALID, flags
        assert kdf(ctx, 0, s, p, flags, None, k, o) == INVALID, flags
    for a in ((None, p, k, o), (s, None, k, o), (s, p, None, o), (s, p, k, None)):                    # a NULL array with n > 0
        assert kdf(ctx, n, a[0], a[1], 0, None, a[2], a[3]) == INVALID
    for j in range(4):                                                                                # a misaligned device pointer, in every place
        a = [s, p, k, o]
        a[j] = dany.data_ptr() + 8
        assert kdf(ctx, n, a[0], a[1], 0, None, a[2], a[3]) == INVALID, j
        assert b"16-byte aligned" in lib.jj_last_error(ctx)
    assert kdf(ctx, n, s, p, 0, None, dkeys.data_ptr() + 4, dok.data_ptr()) == INVALID and kdf(ctx, n, s, p, 0, None, dkeys.data_ptr(), dok.data_ptr() + 1) == INVALID
    # the cipher
    data = KC.rng_bytes(8900, n, 56)
    out = np.full((n + 1, 52), 0xEE, np.uint8)
    dout = torch.full((n + 1, 52), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    kk, d, oo = encs.ctypes.data, data.ctypes.data, out.ctypes.data
    xor = lib.jj_chacha20_xor
    assert xor(ctx, 0, None, None, 0, None, 52, 52, None) == 0 and xor(ctx, 0, kk, None, 1, d, 52, 56, oo) == 0
    assert xor(None, n, kk, None, 1, d, 52, 56, oo) == INVALID
    for length, stride in ((0, 56), (2, 56), (6, 56), (50, 56), (1028, 1028), (2048, 2048), (52, 48), (52, 54), (52, 0)):      # len and in_stride
        assert xor(ctx, n, kk, None, 1, d, length, stride, oo) == INVALID, (length, stride)
        assert xor(ctx, 0, kk, None, 1, d, length, stride, oo) == INVALID, (length, stride)
    assert xor(ctx, (1 << 30) + 1, kk, None, 1, d, 4, 4, oo) == INVALID                               # n * in_stride > 2^32, before anything is read
    assert xor(ctx, (1 << 22) + 1, kk, None, 1, d, 1024, 1024, oo) == INVALID
    for a in ((None, d, oo), (kk, None, oo), (kk, d, None)):
        assert xor(ctx, n, a[0], None, 1, a[1], 52, 56, a[2]) == INVALID
    assert xor(ctx, n, kk, None, 1, d, 52, 56, d) == INVALID and xor(ctx, n, kk, None, 1, d, 52, 56, d + 4 * 56 - 8) == INVALID      # in and out overlap
    assert b"overlap" in lib.jj_last_error(ctx)
    assert xor(ctx, n, kk, None, 1, oo + 52, 52, 52, oo) == INVALID
    for j in range(3):
        a = [kk, d, oo]
        a[j] = dany.data_ptr() + 8
        assert xor(ctx, n, a[0], None, 1, a[1], 52, 56, a[2]) == INVALID, j
    assert xor(ctx, n, kk, None, 1, d, 52, 56, dout.data_ptr() + 4) == INVALID
    assert lib.jj_ctx_sync(ctx) == 0
    assert (keys == 0xEE).all() and (ok == 0xEE).all() and (out == 0xEE).all()                        # the outputs untouched by every refused call
    assert bool((dkeys == 0xEE).all()) and bool((dok == 0xEE).all()) and bool((dout == 0xEE).all())
    assert np.array_equal(encs, KC.tiled(n, shift=18)) and np.array_equal(data, KC.rng_bytes(8900, n, 56))
    # the context is as good as before
    assert kdf(ctx, n, s, p, KC.SAPLING_FLAGS, KC.SAPLING_PERSONAL, k, o) == 0
    want_keys, want_ok = KC.expected(KC.SCALARS[-1], encs, KC.SAPLING_FLAGS, KC.SAPLING_PERSONAL)
    same(keys[:n], want_keys, "after the refused calls")
    assert (ok[:n] == want_ok).all() and ok[n] == 0xEE and (keys[n] == 0xEE).all() and want_ok.all()
    assert xor(ctx, n, k, None, 1, d, 52, 56, oo) == 0
    same(out[:n], KC.chacha20_xor(want_keys, data, 52, None, 1), "cipher after the refused calls")
    assert (out[n] == 0xEE).all()
    with pytest.raises(ValueError):
        eng.ka_kdf(KC.SCALARS[0], encs, b"short")
    with pytest.raises(ValueError):
        eng.ka_kdf(KC.SCALARS[0] * 2, encs)
    with pytest.raises(ValueError):
        eng.chacha20_xor(encs, data, length=50)
    with pytest.raises(ValueError):
        eng.chacha20_xor(encs[:2], data)


def test_neighbours_on_the_same_context_are_unchanged(eng):
    """a jj_sig_challenge and a jj_fixedbase_mul call before and after the new calls give the same bytes, and those are the oracle's"""
    from oracle import c_oracle as O
    from oracle import jubjub_ref as J
    from tests import sig_challenge_cases as CC

    n = 65
    R, A = CC.parts(n, "both", seed=4)
    msgs = CC.fixed(n, 33, seed=4)
    scalars = KC.rng_bytes(8950, n, 32)
    base = np.frombuffer(J.GENERATOR[0].to_bytes(32, "little") + J.GENERATOR[1].to_bytes(32, "little"), dtype=np.uint8)
    tab = eng.fixedbase_table(base)
    try:
        before = (eng.sig_challenge(R, A, msgs, CC.REDJUBJUB).copy(), eng.fixedbase_mul(tab, scalars).copy())
        encs = KC.tiled(1025)
        keys, ok = eng.ka_kdf(KC.SCALARS[-1], encs, KC.SAPLING_PERSONAL, KC.SAPLING_FLAGS)
        eng.chacha20_xor(keys, KC.rng_bytes(8960, 1025, 564), None, 1)
        dkeys, _ = eng.ka_kdf(cuda(sk_array(KC.SCALARS[3])), cuda(encs), None, KC.TORSION_FREE | KC.NOT_SMALL_ORDER)
        eng.chacha20_xor(dkeys, cuda(KC.rng_bytes(8961, 1025, 56)), KC.NONCE, 0, 52)
        after = (eng.sig_challenge(R, A, msgs, CC.REDJUBJUB), eng.fixedbase_mul(tab, scalars))
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        same(after[0], CC.expected(CC.REDJUBJUB, R, A, [bytes(m) for m in msgs]), "sig_challenge after ka_kdf")
        same(after[1], O.fixedbase_mul(scalars, base), "fixedbase_mul after ka_kdf")
    finally:
        tab.close()
