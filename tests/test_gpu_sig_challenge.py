"""
GPU tests of jj_sig_challenge (Schnorr challenges hashed on the device: k_sig_challenge, jj_blake2b.h; Engine.sig_challenge,
Engine.sigverify_each_msgs, Engine.sigbatch_verify_msgs).  Every check demands byte equality with the oracle of tests/sig_challenge_cases.py --
hashlib.blake2b(data, digest_size=64, person=personal), then oracle.jubjub_ref.FR.from_bytes_wide --; no unit is sampled or tolerated.
Fixed stride: every hashed length of the case table in every part combination, at n around a wave and a workgroup, under every
personalisation.  Ragged: one wave holding a three-block message among empty ones, empty messages at both ends, neighbours straddling the
block edges, start offsets of every residue modulo 16, and the same messages reversed.  Every kind of pointer; the entry point's
buffer-discipline row through the guarded arenas; every refused call with the output watched; the compositions on valid and on tampered
signatures, on device tensors and on numpy arrays.

The wide reduction's own edge values (digests at and around multiples of r, the all-ones digest) cannot be planted through a hash: no input with
such a digest is known.  The challenges here exercise Fr::from_words_wide on 512-bit values as the hash gives them; its edge values are held by
the jj_fr_from_bytes_wide tests (tests/test_gpu_field_matrix.py, tests/test_gpu_parity.py), which run the same Fr::from_words_wide.
"""
import ctypes as C

import numpy as np
import pytest

from tests import sig_challenge_buffer_row as BR
from tests import sig_challenge_cases as CC

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
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert not len(bad), "%s: %d of %d units differ from the oracle, the first is unit %d" % (what, len(bad), len(want), bad[0])


@pytest.mark.parametrize("pname", list(CC.PERSONALS))
def test_fixed_stride_every_length_combination_and_size(eng, pname):
    personal = CC.PERSONALS[pname]
    for j, (total, combo, msg_len) in enumerate(CC.CASES):
        for n in CC.SIZES:
            R, A = CC.parts(n, combo, seed=j)
            msgs = CC.fixed(n, msg_len, seed=j)
            want = CC.expected(personal, R, A, [bytes(m) for m in msgs])
            same(eng.sig_challenge(R, A, msgs, personal), want, "total %d (%s, message %d), n %d, personal %s" % (total, combo, msg_len, n, pname))


def test_null_personal_equals_sixteen_zero_bytes(eng):
    R, A = CC.parts(65, "both")
    msgs = CC.fixed(65, 33)
    a, b = eng.sig_challenge(R, A, msgs, None), eng.sig_challenge(R, A, msgs, bytes(16))
    assert np.array_equal(a, b) and not np.array_equal(a, eng.sig_challenge(R, A, msgs, CC.REDJUBJUB))


@pytest.mark.parametrize("combo", CC.COMBOS)
@pytest.mark.parametrize("reverse", [False, True], ids=["planted", "reversed"])
def test_ragged_one_wave_of_everything(eng, combo, reverse):
    msgs = CC.ragged(CC.PREFIX[combo], reverse=reverse)
    n = len(msgs)
    assert n == 300 and CC.start_residues(msgs) == set(range(16)) and len(msgs[0]) == 0 and len(msgs[-1]) == 0
    R, A = CC.parts(n, combo, seed=9)
    want = CC.expected(CC.REDJUBJUB, R, A, msgs)
    flat, offsets = CC.pack(msgs)
    same(eng.sig_challenge(R, A, flat, CC.REDJUBJUB, offsets=offsets), want, "ragged host (%s)" % combo)
    same(eng.sig_challenge(R, A, msgs, CC.REDJUBJUB), want, "ragged list of bytes (%s)" % combo)
    dflat = cuda(flat)
    dev = [None if x is None else cuda(x) for x in (R, A)]
    out = eng.sig_challenge(dev[0], dev[1], dflat, CC.REDJUBJUB, offsets=offsets)
    assert out.is_cuda
    same(out, want, "ragged device (%s)" % combo)
    assert np.array_equal(dflat.cpu().numpy(), flat)


def test_all_messages_empty_and_null_msgs(eng):
    n = 65
    R, A = CC.parts(n, "both")
    want = CC.expected(CC.REDJUBJUB, R, A, [b""] * n)
    same(eng.sig_challenge(R, A, np.zeros((n, 0), np.uint8), CC.REDJUBJUB), want, "msg_len 0")
    same(eng.sig_challenge(R, A, [b""] * n, CC.REDJUBJUB), want, "offsets all zero")
    lib, ctx = eng._lib, eng._ctx
    out = np.zeros((n, 32), np.uint8)
    assert lib.jj_sig_challenge(ctx, n, CC.REDJUBJUB, R.ctypes.data, A.ctypes.data, None, 0, None, out.ctypes.data) == 0
    same(out, want, "NULL msgs with msg_len 0")
    same(eng.sig_challenge(None, None, np.zeros((3, 0), np.uint8)), CC.expected(None, None, None, [b""] * 3), "the empty input")


def test_pointer_kinds(eng):
    import torch

    n, L = 257, 33
    R, A = CC.parts(n, "both", seed=3)
    msgs = CC.fixed(n, L, seed=3)
    want = CC.expected(CC.REDJUBJUB, R, A, [bytes(m) for m in msgs])
    dR, dA, dM = cuda(R), cuda(A), cuda(msgs)
    assert dM.data_ptr() % 16 == 0                                            # an aligned base, stride 33: the messages start at every residue
    same(eng.sig_challenge(R, A, msgs, CC.REDJUBJUB), want, "all host")
    out = eng.sig_challenge(dR, dA, dM, CC.REDJUBJUB)
    assert out.is_cuda and tuple(out.shape) == (n, 32)
    same(out, want, "all device")
    mixed = eng.sig_challenge(dR, dA, msgs, CC.REDJUBJUB)
    assert mixed.is_cuda
    same(mixed, want, "device R and A, host messages")
    rev = eng.sig_challenge(R, A, dM, CC.REDJUBJUB)
    assert isinstance(rev, np.ndarray)
    same(rev, want, "host R and A, device messages")
    same(eng.sig_challenge(None, dA, dM, CC.REDJUBJUB), CC.expected(CC.REDJUBJUB, None, A, [bytes(m) for m in msgs]), "A only, device")
    same(eng.sig_challenge(dR, None, msgs, CC.REDJUBJUB), CC.expected(CC.REDJUBJUB, R, None, [bytes(m) for m in msgs]), "R only, mixed")
    same(eng.sig_challenge(None, None, dM, CC.REDJUBJUB), CC.expected(CC.REDJUBJUB, None, None, [bytes(m) for m in msgs]), "messages alone, device")
    for d, h in ((dR, R), (dA, A), (dM, msgs)):
        assert np.array_equal(d.cpu().numpy(), h)                             # inputs as they were
    own = np.zeros((n, 32), np.uint8)
    assert eng.sig_challenge(R, A, msgs, CC.REDJUBJUB, out=own) is own
    same(own, want, "caller-owned result")
    # a device result with its neighbours watched, through the C ABI
    lib, ctx = eng._lib, eng._ctx
    lib.jj_ctx_use_own_stream(ctx)
    dres = torch.full((n + 2, 32), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert lib.jj_sig_challenge(ctx, n, CC.REDJUBJUB, dR.data_ptr(), A.ctypes.data, dM.data_ptr(), L, None, dres.data_ptr()) == 0 and lib.jj_ctx_sync(ctx) == 0
    same(dres[:n], want, "device result, mixed inputs")
    assert bool((dres[n:] == 0xAB).all())


def test_buffer_discipline_row():
    """the row of tests/sig_challenge_buffer_row.py through the runner of tests/test_gpu_buffers.py (its Env, checked_call, placements and skews):
    every size of the table x every skew (0, 16, 496 and the mixed one) in one device arena, the host arenas and the mixed placements at the host
    sizes, n = 0: return code 0, the n x 32 challenge bytes equal to the oracle, guards and inputs untouched"""
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


def test_empty_and_invalid_calls(eng):
    import torch

    from jubjub_amd import _lib

    lib, ctx = eng._lib, eng._ctx
    lib.jj_ctx_use_own_stream(ctx)
    INVALID = _lib.JJ_ERR_INVALID
    n = 4
    R, A = CC.parts(n, "both")
    msgs = CC.fixed(n, 8)
    out = np.full((n + 1, 32), 0xEE, np.uint8)
    dout = torch.full((n + 1, 32), 0xEE, dtype=torch.uint8, device="cuda")
    dany = torch.zeros(256, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r, a, m, o = R.ctypes.data, A.ctypes.data, msgs.ctypes.data, out.ctypes.data
    good = np.array([0, 8, 16, 24, 32], np.uint64)
    call = lib.jj_sig_challenge

    def offs(*v):
        arr = np.array(v, np.uint64)
        return arr, arr.ctypes.data

    assert call(ctx, 0, None, None, None, None, 0, None, None) == 0                                    # n = 0 succeeds with NULL arrays
    assert call(ctx, 0, CC.REDJUBJUB, r, a, m, 8, None, o) == 0 and call(ctx, 0, None, r, a, m, 0, good.ctypes.data, dout.data_ptr()) == 0   # ... and touches nothing
    assert eng.sig_challenge(np.zeros((0, 32), np.uint8), None, np.zeros((0, 5), np.uint8)).shape == (0, 32)
    assert call(None, n, None, r, a, m, 8, None, o) == INVALID                                          # a NULL context
    assert call(ctx, n, None, r, a, m, 8, None, None) == INVALID                                        # NULL c32 with n > 0
    assert call(ctx, n, None, r, a, None, 8, None, o) == INVALID                                        # NULL msgs with a non-zero total length
    assert call(ctx, n, None, r, a, None, 0, good.ctypes.data, o) == INVALID                            # ... ragged
    assert call(ctx, n, None, r, a, m, 8, good.ctypes.data, o) == INVALID                               # offsets together with msg_len != 0
    for bad in (offs(1, 8, 16, 24, 32), offs(0, 8, 7, 24, 32), offs(0, 8, 16, 24, 23)):                 # offsets[0] != 0, a decreasing pair
        assert call(ctx, n, None, r, a, m, 0, bad[1], o) == INVALID, bad[0]
    doffs = torch.from_numpy(good.view(np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    assert call(ctx, n, None, r, a, m, 0, doffs.data_ptr(), o) == INVALID                               # offsets in device memory
    assert b"host" in lib.jj_last_error(ctx)
    assert call(ctx, (1 << 24) + 1, None, r, a, m, 0, None, o) == INVALID                               # n > 2^24, before anything is read
    big = offs(0, (1 << 32) + 1)
    assert call(ctx, 1, None, None, None, m, 0, big[1], o) == INVALID                                   # more than 2^32 message bytes: the offsets alone say so
    assert b"2^32" in lib.jj_last_error(ctx)
    assert call(ctx, 1 << 20, None, None, None, m, (1 << 12) + 1, None, o) == INVALID                   # ... and n x msg_len
    for k in range(4):                                                                                  # a misaligned device pointer, in every place
        args = [r, a, m, o]
        args[k] = dany.data_ptr() + 8
        assert call(ctx, n, None, args[0], args[1], args[2], 8, None, args[3]) == INVALID, k
        assert b"16-byte aligned" in lib.jj_last_error(ctx)
    assert call(ctx, n, None, r, a, m, 8, None, dout.data_ptr() + 4) == INVALID
    assert lib.jj_ctx_sync(ctx) == 0
    assert (out == 0xEE).all() and bool((dout == 0xEE).all())                                           # c32 untouched by every refused call
    for x, y in ((R, CC.parts(n, "both")[0]), (msgs, CC.fixed(n, 8))):
        assert np.array_equal(x, y)
    assert call(ctx, n, None, r, a, m, 8, None, o) == 0                                                  # the context is as good as before
    same(out[:n], CC.expected(None, R, A, [bytes(x) for x in msgs]), "after the refused calls")
    assert (out[n] == 0xEE).all()
    with pytest.raises(ValueError):
        eng.sig_challenge(R, A, msgs, b"short")
    with pytest.raises(ValueError):
        eng.sig_challenge(R[:2], A, msgs)


# ---- the compositions: hash, then check
N_SIG = 65


@pytest.fixture(scope="module")
def signatures():
    """65 signatures built with the oracle over the generator: R = [k]B, A = [sk]B, c = H(R || A || M), s = k + c sk"""
    from oracle import c_oracle as O
    from tests import sig_batch_cases as SC

    B = SC.bases()["order8r"]
    sk = [SC.SK[i % len(SC.SK)] for i in range(N_SIG)]
    k = [SC.NONCE[(3 * i + 1) % len(SC.NONCE)] for i in range(N_SIG)]
    A = O.compress(O.fixedbase_mul(np.stack([SC.b32(x) for x in sk]), B))
    R = O.compress(O.fixedbase_mul(np.stack([SC.b32(x) for x in k]), B))
    msgs = [CC.rng_bytes(600 + i, 32 + (i % 5)).tobytes() for i in range(N_SIG)]
    c = CC.expected(CC.REDJUBJUB, R, A, msgs)
    s = np.stack([SC.b32((k[i] + SC.to_int(c[i]) * sk[i]) % SC.R) for i in range(N_SIG)])
    return B, R, A, s, msgs


@pytest.mark.parametrize("where", ["device", "numpy"])
def test_compositions_accept_valid_and_name_the_tampered_message(eng, signatures, where):
    from jubjub_amd.engine import REDJUBJUB_PERSONAL, SIG_OK, SIG_REJECT

    B, R, A, s, msgs = signatures
    tab = eng.fixedbase_table(B, 13)
    try:
        flat, offsets = CC.pack(msgs)
        bad = 37
        o = int(offsets[bad])
        tampered = flat.copy()
        tampered[o + 5] ^= 0x10                                                  # one bit of one message
        put = cuda if where == "device" else (lambda x: x)
        r_, a_, s_, b_ = put(R), put(A), put(s), put(B)
        # (no host synchronisation is written between the hash and the check: the wrapper hands the challenges over as they are)
        for m, bad_units in ((put(flat), []), (put(tampered), [bad])):
            v = eng.sigverify_each_msgs(tab, r_, a_, s_, m, REDJUBJUB_PERSONAL, offsets=offsets)
            assert (hasattr(v, "is_cuda") and v.is_cuda) == (where == "device")
            v = host(v)
            assert [int(i) for i in np.nonzero(v != SIG_OK)[0]] == bad_units and all(v[i] == SIG_REJECT for i in bad_units)
            assert eng.sigbatch_verify_msgs(b_, r_, a_, s_, m, REDJUBJUB_PERSONAL, offsets=offsets) == ("reject" if bad_units else "ok")
        if where == "numpy":                                                     # the list form packs the same bytes
            assert (host(eng.sigverify_each_msgs(tab, R, A, s, msgs, REDJUBJUB_PERSONAL)) == SIG_OK).all()
            assert eng.sigbatch_verify_msgs(B, R, A, s, msgs, REDJUBJUB_PERSONAL) == "ok"
            assert eng.sigbatch_verify_msgs(B, R, A, s, msgs, None) == "reject"   # another personalisation, other challenges
    finally:
        tab.close()
