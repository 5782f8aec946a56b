"""tests/ka_cases.py, pinned without a GPU: the cipher of the restatement gives the block of RFC 8439 section 2.3.2, the KDF is BLAKE2b with a
32-byte digest and not BLAKE2b-512 cut short, the planted points are what their names say and the decoder bits separate them as claimed, the
scalars are taken as integers (bits 252..255 ignored, r not reduced away), [8]([sk]P) differs from [8 sk mod r]P on the planted torsion inputs --
so the cases can tell an integer ladder from one that reduces its scalar --, the interval bounds of the cofactor doublings hold, and the two
buffer-discipline rows stand in the table with the restatement's bytes."""
import hashlib

import numpy as np

from oracle import jubjub_ref as J
from tests import ka_buffer_row as BR  # joins buffer_cases.CASES at collection, before the table's coverage pin runs
from tests import ka_cases as KC

RFC_KEYSTREAM = ("10f1e7e4d13b5915500fdd1fa32071c4c7d1f4c733c068030422aa9ac3d46c4ed2826446079faa0914c2d705d98b02a2"
                 "b5129cd1de164eb9cbd083e8a2503c4e")


def test_chacha20_restatement_gives_the_rfc_8439_block():
    key, nonce = bytes(range(32)), bytes.fromhex("000000090000004a00000000")
    assert KC.NONCE == nonce
    assert KC.chacha20_block(key, 1, nonce).hex() == RFC_KEYSTREAM
    assert KC.keystream(key, 1, nonce, 64).hex() == RFC_KEYSTREAM and KC.keystream(key, 1, nonce, 52).hex() == RFC_KEYSTREAM[:104]
    # blocks follow each other, and the counter wraps modulo 2^32
    two = KC.keystream(key, 0, nonce, 128)
    assert two[64:] == bytes.fromhex(RFC_KEYSTREAM) and two[:64] != two[64:]
    wrap = KC.keystream(key, (1 << 32) - 1, nonce, 192)
    assert wrap[64:] == two and wrap[:64] == KC.chacha20_block(key, (1 << 32) - 1, nonce)
    data = KC.rng_bytes(1, 3, 72)
    keys = np.stack([np.frombuffer(key, dtype=np.uint8)] * 3)
    out = KC.chacha20_xor(keys, data, 68, nonce, 1)
    assert out.shape == (3, 68) and (out[1] ^ data[1, :68]).tobytes() == KC.keystream(key, 1, nonce, 68)
    assert KC.keystream(key, 1, None, 64) == KC.chacha20_block(key, 1, bytes(12))


def test_kdf_is_blake2b_with_a_32_byte_digest():
    share, enc = bytes(range(32)), bytes(range(32, 64))
    for personal in KC.PERSONALS.values():
        assert KC.kdf(personal, share, enc, 0) == hashlib.blake2b(share, digest_size=32, person=personal or b"").digest()
        assert KC.kdf(personal, share, enc, KC.KA_HASH_INPUT) == hashlib.blake2b(share + enc, digest_size=32, person=personal or b"").digest()
        assert KC.kdf(personal, share, enc, 0) != hashlib.blake2b(share, digest_size=64, person=personal or b"").digest()[:32]
    assert KC.SAPLING_PERSONAL == b"Zcash_SaplingKDF" and len(KC.SAPLING_PERSONAL) == 16
    assert KC.SAPLING_FLAGS == 1 | 32 | 64


def test_flag_values():
    assert len(KC.FLAGS) == 32 == len(set(KC.FLAGS)) and all(not f & KC.CLEAR_COFACTOR for f in KC.FLAGS)
    assert (KC.KA_COFACTOR | KC.KA_HASH_INPUT) & (KC.DECODER_BITS | KC.CLEAR_COFACTOR | 16) == 0


def test_planted_points_are_what_they_say_and_the_flags_separate_them():
    pts = dict(KC.points())
    assert len(pts) == len(KC.points()) == 22 and len(set(pts.values())) == 20         # the identity and (0, -1) stand among the eight torsion points too
    assert pts["identity"] == pts["torsion7_order1"] and pts["minus_one"] == pts["torsion3_order2"]
    ok = lambda name, flags: KC.decode(pts[name], flags)[1]                         # noqa: E731
    assert KC.decode(pts["identity"], 0) == ((0, 1), True) and KC.decode(pts["minus_one"], 0) == ((0, J.Q - 1), True)
    orders = sorted(int(n.split("order")[1]) for n in pts if n.startswith("torsion"))
    assert orders == [1, 2, 4, 4, 8, 8, 8, 8]
    for name in pts:
        if name.startswith("torsion") or name in ("identity", "minus_one"):
            assert ok(name, 0) and ok(name, KC.ZIP216) and not ok(name, KC.NOT_SMALL_ORDER)
            assert ok(name, KC.TORSION_FREE) == (name in ("identity", "torsion7_order1")), name     # only the identity is in the subgroup
        elif name.startswith("prime_plus"):
            assert ok(name, KC.ZIP216) and ok(name, KC.NOT_SMALL_ORDER) and not ok(name, KC.TORSION_FREE), name
        elif name.startswith("prime"):
            assert all(ok(name, f) for f in range(8)), name
        elif name.startswith("zip216"):
            assert ok(name, 0) and not ok(name, KC.ZIP216), name                       # decodes under the old rule only
            assert KC.decode(pts[name], 0)[0][0] == 0
        else:
            assert name in ("v_is_q_plus_5", "no_root", "no_root_signed") and not any(ok(name, f) for f in range(8)), name
    # the identity with its sign bit set decodes (old rule) to the identity: inside the subgroup, of small order
    assert ok("zip216_identity_signed", KC.TORSION_FREE) and not ok("zip216_minus_one_signed", KC.TORSION_FREE)
    for name, enc in pts.items():                                                     # an undecodable encoding gives the zero key whatever else is set
        for flags in KC.FLAGS:
            key, good = KC.expected_one(KC.SCALARS[1], enc, flags, None)
            assert good == int(KC.decode(enc, flags)[1]) and (good or key == bytes(32))


def test_scalars_are_integers_of_252_bits():
    assert len(KC.SCALARS) == len(set(KC.SCALARS)) == 12 and all(len(s) == 32 for s in KC.SCALARS)
    ints = [int.from_bytes(s, "little") for s in KC.SCALARS]
    assert ints[:8] == [0, 1, 2, J.R_MOD - 1, J.R_MOD, J.R_MOD + 1, 1 << 251, (1 << 252) - 1]
    hi, lo = KC.HIGH_PAIR
    assert ints[hi] >> 252 == 0xF and ints[hi] & ((1 << 252) - 1) == ints[lo]
    enc = KC.encodings()
    for flags in (0, KC.SAPLING_FLAGS):
        a, b = KC.expected(KC.SCALARS[hi], enc, flags, None), KC.expected(KC.SCALARS[lo], enc, flags, None)
        assert (a[0] == b[0]).all() and (a[1] == b[1]).all()
    pts = dict(KC.points())
    t8 = KC.decode(pts["torsion0_order8"], 0)[0]
    # sk = r is not sk = 0 off the subgroup: [r]T = [r mod 8]T for T of order 8, and r is odd
    assert KC.shares(KC.SCALARS[4], t8)[0] != KC.shares(KC.SCALARS[0], t8)[0] == J.affine_to_bytes(J.AFFINE_IDENTITY)
    q = KC.decode(pts["prime0"], 0)[0]
    assert KC.shares(KC.SCALARS[4], q)[0] == J.affine_to_bytes(J.AFFINE_IDENTITY)     # ... and it is on it
    assert KC.shares(KC.SCALARS[5], q)[0] == pts["prime0"] == KC.shares(KC.SCALARS[1], q)[0]
    assert KC.shares(KC.SCALARS[2], q)[1] == J.affine_to_bytes(J.scalar_mul_fast(q, 16))


def test_cofactored_share_differs_from_the_reduced_scalar_on_torsion_inputs():
    """[8]([sk]P) against [8 sk mod r]P: equal on the subgroup, different where P has a torsion component and 8 sk mod r is no multiple of its
    order -- the planted inputs must hold such pairs, or the cases could not tell an integer ladder from a reducing one"""
    pts = dict(KC.points())
    for name in ("prime_plus_order2", "prime_plus_order4", "prime_plus_order8", "torsion0_order8", "minus_one"):
        p = KC.decode(pts[name], 0)[0]
        differ = 0
        for sk in KC.SCALARS[1:]:
            k = int.from_bytes(sk, "little") & ((1 << 252) - 1)
            reduced = J.affine_to_bytes(J.scalar_mul_fast(p, 8 * k % J.R_MOD))
            exact = J.affine_to_bytes(J.scalar_mul_fast(p, 8 * k))
            assert KC.shares(sk, p)[1] == exact, (name, k)
            differ += reduced != exact
        assert differ >= 1, name                                   # every torsion order is told apart by at least one planted scalar
    q = KC.decode(pts["prime1"], 0)[0]
    for sk in KC.SCALARS:
        k = int.from_bytes(sk, "little") & ((1 << 252) - 1)
        assert KC.shares(sk, q)[1] == J.affine_to_bytes(J.scalar_mul_fast(q, 8 * k % J.R_MOD))


def test_cofactor_doublings_stay_inside_the_checked_bounds():
    import os
    import sys

    sys.path.insert(0, os.path.join(KC.ROOT, "tools"))
    import bounds_check

    bounds_check.check_ka_cofactor(verbose=False)


def test_buffer_rows_join_the_table():
    import buffer_cases as BC

    ids = {c.id for c in BC.CASES}
    assert {"jj_ka_kdf", "jj_chacha20_xor"} <= ids and BR.ROW_KDF.covers == ("jj_ka_kdf",) and BR.ROW_CIPHER.covers == ("jj_chacha20_xor",)
    assert (BR.LEN, BR.STRIDE) == (52, 56) and BR.ROW_CIPHER.out_bytes(5) == {"out": 5 * 52} and dict(BR.ROW_CIPHER.ins)["c"] == 56
    for case in (BR.ROW_KDF, BR.ROW_CIPHER):
        for n in (0, 3, 65):
            ins, outs = case.data(n)
            for name, w in case.ins:
                assert ins[name].dtype == np.uint8 and ins[name].shape == (case.nrows(name, n), w)
            for name, w in case.outs:
                assert outs[name].dtype == np.uint8 and outs[name].shape == (case.nrows(name, n), w)
    ins, outs = BR.ROW_KDF.data(65)
    assert 0 < int(outs["ok"].sum()) < 65 and not outs["key"][outs["ok"][:, 0] == 0].any() and outs["key"][outs["ok"][:, 0] == 1].any(axis=1).all()
    ins, outs = BR.ROW_CIPHER.data(3)
    assert outs["out"].reshape(3, 52)[2].tobytes() == bytes(a ^ b for a, b in zip(ins["c"][2, :52].tobytes(), KC.keystream(ins["k"][2].tobytes(), 1, KC.NONCE, 52)))
