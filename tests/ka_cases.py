"""Cases of jj_ka_kdf and jj_chacha20_xor (key agreement with one secret scalar, its KDF, one ChaCha20 key per row).  The restatement is built
from oracle.jubjub_ref -- affine_from_bytes, the integer ladder ext_multiply (bits 251..0 of the 32-byte pattern, never reduced mod r),
ext_double, affine_to_bytes -- and hashlib.blake2b(digest_size=32, person=...); the cipher is a pure-Python ChaCha20 (RFC 8439 section 2.3),
pinned by the RFC's block in tests/test_ka_cases_cpu.py.  Nothing here runs the library.  Everything is seeded and small: the ladder runs once
per (scalar, point) pair -- SCALARS x POINTS, a few hundred -- and every flag combination is derived from those shares.  Test infrastructure only.

SCALARS: 0, 1, 2, r - 1, r, r + 1, 2^251, 2^252 - 1, a pattern with bits 252..255 set (which must give what the pattern without them gives:
the next entry), seeded random patterns.  POINTS (encodings): the identity, (0, -1), all eight torsion points, Q + T for a prime-order Q and T of
order 2, 4 and 8, the two non-canonical encodings ZIP 216 rejects, encodings that do not decode (v >= q; v with (v^2 - 1)/(1 + d v^2) a
non-square), seeded prime-order points.  FLAGS: every combination of the three decoder bits with the two KA flags."""
import hashlib
import json
import os
import struct

import numpy as np

from oracle import jubjub_ref as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q, R = J.Q, J.R_MOD
ZIP216, TORSION_FREE, NOT_SMALL_ORDER, CLEAR_COFACTOR, KA_COFACTOR, KA_HASH_INPUT = 1, 2, 4, 8, 32, 64
DECODER_BITS = ZIP216 | TORSION_FREE | NOT_SMALL_ORDER
FLAGS = [d | k for d in range(8) for k in (0, KA_COFACTOR, KA_HASH_INPUT, KA_COFACTOR | KA_HASH_INPUT)]
SAPLING_FLAGS = ZIP216 | KA_COFACTOR | KA_HASH_INPUT
SAPLING_PERSONAL = b"Zcash_SaplingKDF"
PERSONALS = {"null": None, "sapling": SAPLING_PERSONAL, "ones": b"\xff" * 16}
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1024, 1025)      # wave edges, workgroup edges, the 16 x 64-unit group of k_varbase_mont_x1


def b32(x):
    return int(x).to_bytes(32, "little")


def rng_bytes(seed, *shape):
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------- planted scalars
HIGH_BITS = (0xF << 252) | 0x1234567
SCALARS = [b32(x) for x in (0, 1, 2, R - 1, R, R + 1, 1 << 251, (1 << 252) - 1, HIGH_BITS, HIGH_BITS & ((1 << 252) - 1))] + \
          [rng_bytes(9100 + k, 32).tobytes() for k in range(2)]
HIGH_PAIR = (8, 9)               # indices of the pattern with bits 252..255 set and of the same pattern without them


# ---------------------------------------------------------------------------------------------------- planted points
def torsion_points():
    with open(os.path.join(ROOT, "tests", "golden", "reference_vectors.json")) as f:
        g = json.load(f)
    lim = lambda hs: sum(int(h, 16) << (64 * i) for i, h in enumerate(hs))     # noqa: E731
    return [(lim(p["u"]), lim(p["v"])) for p in g["EIGHT_TORSION_raw"]["points"]]


def order_of(p):
    """the order of a torsion point: 1, 2, 4 or 8"""
    k, e = 1, J.affine_to_extended(p)
    while not J.ext_is_identity(e):
        e, k = J.ext_double(e), 2 * k
        assert k <= 8
    return k


def prime_order(k):
    """[8 k]G: torsion-free whatever the order of G is"""
    return J.scalar_mul_fast(J.GENERATOR, 8 * k)


def non_square_v():
    """the smallest v >= 2 for which (v^2 - 1)/(1 + d v^2) has no square root: an encoding that passes the range check and fails the root"""
    v = 2
    while J.affine_from_bytes(b32(v), True)[1]:
        v += 1
    return v


def _points():
    tors = torsion_points()
    by_order = {order_of(t): t for t in tors}
    assert sorted(order_of(t) for t in tors) == [1, 2, 4, 4, 8, 8, 8, 8]
    Qp = prime_order(0x1F2E3D4C5B6A7988)
    enc = lambda p: J.affine_to_bytes(p)                                          # noqa: E731
    pts = [("identity", enc(J.AFFINE_IDENTITY)), ("minus_one", enc((0, Q - 1)))]
    pts += [("torsion%d_order%d" % (k, order_of(t)), enc(t)) for k, t in enumerate(tors)]
    pts += [("prime_plus_order%d" % o, enc(J.affine_add_fast(Qp, by_order[o]))) for o in (2, 4, 8)]
    pts += [("zip216_identity_signed", b32(1 | (1 << 255))), ("zip216_minus_one_signed", b32((Q - 1) | (1 << 255)))]
    pts += [("v_is_q_plus_5", b32(Q + 5)), ("no_root", b32(non_square_v())), ("no_root_signed", b32(non_square_v() | (1 << 255)))]
    pts += [("prime%d" % k, enc(prime_order(0x9E3779B97F4A7C15 * (k + 1) % R))) for k in range(4)]
    return pts


_MEMO = {}


def points():
    """[(name, 32-byte encoding)]"""
    if "points" not in _MEMO:
        _MEMO["points"] = _points()
    return _MEMO["points"]


def encodings():
    """(len(points()), 32) uint8"""
    return np.stack([np.frombuffer(e, dtype=np.uint8) for _, e in points()])


# ---------------------------------------------------------------------------------------------------- the restatement
def decode(enc, flags):
    """((u, v), ok) under the decoder bits of `flags`: AffinePoint::from_bytes with or without the ZIP 216 rule, then the subgroup and the
    small-order rules"""
    enc = bytes(enc)
    key = ("dec", enc, flags & ZIP216)
    if key not in _MEMO:
        p, ok = J.affine_from_bytes(enc, zip216=bool(flags & ZIP216))
        e = J.affine_to_extended(p)
        _MEMO[key] = (p, ok, bool(ok and J.ext_is_torsion_free(e)), bool(ok and J.ext_is_small_order(e)))
    p, ok, tf, small = _MEMO[key]
    ok = bool(ok) and (tf or not flags & TORSION_FREE) and (not small or not flags & NOT_SMALL_ORDER)
    return p, ok


def shares(sk, p):
    """(to_bytes([sk]P), to_bytes([8]([sk]P))) with sk a 32-byte pattern taken as an INTEGER (bits 251..0): exact on the whole curve"""
    key = ("share", bytes(sk), p)
    if key not in _MEMO:
        e = J.ext_multiply(J.affine_to_extended(p), bytes(sk))
        _MEMO[key] = (J.affine_to_bytes(J.ext_to_affine(e)), J.affine_to_bytes(J.ext_to_affine(J.ext_double(J.ext_double(J.ext_double(e))))))
    return _MEMO[key]


def kdf(personal, share, enc, flags):
    return hashlib.blake2b(share + (bytes(enc) if flags & KA_HASH_INPUT else b""), digest_size=32, person=personal or b"").digest()


def expected_one(sk, enc, flags, personal):
    """(key: 32 bytes, ok) of one unit"""
    p, ok = decode(enc, flags)
    if not ok:
        return bytes(32), 0
    return kdf(personal, shares(sk, p)[1 if flags & KA_COFACTOR else 0], enc, flags), 1


def expected(sk, encs, flags, personal):
    """(keys (n, 32), ok (n,)) uint8 for n encodings; equal encodings share their ladder"""
    n = len(encs)
    keys, ok = np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8)
    seen = {}
    for i in range(n):
        e = bytes(encs[i])
        if e not in seen:
            seen[e] = expected_one(sk, e, flags, personal)
        keys[i], ok[i] = np.frombuffer(seen[e][0], dtype=np.uint8), seen[e][1]
    return keys, ok


def tiled(n, shift=0):
    """n encodings: the planted list repeated, starting at entry `shift`"""
    e = encodings()
    return np.ascontiguousarray(e[(np.arange(n) + shift) % len(e)])


# ---------------------------------------------------------------------------------------------------- ChaCha20, RFC 8439 section 2.3
def chacha20_block(key, counter, nonce):
    """the 64-byte keystream block of a 32-byte key, a 32-bit block counter and a 12-byte nonce"""
    s = list(struct.unpack("<4I", b"expand 32-byte k")) + list(struct.unpack("<8I", bytes(key))) + [counter & 0xFFFFFFFF] + list(struct.unpack("<3I", bytes(nonce)))
    x = list(s)
    rotl = lambda v, n: ((v << n) | (v >> (32 - n))) & 0xFFFFFFFF                 # noqa: E731

    def qr(a, b, c, d):
        x[a] = (x[a] + x[b]) & 0xFFFFFFFF; x[d] = rotl(x[d] ^ x[a], 16)           # noqa: E702
        x[c] = (x[c] + x[d]) & 0xFFFFFFFF; x[b] = rotl(x[b] ^ x[c], 12)           # noqa: E702
        x[a] = (x[a] + x[b]) & 0xFFFFFFFF; x[d] = rotl(x[d] ^ x[a], 8)            # noqa: E702
        x[c] = (x[c] + x[d]) & 0xFFFFFFFF; x[b] = rotl(x[b] ^ x[c], 7)            # noqa: E702

    for _ in range(10):
        qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15)      # noqa: E702
        qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14)      # noqa: E702
    return struct.pack("<16I", *[(a + b) & 0xFFFFFFFF for a, b in zip(x, s)])


def keystream(key, counter, nonce, length):
    nonce = bytes(12) if nonce is None else bytes(nonce)
    return b"".join(chacha20_block(key, counter + b, nonce) for b in range(-(-length // 64)))[:length]


def chacha20_xor(keys, data, length, nonce=None, counter=0):
    """keys (n, 32), data (n, stride) -> (n, length): each row's first `length` bytes xor its key's stream from block `counter` on (mod 2^32)"""
    n = len(keys)
    out = np.zeros((n, length), np.uint8)
    cache = {}
    for i in range(n):
        k = bytes(keys[i])
        if k not in cache:
            cache[k] = np.frombuffer(keystream(k, counter, nonce, length), dtype=np.uint8)
        out[i] = data[i, :length] ^ cache[k]
    return out


CIPHER_LENS = (4, 52, 60, 64, 68, 128, 564, 1024)
CIPHER_COUNTERS = (0, 1, (1 << 32) - 1)
NONCE = bytes.fromhex("000000090000004a00000000")          # the nonce of RFC 8439 section 2.3.2
