"""Cases and restatements of jj_blake2b and jj_ka_kdf_each (raw BLAKE2b digests over rows gathered from several arrays; the key agreement with one
secret scalar per row), and of the two compositions built on them, Engine.note_encrypt and Engine.ovk_open.  The hash is
hashlib.blake2b(digest_size, person) over the concatenated rows; the key agreement is tests/ka_cases.py's decode, ladder and doublings with a
scalar per row; the AEAD is the pure-Python one of tests/aead_cases.py.  tests/test_ovk_cases_cpu.py pins them.  Nothing here runs the
library; everything is seeded and small.  Test infrastructure only.

A BLAKE2b case: a prefix of prefix_len bytes, some backing arrays of a row stride each, and the sources as (array, skew, length): source s is
the `length` bytes at byte `skew` of every row of its array -- so one array may serve two sources, and a stride is larger than a length
wherever skew + length < stride.  Skews are 0 or 16: a device pointer stays 16-byte aligned.

B2B_CASES: prefix lengths {0, 4, 32, 124, 128, 132, 256} crossed with totals {0, 4, 124, 128, 132, 252, 256, 260, 384} (every total that is
at least the prefix; the rest cut into one to four sources by a rule that moves the cuts from case to case), which holds totals that are exact
multiples of 128 (the last block is final, no empty block behind it), a prefix of 128 and of 256 bytes with no source (the host must not have
compressed the final block), sources that straddle a block boundary and pieces that end exactly on one; then by name: four sources, one array
serving two sources, strides larger than the lengths at skews 0 and 16, the ock shape (prefix 32, three sources of 32), the longest prefix
and the longest source."""
import functools
import hashlib

import numpy as np

from oracle import jubjub_ref as J
from tests import aead_cases as AC
from tests import ka_cases as KC

R = J.R_MOD
DIGESTS = (32, 64)
PREFIX_LENS = (0, 4, 32, 124, 128, 132, 256)
TOTALS = (0, 4, 124, 128, 132, 252, 256, 260, 384)
SIZES = KC.SIZES
SAPLING_OCK_PERSONAL = b"Zcash_Derive_ock"
PERSONALS = {"null": None, "ock": SAPLING_OCK_PERSONAL, "ones": b"\xff" * 16}
RFC7693_ABC = bytes.fromhex("ba80a53f981c4d0d6a2797b69f12f6e94c212f14685ac4b74b12bb6fdbffa2d1"      # BLAKE2b-512("abc"), RFC 7693 appendix A
                            "7d87c5392aab792dc252d5de4533cc9518d38aa8dbf1925ab92386edd4009923")


class B2bCase:
    def __init__(self, name, prefix_len, strides, parts, nrows=None):
        self.name, self.prefix_len, self.strides, self.parts, self.nrows = name, prefix_len, tuple(strides), tuple(parts), nrows
        assert prefix_len % 4 == 0 and 0 <= prefix_len <= 4096 and len(self.parts) <= 4
        for a, skew, length in self.parts:
            assert skew in (0, 16) and length % 4 == 0 and 4 <= length <= 65536 and skew + length <= self.strides[a] and self.strides[a] % 4 == 0

    @property
    def total(self):
        return self.prefix_len + sum(length for _, _, length in self.parts)

    @property
    def lens(self):
        return [length for _, _, length in self.parts]

    def prefix(self, seed=0):
        return KC.rng_bytes(7700 + seed + self.prefix_len, max(self.prefix_len, 1)).tobytes()[:self.prefix_len]

    def arrays(self, n, seed=0):
        """the backing arrays, (n, stride) uint8 each, read-only; rows 0 and 1 are all zero and all one bits"""
        out = []
        for k, st in enumerate(self.strides):
            a = KC.rng_bytes(7800 + 31 * seed + 7 * k + st, n, st)
            if n > 1:
                a[0], a[1] = 0, 0xFF
            a.setflags(write=False)
            out.append(a)
        return out

    def views(self, arrays):
        """the sources as strided views of the backing arrays (numpy arrays or tensors)"""
        return [arrays[a][:, skew:skew + length] for a, skew, length in self.parts]

    def want(self, arrays, n, digest_len, personal, prefix):
        return digests([np.asarray(v) for v in self.views(arrays)], n, digest_len, personal, prefix)


def digests(sources, n, digest_len, personal, prefix):
    """(n, digest_len) uint8: hashlib's BLAKE2b-digest_len(personal; prefix || sources[0][i] || ..) of every row"""
    out = np.zeros((n, digest_len), np.uint8)
    for i in range(n):
        msg = bytes(prefix) + b"".join(np.asarray(s[i]).tobytes() for s in sources)
        out[i] = np.frombuffer(hashlib.blake2b(msg, digest_size=digest_len, person=personal or b"").digest(), dtype=np.uint8)
    return out


def _cut(rest, k):
    """`rest` bytes (a multiple of 4) as k lengths, each a positive multiple of 4"""
    d = rest // 4
    base = [d // k] * k
    base[-1] += d - sum(base)
    return [4 * x for x in base]


def _cross():
    cases = []
    for pl in PREFIX_LENS:
        for total in TOTALS:
            if total < pl:
                continue
            rest = total - pl
            if rest == 0:
                cases.append(B2bCase("prefix%d_total%d" % (pl, total), pl, (), ()))
                continue
            k = min(4, rest // 4, 1 + (pl // 4 + total // 4) % 4)
            lens = _cut(rest, k)
            # every source in an array of its own, wider than the source by 0, 4, 8 or 12 bytes
            cases.append(B2bCase("prefix%d_total%d" % (pl, total), pl, [length + 4 * (j % 4) for j, length in enumerate(lens)], [(j, 0, length) for j, length in enumerate(lens)]))
    return cases


B2B_CASES = _cross() + [
    B2bCase("straddle", 32, (120, 40), ((0, 0, 120), (1, 0, 40))),                    # source 0 covers bytes 32..152 of the string: across the block boundary
    B2bCase("piece_ends_on_block", 32, (96, 32), ((0, 0, 96), (1, 0, 32))),           # source 0 ends at byte 128; source 1 is the final block's start
    B2bCase("four_sources_128", 0, (32, 32, 32, 32), ((0, 0, 32), (1, 0, 32), (2, 0, 32), (3, 0, 32))),      # exactly one block, final
    B2bCase("four_sources_uneven", 4, (48, 64, 36, 160), ((0, 16, 20), (1, 0, 64), (2, 0, 36), (3, 16, 144))),
    B2bCase("one_array_two_sources", 32, (80,), ((0, 0, 32), (0, 16, 64))),           # the second source overlaps the first's bytes 16..32
    B2bCase("one_array_swapped", 0, (96, 32), ((0, 16, 80), (1, 0, 32), (0, 0, 16))),
    B2bCase("stride_over_len_skew0", 32, (112,), ((0, 0, 64),)),
    B2bCase("stride_over_len_skew16", 32, (112,), ((0, 16, 64),)),
    B2bCase("ock", 32, (32, 32, 32), ((0, 0, 32), (1, 0, 32), (2, 0, 32))),
    B2bCase("ock_in_one_record", 32, (128,), ((0, 0, 32), (0, 16, 32), (0, 0, 32))),      # three sources of 32 in records of 128 bytes
    B2bCase("longest_prefix", 4096, (8,), ((0, 0, 8),), nrows=65),
    B2bCase("longest_prefix_alone", 4096, (), (), nrows=65),
    B2bCase("longest_source", 4, (65536,), ((0, 0, 65536),), nrows=3),
]
B2B_BY_NAME = {c.name: c for c in B2B_CASES}
assert len(B2B_BY_NAME) == len(B2B_CASES)
B2B_SMALL = [c for c in B2B_CASES if c.nrows is None]                                 # the cases that run at every size


# ---------------------------------------------------------------------------------------------------- the key agreement, one scalar per row
def ka_one(sk, enc, flags, personal, h=None):
    """(key: 32 bytes, ok) of one row: ka_cases.expected_one with the second hashed part h (when given) in the place of the encoding"""
    p, ok = KC.decode(enc, flags)
    if not ok:
        return bytes(32), 0
    return KC.kdf(personal, KC.shares(sk, p)[1 if flags & KC.KA_COFACTOR else 0], bytes(enc) if h is None else bytes(h), flags), 1


def ka_each(sks, encs, flags, personal, h=None):
    """(keys (n, 32), ok (n,)) uint8; equal (scalar, encoding) pairs share their ladder through ka_cases' memo"""
    n = len(encs)
    keys, ok = np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8)
    for i in range(n):
        k, ok[i] = ka_one(bytes(sks[i]), bytes(encs[i]), flags, personal, None if h is None else bytes(h[i]))
        keys[i] = np.frombuffer(k, dtype=np.uint8)
    return keys, ok


def ka_grid(n, shift=0):
    """n rows of ka_cases.SCALARS x points(), one scalar per row: row i carries scalar (i + shift) mod |SCALARS| and, so that every pair
    comes up within |SCALARS| * |points| rows, point (i // |SCALARS|) mod |points| -> (sks (n, 32), encs (n, 32))"""
    S, E = KC.SCALARS, KC.encodings()
    i = np.arange(n)
    sks = np.stack([np.frombuffer(s, dtype=np.uint8) for s in S])[(i + shift) % len(S)] if n else np.zeros((0, 32), np.uint8)
    encs = E[(i // len(S)) % len(E)]
    return np.ascontiguousarray(sks), np.ascontiguousarray(encs)


GRID = len(KC.SCALARS) * 22            # rows after which ka_grid has shown every pair (22 planted points; the CPU test holds the count)


def hash_rows(n, seed=5):
    """n x 32 bytes for h32: nothing a decoder would accept as it stands"""
    return KC.rng_bytes(8800 + seed, max(n, 1), 32)[:n]


# ---------------------------------------------------------------------------------------------------- points as the library passes them
def point_bytes(p):
    return np.frombuffer(int(p[0]).to_bytes(32, "little") + int(p[1]).to_bytes(32, "little"), dtype=np.uint8)


def point_of(b64):
    b = bytes(b64)
    return int.from_bytes(b[:32], "little"), int.from_bytes(b[32:], "little")


def mul_compressed(sk, p):
    """to_bytes([sk]P), sk a 32-byte pattern taken as an integer of 252 bits"""
    return J.affine_to_bytes(J.ext_to_affine(J.ext_multiply(J.affine_to_extended(p), bytes(sk))))


# ---------------------------------------------------------------------------------------------------- the two compositions
def note_encrypt(esk, gd64, pkd32, plain, ovk, cv, cmu, kdf_personal, ock_personal, flags=KC.SAPLING_FLAGS):
    """(epk (n, 32), c_enc (n, L + 16), c_out (n, 80)): epk = [esk]g_d; the note key from ka_one(esk, pk_d, h = epk); c_enc sealed under it;
    ock = BLAKE2b-256(ock_personal; ovk || cv || cmu || epk); c_out = pk_d || esk sealed under ock.  A pk_d that does not decode gives the
    all-zero note key, as the library's ka_kdf_each does."""
    n, L = plain.shape
    epk, c_enc, c_out = np.zeros((n, 32), np.uint8), np.zeros((n, L + 16), np.uint8), np.zeros((n, 80), np.uint8)
    for i in range(n):
        e = mul_compressed(esk[i], point_of(gd64[i]))
        key, _ = ka_one(bytes(esk[i]), bytes(pkd32[i]), flags, kdf_personal, e)
        ock = hashlib.blake2b(bytes(ovk) + bytes(cv[i]) + bytes(cmu[i]) + e, digest_size=32, person=ock_personal).digest()
        epk[i] = np.frombuffer(e, dtype=np.uint8)
        c_enc[i] = np.frombuffer(AC.seal_one(key, None, b"", bytes(plain[i])), dtype=np.uint8)
        c_out[i] = np.frombuffer(AC.seal_one(ock, None, b"", bytes(pkd32[i]) + bytes(esk[i])), dtype=np.uint8)
    return epk, c_enc, c_out


def ovk_open(ovk, cv, cmu, epk, c_out, c_enc, kdf_personal, ock_personal, flags=KC.SAPLING_FLAGS):
    """(plain (n, L), op (n, 64), ok (n,), verdicts (n, 4)): ock, the AEAD over c_out, then on the rows that hit the canonicity of esk, the
    key agreement and the AEAD over c_enc.  ok is the AND of the four verdicts (out tag, esk < r, pk_d decodes, enc tag; a row that missed
    the first has zeros in the other three); every row that is not ok is zeros in plain and in op."""
    n, L = len(c_enc), c_enc.shape[1] - 16
    plain, op, ok, verdicts = np.zeros((n, L), np.uint8), np.zeros((n, 64), np.uint8), np.zeros(n, np.uint8), np.zeros((n, 4), np.uint8)
    for i in range(n):
        ock = hashlib.blake2b(bytes(ovk) + bytes(cv[i]) + bytes(cmu[i]) + bytes(epk[i]), digest_size=32, person=ock_personal).digest()
        o, hit = AC.open_one(ock, None, b"", bytes(c_out[i]))
        verdicts[i, 0] = hit
        if not hit:
            continue
        pkd, esk = o[:32], o[32:]
        verdicts[i, 1] = int(int.from_bytes(esk, "little") < R)
        key, verdicts[i, 2] = ka_one(esk, pkd, flags, kdf_personal, bytes(epk[i]))
        p, verdicts[i, 3] = AC.open_one(key, None, b"", bytes(c_enc[i]))
        if verdicts[i].all():
            plain[i], op[i], ok[i] = np.frombuffer(p, dtype=np.uint8), np.frombuffer(o, dtype=np.uint8), 1
    return plain, op, ok, verdicts


# ---------------------------------------------------------------------------------------------------- the planted batch of the round trip
PLANTED_ROWS = 96
PLANT = {7: "c_out tag", 19: "c_enc tag", 23: "esk >= r", 31: "pk_d does not decode", 40: "pk_d of small order", 41: "c_out tag", 64: "c_enc tag", 95: "esk >= r"}
NOTE_LEN = 564
OPEN_FLAGS = KC.SAPLING_FLAGS | KC.NOT_SMALL_ORDER


@functools.lru_cache(maxsize=None)
def planted_batch():
    """the inputs of a note_encrypt call over PLANTED_ROWS rows, PLANT's rows carrying what its name says (the tag flips are applied to the
    ciphertexts afterwards: tamper()) -> dict of read-only arrays and the ivk the pk_d were made with"""
    n = PLANTED_ROWS
    rng = np.random.default_rng(4242)
    ivk = int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") % (1 << 251)
    pool = [KC.prime_order(0x1234567 + 97 * k) for k in range(4)]                     # g_d: four diversified bases, prime order
    gd = [pool[i % 4] for i in range(n)]
    pk = {k: J.scalar_mul_fast(g, ivk) for k, g in enumerate(pool)}
    gd64 = np.stack([point_bytes(g) for g in gd])
    pkd = np.stack([np.frombuffer(J.affine_to_bytes(pk[i % 4]), dtype=np.uint8) for i in range(n)]).copy()
    esk = np.stack([np.frombuffer(KC.b32(int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") % R), dtype=np.uint8) for _ in range(n)]).copy()
    for i, what in PLANT.items():
        if what == "esk >= r":
            esk[i] = np.frombuffer(KC.b32(R + 5 + i), dtype=np.uint8)
        elif what == "pk_d does not decode":
            pkd[i] = np.frombuffer(dict(KC.points())["no_root"], dtype=np.uint8)
        elif what == "pk_d of small order":
            pkd[i] = np.frombuffer(next(e for name, e in KC.points() if name.startswith("torsion") and name.endswith("order8")), dtype=np.uint8)
    plain = rng.integers(0, 256, (n, NOTE_LEN), dtype=np.uint8)
    out = dict(esk=esk, gd64=gd64, pkd=pkd, plain=plain, ovk=rng.integers(0, 256, 32, dtype=np.uint8), cv=rng.integers(0, 256, (n, 32), dtype=np.uint8),
               cmu=rng.integers(0, 256, (n, 32), dtype=np.uint8))
    for a in out.values():
        a.setflags(write=False)
    out["ivk"] = KC.b32(ivk)
    return out


def tamper(c_enc, c_out):
    """copies with one bit of the tag flipped in PLANT's tag rows"""
    c_enc, c_out = c_enc.copy(), c_out.copy()
    for i, what in PLANT.items():
        if what == "c_out tag":
            c_out[i, 64 + i % 16] ^= 1 << (i % 8)
        elif what == "c_enc tag":
            c_enc[i, NOTE_LEN + i % 16] ^= 1 << (i % 8)
    return c_enc, c_out
