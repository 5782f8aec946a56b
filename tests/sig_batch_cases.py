"""Batches of Schnorr signatures for jj_sigbatch_begin, built with the oracle, and what the job's finish must write for each planted variant.
Plain data (numpy + the oracle, no GPU import); tests/test_sig_batch_cpu.py pins every expected value to the oracle's evaluation of the whole
sum, tests/test_gpu_sig_batch.py runs the same cases through the C ABI.  Test infrastructure only.

A signature over the base B: R = [k]B, A = [sk]B, c a seeded Fr element, s = k + c sk mod r.  Eight secret keys, a pool of 64 nonces.
The batch check:   out = [8] (sum [z_i] R_i + sum [z_i c_i mod r] A_i - [sum z_i s_i mod r] B)   ->   (0, 1) accept, (0, -1) malformed."""
import functools

import numpy as np

from oracle import c_oracle as O
from oracle import jubjub_ref as J

Q, R = J.Q, J.R_MOD
NKEYS, NNONCES = 8, 64
ZIP216 = 1


def b32(x):
    return np.frombuffer(int(x).to_bytes(32, "little"), dtype=np.uint8)


def pt64(p):
    return np.concatenate([b32(p[0]), b32(p[1])])


def to_int(row):
    return int.from_bytes(bytes(row), "little")


IDENTITY = pt64((0, 1))
MALFORMED = pt64((0, Q - 1))
SK = [J.synth_scalar(i, seed=0x51C0) or 1 for i in range(NKEYS)]
NONCE = [J.synth_scalar(i, seed=0x51C1) or 1 for i in range(NNONCES)]
T8 = pt64(J.scalar_mul_fast(J.GENERATOR, R))       # [r]G: G has order 8r, so T8 has order 8 (checked in the CPU tests)
NONCANONICAL_IDENTITY = np.concatenate([b32(1)[:31], np.array([0x80], np.uint8)])      # v = 1, sign bit set with u = 0: rejected under ZIP-216 only


def _mul(k, p):
    """[k]p for an integer 0 <= k < 2^252 (the oracle's ladder)"""
    return O.varbase_mul(b32(k)[None], np.asarray(p, np.uint8).reshape(1, 64))[0]


@functools.lru_cache(maxsize=None)
def bases():
    """name -> 64-byte base: a point of prime order, and the generator of the whole group (order 8r)"""
    g = pt64(J.GENERATOR)
    return {"prime": O.point_op("mul_by_cofactor", g[None])[0], "order8r": g}


@functools.lru_cache(maxsize=None)
def _pools(base_name):
    B = bases()[base_name]
    A = O.fixedbase_mul(np.stack([b32(x) for x in SK]), B)
    Rp = O.fixedbase_mul(np.stack([b32(x) for x in NONCE]), B)
    return A, Rp, O.compress(A), O.compress(Rp)


@functools.lru_cache(maxsize=None)
def off_curve_encoding():
    """the first v = 2, 3, ... that is the v of no curve point"""
    for v in range(2, 64):
        enc = b32(v)
        if not O.decompress(enc[None], 0)[1][0]:
            return enc
    raise AssertionError("no off-curve encoding found")


class Batch:
    """one call's arguments (host arrays) + what jj_msm_finish must write"""

    def __init__(self, name, base, r, a, s, c, z, flags, expected):
        self.name, self.base, self.r, self.a, self.s, self.c, self.z, self.flags, self.expected = name, base, r, a, s, c, z, flags, expected

    @property
    def n(self):
        return len(self.s)

    def arrays(self):
        return self.r, self.a, self.s, self.c, self.z


@functools.lru_cache(maxsize=None)
def _valid(n, base_name):
    """(r32, a32, s32, c32, z16, key index, nonce index) of n valid signatures; read-only arrays shared by every variant of this size"""
    _, _, Aenc, Renc = _pools(base_name)
    rng = np.random.default_rng(0x5160 + n)
    ki = rng.integers(0, NKEYS, n)
    mi = rng.integers(0, NNONCES, n)
    c = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    c[:, 31] &= 0x0F
    z = rng.integers(0, 256, size=(n, 16), dtype=np.uint8)
    z[~z.any(axis=1), 0] = 1
    s = np.zeros((n, 32), np.uint8)
    for i in range(n):
        ci = to_int(c[i])
        if ci >= R:
            ci -= R
            c[i] = b32(ci)
        s[i] = b32((NONCE[mi[i]] + ci * SK[ki[i]]) % R)
    out = (Renc[mi], Aenc[ki], s, c, z, ki, mi)
    for x in out:
        x.setflags(write=False)
    return out


def positions(n):
    """where a variant is planted: the ends, the 63 / 64 wave boundary, the middle"""
    return sorted({0, n - 1, n // 2} | {p for p in (63, 64) if p < n})


def variants(n):
    """[(variant name, position)]: every planted variant of a batch of n signatures"""
    out = [("valid", None), ("order8r", None), ("c_plus_r", None)]
    for k in positions(n):
        out += [(v, k) for v in ("torsion_r", "bad_s", "bad_r", "s_plus_r", "off_curve_r", "noncanonical_a_zip216", "noncanonical_a")]
    return out


def batch(n, variant="valid", k=None):
    """the batch of n signatures with `variant` planted at position k, and its expected 64 bytes.  Closed forms: one oracle scalar multiplication
    whatever n is."""
    base_name = "order8r" if variant == "order8r" else "prime"
    B = bases()[base_name]
    r, a, s, c, z, ki, mi = _valid(n, base_name)
    flags, expected = 0, IDENTITY
    name = "%s n=%d%s" % (variant, n, "" if k is None else " k=%d" % k)
    if variant in ("valid", "order8r"):
        pass
    elif variant == "c_plus_r":
        c = np.stack([b32(to_int(row) + R) for row in c]) if n else c                   # the same challenges, not reduced
    elif variant == "torsion_r":
        r = r.copy()
        r[k] = O.compress(O.point_op("add", _pools(base_name)[1][mi[k]][None], T8[None]))[0]       # [8] T8 = O: accepted by the cofactored check
    elif variant == "bad_s":
        s0, s = to_int(s[k]), s.copy()
        s[k] = b32((s0 + 5) % R)
        delta = (to_int(s[k]) - s0) % R
        expected = O.point_op("neg", _mul(to_int(z[k]) * delta % R, O.point_op("mul_by_cofactor", B[None])[0])[None])[0]      # -[8 z_k delta mod r] B
    elif variant == "bad_r":
        D = _mul(0xD15, B)
        r = r.copy()
        r[k] = O.compress(O.point_op("add", _pools(base_name)[1][mi[k]][None], D[None]))[0]
        expected = _mul(to_int(z[k]), O.point_op("mul_by_cofactor", D[None])[0])                                         # [8 z_k] D
    elif variant == "s_plus_r":
        s = s.copy()
        s[k] = b32(to_int(s[k]) + R)
        expected = MALFORMED
    elif variant == "off_curve_r":
        r = r.copy()
        r[k] = off_curve_encoding()
        expected = MALFORMED
    elif variant in ("noncanonical_a_zip216", "noncanonical_a"):
        # A_k = the identity in its non-canonical encoding, s_k = the nonce: valid when the encoding is accepted (flags = 0)
        a, s = a.copy(), s.copy()
        a[k] = NONCANONICAL_IDENTITY
        s[k] = b32(NONCE[mi[k]])
        if variant == "noncanonical_a_zip216":
            flags, expected = ZIP216, MALFORMED
    else:
        raise KeyError(variant)
    return Batch(name, B, r, a, s, c, z, flags, expected)


def full_evaluation(b):
    """what the issue defines, evaluated term by term by the oracle: decode, the 2n + 1 scalars with Python integers, O.msm, three doublings"""
    n = b.n
    if n == 0:
        return IDENTITY
    rp, rok = O.decompress(b.r, b.flags)
    ap, aok = O.decompress(b.a, b.flags)
    sv = [to_int(x) for x in b.s]
    bad = not rok.all() or not aok.all() or any(x >= R for x in sv)
    rp[rok == 0] = IDENTITY
    ap[aok == 0] = IDENTITY
    zv = [to_int(x) for x in b.z]
    cv = [to_int(x) % R for x in b.c]
    sigma = sum(zi * si for zi, si in zip(zv, sv)) % R
    scalars = np.stack([b32(zi) for zi in zv] + [b32(zi * ci % R) for zi, ci in zip(zv, cv)] + [b32((R - sigma) % R)])
    total = O.msm(scalars, np.concatenate([rp, ap, b.base[None]]))[None]
    for _ in range(3):
        total = O.point_op("double", total)
    return MALFORMED if bad else total[0]
