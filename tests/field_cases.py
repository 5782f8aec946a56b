"""
The edge matrix of the field and point entry points.  Plain data and constructors (numpy, Python integers, the
oracle): no GPU import.  tests/test_field_cases_cpu.py pins the cases, runs them through the host emulation of jj_field.h and shows which
branches of Field::to_plain / is_zero and of canon_plain_product they execute; tests/test_gpu_field_matrix.py runs the same cases through
the kernels.  tests/test_emu_invert.py takes its edge values from inversion_values below: the emulator and the device invert one list.
"""
import functools

import numpy as np

import backend_cases as B
from oracle import jubjub_ref as J
from util import arr32, arr64, b32, to_int

Q, R = J.Q, J.R_MOD
M256 = (1 << 256) - 1
MONT_R = 1 << 261                                          # the device's Montgomery radix (jj_field.h: 9 limbs of 29 bits)
FIELDS = {"fq": (0, Q), "fr": (1, R)}                      # name -> (the oracle's and the emulator's field number, modulus)
GENERATORS = {"fq": 7, "fr": 6}                            # the multiplicative generators the reference names (both are non-residues)

# What the matrix was searched for and does not contain: {name: the search that was made}.  tests/test_field_cases_cpu.py fails when an
# entry here turns out to be reached, and when something unreached is missing here.
UNREACHED = {
    "fr sub: zero as -p": "Fr: a - b = 0 mod p never leaves to_plain's product at the digits of -p: all pairs of the matrix (the cross product of the "
                          "fixed values and the seven relation pairs of every value, 32 random patterns included) give the digits 0; Fq has such pairs",
    "fq mul: zero as -p": "a product is 0 mod p only when a factor is: from_words(k p) times anything, every such pair of the matrix gives the digits 0",
    "fr mul: zero as -p": "as for Fq",
    "normaliser: 2 additions of q": "canon_plain_product allows a value in (-2q, q); k_normalize gives it mul(U, zp) in (U zp / 2^261 - q, U zp / 2^261] with "
                                    "|U zp| / 2^261 < 1.44 q^2 / 2^261 < q / 49, so a second addition needs U zp < 0 (0.24 q^2 / 2^261 at the most) and the product within q / 294 below -q: "
                                    "every x of X times sixteen (U, V) (0, 1, 2, q - 1, q - 2, (q - 1) / 2, (q + 1) / 2, 2^254 - 1, eight random) and the whole plant give 0 or 1 additions",
}


def _dedupe(xs):
    return list(dict.fromkeys(int(x) for x in xs))


def _rand256(seed, count):
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(32), "little") for _ in range(count)]


# ------------------------------------------------------------------------------------------------------------------ values
@functools.lru_cache(maxsize=None)
def fixed_values(name):
    """the non-random values of V(p): 256-bit integers, some of them above p (from_words reduces)"""
    p = FIELDS[name][1]
    vs = [0, 1, 2, 3, p - 1, p - 2, p - 3, (p - 1) // 2, (p + 1) // 2,
          (1 << 29) - 1, 1 << 29, 1 << 58, (1 << 232) - 1, 1 << 232, (1 << 252) - 1, 1 << 252, (1 << 255) - 1, 1 << 255, M256]
    k = 1
    while k * p <= M256:                                   # p, 2p for Fq; p ... 17p for Fr
        vs += [x for x in (k * p - 1, k * p, k * p + 1) if x <= M256]
        k += 1
    rinv = pow(MONT_R, -1, p)
    # Montgomery forms 1, p - 1, 2^232, 2^29 - 1 in every one of the nine limbs (2^261 - 1, reduced) and in the low eight (2^232 - 1)
    vs += [m % p * rinv % p for m in (1, p - 1, 1 << 232, MONT_R - 1, (1 << 232) - 1)]
    return tuple(_dedupe(vs))


@functools.lru_cache(maxsize=None)
def random_values(name):
    return tuple(_rand256(0x56414C + FIELDS[name][0], 32))


def values(name):
    """V(p)"""
    return tuple(_dedupe(fixed_values(name) + random_values(name)))


RELATIONS = ("v,v", "v,p-v", "v,2p-v", "v,1/v", "v,-1/v", "v,v+1", "v,v+p")


def relation_pairs(name):
    """[(relation, a, b)] for every v of V(p); the relations are taken on v mod p where v is above p, and left out where b has no 256 bits
    (or v has no inverse)"""
    p = FIELDS[name][1]
    out = []
    for v in values(name):
        r = v % p
        out += [("v,v", v, v), ("v,p-v", v, p - r)]
        if 2 * p - r <= M256:
            out.append(("v,2p-v", v, 2 * p - r))
        if r:
            inv = pow(r, -1, p)
            out += [("v,1/v", v, inv), ("v,-1/v", v, p - inv)]
        if v + 1 <= M256:
            out.append(("v,v+1", v, v + 1))
        if v + p <= M256:
            out.append(("v,v+p", v, v + p))
    return out


@functools.lru_cache(maxsize=None)
def pairs(name):
    """(A, B): n x 32 bytes each -- the full cross product of the fixed values, then the relation pairs of every value"""
    f = fixed_values(name)
    ab = [(a, b) for a in f for b in f] + [(a, b) for _, a, b in relation_pairs(name)]
    return arr32([a for a, _ in ab]), arr32([b for _, b in ab])


@functools.lru_cache(maxsize=None)
def unary_values(name):
    """every value that appears in the matrix, once"""
    _, b = pairs(name)
    return arr32(_dedupe(list(values(name)) + [to_int(r) for r in b]))


BINARY = {"add": lambda a, b, p: (a % p + b % p) % p, "sub": lambda a, b, p: (a % p - b % p) % p, "mul": lambda a, b, p: (a % p) * (b % p) % p}
UNARY = {"neg": lambda a, p: -a % p, "square": lambda a, p: a * a % p, "double": lambda a, p: 2 * a % p}
EMU_OPS = {"add": 0, "sub": 1, "mul": 2, "neg": 3, "square": 4, "double": 5, "invert": 6, "eq": 9}       # emu_fq_op / emu_fr_op


def expect_binary(name, op, A, B_):
    p = FIELDS[name][1]
    return arr32([BINARY[op](to_int(a), to_int(b), p) for a, b in zip(A, B_)])


def expect_unary(name, op, A):
    p = FIELDS[name][1]
    return arr32([UNARY[op](to_int(a), p) for a in A])


def expect_invert(name, A):
    """(inverse or 0, 1 where there is an inverse)"""
    p = FIELDS[name][1]
    xs = [to_int(a) % p for a in A]
    return arr32([pow(x, -1, p) if x else 0 for x in xs]), np.array([1 if x else 0 for x in xs], np.uint8)


def expect_from_bytes(name, A):
    """the checked decoding: (value or 0, 1 where the integer is below p)"""
    p = FIELDS[name][1]
    xs = [to_int(a) for a in A]
    return arr32([x if x < p else 0 for x in xs]), np.array([1 if x < p else 0 for x in xs], np.uint8)


def expect_bits(name, A):
    p = FIELDS[name][1]
    return np.array([[(to_int(a) % p >> b) & 1 for b in range(256)] for a in A], dtype=np.uint8)


# --------------------------------------------------------------------------------------------------------------------- pow
@functools.lru_cache(maxsize=None)
def pow_matrix(name):
    """(A, E): bases x exponents.  2^(32 w) and 2^(32 w + 31) for every word w: the lowest and the highest bit of each word k_field_pow selects
    with (bit >> 5) == w"""
    p = FIELDS[name][1]
    bases = _dedupe([0, 1, 2, p - 1, p, p + 1, M256, GENERATORS[name]] + _rand256(0x504F57 + FIELDS[name][0], 5))
    exps = [0, 1, 2, 3, p - 2, p - 1, p, p + 1, (p - 1) // 2, M256]
    for w in range(8):
        exps += [1 << (32 * w), 1 << (32 * w + 31)]
    exps += [1 << k for k in (33, 63, 64, 224, 255)] + _rand256(0x455850 + FIELDS[name][0], 5)
    exps = _dedupe(exps)
    return arr32([a for a in bases for _ in exps]), arr32([e for _ in bases for e in exps])


def expect_pow(name, A, E):
    p = FIELDS[name][1]
    return arr32([pow(to_int(a) % p, to_int(e), p) for a, e in zip(A, E)])


# -------------------------------------------------------------------------------------------------------------------- wide
@functools.lru_cache(maxsize=None)
def wide_values(name):
    """512-bit integers for from_bytes_wide"""
    p = FIELDS[name][1]
    halves = [0, 1, p - 1, p, p + 1, M256] + _rand256(0x57494445 + FIELDS[name][0], 3)
    top = ((1 << 512) - 1) // p * p                        # the largest multiple of p below 2^512
    ws = [lo | (hi << 256) for lo in halves for hi in halves] + [p << 256, (p << 256) - 1, top, top - 1, top + 1, (1 << 512) - 1]
    assert top + 1 < 1 << 512
    return tuple(_dedupe(ws))


def wide_bytes(name):
    return np.stack([np.frombuffer(w.to_bytes(64, "little"), np.uint8) for w in wide_values(name)])


def expect_wide(name):
    p = FIELDS[name][1]
    return arr32([w % p for w in wide_values(name)])


# --------------------------------------------------------------------------------------------------------------- inversion
@functools.lru_cache(maxsize=None)
def inversion_values(name):
    """X: what Field::invert_divsteps is given, in the emulator (tests/test_emu_invert.py) and on the device: integers below 2^255, none of
    them 0 mod p, no two of one residue.  Below q all of them, so canonical for Fq; for Fr 2^252 ... 2^254 stay as they are (from_words reduces)."""
    p = FIELDS[name][1]
    xs = [1, p - 1, 2, p - 2]
    for k in range(255):
        xs += [1 << k, (1 << k) - 1]
    xs += [(p - 1) // 2, (p + 1) // 2, 3] + [x >> 2 for x in _rand256(0x494E56 + FIELDS[name][0], 64)]
    seen, out = set(), []
    for x in xs:
        if x % p and x % p not in seen:
            seen.add(x % p)
            out.append(x)
    return tuple(out)


def _canonical_rows(rng, n):
    """n x 32 random bytes below 2^254 (below q)"""
    a = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    a[:, 31] &= 0x3F
    return a


def norm_plant(n, seed=0x4E504C54):
    """(ext160, want64) for jj_batch_normalize on n >= 4 |X| rows: row t < |X| is (U, V, Z) = (seeded, seeded, X[t]), every other row has
    Z = 1 and canonical U, V and is its own result.  Element j of lane t is row t + j T (T = n / CHUNK >= |X|), so lane t inverts exactly
    X[t] * 1 * ... * 1."""
    X = inversion_values("fq")
    m = len(X)
    assert n >= 4 * m
    rng = np.random.default_rng(seed)
    ext = np.zeros((n, 160), np.uint8)
    ext[:, 0:32] = _canonical_rows(rng, n)
    ext[:, 32:64] = _canonical_rows(rng, n)
    ext[:, 64] = 1                                         # Z = 1
    ext[:, 96:] = 0xA5                                     # T1, T2: never read
    ext[:m, 64:96] = arr32(X)
    want = ext[:, :64].copy()
    for t, x in enumerate(X):
        xi = pow(x, -1, Q)
        want[t, :32] = b32(to_int(ext[t, 0:32]) * xi % Q)
        want[t, 32:] = b32(to_int(ext[t, 32:64]) * xi % Q)
    return ext, want


MONT_X1_UNITS = 16                                         # jj_mont.h; units of one lane are 64 apart, a wave owns 64 * 16 units
MONT_WAVE_UNITS = 64 * MONT_X1_UNITS


@functools.lru_cache(maxsize=None)
def mont_points():
    """[(x, (u, v))]: for every x of X that has one, the curve point with 1 - v = x -- the denominator k_varbase_mont_x1 inverts; the sign of u alternates"""
    out = []
    for x in inversion_values("fq"):
        v = (1 - x) % Q
        u = B._sqrt_any((v * v - 1) * pow(1 + J.EDWARDS_D * v * v, -1, Q) % Q)
        if u is None or u == 0:                            # u = 0: v = -1 (v = 1 is x = 0, not in X), kept out so that the sign can alternate
            continue
        out.append((x, ((Q - u) if len(out) & 1 else u, v)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def mont_plant(seed=0x4D504C54):
    """(scalars, points, planted units): point j at unit w * 1024 + l (w = j // 64, l = j % 64), the identity (denominator 0, replaced by 1)
    at the lane's other fifteen units w * 1024 + l + 64 s; the unused lanes of the last wave hold random points.  Lane (w, l) of
    k_varbase_mont_x1 then inverts exactly x * 1^15.  Scalars cycle through 1, 2, r - 1 and seeded full-width patterns."""
    from util import rand_points

    pts = mont_points()
    waves = (len(pts) + 63) // 64
    n = waves * MONT_WAVE_UNITS
    P = np.repeat(arr64([J.AFFINE_IDENTITY]), n, axis=0)
    units = np.array([(j // 64) * MONT_WAVE_UNITS + j % 64 for j in range(len(pts))], dtype=np.int64)
    P[units] = arr64([pt for _, pt in pts])
    spare = [(waves - 1) * MONT_WAVE_UNITS + l + 64 * s for l in range(len(pts) - 64 * (waves - 1), 64) for s in range(MONT_X1_UNITS)]
    if spare:
        P[spare] = rand_points(seed, len(spare))
    rng = np.random.default_rng(seed)
    S = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    for k, s in enumerate((1, 2, R - 1)):
        S[k::4] = b32(s)
    return S, P, units


# ------------------------------------------------------------------------------------------------------------------ points
@functools.lru_cache(maxsize=None)
def points():
    """A: the eight torsion points, G, -G, a point S of prime order, S + t for every torsion point t, two random points of the full group"""
    from util import rand_points, to_pt

    tors = [to_pt(r) for r in B.torsion_points()]
    S = J.scalar_mul_fast(J.GENERATOR, 8 * 0x5EED5EED5EED)
    pts = tors + [J.GENERATOR, J.affine_neg(J.GENERATOR)] + [J.affine_add_fast(S, t) for t in tors] + [to_pt(r) for r in rand_points(0x41, 2)]
    assert len(set(pts)) == len(pts)
    return arr64(pts)


def point_pairs():
    """all ordered pairs A x A"""
    A = points()
    n = len(A)
    return np.repeat(A, n, axis=0), np.tile(A, (n, 1))
