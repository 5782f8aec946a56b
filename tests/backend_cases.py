"""
Cases for the three pieces of shared code behind almost every result: k_normalize<4|16|32|64> (normalize_launch, jj_abi.hip), the
sum tree (sum_reduce / k_sum_pass<32>) and fq_sqrt_fast.  Plain data and constructors (numpy, the oracle, Python integers): no GPU
import.  tests/test_backend_cases_cpu.py pins the tables below to the source and shows that the cases are what they say;
tests/test_gpu_backend_matrix.py runs them through the kernels.
"""
import functools

import numpy as np

from oracle import jubjub_ref as J
from util import arr32, arr64, b32

Q = J.Q
M256 = (1 << 256) - 1

# ------------------------------------------------------------------------------------------------------------- normaliser
LANES_PER_CU = 512                                         # lanes_wanted = cus * 64 * 8
NORM_TABLE = ((128, 64), (32, 32), (4, 16))                # n >= multiplier * lanes -> CHUNK, first match; below all of them: 4
NORM_SMALL = (1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257, 1023, 1024, 1025)


def norm_chunk(n, lanes):
    """CHUNK of the k_normalize launch normalize_launch picks (jj_abi.hip)"""
    for mult, chunk in NORM_TABLE:
        if n >= mult * lanes:
            return chunk
    return 4


def _norm_specs():
    """(variant, multiplier, offset): n = multiplier * lanes + offset takes k_normalize<variant> on any device (lanes >= 512)"""
    specs = [(4, 0, n) for n in NORM_SMALL]
    below = 4
    for mult, chunk in sorted(NORM_TABLE):
        specs += [(below, mult, -1), (chunk, mult, 0), (chunk, mult, chunk // 2 + 1)]      # T - 1, T, a short last lane
        below = chunk
    return tuple(specs)


NORM_SPECS = _norm_specs()
NORM_RAGGED = ((4, 0, 1025),) + tuple(s for s in NORM_SPECS if s[1] and s[2] > 0)          # one size per variant, n % CHUNK != 0


def norm_spec_id(spec):
    chunk, mult, off = spec
    return "k_normalize<%d>-%s" % (chunk, "%dxlanes%+d" % (mult, off) if mult else "n%d" % off)


def norm_sizes(lanes):
    return [mult * lanes + off for _, mult, off in NORM_SPECS]


def plant_positions(n, T, chunk):
    """the scheme of _plant (tests/test_gpu_planner.py): lanes 0, 1, 2, T // 2, T - 2 at positions 0, chunk // 2, chunk - 1, and the
    whole groups of lanes 3, T // 3 and T - 1 (the ragged last lane); element j of lane t is row t + j * T"""
    idx = set()
    for t in {0, 1, 2, T // 2, T - 2}:
        for j in {0, chunk // 2, chunk - 1}:
            if 0 <= t and t + j * T < n:
                idx.add(t + j * T)
    for t in {3, T // 3, T - 1}:
        idx.update(t + j * T for j in range(chunk) if 0 <= t < T and t + j * T < n)
    return np.array(sorted(idx), dtype=np.int64)


def _rnd(rng):
    return int.from_bytes(rng.bytes(32), "little")


def _k_z(z):
    return lambda rng: (_rnd(rng), _rnd(rng), z)


def _k_plus_q(rng):
    u, v, z = _rnd(rng) % Q, _rnd(rng) % Q, 1 + _rnd(rng) % (Q - 1)
    return (u + Q if u + Q <= M256 else u, v + Q if v + Q <= M256 else v, z)


def _k_id(sign):
    def make(rng):
        z = 1 + _rnd(rng) % (Q - 1)
        return (0, (sign * z) % Q, z)
    return make


# (name, Z is 0 mod q, rng -> (U, V, Z) as 256-bit integers)
norm_kinds = (
    ("Z=0", True, _k_z(0)),
    ("Z=q", True, _k_z(Q)),
    ("Z=1", False, _k_z(1)),
    ("Z=q+1", False, _k_z(Q + 1)),
    ("Z=q-1", False, _k_z(Q - 1)),
    ("U+q,V+q", False, _k_plus_q),
    ("(0,z,z)", False, _k_id(1)),
    ("(0,-z,z)", False, _k_id(-1)),
    ("all-ones", False, lambda rng: (M256, M256, M256)),
    ("off-curve", False, lambda rng: (_rnd(rng), _rnd(rng), _rnd(rng))),
)
_ZERO_KINDS = tuple(k for k, kind in enumerate(norm_kinds) if kind[1])


def norm_plant(n, T, chunk, seed):
    """(rows, kind of each row, ext160 of each row, {"all-zero": lane, "one-nonzero": lane} or {}): the norm_kinds cycled over
    plant_positions; where the lanes are apart (T >= 16) every Z of lane 3 is zero, so that its shared product is the empty one, and
    every Z of lane T // 3 but the middle one"""
    rng = np.random.default_rng(seed)
    idx = plant_positions(n, T, chunk)
    kinds = {int(i): (a + n) % len(norm_kinds) for a, i in enumerate(idx)}
    groups = {}
    if T >= 16:
        for name, t in (("all-zero", 3), ("one-nonzero", T // 3)):
            rows = [t + j * T for j in range(chunk) if t + j * T < n]
            for a, i in enumerate(rows):
                kinds[i] = _ZERO_KINDS[a % len(_ZERO_KINDS)]
            if name == "one-nonzero":
                kinds[rows[len(rows) // 2]] = 9
            groups[name] = t
    kind = np.array([kinds[int(i)] for i in idx])
    ext = np.frombuffer(rng.bytes(160 * len(idx)), np.uint8).reshape(-1, 160).copy()       # T1, T2: random bytes, never read
    for a, k in enumerate(kind):
        for c, x in enumerate(norm_kinds[k][2](rng)):
            ext[a, 32 * c: 32 * c + 32] = b32(x)
    return idx, kind, ext, groups


def bad_encodings(count, seed):
    """count x 32 bytes that decode to (0, 0), in turn: v >= q, u^2 a non-square, u = 0 with the sign bit set (v = 1, v = q - 1:
    rejected under ZIP-216), all ones"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        kind = len(out) % 5
        sign = int(rng.integers(0, 2)) << 255
        if kind == 0:
            out.append((Q + int(rng.integers(0, 1 << 30))) | sign)
        elif kind == 1:
            v = _rnd(rng) % Q
            u2 = (v * v - 1) * pow(1 + J.EDWARDS_D * v * v, -1, Q) % Q
            if pow(u2, (Q - 1) // 2, Q) == Q - 1:
                out.append(v | sign)
        elif kind == 2:
            out.append(1 | (1 << 255))
        elif kind == 3:
            out.append((Q - 1) | (1 << 255))
        else:
            out.append(M256)
    return arr32(out)


def ext160_to_ints(row):
    return tuple(int.from_bytes(bytes(row[32 * c: 32 * c + 32]), "little") for c in range(5))


# --------------------------------------------------------------------------------------------------------------- sum tree
SUM_FOLD = 32                                              # FOLD of sum_reduce
sum_sizes = (1, 2, 31, 32, 33, 1023, 1024, 1025, 32767, 32768, 32769, 1048575, 1048577)
SUM_LAYOUTS = ("planted", "to-identity", "all-identity", "same-point")


def sum_passes(n):
    """the sizes of the passes of sum_reduce: n -> ceil(n / 32) until one point is left"""
    out = []
    while n > 1:
        out.append(n)
        n = (n + SUM_FOLD - 1) // SUM_FOLD
    return out


@functools.lru_cache(maxsize=None)
def torsion_points():
    """the eight points of order dividing 8 (the identity first)"""
    g8 = J.scalar_mul_fast(J.GENERATOR, J.R_MOD)
    pts = [J.AFFINE_IDENTITY] + [J.scalar_mul_fast(g8, k) for k in range(1, 8)]
    assert len(set(pts)) == 8 and J.scalar_mul_fast(g8, 8) == J.AFFINE_IDENTITY
    return arr64(pts)


@functools.lru_cache(maxsize=None)
def sum_pool():
    """1021 points of the full group and their negations (a prime count: the tiling never lines up with the lanes)"""
    from oracle import c_oracle as O
    from util import rand_points

    P = rand_points(0x53554D, 1021)
    return P, O.point_op("neg", P)


def sum_layout(n, layout):
    """n x 64 bytes.  planted: pool points with the identity and the torsion points at the first and the last unit and on both
    sides of every lane boundary of the first pass (rows j * T - 1, j * T), and pairs P, -P at rows i, i + T (T = ceil(n / 32)): lane i
    passes through the identity in the middle of its fold.  to-identity: rows i and i + n // 2 cancel, an odd last row is the
    identity.  all-identity, same-point: one row repeated."""
    P, N = sum_pool()
    ident = arr64([J.AFFINE_IDENTITY])
    if layout == "all-identity":
        return np.repeat(ident, n, axis=0)
    if layout == "same-point":
        return np.repeat(P[:1], n, axis=0)
    if layout == "to-identity":
        h = n // 2
        pick = np.arange(h) % len(P)
        return np.concatenate([P[pick], N[pick], np.repeat(ident, n - 2 * h, axis=0)])
    assert layout == "planted"
    out = P[(np.arange(n) * 7) % len(P)].copy()
    T = (n + SUM_FOLD - 1) // SUM_FOLD
    for i in {2, 5, T // 2, T - 3}:
        for j in (0, 7, 29):                                                     # rows j and j + 1 of lane i
            if 0 <= i < T and i + (j + 1) * T < n:
                out[i + j * T] = P[(i + j) % len(P)]
                out[i + (j + 1) * T] = N[(i + j) % len(P)]
    spots = {0, 1, n - 2, n - 1}
    for j in range(1, SUM_FOLD):
        spots.update((j * T - 1, j * T))
    special = np.concatenate([ident, torsion_points()])
    for a, i in enumerate(sorted(s for s in spots if 0 <= s < n)):
        out[i] = special[a % len(special)]
    return out


# ---------------------------------------------------------------------------------------------------------------- Fq root
FQ_S = 32
FQ_T = (Q - 1) >> FQ_S                                     # q - 1 = 2^32 t
FQ_G = pow(7, FQ_T, Q)                                     # the generator of the 2^32-torsion fq_sqrt_fast takes logs to
_T_INV = pow(FQ_T, -1, 1 << FQ_S)


@functools.lru_cache(maxsize=None)
def sqrt_patterns():
    """the logs e of a^t = g^e: every digit value alone in every digit, the borrows of e >> 1 across the digit boundaries, 64 random"""
    es = [d << (8 * i) for i in range(4) for d in range(1, 256)]
    es += [0, 1, 2, 0xFF, 0x100, 0x101, 0xFFFF, 0x10000, 0xFF00, 0x100FE, 0x00FF00FE, 1 << 24, 0xFE000000, 1 << 31, (1 << 32) - 2,
           (1 << 32) - 1]
    es += [int(x) for x in np.random.default_rng(0x53515254).integers(0, 1 << 32, size=64, dtype=np.uint64)]
    return tuple(dict.fromkeys(es))


def fq_with_log(e, seed):
    """a with a^t = g^e: g^(e t^-1 mod 2^32) times a 2^32-th power"""
    c = 1 + int.from_bytes(np.random.default_rng([seed, e]).bytes(32), "little") % (Q - 1)
    return pow(FQ_G, (e * _T_INV) % (1 << FQ_S), Q) * pow(c, 1 << FQ_S, Q) % Q


def _sqrt_any(a):
    """a root of a square a (Tonelli-Shanks on Python integers, either sign), None for a non-square"""
    if a == 0:
        return 0
    if pow(a, (Q - 1) // 2, Q) != 1:
        return None
    x, b, g, r = pow(a, (FQ_T + 1) // 2, Q), pow(a, FQ_T, Q), FQ_G, FQ_S
    while b != 1:
        m, t = 0, b
        while t != 1:
            t, m = t * t % Q, m + 1
        c = pow(g, 1 << (r - m - 1), Q)
        x, g, r = x * c % Q, c * c % Q, m
        b = b * g % Q
    assert x * x % Q == a
    return x


def encoding_with_u2(a, sign):
    """the encoding (an integer: v with the sign bit on top) whose decoder takes the root of exactly a = (v^2 - 1) / (1 + d v^2):
    v^2 = (1 + a) / (1 - d a).  None when the right-hand side is a non-square or 1 - d a == 0"""
    den = (1 - J.EDWARDS_D * a) % Q
    if den == 0:
        return None
    v = _sqrt_any((1 + a) * pow(den, -1, Q) % Q)
    if v is None:
        return None
    assert (v * v - 1) * pow(1 + J.EDWARDS_D * v * v, -1, Q) % Q == a
    return v | (sign << 255)


@functools.lru_cache(maxsize=None)
def sqrt_cases():
    """(e, a, encoding or None) per pattern: as many seeds as it takes to find an a with an encoding (64 at the most)"""
    out = []
    for k, e in enumerate(sqrt_patterns()):
        a, enc = fq_with_log(e, 0), None
        for seed in range(64):
            a = fq_with_log(e, seed)
            enc = encoding_with_u2(a, (k + seed) & 1)
            if enc is not None:
                break
        out.append((e, a, enc))
    return tuple(out)


def sqrt_inputs():
    """(A, E): the a of every pattern and the encodings, 32 bytes each, in the order of sqrt_patterns()"""
    cases = sqrt_cases()
    return arr32([a for _, a, _ in cases]), arr32([enc for _, _, enc in cases if enc is not None])
