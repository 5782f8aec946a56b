"""Cases of the windowed Pedersen hash (jj_pedersen_table_create, jj_pedersen_hash_vartime, jj_pedersen_scalars) and the restatement of the
function on the oracle's point arithmetic.  Nothing here runs the library; everything is seeded and small.  Test infrastructure only.

The function (include/jubjub_hip.h): the message bits M -- a prefix, then the fields of the unit's row, LSB-first within a byte -- are padded
with zero bits to a multiple of 3 and cut into chunks (s0, s1, s2); enc = (1 - 2 s2)(1 + s0 + 2 s1); segment j takes seg_chunks chunks,
<M_j> = sum_i enc(m_i) 16^i, H(M) = sum_j [<M_j>] P_j.  The empty message gives the identity; a chunk that is not there contributes nothing.

Two formulations: expected() multiplies every generator by the integer <M_j> (oracle scalar multiplication, negated for a negative one) and
adds with ext_add; by_chunks() adds [enc 16^i] P_j one chunk at a time from repeated doublings of P_j.  tests/test_pedersen_cases_cpu.py
holds them together over the whole table.

CASES: the Merkle shape (three segments of 63, fields (0, 255), (32, 255) of rows of 64 bytes, a 6-bit prefix), the tiny shape (three segments
of 3 chunks, every message length 0 .. 27 bits: segment ends, window ends and both paddings inside one dword; 27 bits is exactly at capacity),
a one-field shape with row_stride 9 and byte_offset 1 (rows start at every residue modulo 4 and the array ends mid-dword), overlapping fields,
a prefix-only shape, and the twin shape over generators with P_1 = P_0, which plants a message whose halves cancel (H is the identity, u = 0)
and one whose halves are equal (the accumulator meets its own value: the addition is a doubling).  Rows 0 and 1 of every case with fields are
all zero bits (every chunk +1) and all one bits (every chunk -4)."""
import functools

import numpy as np

from oracle import jubjub_ref as J

SIZES = (1, 63, 64, 65, 257)
WINDOWS = (1, 2, 3, 4)
NROWS = max(SIZES)
ENC_TABLE = {(0, 0, 0): 1, (1, 0, 0): 2, (0, 1, 0): 3, (1, 1, 0): 4, (0, 0, 1): -1, (1, 0, 1): -2, (0, 1, 1): -3, (1, 1, 1): -4}      # (s0, s1, s2) -> enc


def enc(s0, s1, s2):
    return (1 - 2 * s2) * (1 + s0 + 2 * s1)


@functools.lru_cache(maxsize=None)
def synth_generators(count):
    """`count` distinct prime-order points (tools/pedersen_ab.py takes four for its four-segment shape)"""
    return tuple(J.synth_point(900 + k, subgroup=True)[0] for k in range(count))


@functools.lru_cache(maxsize=None)
def generators(name):
    """affine generators as integer pairs: three (or the first two) distinct prime-order points, or the planted set with P_1 = P_0"""
    p = synth_generators(3)
    return {"three": (p[0], p[1], p[2]), "two": (p[0], p[1]), "twin": (p[0], p[0]), "one": (p[1],)}[name]


def gens_bytes(name):
    return np.frombuffer(b"".join(u.to_bytes(32, "little") + v.to_bytes(32, "little") for u, v in generators(name)), dtype=np.uint8).reshape(-1, 64).copy()


class Case:
    def __init__(self, id, gens, seg_chunks, row_stride, fields, prefix=0, prefix_bits=0, seed=1, plant=None):
        self.id, self.gens, self.seg_chunks, self.row_stride, self.fields, self.prefix, self.prefix_bits = id, gens, seg_chunks, row_stride, tuple(fields), prefix, prefix_bits
        self.nseg = len(generators(gens))
        self.seed, self.plant = seed, plant
        self.bits_len = prefix_bits + sum(nb for _, nb in self.fields)
        assert self.bits_len <= 3 * seg_chunks * self.nseg and all(nb >= 1 and off + (nb + 7) // 8 <= row_stride for off, nb in self.fields)

    @functools.cached_property
    def rows(self):
        """(NROWS, row_stride) uint8, read-only: row 0 all zero bits, row 1 all one bits, then what the case plants, then seeded random rows"""
        r = np.random.default_rng(7000 + self.seed).integers(0, 256, size=(NROWS, max(self.row_stride, 1)), dtype=np.uint8)
        r[0], r[1] = 0, 0xFF
        if self.plant:
            self.plant(r)
        r.setflags(write=False)
        return r

    def bits(self, i):
        """the message bits of unit i"""
        out = [(self.prefix >> k) & 1 for k in range(self.prefix_bits)]
        row = self.rows[i]
        for off, nb in self.fields:
            out += [(int(row[off + (k >> 3)]) >> (k & 7)) & 1 for k in range(nb)]
        return out


def chunks_of(bits):
    b = list(bits) + [0] * (-len(bits) % 3)
    return [enc(b[k], b[k + 1], b[k + 2]) for k in range(0, len(b), 3)]


def segment_sums(seg_chunks, nseg, bits):
    """[<M_0>, .., <M_{nseg-1}>] as integers; 0 for a segment the message does not reach"""
    ch = chunks_of(bits)
    assert len(ch) <= seg_chunks * nseg
    return [sum(e * 16 ** i for i, e in enumerate(ch[j * seg_chunks:(j + 1) * seg_chunks])) for j in range(nseg)]


@functools.lru_cache(maxsize=1 << 16)
def _mul(p, k):
    q = J.scalar_mul_fast(p, abs(k))
    return J.affine_neg(q) if k < 0 else q


def expected(gs, seg_chunks, bits):
    """H(M) as an affine integer pair: every generator times the integer <M_j>, summed with ext_add"""
    acc = J.EXT_IDENTITY
    for p, m in zip(gs, segment_sums(seg_chunks, len(gs), bits)):
        if m:
            acc = J.ext_add(acc, J.affine_to_extended(_mul(p, m)))
    return J.ext_to_affine(acc)


@functools.lru_cache(maxsize=None)
def _powers(p, count):
    """[e 16^i] p for i < count, e = 1 .. 4, as extended points, by doublings and additions alone"""
    out, base = [], J.affine_to_extended(p)
    for _ in range(count):
        two = J.ext_double(base)
        three = J.ext_add(two, base)
        four = J.ext_double(two)
        out.append((base, two, three, four))
        base = J.ext_double(J.ext_double(four))
    return out


def by_chunks(gs, seg_chunks, bits):
    """the second formulation: one chunk at a time"""
    acc = J.EXT_IDENTITY
    for k, e in enumerate(chunks_of(bits)):
        j, i = divmod(k, seg_chunks)
        term = _powers(gs[j], seg_chunks)[i][abs(e) - 1]
        acc = J.ext_add(acc, J.ext_neg(term) if e < 0 else term)
    return J.ext_to_affine(acc)


def point_bytes(p):
    return np.frombuffer(p[0].to_bytes(32, "little") + p[1].to_bytes(32, "little"), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _expected_points(case_id):
    c = BY_ID[case_id]
    out = np.stack([point_bytes(expected(generators(c.gens), c.seg_chunks, c.bits(i))) for i in range(NROWS)])
    out.setflags(write=False)
    return out


def expected_points(case, n):
    """(n, 64) affine bytes of the first n units; computed once per case for all sizes"""
    return _expected_points(case.id)[:n]


def expected_scalars(case, n):
    """(nseg, n, 32): <M_j> mod r as canonical bytes"""
    out = np.zeros((case.nseg, n, 32), np.uint8)
    for i in range(n):
        for j, m in enumerate(segment_sums(case.seg_chunks, case.nseg, case.bits(i))):
            out[j, i] = np.frombuffer((m % J.R_MOD).to_bytes(32, "little"), dtype=np.uint8)
    return out


# ---- planted rows of the twin shape: two segments of 63 chunks over P_1 = P_0, one field of 378 bits in rows of 48 bytes
TWIN_BITS = 2 * 63 * 3


def _set_bits(row, bits):
    row[:] = 0
    for k, b in enumerate(bits):
        row[k >> 3] |= b << (k & 7)


def _plant_twin(r):
    half = [int(b) for b in np.random.default_rng(7777).integers(0, 2, size=189)]
    mirror = [b ^ 1 if k % 3 == 2 else b for k, b in enumerate(half)]          # every chunk's sign flipped: <M_1> = -<M_0>
    _set_bits(r[2], half + mirror)                                             # the halves cancel: the identity
    _set_bits(r[3], half + half)                                               # the halves are equal: acc + acc


TWIN_CANCEL_ROW, TWIN_EQUAL_ROW = 2, 3
MERKLE_FIELDS = ((0, 255), (32, 255))

CASES = [
    Case("merkle", "three", 63, 64, MERKLE_FIELDS, prefix=0b100101, prefix_bits=6, seed=1),
    Case("twin", "twin", 63, 48, ((0, TWIN_BITS),), seed=2, plant=_plant_twin),
    Case("one_field_stride9", "one", 63, 9, ((1, 61),), seed=3),
    Case("overlap", "three", 5, 8, ((0, 17), (1, 9), (0, 13), (6, 5)), prefix=0x5, prefix_bits=1, seed=4),      # 45 bits: exactly the capacity of three segments of 5
    Case("five_pieces", "one", 4, 4, ((0, 3), (1, 2), (2, 4), (3, 1)), prefix=1, prefix_bits=1, seed=7),          # one window of 12 bits from the prefix and four fields
    Case("prefix_only", "three", 4, 1, (), prefix=0xDEADBEEF, prefix_bits=32, seed=5),
    Case("empty", "three", 63, 1, (), seed=6),
]
# the tiny shape: three segments of 3 chunks, one field of L bits at byte 1 of rows of 5 bytes (the units start at every residue modulo 16)
TINY_STRIDE, TINY_OFFSET = 5, 1
TINY = [Case("tiny_%02d" % L, "three", 3, TINY_STRIDE, ((TINY_OFFSET, L),) if L else (), seed=100 + L) for L in range(28)]
CASES += TINY
BY_ID = {c.id: c for c in CASES}
