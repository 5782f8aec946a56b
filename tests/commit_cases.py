"""Cases of the windowed Pedersen commitment (jj_pedersen_commit_vartime) and its restatement on the oracle's point arithmetic.  Nothing here
runs the library; everything is seeded and small.  Test infrastructure only.

The function (include/jubjub_hip.h): out = H(M) + [r mod 2^252] R, H the hash of tests/pedersen_cases.py, M a prefix followed by up to four
fields (src, byte_offset, nbits) that lie in up to four row arrays of their own strides, r 32 raw bytes of which the low 252 bits count.

Two formulations: expected() is pedersen_cases.expected() plus the oracle's scalar multiplication of R; by_chunks() is pedersen_cases.by_chunks()
plus a double-and-add over the 252 bits of r.  tests/test_commit_cases_cpu.py holds them together.

CASES: the note shape (four segments of 63, sources of stride 52, 32, 32, a 6-bit prefix: 582 bits, the last segment holds 5 chunks; at most
65 units, five big-integer ladders each); the tiny shapes (three segments of 3 chunks, sources of stride 5, 3 and 9 read at byte 1, 0 and 2:
every source's rows start at every residue modulo 4 and every array ends mid-dword; `tiny3_two` has windows with pieces of two sources and is
exactly at capacity, `tiny3_three` a window with pieces of three sources and a padded last chunk, `tiny3_padded` two padding bits); fields in
the order source 1, 0, 1 with the two fields of source 1 overlapping; the twin shape with R = P_0 and planted r = -<M_0> (the identity) and
r = <M_0> (the sum meets its own value); the hash-only form; one source, which must equal jj_pedersen_hash_vartime.  In every case rows 0 and 1
of every source are all zero bits and all one bits, and r of units 0..5 is 0, 1, r - 1, r, 2^252 - 1 and thirty-two 0xFF bytes."""
import functools

import numpy as np

from oracle import jubjub_ref as J
from tests import pedersen_cases as PC

SIZES = (1, 63, 64, 65, 257)
WINDOWS = PC.WINDOWS
R_EDGES = (0, 1, J.R_MOD - 1, J.R_MOD, (1 << 252) - 1, (1 << 256) - 1)
TWIN_CANCEL_ROW, TWIN_EQUAL_ROW = 6, 7
NOTE_FIELDS = ((0, 12, 64), (1, 0, 256), (2, 0, 256))
NOTE_PREFIX, NOTE_PREFIX_BITS = 0b111111, 6


@functools.lru_cache(maxsize=None)
def bases():
    """R of the cases: a prime-order point that is no generator of theirs; and P_0 for the twin shape"""
    return {"R": J.synth_point(950, subgroup=True)[0], "P0": PC.synth_generators(4)[0]}


def gens_of(name):
    p = PC.synth_generators(4)
    return {"four": p, "three": p[:3], "one": p[:1]}[name]


def gens_bytes(name):
    return np.stack([PC.point_bytes(g) for g in gens_of(name)]).copy()


class Case:
    def __init__(self, id, gens, seg_chunks, strides, fields, prefix=0, prefix_bits=0, seed=1, rbase="R", nrows=max(SIZES), plant=None):
        self.id, self.gens, self.seg_chunks, self.strides, self.fields = id, gens, seg_chunks, tuple(strides), tuple(fields)
        self.prefix, self.prefix_bits, self.seed, self.rbase, self.nrows, self.plant = prefix, prefix_bits, seed, rbase, nrows, plant
        self.nseg = len(gens_of(gens))
        self.bits_len = prefix_bits + sum(nb for _, _, nb in self.fields)
        self.sizes = tuple(n for n in SIZES if n <= nrows)
        assert self.bits_len <= 3 * seg_chunks * self.nseg
        assert all(s < len(self.strides) and nb >= 1 and off + (nb + 7) // 8 <= self.strides[s] for s, off, nb in self.fields)

    @functools.cached_property
    def data(self):
        """(sources, r): sources[s] is (nrows, stride_s) uint8, r is (nrows, 32) uint8, read-only"""
        rng = np.random.default_rng(9000 + self.seed)
        srcs = [rng.integers(0, 256, size=(self.nrows, st), dtype=np.uint8) for st in self.strides]
        for a in srcs:
            a[0], a[1] = 0, 0xFF
        r = rng.integers(0, 256, size=(self.nrows, 32), dtype=np.uint8)
        for i, v in enumerate(R_EDGES[:self.nrows]):
            r[i] = np.frombuffer(v.to_bytes(32, "little"), dtype=np.uint8)
        if self.plant:
            self.plant(self, srcs, r)
        for a in srcs + [r]:
            a.setflags(write=False)
        return tuple(srcs), r

    @property
    def sources(self):
        return self.data[0]

    @property
    def r(self):
        return self.data[1]

    def bits_of(self, srcs, i):
        out = [(self.prefix >> k) & 1 for k in range(self.prefix_bits)]
        for s, off, nb in self.fields:
            row = srcs[s][i]
            out += [(int(row[off + (k >> 3)]) >> (k & 7)) & 1 for k in range(nb)]
        return out

    def bits(self, i):
        """the message bits of unit i"""
        return self.bits_of(self.sources, i)

    def r_int(self, i):
        """the blinding scalar of unit i as the library reads it: the low 252 bits"""
        return int.from_bytes(self.r[i].tobytes(), "little") & ((1 << 252) - 1)

    def packed(self, n):
        """the composed route's input: (rows (n, stride), pairs (byte_offset, nbits)) with every field's bytes copied side by side"""
        cols, pairs, at = [], [], 0
        for s, off, nb in self.fields:
            w = (nb + 7) // 8
            cols.append(self.sources[s][:n, off:off + w])
            pairs.append((at, nb))
            at += w
        rows = np.concatenate(cols, axis=1) if cols else np.zeros((n, 1), np.uint8)
        return np.ascontiguousarray(rows), tuple(pairs)


def expected(case, i):
    """H(M_i) + [r_i mod 2^252] R as an affine integer pair"""
    h = J.affine_to_extended(PC.expected(gens_of(case.gens), case.seg_chunks, case.bits(i)))
    if case.rbase is None:
        return J.ext_to_affine(h)
    return J.ext_to_affine(J.ext_add(h, J.affine_to_extended(J.scalar_mul_fast(bases()[case.rbase], case.r_int(i)))))


def by_chunks(case, i):
    """the second formulation: the message one chunk at a time, the blinding term bit by bit from the top"""
    acc = J.affine_to_extended(PC.by_chunks(gens_of(case.gens), case.seg_chunks, case.bits(i)))
    if case.rbase is None:
        return J.ext_to_affine(acc)
    base, t, k = J.affine_to_extended(bases()[case.rbase]), J.EXT_IDENTITY, case.r_int(i)
    for b in range(251, -1, -1):
        t = J.ext_double(t)
        if (k >> b) & 1:
            t = J.ext_add(t, base)
    return J.ext_to_affine(J.ext_add(acc, t))


@functools.lru_cache(maxsize=None)
def _expected_points(case_id):
    c = BY_ID[case_id]
    out = np.stack([PC.point_bytes(expected(c, i)) for i in range(c.nrows)])
    out.setflags(write=False)
    return out


def expected_points(case, n):
    """(n, 64) affine bytes of the first n units; computed once per case for all sizes"""
    return _expected_points(case.id)[:n]


def _plant_twin(case, srcs, r):
    """R = P_0 and one segment: unit TWIN_CANCEL_ROW gets r = -<M_0> (H(M) + [r]R is the identity), unit TWIN_EQUAL_ROW r = <M_0>"""
    for row, sign in ((TWIN_CANCEL_ROW, -1), (TWIN_EQUAL_ROW, 1)):
        m = PC.segment_sums(case.seg_chunks, 1, case.bits_of(srcs, row))[0]
        v = (sign * m) % J.R_MOD
        assert v < 1 << 252
        r[row] = np.frombuffer(v.to_bytes(32, "little"), dtype=np.uint8)


TINY_STRIDES = (5, 3, 9)
REORDERED = dict(gens="three", seg_chunks=5, strides=(8, 6), fields=((1, 0, 13), (0, 2, 17), (1, 1, 9)), prefix=1, prefix_bits=1)       # 40 of 45 bits
CASES = [
    Case("note", "four", 63, (52, 32, 32), NOTE_FIELDS, prefix=NOTE_PREFIX, prefix_bits=NOTE_PREFIX_BITS, seed=1, nrows=65),
    Case("tiny3_two", "three", 3, TINY_STRIDES, ((0, 1, 7), (1, 0, 5), (2, 2, 15)), seed=2),           # 27 bits, at capacity: windows of sources 0+1 and 1+2
    Case("tiny3_three", "three", 3, TINY_STRIDES, ((0, 1, 2), (1, 0, 3), (2, 2, 20)), seed=3),         # 25 bits: the first window reads three sources, the last chunk is padded
    Case("tiny3_padded", "three", 3, TINY_STRIDES, ((0, 1, 7), (1, 0, 5), (2, 2, 11)), seed=4),        # 23 bits: one padding bit, the third segment holds two chunks
    Case("reordered", seed=5, **REORDERED),
    Case("twin", "one", 63, (24,), ((0, 0, 189),), seed=6, rbase="P0", plant=_plant_twin),
    Case("hash_only", seed=7, rbase=None, **REORDERED),
    Case("one_source", "three", 5, (8,), ((0, 0, 17), (0, 1, 9), (0, 0, 13), (0, 6, 5)), prefix=0x5, prefix_bits=1, seed=8, rbase=None),
]
BY_ID = {c.id: c for c in CASES}
