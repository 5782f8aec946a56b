"""Signature arrays cut into SEGMENTS for jj_sigbatch_ragged, and the verdict row the call must write for each segment.  Plain data (numpy + the
oracle, no GPU import); tests/test_sig_seg_cases_cpu.py pins every expected row to the oracle, tests/test_gpu_sig_seg.py runs the same cases through
the C ABI.  Test infrastructure only.

A case is the concatenation of sig_batch_cases.batch(L, variant, k) per segment over one base; row g is that batch's own `.expected`, which is the
contract: out64[g] = what jj_sigbatch_begin + jj_msm_finish write for segment g alone.  Segments of equal length hold equal signatures (the batches
are seeded by their size), so the planted cases put their variants where a mix-up of segments would show.
The layout the kernels use (restated here for the brute-force model of the CPU tests):
  segment g owns terms T_g = 2 offsets[g] + g .. T_g + 2 L_g:  R terms | A terms | the term of B;
  k_sig_seg_terms leaves a partial sum of z_i s_i at every run head: offsets[g] and the multiples of 64 strictly inside the segment."""
import functools

import numpy as np

from oracle import c_oracle as O
from tests import sig_batch_cases as SC

R = SC.R
WAVE = 64
JOB_TERMS = 8192                                  # a segment of more terms (2 L + 1) leaves the ragged kernels for an MSM job of its own


class Seg:
    """one call's arguments (host arrays) + the (S, 64) rows it must write"""

    def __init__(self, name, parts, flags=None):
        self.name, self.parts = name, list(parts)
        assert self.parts and len({bytes(p.base) for p in self.parts}) == 1, "one base per call"
        self.base = self.parts[0].base
        self.flags = max(p.flags for p in self.parts) if flags is None else flags
        assert all(p.flags == self.flags or bytes(p.expected) == bytes(SC.IDENTITY) for p in self.parts)
        assert not (self.flags and any("noncanonical_a " in p.name for p in self.parts)), "accepted only without ZIP-216"
        cat = lambda xs, w: np.concatenate(xs) if sum(len(x) for x in xs) else np.zeros((0, w), np.uint8)      # noqa: E731
        self.r, self.a, self.s, self.c = (cat([getattr(p, f) for p in self.parts], 32) for f in "rasc")
        self.z = cat([p.z for p in self.parts], 16)
        self.offsets = np.concatenate([[0], np.cumsum([p.n for p in self.parts])]).astype(np.uint64)
        self.expected = np.stack([p.expected for p in self.parts])

    @property
    def n(self):
        return len(self.s)

    @property
    def S(self):
        return len(self.parts)

    def sizes(self):
        return [p.n for p in self.parts]

    def arrays(self):
        return self.r, self.a, self.s, self.c, self.z

    def slice(self, g):
        """segment g as the batch jj_sigbatch_begin takes, cut out of the concatenated arrays"""
        lo, hi = int(self.offsets[g]), int(self.offsets[g + 1])
        return SC.Batch("%s [segment %d]" % (self.name, g), self.base, self.r[lo:hi], self.a[lo:hi], self.s[lo:hi], self.c[lo:hi], self.z[lo:hi], self.flags, self.expected[g])


def term_offsets(offsets):
    """the CSR offsets of the S sums: 2 offsets[g] + g"""
    return [2 * int(o) + g for g, o in enumerate(offsets)]


def heads(offsets):
    """per segment: its run heads -- the segment's first signature and every multiple of 64 strictly inside it"""
    o = [int(x) for x in offsets]
    return [([lo] + [m for m in range((lo // WAVE + 1) * WAVE, hi, WAVE)]) if hi > lo else [] for lo, hi in zip(o[:-1], o[1:])]


def layout(name, sizes, planted=(), variant="valid", flags=None):
    """segments of the given sizes, each `variant` ("valid", "order8r", "c_plus_r") except the planted ones: {segment: (variant, position)}"""
    planted = dict(planted)
    return Seg(name, [SC.batch(L, *planted[g]) if g in planted else SC.batch(L, variant) for g, L in enumerate(sizes)], flags)


def two_in_one(L, k_reject, k_malformed):
    """one batch of L signatures with a reject unit (bad_s) AND a malformed one (off_curve_r): malformed wins"""
    a, b = SC.batch(L, "bad_s", k_reject), SC.batch(L, "off_curve_r", k_malformed)
    return SC.Batch("bad_s k=%d + off_curve_r k=%d n=%d" % (k_reject, k_malformed, L), a.base, b.r, a.a, a.s, a.c, a.z, 0, SC.MALFORMED)


@functools.lru_cache(maxsize=None)
def geometric_sizes(S=64, mean=8, seed=0x5E6):
    rng = np.random.default_rng(seed)
    return tuple(int(x) - 1 for x in rng.geometric(1.0 / (mean + 1), S))      # lengths 0, 1, 2, ... of mean `mean`


SHAPES = {
    "[5]": [5],
    "[63, 1, 64, 65]": [63, 1, 64, 65],
    "[255, 257]": [255, 257],
    "[256, 256]": [256, 256],
    "[600]": [600],
    "300 x [1]": [1] * 300,
    "[0, 7, 0, 0, 9, 0]": [0, 7, 0, 0, 9, 0],
    "[0, 0, 0]": [0, 0, 0],
    "[4095, 3]": [4095, 3],
    "[3, 4096, 2]": [3, 4096, 2],
}
PLANT = (7, 130, 3)                               # the planted segment is the middle one: signatures 7 .. 136, the wave edge 63 | 64 at its positions 56 | 57
PLANT_POSITIONS = (0, 56, 57, 129)
POSITIONED = ("torsion_r", "bad_s", "bad_r", "s_plus_r", "off_curve_r", "noncanonical_a_zip216", "noncanonical_a")


def shape_cases():
    out = [layout("valid " + name, sizes) for name, sizes in SHAPES.items()]
    out.append(layout("valid geometric, S = 64", geometric_sizes()))
    out.append(layout("valid [63, 1, 64, 65], ZIP-216", [63, 1, 64, 65], flags=SC.ZIP216))
    out.append(layout("order8r base [5, 64, 0, 3]", [5, 64, 0, 3], variant="order8r"))
    out.append(layout("c_plus_r [63, 1, 64, 65]", [63, 1, 64, 65], variant="c_plus_r"))
    return out


def planted_cases():
    out = []
    for v in POSITIONED:
        for k in PLANT_POSITIONS:
            out.append(layout("%s at %d of the middle segment of %r" % (v, k, list(PLANT)), PLANT, {1: (v, k)}))
        out.append(layout("%s in segment 2 of five segments of one" % v, [1] * 5, {2: (v, 0)}))
    out += [
        layout("two failures in two segments", [20, 30, 40], {0: ("bad_s", 19), 2: ("off_curve_r", 0)}),
        layout("two rejects in neighbouring segments", [64, 64, 64], {0: ("bad_r", 63), 1: ("bad_s", 0)}),
        Seg("a malformed and a reject unit in one segment", [SC.batch(9), two_in_one(70, 3, 66), SC.batch(9)]),
        Seg("a reject and a malformed unit in one segment, the other order", [SC.batch(2), two_in_one(70, 65, 0)]),
        layout("300 x [1], failures at segments 0, 63, 64, 255, 256, 299", [1] * 300, {0: ("bad_s", 0), 63: ("off_curve_r", 0), 64: ("bad_r", 0), 255: ("s_plus_r", 0), 256: ("bad_s", 0), 299: ("bad_r", 0)}),
        layout("[0, 7, 0, 0, 9, 0], bad s behind the empty segments", [0, 7, 0, 0, 9, 0], {4: ("bad_s", 0)}),
        layout("[255, 257], malformed at the workgroup edge", [255, 257], {1: ("s_plus_r", 1)}),
        layout("[600], bad s in its last wave", [600], {0: ("bad_s", 599)}),
        layout("[4095, 3], bad s at the long segment's end", [4095, 3], {0: ("bad_s", 4094)}),
        layout("[3, 4096, 2], bad r at the job's end", [3, 4096, 2], {1: ("bad_r", 4095)}),
        layout("[3, 4096, 2], malformed in the job, bad s behind it", [3, 4096, 2], {1: ("off_curve_r", 64), 2: ("bad_s", 1)}),
        layout("geometric, S = 64, ZIP-216, a non-canonical key in segment 40", geometric_sizes(), {40: ("noncanonical_a_zip216", 0)}),
    ]
    assert geometric_sizes()[40] > 0
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    return tuple(shape_cases() + planted_cases())


def cleared_evaluation(b):
    """the formulation the device uses, evaluated by the oracle: decode, mul_by_cofactor on every point and on B, the 2n + 1 scalars, O.msm -- and
    NO doublings.  n = 0: the identity."""
    n = b.n
    if n == 0:
        return SC.IDENTITY
    rp, rok = O.decompress(b.r, b.flags)
    ap, aok = O.decompress(b.a, b.flags)
    sv = [SC.to_int(x) for x in b.s]
    bad = not rok.all() or not aok.all() or any(x >= R for x in sv)
    rp, ap = O.point_op("mul_by_cofactor", rp), O.point_op("mul_by_cofactor", ap)
    rp[rok == 0] = SC.IDENTITY
    ap[aok == 0] = SC.IDENTITY
    zv = [SC.to_int(x) for x in b.z]
    cv = [SC.to_int(x) % R for x in b.c]
    sigma = sum(zi * si for zi, si in zip(zv, sv)) % R
    scalars = np.stack([SC.b32(zi) for zi in zv] + [SC.b32(zi * ci % R) for zi, ci in zip(zv, cv)] + [SC.b32((R - sigma) % R)])
    total = O.msm(scalars, np.concatenate([rp, ap, O.point_op("mul_by_cofactor", b.base[None])]))
    return SC.MALFORMED if bad else total


# ---- locate: one batch with several failing signatures planted, and the list Engine.sigbatch_locate must return
LOCATE_N = 1000
LOCATE_FAILURES = {0: "bad_s", 63: "off_curve_r", 64: "bad_s", 511: "bad_r", 999: "bad_s"}


@functools.lru_cache(maxsize=None)
def locate_batch(valid=False):
    """(base, r, a, s, c, z, expected list): LOCATE_N signatures with LOCATE_FAILURES planted the way SC.batch plants them (none when `valid`)"""
    B = SC.bases()["prime"]
    r, a, s, c, z, ki, mi = SC._valid(LOCATE_N, "prime")
    r, s = r.copy(), s.copy()
    want = []
    for k, v in sorted({} if valid else LOCATE_FAILURES.items()):
        if v == "bad_s":
            s[k] = SC.b32((SC.to_int(s[k]) + 5) % R)
        elif v == "bad_r":
            r[k] = O.compress(O.point_op("add", SC._pools("prime")[1][mi[k]][None], SC._mul(0xD15, B)[None]))[0]
        else:
            r[k] = SC.off_curve_encoding()
        want.append((k, "malformed" if v == "off_curve_r" else "reject"))
    for x in (r, s):
        x.setflags(write=False)
    return B, r, a, s, c, z, want


def verdict(row):
    b = bytes(row)
    return "ok" if b == bytes(SC.IDENTITY) else "malformed" if b == bytes(SC.MALFORMED) else "reject"
