"""Units of the two-term ladder a P + b Q that tests/test_emu_straus.py (host emulation) and tests/test_gpu_varbase_mul2.py (C ABI) share: the edge
matrix and the oracle value of a batch.  Test infrastructure only."""
import numpy as np

from oracle import c_oracle as O
from oracle import jubjub_ref as J
from tests.util import EDGE_SCALARS, R, arr32, arr64, rand_points, torsion_points

M256 = (1 << 256) - 1
# edge scalars as 32-byte patterns (bits above 251 are ignored by the ladder and by the oracle alike)
EDGE_KS = [k & M256 for k in EDGE_SCALARS] + [R - 2, 2 * R - 1, 3, 8 * R % (1 << 252)]


def want(a, p, b, q):
    """the oracle's a P + b Q: its ladder twice and its addition"""
    return O.point_op("add", O.varbase_mul(a, p), O.varbase_mul(b, q))


def special_points(golden):
    """the 8-torsion (identity and (0, -1) among them), the generator, a prime-order point plus each 8-torsion point, three random points"""
    tors = torsion_points(golden)
    gen = arr64([J.GENERATOR])
    mixed = O.point_op("add", np.repeat(rand_points(31, 1, subgroup=True), len(tors), 0), tors)
    return np.concatenate([tors, gen, mixed, rand_points(32, 3)])


def edge_matrix(golden):
    """(a, P, b, Q): every ordered pair of edge scalars, every ordered pair of special points, and the coincidences Q = P, Q = -P, Q = 2P,
    b = a, a + b = r, a = 0, b = 0 on every special point with every edge scalar"""
    pts = special_points(golden)
    npt, nk = len(pts), len(EDGE_KS)
    neg, dbl = O.point_op("neg", pts), O.point_op("double", pts)
    A, P, B, Qs = [], [], [], []

    def unit(a, p, b, q):
        A.append(a); P.append(p); B.append(b); Qs.append(q)

    j = 0
    for a in EDGE_KS:                                     # every ordered pair of scalars; the points run through every class
        for b in EDGE_KS:
            unit(a, pts[j % npt], b, pts[(7 * j + j // npt) % npt])
            j += 1
    for x in range(npt):                                  # every ordered pair of points; the scalar pairs cycle
        for y in range(npt):
            unit(EDGE_KS[j % nk], pts[x], EDGE_KS[(5 * j + j // nk) % nk], pts[y])
            j += 1
    for x in range(npt):                                  # coincidences
        for i, a in enumerate(EDGE_KS):
            b = EDGE_KS[(i + 5) % nk]
            unit(a, pts[x], b, pts[x])                    # Q = P
            unit(a, pts[x], a, pts[x])                    # Q = P, b = a
            unit(a, pts[x], b, neg[x])                    # Q = -P
            unit(a, pts[x], a, neg[x])                    # Q = -P, b = a: the identity
            unit(a, pts[x], b, dbl[x])                    # Q = 2P
            unit(a, pts[x], a, pts[(x + 1) % npt])        # b = a
            unit(a % (1 << 252) % R, pts[x], (R - a % (1 << 252) % R) % (1 << 252), pts[x])   # a + b = r (or 0 + r), Q = P
            unit(a % (1 << 252) % R, pts[x], (R - a % (1 << 252) % R) % (1 << 252), pts[(x + 3) % npt])
            unit(0, pts[x], a, pts[(x + 2) % npt])        # a = 0
            unit(a, pts[x], 0, pts[(x + 2) % npt])        # b = 0
    return arr32(A), np.stack(P), arr32(B), np.stack(Qs)
