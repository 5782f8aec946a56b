"""Units of the fused fixed + variable multiplication a G + b Q that tests/test_emu_fixedvar.py (host emulation) and tests/test_gpu_fixedvar.py
(C ABI) share: the fixed bases (the base kinds of tests/test_gpu_fixedbase_matrix.py), the edge matrix, the oracle value of a batch and the
gathered table of a base as the oracle's affine multiples.  Test infrastructure only."""
import numpy as np

from oracle import c_oracle as O
from oracle import jubjub_ref as J
from tests.fixedbase_cover import gather_layout
from tests.straus_cases import EDGE_KS, special_points
from tests.util import R, arr32, pt64, rand_points, torsion_points

M252 = (1 << 252) - 1


def bases(golden):
    """name -> 64-byte base: the generator, a multiple of it, a point of the whole group, one point of each small order, the identity, and a
    point with a component of order 8"""
    tors = torsion_points(golden)
    ident = pt64(J.AFFINE_IDENTITY)

    def order(p):
        for m in (1, 2, 4, 8):
            if (O.fixedbase_mul(arr32([m]), p)[0] == ident).all():
                return m
        return 0

    by_order = {}
    for t in tors:
        by_order.setdefault(order(t), t)
    g = pt64(J.GENERATOR)
    p = rand_points(901, 1)[0]
    return {"G": g, "8G": O.fixedbase_mul(arr32([8]), g)[0], "P": p, "T2": by_order[2], "T4": by_order[4], "T8": by_order[8],
            "I": ident, "P+T8": O.point_op("add", p[None], by_order[8][None])[0]}


def want(g, a, b, q):
    """the oracle's a G + b Q: its ladder twice and its addition"""
    a = np.ascontiguousarray(a, np.uint8).reshape(-1, 32)
    return O.point_op("add", O.varbase_mul(a, np.tile(np.asarray(g, np.uint8).reshape(1, 64), (len(a), 1))), O.varbase_mul(b, q))


def edge_units(g, pts):
    """(a, b, Q) for one base G: Q over every special point with cycling pairs of edge scalars, and the coincidences Q = G, Q = -G, Q = 2G,
    b = a, a + b = r with Q = G (the identity), a = 0, b = 0 with every edge scalar"""
    g = np.asarray(g, np.uint8).reshape(1, 64)
    neg, dbl = O.point_op("neg", g)[0], O.point_op("double", g)[0]
    npt, nk = len(pts), len(EDGE_KS)
    A, B, Qs = [], [], []

    def unit(a, b, q):
        A.append(a); B.append(b); Qs.append(q)

    for y in range(npt):                                  # Q against this base; the scalar pairs cycle
        unit(EDGE_KS[y % nk], EDGE_KS[(5 * y + 3) % nk], pts[y])
        unit(EDGE_KS[(7 * y + 11) % nk], EDGE_KS[y % nk], pts[y])
    for i, a in enumerate(EDGE_KS):                       # coincidences
        b = EDGE_KS[(i + 5) % nk]
        ar = a % (1 << 252) % R
        unit(a, b, g[0])                                  # Q = G
        unit(a, a, g[0])                                  # Q = G, b = a
        unit(a, b, neg)                                   # Q = -G
        unit(a, a, neg)                                   # Q = -G, b = a: the identity
        unit(a, b, dbl)                                   # Q = 2G
        unit(a, a, pts[(i + 1) % npt])                    # b = a
        unit(ar, (R - ar) % (1 << 252), g[0])             # a + b = r (or 0 + r), Q = G: the identity on a prime-order base
        unit(0, a, pts[(i + 2) % npt])                    # a = 0
        unit(a, 0, pts[(i + 2) % npt])                    # b = 0
        unit(0, a, g[0])
        unit(a, 0, g[0])
    return arr32(A), arr32(B), np.stack(Qs)


def edge_matrix(golden):
    """name -> (G, a, b, Q) for every base kind; the generator also carries every ordered pair of edge scalars (Q through every special
    point), the other bases a stride of those pairs that starts at a different pair each"""
    pts = special_points(golden)
    npt, nk = len(pts), len(EDGE_KS)
    out = {}
    pairs = [(a, b) for a in EDGE_KS for b in EDGE_KS]
    all_b = bases(golden)
    for bi, (name, g) in enumerate(all_b.items()):
        a, b, q = edge_units(g, pts)
        mine = pairs if name == "G" else pairs[bi::len(all_b)]       # together the other bases see every ordered pair once more
        pa = arr32([p[0] for p in mine])
        pb = arr32([p[1] for p in mine])
        pq = np.stack([pts[(7 * j + j // npt + bi) % npt] for j in range(len(mine))])
        out[name] = (g, np.concatenate([pa, a]), np.concatenate([pb, b]), np.concatenate([pq, q]))
    return out


def gather_table_points(g, w):
    """the entries of the gathered table of width w (build_window_table in jj_abi.hip, the layout k_fixedbase_gather and k_varbase_fixed walk) as
    the oracle's affine points: entry i * (E + 1) + j = j * 2^(w i) * G for i < W = ceil(253 / w), j = 0 .. E = 2^(w-1).  Built from doublings and
    additions of the oracle (2^(w i) G by its ladder; 2^(w i) >= 2^252 as the double of 2^(w i - 1) G, since its ladder reads 252 bits)"""
    W, E, _ = gather_layout(w)
    g = np.asarray(g, np.uint8).reshape(1, 64)
    qi = np.zeros((W, 64), np.uint8)
    for i in range(W):
        bit = w * i
        if bit < 252:
            qi[i] = O.varbase_mul(arr32([1 << bit]), g)[0]
        else:
            qi[i] = O.point_op("double", O.varbase_mul(arr32([1 << (bit - 1)]), g))[0]
    tab = np.zeros((W, E + 1, 64), np.uint8)
    tab[:, 0] = pt64(J.AFFINE_IDENTITY)
    tab[:, 1] = qi
    have = 1
    while have < E:                                       # j in (have, 2 have]: even j = 2 (j / 2), odd j = (j - 1) + 1
        hi = min(2 * have, E)
        ev = np.arange(have + 1 + (have + 1) % 2, hi + 1, 2)
        if len(ev):
            tab[:, ev] = O.point_op("double", np.ascontiguousarray(tab[:, ev // 2]).reshape(-1, 64)).reshape(W, len(ev), 64)
        od = np.arange(have + 1 + have % 2, hi + 1, 2)
        if len(od):
            tab[:, od] = O.point_op("add", np.ascontiguousarray(tab[:, od - 1]).reshape(-1, 64),
                                    np.ascontiguousarray(np.repeat(qi[:, None], len(od), 1)).reshape(-1, 64)).reshape(W, len(od), 64)
        have = hi
    return tab.reshape(W * (E + 1), 64)
