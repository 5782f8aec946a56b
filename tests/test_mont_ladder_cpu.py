"""
The Montgomery-form ladder of k_varbase_mont (jubjub_amd/csrc/jj_mont.h), modelled over integers (tests/mont_ladder_model.py), against the
oracle: the curve constants, the map, the ladder, the y-recovery and every exceptional input -- the points of order 1, 2, 4 and 8,
mixed-order points, and scalars that land on them.  No GPU needed.
"""
import os
import random
import re

import pytest

import mont_ladder_model as M
from oracle import jubjub_ref as J
from tests.util import EDGE_SCALARS, to_pt, torsion_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MONT = 1 << 261


def _limbs(x):
    return [(x >> (29 * i)) & ((1 << 29) - 1) for i in range(9)]


def test_constants_match_the_device_header():
    src = open(os.path.join(ROOT, "jubjub_amd", "csrc", "jj_mont.h")).read()
    arr = lambda name: [int(h, 16) for h in re.findall(r"0x([0-9a-f]+)u", re.search(name + r"\[9\] = \{([^}]*)\}", src).group(1))]
    q = J.Q
    assert arr("TWO_A") == _limbs(2 * M.MONT_A * MONT % q)
    assert arr("TWO_B") == _limbs(2 * M.MONT_B * MONT % q)
    assert arr("NEG_ONE") == _limbs((q - 1) * MONT % q)
    assert int(re.search(r"MONT_A24 = (\d+);", src).group(1)) == M.A24
    qmul = int(re.search(r"MONT_A24_QMUL = 0x([0-9a-f]+);", src).group(1), 16)
    assert abs(qmul - M.A24 * (1 << 272) / q) <= 0.5 and qmul < 1 << 31


def test_map_is_on_the_montgomery_curve():
    """x = (1 + v)/(1 - v), y = x/u maps Edwards points onto B y^2 = x^3 + A x^2 + x, and the map back is its inverse"""
    q = J.Q
    rng = random.Random(3)
    for _ in range(20):
        u, v = J.ext_to_affine(J.affine_mul_scalar(J.GENERATOR, rng.getrandbits(250)))
        x, _ = M.to_x1((u, v))
        y = x * pow(u, -1, q) % q
        assert M.MONT_B * y * y % q == (x ** 3 + M.MONT_A * x * x + x) % q
        assert (x * pow(y, -1, q) % q, (x - 1) * pow(x + 1, -1, q) % q) == (u, v)


def _points(golden):
    tors = [to_pt(r) for r in torsion_points(golden)]
    assert (0, 1) in tors and (0, J.Q - 1) in tors and len(tors) == 8
    rng = random.Random(1)
    prime = [J.ext_to_affine(J.ext_mul_by_cofactor(J.affine_mul_scalar(J.GENERATOR, rng.getrandbits(250)))) for _ in range(2)]
    mixed = [J.ext_to_affine(J.ext_add(J.affine_to_extended(prime[0]), J.affine_to_extended(t))) for t in tors]
    return tors + [J.GENERATOR] + prime + mixed


def test_model_matches_the_oracle(golden):
    R = J.R_MOD
    ks = [k & ((1 << 256) - 1) for k in EDGE_SCALARS] + [R - 2, 2 * R - 1, 3, 4, 5, 6, 8 * R % (1 << 252), 4 * R % (1 << 252)]
    rng = random.Random(2)
    ks += [rng.getrandbits(256) for _ in range(4)]
    for p in _points(golden):
        for k in ks:
            want = J.ext_to_affine(J.ext_multiply(J.affine_to_extended(p), k.to_bytes(32, "little")))
            assert M.affine(M.varbase(p, k)) == want, (p, hex(k))


def test_exceptional_branches_are_reached(golden):
    """each mask of the device code is needed: the unmasked recovery is wrong (or undefined) on exactly these inputs"""
    q, R = J.Q, J.R_MOD
    tors = [to_pt(r) for r in torsion_points(golden)]
    gen = J.GENERATOR
    seen = set()
    for p in tors + [gen]:
        x1, ident = M.to_x1(p)
        for k in (0, 1, 2, 3, 4, 7, 8, R - 1, R, 8 * R - 1 & ((1 << 252) - 1)):
            xq, zq, xp, zp = M.ladder(x1, k)
            if ident:
                seen.add("identity")
            elif x1 == 0:
                seen.add("order2-odd" if k & 1 else "order2-even")
            elif zq == 0:
                seen.add("kP=O")
            elif zp == 0:
                seen.add("(k+1)P=O")
            elif xq == 0:
                seen.add("kP=(0,0)")
    assert seen >= {"identity", "order2-odd", "order2-even", "kP=O", "(k+1)P=O", "kP=(0,0)"}, seen
