"""
The ladder step of k_varbase_mont without the masked swap of the state (jubjub_amd/csrc/jj_mont.h mont_xdbladd: only the two inputs of
the doubling are selected on the swap bit, the differential addition is symmetric in its inputs), over exact integers against
tests/mont_ladder_model.py: the state after EVERY bit equals the state that the model's swap-then-xDBLADD leaves, and the end of the
ladder equals the model's ladder().  No GPU needed.
"""
import random

import mont_ladder_model as M
from oracle import jubjub_ref as J

Q = M.Q


def swapfree_step(x1, sw, x2, z2, x3, z3):
    """the device's step: sums and differences of the unswapped state, two selects, DA = D3 S2 and CB = S3 D2 whatever sw is"""
    s2, d2, s3, d3 = (x2 + z2) % Q, (x2 - z2) % Q, (x3 + z3) % Q, (x3 - z3) % Q
    a, b = (s3, d3) if sw else (s2, d2)
    da, cb = d3 * s2 % Q, s3 * d2 % Q
    aa, bb = a * a % Q, b * b % Q
    e = (aa - bb) % Q
    return aa * bb % Q, e * (aa + M.A24 * e) % Q, (da + cb) ** 2 % Q, x1 * (da - cb) ** 2 % Q


def _both_ladders(x1, k):
    new = old = (1, 0, x1, 1)
    prev = 0
    for i in range(M.NBITS - 1, -1, -1):
        b = (k >> i) & 1
        sw = b ^ prev
        prev = b
        x2, z2, x3, z3 = old
        if sw:
            x2, z2, x3, z3 = x3, z3, x2, z2
        old = M.xdbladd(x1, x2, z2, x3, z3)
        new = swapfree_step(x1, sw, *new)
        assert new == old, "bit %d of k=%#x, x1=%#x" % (i, k, x1)
    if prev:
        new = (new[2], new[3], new[0], new[1])
    assert new == M.ladder(x1, k)


def test_swap_free_step_equals_the_model_after_every_bit():
    rng = random.Random(0x5AFE)
    cases = [(rng.randrange(Q), rng.randrange(1 << 256)) for _ in range(200)]
    x1 = M.to_x1(J.GENERATOR)[0]
    cases += [(x, k) for k in (0, 1, 2, J.R_MOD - 1, J.R_MOD, (1 << 252) - 1) for x in (x1, rng.randrange(Q), 0)]
    for x, k in cases:
        _both_ladders(x, k)
