"""MontK::QBIAS (jubjub_amd/csrc/jj_mont.h), the bias that the ladder step subtracts from its three sums, recomputed from the field
modulus of tools/gen_constants.py: q itself with limbs 0..7 moved next to 2^29, and the header must hold exactly these limbs."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gen_constants import LB, NL, Q, limbs  # noqa: E402


def _qbias():
    c = list(limbs(Q))
    for i in range(NL - 1):                    # from limb 0 up: a limb below 2^28 borrows 2^29 from the limb above it
        if c[i] < 1 << 28:
            c[i] += 1 << LB
            c[i + 1] -= 1
    return c


def test_qbias_is_q_in_limbs_near_2_29():
    c = _qbias()
    assert sum(x << (LB * i) for i, x in enumerate(c)) == Q
    assert all(1 << 28 <= x < 3 << 28 for x in c[:NL - 1]), [hex(x) for x in c]
    assert 0 <= c[NL - 1] < 1 << 23


def test_header_holds_the_recomputed_limbs():
    src = open(os.path.join(ROOT, "jubjub_amd", "csrc", "jj_mont.h")).read()
    m = re.search(r"QBIAS\[9\] = \{([^}]*)\}", src)
    assert m, "MontK::QBIAS not found in jj_mont.h"
    got = [int(x.strip().rstrip("u"), 16) for x in m.group(1).split(",")]
    assert got == _qbias(), [hex(x) for x in got]


def test_bounds_checker_uses_the_same_limbs():
    import bounds_check

    assert bounds_check.qbias(Q) == _qbias()
