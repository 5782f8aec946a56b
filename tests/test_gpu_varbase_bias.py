"""
jj_varbase_mul through the ladder step with q-biased sums (jj_mont.h mont_xdbladd; k_varbase_mont split into the ladder and the y-recovery)
against the C oracle, byte for byte, at n = 1 (a lone lane), 65 (a partial second wave) and 300 (a partial second workgroup): random
full-group points plus planted units -- every point of the 8-torsion (the identity and (0, -1) among them) under the scalars 0, 1, 2,
r - 1, 2^251 and the two alternating-bit patterns, the same scalars on random points, and the torsion points under random scalars -- and
against the Edwards ladder (vb_ct_window=3) on the same inputs.
"""
import numpy as np
import pytest

from oracle import c_oracle as O
from oracle import jubjub_ref as J
from util import Q, R, arr32, arr64, rand_points, rand_scalars, torsion_points

pytestmark = pytest.mark.gpu

N = 300
M252 = (1 << 252) - 1
SCALARS = [0, 1, 2, R - 1, 1 << 251, int("55" * 32, 16) & M252, int("aa" * 32, 16) & M252]


@pytest.fixture(scope="module")
def engines():
    from jubjub_amd import Engine

    mont, ct3 = Engine(0, options={"vb_quad_max": 0}), Engine(0, options={"vb_ct_window": 3, "vb_quad_max": 0})
    assert mont.get_option("vb_ct_window") == 0 and ct3.get_option("vb_ct_window") == 3
    yield mont, ct3
    mont.close(); ct3.close()


@pytest.fixture(scope="module")
def units(golden):
    """scalars, points, the oracle's results and the planted rows for n = 300; the smaller sizes are prefixes"""
    S, P = rand_scalars(0xB1A5, N, full_width=True), rand_points(0xB1A6, N)
    tors = torsion_points(golden)
    assert len(tors) == 8 and any((tors == arr64([J.AFFINE_IDENTITY])[0]).all(axis=1)) and any((tors == arr64([(0, Q - 1)])[0]).all(axis=1))
    sc = arr32(SCALARS)
    planted = []
    for t in range(len(tors)):                             # every torsion point x every scalar at rows 3, 8, .., 278: both waves of the first
        for k in range(len(sc)):                           # workgroup and the second workgroup
            i = 3 + 5 * (t * len(sc) + k)
            P[i], S[i] = tors[t], sc[k]
            planted.append(i)
    for k in range(len(sc)):                               # the scalars on random points: the first lanes, and the second workgroup
        for i in ([0, 1, 2, 4, 5, 6, 7][k], 290 + k):
            S[i] = sc[k]
            planted.append(i)
    for t in range(len(tors)):                             # the torsion points under random scalars
        P[280 + t] = tors[t]
        planted.append(280 + t)
    assert len(set(planted)) == len(planted) and max(planted) < N
    return S, P, O.varbase_mul(S, P), sorted(planted)


@pytest.mark.parametrize("n", [1, 65, 300])
def test_varbase_mul_matches_the_oracle_and_ct3(engines, units, n):
    mont, ct3 = engines
    S, P, want, planted = units
    if n == 1:                                             # one unit per call: every planted row on its own, and a random one
        for i in planted + [9]:
            assert (mont.varbase_mul(S[i:i + 1], P[i:i + 1]) == want[i:i + 1]).all(), i
        assert (ct3.varbase_mul(S[:1], P[:1]) == want[:1]).all()
        return
    got = mont.varbase_mul(S[:n], P[:n])
    bad = np.flatnonzero((got != want[:n]).any(axis=1))
    assert bad.size == 0, "n=%d: %d rows differ from the oracle, first %s (planted: %s)" % (n, bad.size, bad[:8].tolist(), [i for i in bad[:8] if i in planted])
    assert (got == ct3.varbase_mul(S[:n], P[:n])).all()
