"""
The default var-base path after the ladder step lost its state swap (jj_mont.h mont_xdbladd) and the two batch-inversion kernels went from
the power chain to divsteps (Field::invert_divsteps in k_varbase_mont_x1 and k_normalize), against the C oracle, byte for byte, every row:
partial waves and partial inversion groups, scalars whose swap keys are all zero or all one, and the identity, (0, -1), the other six
small-order points and the generator at the first, a middle and the last unit of an inversion group.  Then batch_normalize itself at the
three chunk shapes a small batch can take, with a Z = 0 row and a Z = 1 row.
"""
import os
import re

import numpy as np
import pytest

from oracle import c_oracle as O
from oracle import jubjub_ref as J
from util import Q, R, arr32, arr64, rand_points, rand_scalars, torsion_points

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X1_UNITS = int(re.search(r"MONT_X1_UNITS = (\d+);", open(os.path.join(ROOT, "jubjub_amd", "csrc", "jj_mont.h")).read()).group(1))
GROUP = 64 * X1_UNITS                                     # units of one wave of k_varbase_mont_x1; lane L inverts units L + 64 s of it
SIZES = [1, 63, 65, 1023, 1025, GROUP * 2 + 7]
M252 = (1 << 252) - 1
SPECIAL_SCALARS = [0, 1, 2, R - 1, R, M252, int("55" * 32, 16) & M252, int("aa" * 32, 16) & M252]


@pytest.fixture(scope="module")
def eng():
    from jubjub_amd import Engine

    e = Engine(0, options={"vb_quad_max": 0})
    yield e
    e.close()


@pytest.fixture(scope="module")
def units(golden):
    """scalars, points, the planted rows and the oracle's results for the largest size; every smaller size is a prefix of it"""
    n = max(SIZES)
    S, P = rand_scalars(0x7121, n, full_width=True), rand_points(0x7122, n)
    special = np.concatenate([torsion_points(golden), arr64([J.GENERATOR])])      # the 8-torsion (identity and (0, -1) among them) + generator
    assert len(special) == 9 and any((special == arr64([J.AFFINE_IDENTITY])[0]).all(axis=1)) and any((special == arr64([(0, Q - 1)])[0]).all(axis=1))
    sc = arr32(SPECIAL_SCALARS)
    planted = []
    # lane L of the first wave inverts units L, L + 64, ..., L + 64 (X1_UNITS - 1): each special point at the group's first, middle, last unit
    for L in range(len(special)):
        for j, s in enumerate((0, X1_UNITS // 2, X1_UNITS - 1)):
            i = L + 64 * s
            P[i] = special[L]
            S[i] = sc[(L + 3 * j) % len(sc)] if (L + j) % 2 else S[i]
            planted.append(i)
    # the groups that the ragged sizes cut short: unit 64 (second unit of lane 0 at n = 65), the single units of the second and third wave
    for k, i in enumerate([64, GROUP, GROUP + 1, 2 * GROUP, 2 * GROUP + 3, 2 * GROUP + 6]):
        P[i] = special[(2 * k + 1) % len(special)]
        planted.append(i)
    # every special scalar on random points and on a whole inversion group of one lane (lane 20)
    for k in range(len(sc)):
        S[20 + k] = sc[k]
        S[20 + 64 * (k + 1)] = sc[k]
        S[GROUP + 30 + k] = sc[k]
    want = O.varbase_mul(S, P)
    return S, P, want, O.compress(want), sorted(set(planted))


@pytest.mark.parametrize("n", SIZES)
def test_varbase_mul_matches_the_oracle(eng, units, n):
    S, P, want, want_c, planted = units
    if n == 1:                                            # one unit per call: every planted row and every special scalar on its own
        rows = planted + list(range(20, 28))
        for i in rows:
            assert (eng.varbase_mul(S[i:i + 1], P[i:i + 1]) == want[i:i + 1]).all(), i
            assert (eng.varbase_mul_compressed(S[i:i + 1], P[i:i + 1]) == want_c[i:i + 1]).all(), i
        return
    got = eng.varbase_mul(S[:n], P[:n])
    bad = np.flatnonzero((got != want[:n]).any(axis=1))
    assert bad.size == 0, "n=%d: %d rows differ from the oracle, first %s (planted: %s)" % (n, bad.size, bad[:8].tolist(), [i for i in bad[:8] if i in planted])
    got = eng.varbase_mul_compressed(S[:n], P[:n])
    bad = np.flatnonzero((got != want_c[:n]).any(axis=1))
    assert bad.size == 0, "n=%d compressed: %d rows differ from the oracle, first %s" % (n, bad.size, bad[:8].tolist())


@pytest.fixture(scope="module")
def ext_rows():
    n = 4097
    S, P = rand_scalars(0x7123, n), rand_points(0x7124, n)
    ext = O.varbase_mul_ext(S, P)                          # (U, V, Z, T1, T2), 160 canonical bytes a row, Z neither 0 nor 1
    z0, z1 = ext[0].copy(), ext[0].copy()
    z0[64:96] = 0                                          # Z = 0: skipped by the batch inversion, (0, 0) out
    z1[:] = np.concatenate([P[5], arr32([1])[0], P[5]])    # (u, v, 1, u, v)
    return ext, z0, z1


@pytest.mark.parametrize("n", [1, 17, 4097])
def test_batch_normalize_matches_the_oracle(eng, ext_rows, n):
    ext, z0, z1 = ext_rows
    if n == 1:
        for row in (ext[3:4], z0[None], z1[None]):
            assert (eng.batch_normalize(row) == O.batch_normalize(row)).all()
        return
    rows = ext[:n].copy()
    rows[n // 2] = z0                                      # inside a lane's chunk
    rows[n - 1] = z1                                       # the last row: the short chunk
    rows[0] = z1
    rows[1] = z0
    got, want = eng.batch_normalize(rows), O.batch_normalize(rows)
    assert (want[n // 2] == 0).all() and (want[n - 1] == np.concatenate([z1[:32], z1[32:64]])).all()
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, "n=%d: %d rows differ from the oracle, first %s" % (n, bad.size, bad[:8].tolist())
