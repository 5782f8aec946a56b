"""Host emulation of the Montgomery-form ladder of k_varbase_mont (jubjub_amd/csrc/jj_mont.h compiled for the CPU with -DJJ_HOST_EMU,
tests/cpp/emu_mont.cpp) against the oracle: the batch inversion of k_varbase_mont_x1, the ladder, the y-recovery and the masks of the
exceptional cases, edge scalars x torsion / identity / generator / mixed-order points, with a 128-bit shadow of every 64-bit column
accumulator.  Test infrastructure only: the product never loads this library."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

from oracle import c_oracle as O
from oracle import jubjub_ref as J
from tests.util import EDGE_SCALARS, Q, arr32, arr64, b32, rand_points, rand_scalars, to_int, torsion_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "emu_mont.cpp")
OUT = os.path.join(ROOT, "tests", "cpp", "libjj_emu_mont.so")
DEPS = [SRC] + [os.path.join(ROOT, "jubjub_amd", "csrc", f) for f in ("jj_mont.h", "jj_field.h", "jj_curve.h", "jj_constants.h")]


@pytest.fixture(scope="module")
def emu():
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in DEPS):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wno-unknown-pragmas", "-shared", "-fPIC", "-o", OUT, SRC])
    lib = ctypes.CDLL(OUT)
    lib.emu_overflow_reset()
    yield lib
    assert lib.emu_overflow_count() == 0, "a 64-bit column accumulator (or a top limb) overflowed in the emulated ladder"


def _run(emu, scalars, points):
    n = len(scalars)
    s, p = np.ascontiguousarray(scalars, np.uint8), np.ascontiguousarray(points, np.uint8)
    out = np.zeros((n, 64), np.uint8)
    emu.emu_varbase_mont(ctypes.c_int(n), s.ctypes.data_as(ctypes.c_void_p), p.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p))
    return out


def _special_points(golden):
    tors = torsion_points(golden)
    gen = arr64([J.GENERATOR])
    mixed = O.point_op("add", np.repeat(rand_points(11, 1, subgroup=True), len(tors), 0), tors)   # prime-order part + each 8-torsion point
    return np.concatenate([tors, gen, mixed, rand_points(12, 3)])


def test_edge_scalars_on_special_points(emu, golden):
    """every edge scalar on every point of the 8-torsion (identity and (0, -1) among them), the generator, mixed-order points and random
    points; units laid out so that identity bases fall inside batch-inversion groups"""
    pts = _special_points(golden)
    ks = [k & ((1 << 256) - 1) for k in EDGE_SCALARS] + [J.R_MOD - 2, 2 * J.R_MOD - 1, 3, 4, 5, 6, 8 * J.R_MOD % (1 << 252)]
    S = np.repeat(arr32(ks), len(pts), 0)
    P = np.tile(pts, (len(ks), 1))
    got = _run(emu, S, P)
    want = O.varbase_mul(S, P)
    bad = [i for i in range(len(S)) if not np.array_equal(got[i], want[i])]
    assert not bad, "%d of %d rows differ, first: k=%#x" % (len(bad), len(S), to_int(S[bad[0]]))


def test_random_units(emu):
    S = rand_scalars(21, 200, full_width=True)
    P = rand_points(22, 200)
    P[[5, 37, 38, 150]] = arr64([J.AFFINE_IDENTITY] * 4)          # identities inside and at the edge of inversion groups
    P[[6, 199]] = arr64([(0, Q - 1)] * 2)
    assert np.array_equal(_run(emu, S, P), O.varbase_mul(S, P))


def test_a24_scale_and_carry(emu):
    """mont_a24 on the limb patterns the ladder can hand it (E = AA - BB: limbs 0..7 in (-2^29, 2^29), a small signed top limb) and beyond"""
    rng = random.Random(5)
    out = (ctypes.c_uint8 * 32)()
    top = 1 << 25
    cases = [[(1 << 29) - 1] * 8 + [top - 1], [-(1 << 29) + 1] * 8 + [-top + 1], [0] * 9, [0] * 8 + [1], [0] * 8 + [-1]]
    cases += [[rng.randrange(-(1 << 29) + 1, 1 << 29) for _ in range(8)] + [rng.randrange(-top + 1, top)] for _ in range(2000)]
    mont_inv = pow(1 << 261, -1, Q)
    for c in cases:
        arr = (ctypes.c_int32 * 9)(*c)
        emu.emu_mont_a24(arr, out)
        e = sum(x << (29 * i) for i, x in enumerate(c))
        assert to_int(bytes(out)) == 10240 * e * mont_inv % Q, c
