"""Host emulation of the two-term interleaved ladder of k_varbase_mul2 (jubjub_amd/csrc/jj_straus.h compiled for the CPU with -DJJ_HOST_EMU,
tests/cpp/emu_straus.cpp) against the oracle, for both window widths: the two tables, both recodings, the window loop; every pair of edge
scalars, every pair of special points (8-torsion, identity, (0, -1), generator, mixed-order, random), the coincidences Q = P, Q = -P,
Q = 2P, b = a, a + b = r, a = 0, b = 0, and random units -- with a 128-bit shadow of every 64-bit column accumulator, which must count no
overflow.  Test infrastructure only: the product never loads this library."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import jubjub_ref as J
from tests.straus_cases import EDGE_KS, edge_matrix, want
from tests.util import Q, arr64, rand_points, rand_scalars, to_int

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "emu_straus.cpp")
OUT = os.path.join(ROOT, "tests", "cpp", "libjj_emu_straus.so")
DEPS = [SRC] + [os.path.join(ROOT, "jubjub_amd", "csrc", f) for f in ("jj_straus.h", "jj_field.h", "jj_curve.h", "jj_constants.h")]
WIDTHS = (5, 4)


@pytest.fixture(scope="module")
def emu():
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in DEPS):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wno-unknown-pragmas", "-shared", "-fPIC", "-o", OUT, SRC])
    lib = ctypes.CDLL(OUT)
    lib.emu_overflow_reset()
    yield lib
    assert lib.emu_overflow_count() == 0, "a 64-bit column accumulator (or a top limb) overflowed in the emulated ladder"


def _run(emu, w, a, p, b, q):
    n = len(a)
    arrs = [np.ascontiguousarray(x, np.uint8) for x in (a, p, b, q)]
    out = np.zeros((n, 64), np.uint8)
    rc = emu.emu_varbase_mul2(ctypes.c_int(w), ctypes.c_int(n), *[x.ctypes.data_as(ctypes.c_void_p) for x in arrs], out.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0
    return out


@pytest.mark.parametrize("w", WIDTHS)
def test_edge_matrix(emu, golden, w):
    a, p, b, q = edge_matrix(golden)
    got = _run(emu, w, a, p, b, q)
    exp = want(a, p, b, q)
    bad = [i for i in range(len(a)) if not np.array_equal(got[i], exp[i])]
    assert not bad, "%d of %d units differ, first: unit %d a=%#x b=%#x" % (len(bad), len(a), bad[0], to_int(a[bad[0]]), to_int(b[bad[0]]))
    assert emu.emu_overflow_count() == 0


@pytest.mark.parametrize("w", WIDTHS)
def test_random_units(emu, w):
    a, b = rand_scalars(41, 200, full_width=True), rand_scalars(42, 200, full_width=True)
    p, q = rand_points(43, 200), rand_points(44, 200)
    p[[5, 150]] = arr64([J.AFFINE_IDENTITY] * 2)
    q[[6, 150]] = arr64([J.AFFINE_IDENTITY] * 2)
    q[[7, 199]] = arr64([(0, Q - 1)] * 2)
    q[10:20] = p[10:20]                                   # Q = P
    b[15:25] = a[15:25]                                   # b = a
    assert np.array_equal(_run(emu, w, a, p, b, q), want(a, p, b, q))
    assert emu.emu_overflow_count() == 0


@pytest.mark.parametrize("w", WIDTHS)
def test_recoding_digits(emu, w):
    """the signed digits the ladder reads sum back to the low 252 bits of the scalar, every signed digit in [-2^(w-1), 2^(w-1)), the top one
    unsigned and within the table"""
    ks = EDGE_KS + [to_int(r) for r in rand_scalars(45, 300, full_width=True)]
    out = (ctypes.c_int32 * 64)()
    for k in ks:
        kb = (ctypes.c_uint8 * 32)(*int(k).to_bytes(32, "little"))
        nwin = emu.emu_straus_digits(ctypes.c_int(w), kb, out)
        assert nwin == (253 + w - 1) // w
        ds = list(out[:nwin])
        assert all(-(1 << (w - 1)) <= d < (1 << (w - 1)) for d in ds[:-1]) and 0 <= ds[-1] <= (1 << (w - 1)), (hex(k), ds)
        assert sum(d << (w * i) for i, d in enumerate(ds)) == k & ((1 << 252) - 1), hex(k)
