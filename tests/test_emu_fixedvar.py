"""Host emulation of the fused fixed + variable ladder of k_varbase_fixed (jubjub_amd/csrc/jj_fixedvar.h compiled for the CPU with -DJJ_HOST_EMU,
tests/cpp/emu_fixedvar.cpp) against the oracle, for the table widths 8, 11 and 13 (at 11, 253 = 11 x 23: the top window is full and the recoding
carry lands on entry E): the variable term's table, both recodings, both window loops; the edge matrix of tests/fixedvar_cases.py on every base
kind and random full-width units -- with a 128-bit shadow of every 64-bit column accumulator, which must count no overflow.  The window table is
built in the emulation (Curve::to_niels) from the oracle's multiples of the base.  Test infrastructure only: the product never loads this library."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import jubjub_ref as J
from tests.fixedvar_cases import bases, edge_matrix, gather_table_points, want
from tests.straus_cases import EDGE_KS
from tests.util import Q, arr64, rand_points, rand_scalars, to_int

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "emu_fixedvar.cpp")
OUT = os.path.join(ROOT, "tests", "cpp", "libjj_emu_fixedvar.so")
DEPS = [SRC] + [os.path.join(ROOT, "jubjub_amd", "csrc", f) for f in ("jj_fixedvar.h", "jj_straus.h", "jj_field.h", "jj_curve.h", "jj_constants.h")]
WIDTHS = (8, 11, 13)


@pytest.fixture(scope="module")
def emu():
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in DEPS):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wno-unknown-pragmas", "-shared", "-fPIC", "-o", OUT, SRC])
    lib = ctypes.CDLL(OUT)
    lib.emu_table_create.restype = ctypes.c_void_p
    lib.emu_table_create.argtypes = [ctypes.c_int, ctypes.c_void_p]
    lib.emu_table_free.argtypes = [ctypes.c_void_p]
    lib.emu_fixedvar_mul.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 4
    lib.emu_overflow_reset()
    yield lib
    assert lib.emu_overflow_count() == 0, "a 64-bit column accumulator (or a top limb) overflowed in the emulated ladder"


def _run(emu, w, g, a, b, q):
    """a G + b Q over a table of width w built for this call"""
    n = len(a)
    ents = np.ascontiguousarray(gather_table_points(g, w))
    tab = emu.emu_table_create(w, ents.ctypes.data)
    assert tab
    try:
        arrs = [np.ascontiguousarray(x, np.uint8) for x in (a, b, q)]
        out = np.zeros((n, 64), np.uint8)
        assert emu.emu_fixedvar_mul(w, tab, n, *[x.ctypes.data for x in arrs], out.ctypes.data) == 0
    finally:
        emu.emu_table_free(tab)
    return out


@pytest.fixture(scope="module")
def matrix(golden):
    """the edge matrix and its oracle values, computed once for the three widths"""
    return {name: (g, a, b, q, want(g, a, b, q)) for name, (g, a, b, q) in edge_matrix(golden).items()}


@pytest.mark.parametrize("w", WIDTHS)
def test_edge_matrix(emu, matrix, w):
    for name, (g, a, b, q, exp) in matrix.items():
        got = _run(emu, w, g, a, b, q)
        bad = [i for i in range(len(a)) if not np.array_equal(got[i], exp[i])]
        assert not bad, "base %s: %d of %d units differ, first: unit %d a=%#x b=%#x" % (name, len(bad), len(a), bad[0], to_int(a[bad[0]]), to_int(b[bad[0]]))
    assert emu.emu_overflow_count() == 0


@pytest.mark.parametrize("w", WIDTHS)
def test_random_units(emu, golden, w):
    g = bases(golden)["G"]
    a, b = rand_scalars(51, 200, full_width=True), rand_scalars(52, 200, full_width=True)
    q = rand_points(53, 200)
    q[[6, 150]] = arr64([J.AFFINE_IDENTITY] * 2)
    q[[7, 199]] = arr64([(0, Q - 1)] * 2)
    q[10:20] = g                                          # Q = G
    b[15:25] = a[15:25]                                   # b = a
    assert np.array_equal(_run(emu, w, g, a, b, q), want(g, a, b, q))
    assert emu.emu_overflow_count() == 0


@pytest.mark.parametrize("w", WIDTHS)
def test_fixed_digits(emu, w):
    """the fixed term's digits sum back to the low 252 bits of a; every signed digit in [-E, E), the top one unsigned and in [0, E]"""
    ks = EDGE_KS + [to_int(r) for r in rand_scalars(55, 300, full_width=True)]
    E, W = 1 << (w - 1), -(-253 // w)
    out = (ctypes.c_int32 * 64)()
    for k in ks:
        kb = (ctypes.c_uint8 * 32)(*int(k).to_bytes(32, "little"))
        assert emu.emu_fixed_digits(ctypes.c_int(w), kb, out) == W
        ds = list(out[:W])
        assert all(-E <= d < E for d in ds[:-1]) and 0 <= ds[-1] <= E, (hex(k), ds)
        assert sum(d << (w * i) for i, d in enumerate(ds)) == k & ((1 << 252) - 1), hex(k)
    if w == 11:                                           # 253 = 11 x 23: the carry out of a full top window selects entry E itself
        kb = (ctypes.c_uint8 * 32)(*int((1 << 252) - 1).to_bytes(32, "little"))
        emu.emu_fixed_digits(ctypes.c_int(w), kb, out)
        assert out[W - 1] == E
