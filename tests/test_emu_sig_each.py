"""Host emulation of jj_sigverify_each's device functions (jubjub_amd/csrc/jj_sig_each.h compiled for the CPU with -DJJ_HOST_EMU,
tests/cpp/emu_sig_each.cpp) on every planted unit of tests/sig_each_cases.py, for the table widths 8, 11 and 13 and both base kinds (prime
order, order 8r), in both modes and in both forms -- mul_add's accumulator handed to the tail as it is, and its three coordinates taken
through memory and SigEach::from_uvz (what k_sig_each_tail does behind the ladders): the preparation (c mod r, s < r, -A, the identity over a failed decode), FixedVar::mul_add,
SigEach::tail.  The verdicts must equal the cases' bytes, with a 128-bit shadow of every 64-bit column accumulator, which must count no overflow.
The decoder is the oracle's; the window table is built in the emulation from the oracle's multiples of the base.  Test infrastructure only: the
product never loads this library."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import c_oracle as O
from tests import sig_each_cases as EC
from tests.fixedvar_cases import gather_table_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "emu_sig_each.cpp")
OUT = os.path.join(ROOT, "tests", "cpp", "libjj_emu_sig_each.so")
DEPS = [SRC] + [os.path.join(ROOT, "jubjub_amd", "csrc", f) for f in ("jj_sig_each.h", "jj_fixedvar.h", "jj_straus.h", "jj_field.h", "jj_curve.h", "jj_constants.h")]
WIDTHS = (8, 11, 13)
N = 5       # positions 0, 2, 4: three planted kinds per batch, every kind in some batch


@pytest.fixture(scope="module")
def emu():
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in DEPS):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wno-unknown-pragmas", "-shared", "-fPIC", "-o", OUT, SRC])
    lib = ctypes.CDLL(OUT)
    lib.emu_table_create.restype = ctypes.c_void_p
    lib.emu_table_create.argtypes = [ctypes.c_int, ctypes.c_void_p]
    lib.emu_table_free.argtypes = [ctypes.c_void_p]
    lib.emu_sig_each.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 5 + [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.emu_overflow_reset()
    yield lib
    assert lib.emu_overflow_count() == 0, "a 64-bit column accumulator (or a top limb) overflowed in the emulated check"


def _run(emu, w, tab, b, cofactored, route):
    n = b.n
    rp, rok = O.decompress(b.r, b.flags)
    ap, aok = O.decompress(b.a, b.flags)
    points = np.ascontiguousarray(np.concatenate([rp, ap]))
    ok = np.ascontiguousarray(np.concatenate([rok, aok]).astype(np.uint8))
    s, c = np.ascontiguousarray(b.s), np.ascontiguousarray(b.c)
    cprime = np.zeros((n, 32), np.uint8)
    verdict = np.full(n, 0xEE, np.uint8)
    assert emu.emu_sig_each(w, tab, n, points.ctypes.data, ok.ctypes.data, s.ctypes.data, c.ctypes.data, cprime.ctypes.data, int(cofactored), route, verdict.ctypes.data) == 0
    # the preparation's own outputs: c mod r, and -A over every decoded A
    from tests.sig_batch_cases import R, b32, to_int
    assert np.array_equal(cprime, np.stack([b32(to_int(x) % R) for x in c]))
    good_a = aok != 0
    assert np.array_equal(points[n:][good_a], O.point_op("neg", ap[good_a])) if good_a.any() else True
    return verdict


@pytest.mark.parametrize("w", WIDTHS)
def test_planted_units(emu, w):
    seen = set()
    for base_name in ("prime", "order8r"):
        bs = [b for b in EC.batches(N) if b.base_name == base_name]
        ents = np.ascontiguousarray(gather_table_points(bs[0].base, w))
        tab = emu.emu_table_create(w, ents.ctypes.data)
        assert tab
        try:
            for b in bs:
                seen |= {k for _, k in b.planted}
                for cofactored in (True, False):
                    for route in (0, 1):
                        got = _run(emu, w, tab, b, cofactored, route)
                        assert np.array_equal(got, b.expect[cofactored]), (b.name, cofactored, route, got.tolist(), b.expect[cofactored].tolist(), b.planted)
        finally:
            emu.emu_table_free(tab)
    assert seen == {k for k, _, _ in EC.KINDS}
    assert emu.emu_overflow_count() == 0
