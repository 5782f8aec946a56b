"""One step of the Montgomery-form ladder (mont_xdbladd, jubjub_amd/csrc/jj_mont.h compiled for the CPU with -DJJ_HOST_EMU,
tests/cpp/emu_mont_step.cpp) on planted states: the step squares and multiplies sums biased by q (MontK::QBIAS) without a carry, so its
column bounds rest on the limb ranges of the state class that tools/bounds_check.py check_mont_ladder derives.  Here every coordinate of
the state takes the extreme limb patterns of that class -- limbs 0..7 all 0 or all 2^29 - 1, the top limb at either end -- in all
combinations, with both swap values and x1 at its extremes, plus a few thousand random states of the class: no shadow accumulator may
overflow and every output must be the integer step of tests/mont_ladder_model.py mod q.  (What the test holds is the residue and the
range of every output and the absence of an overflow with the bias in place; it cannot show that the bias is needed: with every limb at
2^29 - 1 the emulated square of a plain sum peaks a few 2^35 short of 2^63, inside the margin that the sign-blind static checker cannot
grant.)  Test infrastructure only."""
import ctypes
import itertools
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from tests import mont_ladder_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bounds_check  # noqa: E402

SRC = os.path.join(ROOT, "tests", "cpp", "emu_mont_step.cpp")
OUT = os.path.join(ROOT, "tests", "cpp", "libjj_emu_mont_step.so")
DEPS = [SRC] + [os.path.join(ROOT, "jubjub_amd", "csrc", f) for f in ("jj_mont.h", "jj_field.h", "jj_curve.h", "jj_constants.h")]
Q, LB, NL, MASK = bounds_check.Q, bounds_check.LB, bounds_check.NL, bounds_check.MASK
RINV = pow(bounds_check.MONT, -1, Q)


@pytest.fixture(scope="module")
def emu():
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in DEPS):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wno-unknown-pragmas", "-shared", "-fPIC", "-o", OUT, SRC])
    return ctypes.CDLL(OUT)


@pytest.fixture(scope="module")
def classes():
    """the limb classes of the ladder state and of x1, as check_mont_ladder prints them"""
    st, x1, _ = bounds_check.check_mont_ladder(verbose=False)
    for v in (st, x1):
        assert v.lo[:NL - 1] == [0] * (NL - 1) and v.hi[:NL - 1] == [MASK] * (NL - 1)
    return st, x1


def _value(l):
    return sum(int(x) << (LB * i) for i, x in enumerate(l))


def _extremes(v):
    """limbs 0..7 all 0 or all 2^29 - 1, the top limb at either end of the class"""
    return [[low] * (NL - 1) + [top] for low in (0, MASK) for top in (v.lo[-1], v.hi[-1])]


def _check(emu, states, x1s, sws, st_class):
    """runs the steps; every output against the integer model, and inside the state class again"""
    n = len(states)
    st = np.ascontiguousarray(states, np.int32).reshape(n, 36)
    x1 = np.ascontiguousarray(x1s, np.int32).reshape(n, 9)
    sw = np.ascontiguousarray([0xFFFFFFFF if s else 0 for s in sws], np.uint32)
    out, limbs = np.zeros((n, 128), np.uint8), np.zeros((n, 36), np.int32)
    emu.emu_overflow_reset()
    emu.emu_mont_steps(ctypes.c_int(n), *(a.ctypes.data_as(ctypes.c_void_p) for a in (st, x1, sw, out, limbs)))
    assert emu.emu_overflow_count() == 0, "a 64-bit column accumulator (or a top limb) overflowed in the emulated step"
    for s in range(n):
        x2, z2, x3, z3 = (_value(st[s, 9 * j:9 * j + 9]) * RINV % Q for j in range(4))
        if sws[s]:
            x2, z2, x3, z3 = x3, z3, x2, z2
        want = M.xdbladd(_value(x1[s]) * RINV % Q, x2, z2, x3, z3)
        got = tuple(int.from_bytes(bytes(out[s, 32 * j:32 * j + 32]), "little") for j in range(4))
        assert got == want, (s, st[s].tolist(), x1[s].tolist(), sws[s])
    low = limbs.reshape(n, 4, 9)[:, :, :NL - 1]
    top = limbs.reshape(n, 4, 9)[:, :, NL - 1]
    assert low.min() >= 0 and low.max() <= MASK
    assert top.min() >= st_class.lo[-1] and top.max() <= st_class.hi[-1], (int(top.min()), int(top.max()))


def test_extreme_states(emu, classes):
    """4 patterns per coordinate, all 4^4 combinations of the four coordinates (the 16 combinations of the low limbs among them), both swap
    values, x1 at its four extremes"""
    st_class, x1_class = classes
    states, x1s, sws = [], [], []
    for combo in itertools.product(_extremes(st_class), repeat=4):
        for x1 in _extremes(x1_class):
            for sw in (0, 1):
                states.append([l for c in combo for l in c]); x1s.append(x1); sws.append(sw)
    assert len(states) == 256 * 4 * 2
    _check(emu, states, x1s, sws, st_class)


def test_random_states(emu, classes):
    st_class, x1_class = classes
    rng = random.Random(0xB1A5)
    rand = lambda v: [rng.randrange(0, MASK + 1) for _ in range(NL - 1)] + [rng.randrange(v.lo[-1], v.hi[-1] + 1)]
    n = 4000
    _check(emu, [[l for _ in range(4) for l in rand(st_class)] for _ in range(n)], [rand(x1_class) for _ in range(n)],
           [rng.randrange(2) for _ in range(n)], st_class)
