"""Host emulation of Field::invert_divsteps (jubjub_amd/csrc/jj_field.h compiled for the CPU with -DJJ_HOST_EMU, tests/cpp/emu_invert.cpp)
against Field::invert, the power chain it replaces in k_normalize and k_varbase_mont_x1, and against Python's pow: both fields, 10^5 seeded
random values, the edge values (0, +-1, +-2, p - 1, 2^k and 2^k - 1 for every k < 255) and representatives that are not canonical (sums and
differences of two products, a value in (-1.2p, 0)).  Every 64-bit accumulator is mirrored in 128 bits, and after every batch of divsteps d
and e must lie in (-2p, p), the range the update assumes.  Test infrastructure only: the product never loads this library."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import jubjub_ref as J
from field_cases import inversion_values
from tests.util import arr32, to_int

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "emu_invert.cpp")
OUT = os.path.join(ROOT, "tests", "cpp", "libjj_emu_invert.so")
DEPS = [SRC] + [os.path.join(ROOT, "jubjub_amd", "csrc", f) for f in ("jj_field.h", "jj_constants.h")]
MONT_R = 1 << 261
FIELDS = {"Fq": (0, J.Q), "Fr": (1, J.R_MOD)}
N_RANDOM = 100000


@pytest.fixture(scope="module")
def emu():
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in DEPS):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-Wno-unknown-pragmas", "-shared", "-fPIC", "-o", OUT, SRC])
    lib = ctypes.CDLL(OUT)
    lib.emu_invert_both.argtypes = [ctypes.c_int, ctypes.c_size_t] + [ctypes.c_void_p] * 5 + [ctypes.c_int]
    lib.emu_overflow_reset()
    yield lib
    assert lib.emu_overflow_count() == 0, "an accumulator overflowed, a batch was not exact, or d / e left (-2p, p) in the emulated inversion"


def _run(emu, field, ops, a, b):
    n = len(ops)
    ops = np.ascontiguousarray(ops, np.uint8)
    a, b = np.ascontiguousarray(a, np.uint8), np.ascontiguousarray(b, np.uint8)
    assert a.shape == (n, 32) and b.shape == (n, 32)
    div, ref = np.zeros((n, 32), np.uint8), np.zeros((n, 32), np.uint8)
    ptr = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    emu.emu_invert_both(FIELDS[field][0], n, ptr(ops), ptr(a), ptr(b), ptr(div), ptr(ref), min(8, os.cpu_count() or 1))
    assert emu.emu_overflow_count() == 0
    return div, ref


def _check(emu, field, ops, a, b, values):
    """values: the field element each case stands for (an integer mod p); the outputs are Montgomery-form canonical integers"""
    p = FIELDS[field][1]
    div, ref = _run(emu, field, ops, a, b)
    bad = np.flatnonzero((div != ref).any(axis=1))
    assert bad.size == 0, "%s: %d of %d inverses differ from invert(), first: case %d" % (field, bad.size, len(ops), bad[0])
    for i, x in enumerate(values):
        want = pow(x % p, -1, p) * MONT_R % p if x % p else 0
        assert to_int(div[i]) == want, (field, i, hex(x % p))


@pytest.mark.parametrize("field", ["Fq", "Fr"])
def test_edge_values(emu, field):
    p = FIELDS[field][1]
    X = list(inversion_values(field.lower()))              # the list the device inverts too (tests/test_gpu_field_matrix.py)
    assert {1, 2, 3, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2} <= set(X)
    assert all(1 << k in X and (k < 3 or (1 << k) - 1 in X) for k in range(255))   # as integers, not reduced: 2^252 ... 2^254 exceed Fr's modulus
    xs = [0] + X + [p, p + 1, (1 << 256) - 1]              # zero, and from_words reduces any 256-bit integer
    zeros = np.zeros((len(xs), 32), np.uint8)
    _check(emu, field, np.zeros(len(xs), np.uint8), arr32(xs), zeros, xs)


@pytest.mark.parametrize("field", ["Fq", "Fr"])
def test_random_values(emu, field):
    rng = np.random.default_rng(0xD1F5 + FIELDS[field][0])
    a = rng.integers(0, 256, size=(N_RANDOM, 32), dtype=np.uint8)
    div, ref = _run(emu, field, np.zeros(N_RANDOM, np.uint8), a, np.zeros_like(a))
    assert np.array_equal(div, ref)
    p = FIELDS[field][1]
    for i in range(0, N_RANDOM, 997):                      # the power chain is the reference; pow() holds a sample of it
        x = to_int(a[i]) % p
        assert to_int(div[i]) == pow(x, -1, p) * MONT_R % p


@pytest.mark.parametrize("field", ["Fq", "Fr"])
def test_non_canonical_representatives(emu, field):
    """lazy sums and differences of two products, and a negative value: canonical Montgomery digits - p - b with b < 0.2 p, in (-1.2p, 0)"""
    p = FIELDS[field][1]
    n = 3000
    rng = np.random.default_rng(0xABCD + FIELDS[field][0])
    a = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    b = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    ops = (np.arange(n) % 3 + 1).astype(np.uint8)
    small = [to_int(b[i]) % (p // 5) for i in range(n)]
    for i in range(n):
        if ops[i] == 3:
            b[i] = arr32([small[i]])[0]
    # planted: a - a = 0, a + (p - a) = 0, the most negative value of case 3
    ai = [to_int(r) for r in a]
    b[0] = a[0]
    b[1] = arr32([(p - ai[1] % p) % p])[0]
    b[2] = arr32([p // 5 - 1])[0]
    small[2] = p // 5 - 1
    bi = [to_int(r) for r in b]
    rinv = pow(MONT_R, -1, p)
    values = []
    for i in range(n):
        if ops[i] == 1:
            values.append(ai[i] - bi[i])
        elif ops[i] == 2:
            values.append(ai[i] + bi[i])
        else:                                              # digits hold a R mod p as an integer; minus p, minus b: the element (a R - b) / R
            values.append((ai[i] * MONT_R - small[i]) * rinv)
    _check(emu, field, ops, a, b, values)
