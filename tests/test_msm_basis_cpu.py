"""CPU checks of the fixed-basis MSM (jj_msm_basis_*): exported and declared, arguments refused before any device is touched, the planner
jj_plan_msm_basis, the identity the window table rests on (sum_w d_w (2^start_w P) = k P for the digits of msm_layout / msm_digit_raw,
restated here), Engine's shape checks, and a C++ caller of jubjub_hip.hpp's MsmBasis compiles and links."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from util import EDGE_SCALARS, R

NAMES = ("jj_msm_basis_create", "jj_msm_basis_destroy", "jj_msm_basis_info", "jj_msm_basis_mul", "jj_plan_msm_basis")
SMALL_MAX = 8192                 # rows up to this many terms take the small tables (MSM_BATCH_MAX)
TAB, ROW = 1296, 128             # bytes per point: {0..8} P tables | one gathered-Niels record


def lib():
    from jubjub_amd import _lib

    return _lib.load(), _lib


def test_symbols_exported_and_declared():
    import __graft_entry__ as ge

    ge.build()
    so = ctypes.CDLL(os.path.join(ROOT, "jubjub_amd", "lib", "libjubjub_hip.so"))
    header = open(os.path.join(ROOT, "include", "jubjub_hip.h")).read()
    from jubjub_amd import _lib

    for name in NAMES:
        assert hasattr(so, name), name
        assert name + "(" in header, name
        assert name in _lib.EXPORTS, name


def test_refuses_bad_arguments_without_a_device():
    L, _lib = lib()
    INVALID = _lib.JJ_ERR_INVALID
    buf = (ctypes.c_uint8 * 64)()
    h = ctypes.c_void_p()
    out4 = (ctypes.c_int64 * 4)()
    assert L.jj_msm_basis_create(None, 1, buf, 0, 0, ctypes.byref(h)) == INVALID and not h.value
    assert L.jj_msm_basis_create(None, 1, buf, 0, 0, None) == INVALID
    assert L.jj_msm_basis_destroy(None, None) == INVALID
    assert L.jj_msm_basis_info(None, out4) == INVALID
    assert L.jj_msm_basis_mul(None, None, 1, 1, buf, buf) == INVALID
    assert L.jj_msm_basis_mul(None, None, 0, 0, None, None) == INVALID                       # no context: refused even where B = 0 would succeed
    # (a NULL out, m > n and an overflowing B * m need a basis to get past the first check: tests/test_gpu_msm_basis.py::test_refused_arguments)
    assert L.jj_plan_msm_basis(100, 0, 0, 1 << 30, None) == INVALID
    for mode in (-1, 3, 7):
        assert L.jj_plan_msm_basis(100000, mode, 0, 1 << 40, out4) == INVALID, mode
    for w in (-1, 1, 15, 37, 64):
        assert L.jj_plan_msm_basis(100000, 2, w, 1 << 40, out4) == INVALID, w
    assert L.jj_plan_msm_basis((1 << 24) + 1, 1, 0, 1 << 40, out4) == INVALID                # the documented cap on n
    assert L.jj_plan_msm_basis(1 << 24, 1, 0, 1 << 40, out4) == 0


def plan(n, mode=0, windows=0, budget=1 << 50):
    L, _ = lib()
    out = (ctypes.c_int64 * 4)()
    assert L.jj_plan_msm_basis(n, mode, windows, budget, out) == 0, (n, mode, windows)
    return tuple(out)


def default_windows(n):
    return 16 if n >= 1 << 18 else 17 if n >= 9 << 14 else 23


def test_plan_properties():
    sizes = sorted({max(1, (1 << k) + d) for k in range(0, 23) for d in (-1, 0, 1)} | {SMALL_MAX, SMALL_MAX + 1, (9 << 14) - 1, 9 << 14})
    sizes = [n for n in sizes if n <= 1 << 22]
    for n in sizes:
        route = 1 if n > SMALL_MAX else 0
        small = min(n, SMALL_MAX) * TAB
        for mode in (1, 2):
            m, W, nbytes, r = plan(n, mode)
            assert r == route and m == mode, (n, mode)                 # the route flips above 8192 terms; an explicit mode is honoured
            if not route:
                assert W == 64 and nbytes == n * TAB                    # both modes keep the per-term tables and differ in nothing
            else:
                assert W == default_windows(n)
                assert nbytes == small + n * ROW * (W if mode == 2 else 1), (n, mode)
        for W in (16, 17, 23, 36):
            m, w, nbytes, r = plan(n, 2, W)
            assert w == (W if route else 64) and (not route or nbytes == small + n * W * ROW), (n, W)
        # auto: never beyond the budget when mode 1 fits it, and mode 1 whenever the window table would not fit
        b1, b2 = plan(n, 1)[2], plan(n, 2)[2]
        for budget in (0, b1, b2 - 1, b2, 1 << 50):
            m, W, nbytes, r = plan(n, 0, 0, budget)
            assert m in (1, 2) and nbytes == (b2 if m == 2 else b1)
            if m == 2:
                assert route and nbytes <= budget, (n, budget)
            if budget < b2:
                assert m == 1, (n, budget)
    assert plan(0) == (1, 64, 0, 0)


def layout(W):
    """msm_layout of jj_msm.hip: 253 = W c + r, the r low windows are c + 1 bits wide; recode = sum over w < W - 1 of 2^(start_w + width_w - 1)"""
    c, r = divmod(253, W)
    wins, bit, recode = [], 0, 0
    for w in range(W):
        width = c + (1 if w < r else 0)
        wins.append((bit, width))
        if w < W - 1:
            recode += 1 << (bit + width - 1)
        bit += width
    assert bit == 253
    return wins, recode


def test_restated_layout_is_the_records_layout():
    """layout() above against tests/util.msm_window_layout / msm_signed_digits, which the record tests (oracle_msm_record against jj_msm_partial on
    the GPU, jj_msm_combine on the host) tie to msm_layout of jj_msm.hip; and the planner's window counts are layouts the restatement covers"""
    from util import msm_signed_digits, msm_window_layout

    rnd = random.Random(3)
    for W in list(range(16, 37)) + [64]:
        wins, recode = layout(W)
        assert wins == msm_window_layout(W)
        assert max(wd for _, wd in wins) - min(wd for _, wd in wins) <= 1 and wins[0][1] == max(wd for _, wd in wins)      # window 0 is the widest: the folded set's
        for k in [rnd.getrandbits(256) for _ in range(8)] + list(EDGE_SCALARS):
            assert [(-a if neg else a) for a, neg in digits(k, W)[0]] == msm_signed_digits(k, W)
    for n in (8193, 1 << 14, 9 << 14, 1 << 18, 1 << 22):
        assert plan(n, 2)[1] in (16, 17, 23)
        for W in (16, 17, 23, 36):
            assert plan(n, 2, W)[1] == W


def digits(k, W):
    """msm_recode + msm_digit_raw: (|d|, negative) per window of the low 252 bits of the raw pattern k"""
    wins, recode = layout(W)
    kp = (k & ((1 << 252) - 1)) + recode
    out = []
    for w, (start, width) in enumerate(wins):
        raw = (kp >> start) & ((1 << width) - 1)
        if w == W - 1:
            out.append((raw, 0))
        else:
            d = raw - (1 << (width - 1))
            out.append((abs(d), 1 if d < 0 else 0))
    return out, wins


def test_window_table_identity(golden):
    """every window adds d_w * (2^start_w P) into one bucket set: the sum must be k P on the whole curve, for every layout the table may have"""
    from oracle import jubjub_ref as J
    from util import to_pt, torsion_points

    rnd = random.Random(20)
    scalars = list(EDGE_SCALARS) + [rnd.getrandbits(256) for _ in range(64)]
    p8 = next(to_pt(q) for q in torsion_points(golden) if J.scalar_mul_fast(to_pt(q), 4) != J.AFFINE_IDENTITY)      # order 8
    for P in (J.GENERATOR, p8, J.AFFINE_IDENTITY):
        for W in (16, 17, 23, 36, 64):
            wins = layout(W)[0]
            rows = [J.affine_to_extended(J.scalar_mul_fast(P, 1 << start)) if start else J.affine_to_extended(P) for start, _ in wins]
            for k in scalars:
                ds, _ = digits(k, W)
                assert all(a <= 1 << (wd - 1) for (a, _), (_, wd) in zip(ds, wins))            # bucket |d| - 1 exists
                # sum over the buckets: bucket b collects +-rows[w] of the windows with |d_w| = b + 1; then sum_b (b + 1) bucket_b
                acc = J.EXT_IDENTITY
                for (a, neg), row in zip(ds, rows):
                    if a:
                        t = J.affine_to_extended(J.scalar_mul_fast(J.ext_to_affine(row), a))
                        acc = J.ext_add(acc, J.ext_neg(t) if neg else t)
                assert J.ext_to_affine(acc) == J.scalar_mul_fast(P, k & ((1 << 252) - 1)), (W, hex(k))


def test_engine_shape_checks():
    import threading

    from jubjub_amd import Engine, MsmBasis
    from jubjub_amd.engine import _msm_basis_shapes as shapes

    assert shapes(10, np.zeros((10, 32), np.uint8)) == (1, 10, True)
    assert shapes(10, np.zeros((4, 32), np.uint8)) == (1, 4, True)
    assert shapes(10, np.zeros((3, 7, 32), np.uint8)) == (3, 7, False)
    assert shapes(10, np.zeros((0, 7, 32), np.uint8)) == (0, 7, False)
    for s in ((32,), (11, 32), (3, 11, 32), (3, 7, 31), (2, 3, 7, 32)):
        with pytest.raises(ValueError):
            shapes(10, np.zeros(s, np.uint8))
    e = object.__new__(Engine)                       # no context: the checks must come before it is touched
    e._mu = threading.RLock()
    for pts, kw in ((np.zeros((5, 32), np.uint8), {}), (np.zeros((64,), np.uint8), {}), (np.zeros((5, 64), np.uint8), {"mode": "fast"}),
                    (np.zeros((5, 64), np.uint8), {"windows": 15}), (np.zeros((5, 64), np.uint8), {"windows": 37})):
        with pytest.raises(ValueError):
            e.msm_basis(pts, **kw)
    b = MsmBasis(e, None, 10)
    with pytest.raises(ValueError):
        e.msm_basis_mul(b, np.zeros((11, 32), np.uint8))
    with pytest.raises(ValueError):
        e.msm_basis_mul(b, np.zeros((3, 4, 31), np.uint8))


def test_cpp_caller_compiles(tmp_path):
    src = tmp_path / "msm_basis.cpp"
    src.write_text(r'''
#include "jubjub_hip.hpp"
int main() {
  try {
    jubjub::Context c(0);
    jubjub::AffineBatch pts = jubjub::AffineBatch::identity(c, 4);
    jubjub::MsmBasis basis(c, pts, 2, 16);
    std::vector<jubjub::FrBatch> rows;
    jubjub::AffineBatch a = jubjub::msm(basis, rows);
    return (int)(a.len() + basis.len() + basis.info().size());
  } catch (const jubjub::Error& e) {
    return 1;
  }
}
''')
    lib_dir = os.path.join(ROOT, "jubjub_amd", "lib")
    out = tmp_path / "msm_basis"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-L", lib_dir, "-ljubjub_hip",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", str(out)])
    assert out.exists()
