"""CPU checks of jj_msm_batch / jj_multi_msm_batch: exported and declared, arguments refused before any device is touched,
Engine.msm_batch's shape checks, and a C++ caller of jubjub_hip.hpp's msm_batch compiles and links."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT


def lib():
    from jubjub_amd import _lib

    return _lib.load(), _lib


def test_symbols_exported_and_declared():
    import __graft_entry__ as ge

    ge.build()
    so = ctypes.CDLL(os.path.join(ROOT, "jubjub_amd", "lib", "libjubjub_hip.so"))
    header = open(os.path.join(ROOT, "include", "jubjub_hip.h")).read()
    for name in ("jj_msm_batch", "jj_multi_msm_batch"):
        assert hasattr(so, name), name
        assert name + "(" in header, name


def test_refuses_bad_arguments_without_a_device():
    L, _lib = lib()
    out = (ctypes.c_uint8 * 64)()
    buf = (ctypes.c_uint8 * 64)()
    INVALID = _lib.JJ_ERR_INVALID
    # no context (every other argument well-formed, empty or not)
    assert L.jj_msm_batch(None, 1, 1, buf, buf, 1, out) == INVALID
    assert L.jj_msm_batch(None, 0, 0, None, None, 0, None) == INVALID
    assert L.jj_multi_msm_batch(None, 1, 1, buf, buf, 1, out) == INVALID
    # points_shared other than 0 / 1, and sizes whose byte count overflows size_t, are refused before the context is looked at
    assert L.jj_msm_batch(None, 1, 1, buf, buf, 2, out) == INVALID
    assert L.jj_msm_batch(None, 1 << 40, 1 << 30, buf, buf, 0, out) == INVALID
    assert L.jj_multi_msm_batch(None, 1, 1, buf, buf, -1, out) == INVALID


def test_engine_shape_checks():
    import threading

    from jubjub_amd import Engine, MultiEngine
    from jubjub_amd.engine import _msm_batch_shapes as shapes

    assert shapes(np.zeros((3, 5, 32), np.uint8), np.zeros((5, 64), np.uint8)) == (3, 5, 1)
    assert shapes(np.zeros((3, 5, 32), np.uint8), np.zeros((3, 5, 64), np.uint8)) == (3, 5, 0)
    assert shapes(np.zeros((0, 5, 32), np.uint8), np.zeros((5, 64), np.uint8)) == (0, 5, 1)
    bad = [((5, 32), (5, 64)), ((3, 5, 31), (5, 64)), ((3, 5, 32), (4, 64)), ((3, 5, 32), (2, 5, 64)), ((3, 5, 32), (3, 5, 32)), ((3, 5, 32), (3 * 5, 64))]
    for s, p in bad:
        with pytest.raises(ValueError):
            shapes(np.zeros(s, np.uint8), np.zeros(p, np.uint8))
    # the public methods check the shapes before they touch a context
    e, m = object.__new__(Engine), object.__new__(MultiEngine)
    e._mu = threading.RLock()
    for call in (e.msm_batch, m.msm_batch):
        with pytest.raises(ValueError):
            call(np.zeros((3, 5, 32), np.uint8), np.zeros((4, 64), np.uint8))


def test_cpp_caller_compiles(tmp_path):
    src = tmp_path / "msm_batch.cpp"
    src.write_text(r'''
#include "jubjub_hip.hpp"
int main() {
  try {
    jubjub::Context c(0);
    jubjub::AffineBatch pts = jubjub::AffineBatch::identity(c, 4);
    std::vector<jubjub::FrBatch> rows;
    std::vector<jubjub::AffineBatch> row_pts(2, pts);
    jubjub::AffineBatch a = jubjub::msm_batch(c, pts, rows);
    jubjub::AffineBatch b = jubjub::msm_batch(c, row_pts, rows);
    return (int)(a.len() + b.len());
  } catch (const jubjub::Error& e) {
    return 1;
  }
}
''')
    lib_dir = os.path.join(ROOT, "jubjub_amd", "lib")
    out = tmp_path / "msm_batch"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-L", lib_dir, "-ljubjub_hip",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", str(out)])
    assert out.exists()
