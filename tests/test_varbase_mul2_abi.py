"""The C ABI of the two-term variable-base multiplication (jj_varbase_mul2_vartime, _compressed, jj_varbase_mul2_scalars), without a device: the
symbols are exported and bound, and arguments are checked before any device work."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["jj_varbase_mul2_vartime", "jj_varbase_mul2_vartime_compressed", "jj_varbase_mul2_scalars"]


def test_symbols_are_exported_and_bound():
    from jubjub_amd import _lib

    lib = _lib.load()
    dyn = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (\w+)", dyn))
    for name in NAMES:
        assert name in _lib.EXPORTS and name in exported, name
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int
    assert len(lib.jj_varbase_mul2_vartime.argtypes) == 7 and len(lib.jj_varbase_mul2_vartime_compressed.argtypes) == 7
    assert len(lib.jj_varbase_mul2_scalars.argtypes) == 6


def test_header_declares_the_entry_points():
    with open(os.path.join(ROOT, "include", "jubjub_hip.h")) as f:
        h = f.read()
    assert re.search(r"int jj_varbase_mul2_vartime\(jj_ctx\*, size_t n, const void\* a32, const void\* p64, const void\* b32, const void\* q64, void\* out64\);", h)
    assert re.search(r"int jj_varbase_mul2_vartime_compressed\(jj_ctx\*, size_t n, const void\* a32, const void\* p64, const void\* b32, const void\* q64, void\* out32\);", h)
    assert re.search(r"int jj_varbase_mul2_scalars\(jj_ctx\*, size_t n, const void\* ab64, const void\* p64, const void\* q64, void\* out64\);", h)
    assert "vb_mul2_window" in h


def test_entry_points_refuse_null_arguments():
    """a NULL context, and NULL ab64 whatever the context: JJ_ERR_INVALID before any device work (no crash, no CPU fallback)"""
    from jubjub_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for n in (0, 1):
        assert lib.jj_varbase_mul2_vartime(None, n, p, p, p, p, p) == _lib.JJ_ERR_INVALID
        assert lib.jj_varbase_mul2_vartime_compressed(None, n, p, p, p, p, p) == _lib.JJ_ERR_INVALID
        assert lib.jj_varbase_mul2_scalars(None, n, p, p, p, p) == _lib.JJ_ERR_INVALID
        assert lib.jj_varbase_mul2_scalars(None, n, None, p, p, p) == _lib.JJ_ERR_INVALID
    assert lib.jj_varbase_mul2_vartime(None, 1, None, None, None, None, None) == _lib.JJ_ERR_INVALID
