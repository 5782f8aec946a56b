"""The C ABI of the fused fixed + variable multiplication (jj_fixedvar_mul_vartime, _compressed), without a device: the symbols are exported and
bound, the header declares them, and a NULL context is refused before any device work."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["jj_fixedvar_mul_vartime", "jj_fixedvar_mul_vartime_compressed"]


def test_symbols_are_exported_and_bound():
    from jubjub_amd import _lib

    lib = _lib.load()
    dyn = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (\w+)", dyn))
    for name in NAMES:
        assert name in _lib.EXPORTS and name in exported, name
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int
        assert len(fn.argtypes) == 7


def test_header_declares_the_entry_points():
    with open(os.path.join(ROOT, "include", "jubjub_hip.h")) as f:
        h = f.read()
    assert re.search(r"int jj_fixedvar_mul_vartime\(jj_ctx\*, const jj_table\* t, size_t n, const void\* a32, const void\* b32, const void\* q64, void\* out64\);", h)
    assert re.search(r"int jj_fixedvar_mul_vartime_compressed\(jj_ctx\*, const jj_table\* t, size_t n, const void\* a32, const void\* b32, const void\* q64, void\* out32\);", h)


def test_entry_points_refuse_a_null_context():
    """JJ_ERR_INVALID before any device work (no crash, no CPU fallback), whatever the table pointer and n"""
    from jubjub_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for n in (0, 1):
        for fn in (lib.jj_fixedvar_mul_vartime, lib.jj_fixedvar_mul_vartime_compressed):
            assert fn(None, None, n, p, p, p, p) == _lib.JJ_ERR_INVALID
            assert fn(None, None, n, None, None, None, None) == _lib.JJ_ERR_INVALID
