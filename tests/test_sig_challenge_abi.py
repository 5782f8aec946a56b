"""CPU-side checks of jj_sig_challenge's place in the C ABI: the header declares the prototype the issue fixes and no longer says that the
library knows no hash, the library exports the symbol, the Python, C++ and Rust bindings name it with the same argument list, the RedJubjub
personalisation lives in the Python module and not in the C library, and the argument errors that need no device are refused.  No GPU."""
import ctypes
import os
import re

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "jubjub_hip.h")


def test_header_declares_the_prototype():
    text = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    proto = re.search(r"int\s+jj_sig_challenge\s*\(([^)]*)\)\s*;", code)
    assert proto, "jj_sig_challenge is not declared"
    args = [re.sub(r"\s+", " ", a.strip()) for a in proto.group(1).split(",")]
    assert args == ["jj_ctx*", "size_t n", "const void* personal16", "const void* r32", "const void* a32", "const void* msgs", "size_t msg_len", "const uint64_t* offsets", "void* c32"]
    assert "knows no hash" not in text and "the caller hashes" not in text
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int jj_sig_challenge", text, re.S)
    assert m and "BLAKE2b-512" in m.group(1) and "JJ_ERR_INVALID" in m.group(1) and "k_sig_challenge" in m.group(1) and "jj_sigbatch_begin" in m.group(1)


def test_library_exports_the_symbol_and_bindings_name_it():
    import __graft_entry__ as ge

    ge.build()
    lib = ctypes.CDLL(os.path.join(ROOT, "jubjub_amd", "lib", "libjubjub_hip.so"))
    assert hasattr(lib, "jj_sig_challenge")
    from jubjub_amd import _lib, engine

    assert "jj_sig_challenge" in _lib.EXPORTS
    sig = _lib._SIGS["jj_sig_challenge"]
    assert len(sig) + 1 == 9                                                  # the context comes first
    assert sig[0] is ctypes.c_size_t and sig[5] is ctypes.c_size_t and all(t is ctypes.c_void_p for k, t in enumerate(sig) if k not in (0, 5))
    for name in ("sig_challenge", "sigverify_each_msgs", "sigbatch_verify_msgs"):
        assert callable(getattr(engine.Engine, name)), name
    assert engine.REDJUBJUB_PERSONAL == b"Zcash_RedJubjubH"
    ffi = open(os.path.join(ROOT, "rust-shim", "src", "ffi.rs")).read()
    assert ("pub fn jj_sig_challenge(ctx: *mut JjCtx, n: usize, personal16: *const c_void, r32: *const c_void, a32: *const c_void, msgs: *const c_void, "
            "msg_len: usize, offsets: *const u64, c32: *mut c_void) -> c_int;") in ffi
    assert "jj_sig_challenge(" in open(os.path.join(ROOT, "rust-shim", "src", "lib.rs")).read()
    assert "jj_sig_challenge(" in open(os.path.join(ROOT, "include", "jubjub_hip.hpp")).read()
    # the .hpp wrapper is EXECUTED by tests/test_cpp_mirror.py (group sig, on the GPU) and tests/test_cpp_mirror_stub_cpu.py (offsets, NULLs)


def test_the_c_library_holds_no_protocol_string():
    from jubjub_amd import _lib

    blob = open(_lib.LIB_PATH, "rb").read()
    assert b"RedJubjub" not in blob and b"Zcash" not in blob
    csrc = os.path.join(ROOT, "jubjub_amd", "csrc")
    assert "getenv" not in open(os.path.join(csrc, "jj_blake2b.h")).read()


def test_argument_errors_that_need_no_device():
    """a NULL context is refused before anything is looked at, whatever else is given; the output stays as it was"""
    import __graft_entry__ as ge

    ge.build()
    from jubjub_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_uint8 * 64)(*([0xEE] * 64))
    p = ctypes.cast(buf, ctypes.c_void_p)
    offsets = (ctypes.c_uint64 * 2)(0, 4)
    for n in (0, 1):
        assert lib.jj_sig_challenge(None, n, None, p, p, p, 4, None, p) == _lib.JJ_ERR_INVALID
        assert lib.jj_sig_challenge(None, n, b"Zcash_RedJubjubH", None, None, p, 0, ctypes.cast(offsets, ctypes.c_void_p), p) == _lib.JJ_ERR_INVALID
    assert bytes(buf) == b"\xee" * 64
