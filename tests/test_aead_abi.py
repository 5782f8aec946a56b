"""CPU-side checks of jj_poly1305's, jj_aead_open's and jj_aead_seal's place in the C ABI: the header declares the three prototypes the issue
fixes, behind jj_chacha20_xor, and documents the contract, the refusals, the timing claim and the Sapling shapes; "Poly1305" is no longer
out of scope; the library exports the symbols; the Python, C++ and Rust bindings name them with the same argument lists; the Engine's shape
checks raise before any C call; and the argument errors that need no device are refused with the outputs untouched.  No GPU."""
import ctypes
import os
import re
import threading

import numpy as np
import pytest
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "jubjub_hip.h")
MAC_ARGS = ["jj_ctx*", "size_t n", "const void* keys32", "const void* in", "size_t len", "size_t in_stride", "void* tag16"]
OPEN_ARGS = ["jj_ctx*", "size_t n", "const void* keys32", "const void* nonce12", "const void* aad", "size_t aad_len", "const void* in", "size_t len", "size_t in_stride",
             "void* out", "uint8_t* ok"]
SEAL_ARGS = OPEN_ARGS[:-1]


def _header():
    text = open(HEADER).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _args(code, name):
    proto = re.search(r"int\s+%s\s*\(([^)]*)\)\s*;" % name, code)
    assert proto, "%s is not declared" % name
    return [re.sub(r"\s+", " ", a.strip()) for a in proto.group(1).split(",")]


def test_header_declares_and_documents_the_prototypes():
    text, code = _header()
    assert _args(code, "jj_poly1305") == MAC_ARGS and _args(code, "jj_aead_open") == OPEN_ARGS and _args(code, "jj_aead_seal") == SEAL_ARGS
    assert code.index("jj_chacha20_xor(") < code.index("jj_poly1305(") < code.index("jj_aead_open(") < code.index("jj_aead_seal(") < code.index("jj_blake2s(")
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int jj_poly1305\(", text, re.S)
    assert m, "no comment in front of the three entry points"
    doc = re.sub(r"\s*\n \*\s*", " ", m.group(1))
    for needle in ("RFC 8439", "JJ_ERR_INVALID", "k_poly1305", "k_aead<false>", "k_aead<true>", "neither the instruction stream nor any memory address depends on keys, data, tags or verdicts",
                   "len 564 in a stride of 580", "len 64 in a stride of 80", "a multiple of 4 in 4..1024", "n * in_stride <= 2^32", "aad_len <= 64", "NULL = twelve zero bytes",
                   "must not overlap", "n = 0 succeeds and touches nothing", "(n - 1) * in_stride + len", "launch stream", "tests/test_codegen_aead.py", "profiles/aead_ab.txt",
                   "a failed row never holds plaintext", "OUT OF SCOPE", "per-unit scalars", "note-commitment", "per-row nonces or aad", "not a multiple of 4", "0 - ok"):
        assert needle in doc, needle
    # Poly1305 has left the out-of-scope sentence of the key agreement's block
    ka = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*#define JJ_KA_COFACTOR", text, re.S).group(1)
    scope = re.sub(r"\s*\n \*\s*", " ", ka).split("OUT OF SCOPE:")[1].split(".")[0]
    assert "Poly1305" not in scope and "per-unit scalars" in scope
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for line in design.splitlines():
        if line.startswith("**Out of scope**"):
            assert "Poly1305" not in line
    assert "jj_aead_open" in design and "jj_poly1305.h" in design
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "aead_open(" in readme and "jj_poly1305.h" in readme
    assert "jj_aead_open" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "tests/cpp/emu_aead" in open(os.path.join(ROOT, ".gitignore")).read().split()
    build = open(os.path.join(ROOT, "jubjub_amd", "build.py")).read()
    assert '"jj_chacha20.h", "jj_poly1305.h"' in build


def test_library_exports_the_symbols_and_bindings_name_them():
    import __graft_entry__ as ge

    ge.build()
    lib = ctypes.CDLL(os.path.join(ROOT, "jubjub_amd", "lib", "libjubjub_hip.so"))
    assert all(hasattr(lib, f) for f in ("jj_poly1305", "jj_aead_open", "jj_aead_seal"))
    from jubjub_amd import _lib, engine

    assert {"jj_poly1305", "jj_aead_open", "jj_aead_seal"} <= set(_lib.EXPORTS)
    sz, vp = ctypes.c_size_t, ctypes.c_void_p
    assert _lib._SIGS["jj_poly1305"] == [sz, vp, vp, sz, sz, vp]
    assert _lib._SIGS["jj_aead_open"] == [sz, vp, vp, vp, sz, vp, sz, sz, vp, vp]
    assert _lib._SIGS["jj_aead_seal"] == [sz, vp, vp, vp, sz, vp, sz, sz, vp]
    for name in ("poly1305", "aead_open", "aead_seal", "ka_open_aead", "ka_open", "chacha20_xor"):
        assert callable(getattr(engine.Engine, name)), name
    import inspect

    assert list(inspect.signature(engine.Engine.aead_open).parameters) == ["self", "keys", "data", "nonce", "aad", "length", "out"]
    assert list(inspect.signature(engine.Engine.aead_seal).parameters) == ["self", "keys", "data", "nonce", "aad", "length", "out"]
    assert list(inspect.signature(engine.Engine.poly1305).parameters) == ["self", "keys", "data", "length", "out"]
    assert list(inspect.signature(engine.Engine.ka_open_aead).parameters) == ["self", "sk", "P", "ct", "personal", "flags", "nonce", "aad", "length"]
    assert list(inspect.signature(engine.Engine.ka_open).parameters) == ["self", "sk", "P", "ct", "personal", "flags", "nonce", "counter", "length"]      # as it was
    ffi = open(os.path.join(ROOT, "rust-shim", "src", "ffi.rs")).read()
    assert "pub fn jj_poly1305(ctx: *mut JjCtx, n: usize, keys32: *const c_void, in_: *const c_void, len: usize, in_stride: usize, tag16: *mut c_void) -> c_int;" in ffi
    assert ("pub fn jj_aead_open(ctx: *mut JjCtx, n: usize, keys32: *const c_void, nonce12: *const c_void, aad: *const c_void, aad_len: usize, in_: *const c_void, len: usize, "
            "in_stride: usize, out: *mut c_void, ok: *mut u8) -> c_int;") in ffi
    assert ("pub fn jj_aead_seal(ctx: *mut JjCtx, n: usize, keys32: *const c_void, nonce12: *const c_void, aad: *const c_void, aad_len: usize, in_: *const c_void, len: usize, "
            "in_stride: usize, out: *mut c_void) -> c_int;") in ffi
    for f in (os.path.join("rust-shim", "src", "lib.rs"), os.path.join("include", "jubjub_hip.hpp")):
        src = open(os.path.join(ROOT, f)).read()
        assert "jj_poly1305(" in src and "jj_aead_open(" in src and "jj_aead_seal(" in src, f
        # the .hpp wrappers are EXECUTED by tests/test_cpp_mirror.py (group aead, on the GPU) and tests/test_cpp_mirror_stub_cpu.py (sizes, strides, NULLs)


class _NoCalls:
    """stands in for the loaded library: any C call is a failure of the test"""

    def __getattr__(self, name):
        raise AssertionError("the C library was called (%s) before the shapes were checked" % name)


def test_engine_shape_checks_raise_before_any_c_call():
    from jubjub_amd.engine import Engine

    eng = Engine.__new__(Engine)
    eng._lib, eng._ctx, eng._mu = _NoCalls(), None, threading.RLock()
    keys = np.zeros((3, 32), np.uint8)
    bad = [
        lambda: eng.poly1305(keys, np.zeros((3, 50), np.uint8)),                         # stride no multiple of 4
        lambda: eng.poly1305(keys, np.zeros((3, 56), np.uint8), length=50),
        lambda: eng.poly1305(keys, np.zeros((3, 56), np.uint8), length=0),
        lambda: eng.poly1305(keys, np.zeros((3, 56), np.uint8), length=60),              # longer than the stride
        lambda: eng.poly1305(keys, np.zeros((3, 1028), np.uint8)),
        lambda: eng.poly1305(keys[:2], np.zeros((3, 56), np.uint8)),
        lambda: eng.poly1305(keys.reshape(-1), np.zeros((3, 56), np.uint8)),
        lambda: eng.poly1305(keys, np.zeros((3, 56), np.uint8), out=np.zeros((3, 15), np.uint8)),
        lambda: eng.aead_seal(keys, np.zeros((3, 56), np.uint8), length=54),
        lambda: eng.aead_seal(keys, np.zeros((3, 56), np.uint8), nonce=b"short"),
        lambda: eng.aead_seal(keys, np.zeros((3, 56), np.uint8), aad=bytes(65)),
        lambda: eng.aead_seal(keys, np.zeros((3, 56), np.uint8), out=np.zeros((3, 56), np.uint8)),      # len + 16 = 72 expected
        lambda: eng.aead_open(keys, np.zeros((3, 16), np.uint8)),                         # nothing in front of the tag
        lambda: eng.aead_open(keys, np.zeros((3, 68), np.uint8), length=56),              # no room for the tag
        lambda: eng.aead_open(keys, np.zeros((3, 1044), np.uint8)),                       # len 1028
        lambda: eng.aead_open(keys, np.zeros((3, 68), np.uint8), aad=bytes(65)),
        lambda: eng.aead_open(keys, np.zeros((3, 68), np.uint8), nonce=bytes(13)),
        lambda: eng.aead_open(keys, np.zeros((3, 68), np.uint8), out=np.zeros((3, 52), np.uint8)),      # (plain, ok) expected
        lambda: eng.aead_open(keys, np.zeros((3, 68), np.uint8), out=(np.zeros((3, 52), np.uint8), np.zeros(4, np.uint8))),
        lambda: eng.aead_open(np.zeros((4, 32), np.uint8), np.zeros((3, 68), np.uint8)),
    ]
    for k, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            raise AssertionError("case %d was not refused" % k)


def test_argument_errors_that_need_no_device():
    """a NULL context is refused before anything is looked at, whatever else is given; the outputs stay as they were"""
    import __graft_entry__ as ge

    ge.build()
    from jubjub_amd import _lib

    lib = _lib.load()
    INVALID = _lib.JJ_ERR_INVALID
    buf = (ctypes.c_uint8 * 4096)(*([0xEE] * 4096))
    p = ctypes.cast(buf, ctypes.c_void_p)
    q = ctypes.c_void_p(p.value + 2048)
    for n in (0, 1):
        for length, stride in ((52, 72), (564, 580), (4, 20), (1024, 1040), (0, 16), (6, 24), (1028, 1044), (52, 64), (52, 70)):
            assert lib.jj_poly1305(None, n, p, p, length, stride, q) == INVALID
            for aad, aad_len in ((None, 0), (b"x" * 12, 12), (None, 5), (b"x" * 65, 65)):
                assert lib.jj_aead_open(None, n, p, None, aad, aad_len, p, length, stride, q, q) == INVALID
                assert lib.jj_aead_seal(None, n, p, None, aad, aad_len, p, length, stride, q) == INVALID
    assert bytes(buf) == b"\xee" * 4096
