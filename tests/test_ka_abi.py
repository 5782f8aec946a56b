"""CPU-side checks of jj_ka_kdf's and jj_chacha20_xor's place in the C ABI: the header declares the two prototypes the issue fixes and states the
constant-time claim in the words jj_varbase_mul uses, the flag values are disjoint from the JJ_DECOMPRESS_* bits, the library exports the
symbols, the Python, C++ and Rust bindings name them with the same argument lists, the Sapling personalisation lives in the Python module and
not in the C library, and the argument errors that need no device are refused with the outputs untouched.  No GPU."""
import ctypes
import os
import re

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "jubjub_hip.h")


def _header():
    text = open(HEADER).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _args(code, name):
    proto = re.search(r"int\s+%s\s*\(([^)]*)\)\s*;" % name, code)
    assert proto, "%s is not declared" % name
    return [re.sub(r"\s+", " ", a.strip()) for a in proto.group(1).split(",")]


def test_header_declares_the_prototypes():
    text, code = _header()
    assert _args(code, "jj_ka_kdf") == ["jj_ctx*", "size_t n", "const void* sk32", "const void* p32", "unsigned flags", "const void* personal16", "void* key32", "uint8_t* ok"]
    assert _args(code, "jj_chacha20_xor") == ["jj_ctx*", "size_t n", "const void* keys32", "const void* nonce12", "unsigned counter", "const void* in", "size_t len",
                                              "size_t in_stride", "void* out"]
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*#define JJ_KA_COFACTOR", text, re.S)
    assert m, "no comment in front of the two entry points"
    doc = re.sub(r"\s*\n \*\s*", " ", m.group(1))
    for needle in ("CONSTANT-TIME in sk32 and in the share", "neither the instruction stream nor any memory address depends on", "JJ_ERR_INVALID", "k_varbase_mont_ka",
                   "k_ka_kdf", "k_chacha20_xor", "no quad-of-lanes form", "0x01010020", "tests/test_codegen_ka.py", "per-unit scalars", "Poly1305", "note-commitment", "_vartime variant",
                   "launch stream", "Zcash_SaplingKDF", "RFC 8439"):
        assert needle in doc, needle
    # the words of jj_varbase_mul's own claim
    vb = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int jj_varbase_mul\(", text, re.S).group(1)
    assert "neither the instruction stream nor any memory" in vb


def test_flag_values_are_disjoint_from_the_decoder_bits():
    _, code = _header()
    val = lambda name: int(re.search(r"#define %s\s+(\d+)u" % name, code).group(1))      # noqa: E731
    cof, inp = val("JJ_KA_COFACTOR"), val("JJ_KA_HASH_INPUT")
    assert (cof, inp) == (32, 64)
    dec = [val("JJ_DECOMPRESS_" + n) for n in ("ZIP216", "TORSION_FREE", "NOT_SMALL_ORDER", "CLEAR_COFACTOR")]
    assert dec == [1, 2, 4, 8]
    every = dec + [val("JJ_SIG_COFACTORLESS"), cof, inp]
    assert sum(every) == 127 and all(v & (v - 1) == 0 for v in every)                    # seven flags, seven different bits
    from jubjub_amd import engine

    assert (engine.FLAG_KA_COFACTOR, engine.FLAG_KA_HASH_INPUT) == (cof, inp) and engine.KA_SAPLING_FLAGS == 1 | cof | inp


def test_library_exports_the_symbols_and_bindings_name_them():
    import __graft_entry__ as ge

    ge.build()
    lib = ctypes.CDLL(os.path.join(ROOT, "jubjub_amd", "lib", "libjubjub_hip.so"))
    assert hasattr(lib, "jj_ka_kdf") and hasattr(lib, "jj_chacha20_xor")
    from jubjub_amd import _lib, engine

    assert {"jj_ka_kdf", "jj_chacha20_xor"} <= set(_lib.EXPORTS)
    sig = _lib._SIGS["jj_ka_kdf"]
    assert len(sig) + 1 == 8 and sig[0] is ctypes.c_size_t and sig[3] is ctypes.c_uint and all(t is ctypes.c_void_p for k, t in enumerate(sig) if k not in (0, 3))
    sig = _lib._SIGS["jj_chacha20_xor"]
    assert len(sig) + 1 == 9 and sig[3] is ctypes.c_uint and [k for k, t in enumerate(sig) if t is ctypes.c_size_t] == [0, 5, 6]
    for name in ("ka_kdf", "chacha20_xor", "ka_open"):
        assert callable(getattr(engine.Engine, name)), name
    assert engine.SAPLING_KDF_PERSONAL == b"Zcash_SaplingKDF"
    ffi = open(os.path.join(ROOT, "rust-shim", "src", "ffi.rs")).read()
    assert ("pub fn jj_ka_kdf(ctx: *mut JjCtx, n: usize, sk32: *const c_void, p32: *const c_void, flags: c_uint, personal16: *const c_void, key32: *mut c_void, "
            "ok: *mut u8) -> c_int;") in ffi
    assert ("pub fn jj_chacha20_xor(ctx: *mut JjCtx, n: usize, keys32: *const c_void, nonce12: *const c_void, counter: c_uint, in_: *const c_void, len: usize, "
            "in_stride: usize, out: *mut c_void) -> c_int;") in ffi
    for f in (os.path.join("rust-shim", "src", "lib.rs"), os.path.join("include", "jubjub_hip.hpp")):
        src = open(os.path.join(ROOT, f)).read()
        assert "jj_ka_kdf(" in src and "jj_chacha20_xor(" in src, f
        # the .hpp wrappers are EXECUTED by tests/test_cpp_mirror.py (group ka, on the GPU) and tests/test_cpp_mirror_stub_cpu.py (sizes, strides, NULLs)


def test_the_c_library_holds_no_protocol_string():
    from jubjub_amd import _lib

    blob = open(_lib.LIB_PATH, "rb").read()
    assert b"Sapling" not in blob and b"Zcash" not in blob
    csrc = os.path.join(ROOT, "jubjub_amd", "csrc")
    assert "getenv" not in open(os.path.join(csrc, "jj_chacha20.h")).read()


def test_argument_errors_that_need_no_device():
    """a NULL context is refused before anything is looked at, whatever else is given -- valid arguments, n = 0, flags or lengths that are errors
    of their own --; the outputs stay as they were"""
    import __graft_entry__ as ge

    ge.build()
    from jubjub_amd import _lib

    lib = _lib.load()
    INVALID = _lib.JJ_ERR_INVALID
    buf = (ctypes.c_uint8 * 256)(*([0xEE] * 256))
    p = ctypes.cast(buf, ctypes.c_void_p)
    q = ctypes.c_void_p(p.value + 128)
    for n in (0, 1):
        for flags in (0, 1 | 32 | 64, 8, 128):
            assert lib.jj_ka_kdf(None, n, p, p, flags, None, q, q) == INVALID
            assert lib.jj_ka_kdf(None, n, p, p, flags, b"Zcash_SaplingKDF", q, q) == INVALID
        for length, stride in ((52, 52), (52, 56), (4, 4), (1024, 1024), (0, 4), (6, 8), (1028, 1028), (8, 4), (8, 10)):
            assert lib.jj_chacha20_xor(None, n, p, None, 1, p, length, stride, q) == INVALID
    assert bytes(buf) == b"\xee" * 256
