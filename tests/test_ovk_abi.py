"""CPU-side checks of the place of jj_blake2b and jj_ka_kdf_each in the C ABI: the header declares the two prototypes exactly and their comment
carries the contract, the library exports the symbols, the Python, C++ and Rust bindings name them, the protocol's constant lives in the
Python package alone, and a NULL context is refused with the outputs untouched.  No GPU."""
import ctypes
import os
import re

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "jubjub_hip.h")
PROTOS = {
    "jj_blake2b": ["jj_ctx*", "size_t n", "int digest_len", "const void* personal16", "const void* prefix", "size_t prefix_len", "int nsrc", "const void* const* srcs",
                   "const size_t* lens", "const size_t* strides", "void* out"],
    "jj_ka_kdf_each": ["jj_ctx*", "size_t n", "const void* sk32", "const void* p32", "const void* h32", "unsigned flags", "const void* personal16", "void* key32", "uint8_t* ok"],
}
WORDS = ("CONSTANT-TIME", "JJ_ERR_INVALID", "n = 0 succeeds and touches nothing", "knows no protocol", "OUT OF SCOPE", "k_blake2b<32|64>", "k_varbase_mont_ka_each<cofactor>",
         "k_ka_kdf<true>", "RFC 7693", "0x01010000 | digest_len", "32 or 64", "NULL = sixteen zero bytes", "0..4096 and a multiple of 4", "a multiple of 4 in 4..65536",
         "n * strides[s] <= 2^32", "n <= 2^24", "HOST arrays", "(n - 1) * stride + len", "out must not overlap a source", "16-byte aligned", "jj_aead_open", "keys32",
         "the low 252 bits", "A non-NULL h32 without that flag", "cleared on the launch stream behind the last chunk", "tests/test_codegen_ovk.py", "profiles/ovk_ab.txt",
         "compaction of hit rows", "quad-of-lanes form", "ragged lengths", "keyed or salted BLAKE2b", "digest lengths other than 32 and 64", "per-row nonces", "jj_multi_* form")


def _header():
    text = open(HEADER).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_prototypes_and_states_the_contract():
    text, code = _header()
    for name, want in PROTOS.items():
        proto = re.search(r"int\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert proto, "%s is not declared" % name
        assert [re.sub(r"\s+", " ", a.strip()) for a in proto.group(1).split(",")] == want, name
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int jj_blake2b\(", text, re.S)
    assert m, "no comment in front of the two prototypes"
    comment = re.sub(r"\s*\n \*\s*", " ", m.group(1))
    assert all(w in comment for w in WORDS), [w for w in WORDS if w not in comment]
    assert code.index("jj_group_hash(") < code.index("jj_blake2b(") < code.index("jj_ka_kdf_each(")
    # the two sentences that named the sender's side as missing now point at the new calls
    ka = re.sub(r"\s*\n \*\s*", " ", re.search(r"/\*((?:(?!\*/).)*?)\*/\s*#define JJ_KA_COFACTOR", text, re.S).group(1))
    aead = re.sub(r"\s*\n \*\s*", " ", re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int jj_poly1305\(", text, re.S).group(1))
    assert "jj_ka_kdf_each" in ka.split("OUT OF SCOPE:")[1].split(".")[0] and "a hash of the caller's" not in ka
    assert "jj_ka_kdf_each" in aead.split("OUT OF SCOPE:")[1] and "jj_blake2b" in aead.split("OUT OF SCOPE:")[1]


def test_library_exports_the_symbols_and_bindings_name_them():
    import __graft_entry__ as ge

    ge.build()
    lib = ctypes.CDLL(os.path.join(ROOT, "jubjub_amd", "lib", "libjubjub_hip.so"))
    from jubjub_amd import _lib, engine

    ffi = open(os.path.join(ROOT, "rust-shim", "src", "ffi.rs")).read()
    rs = open(os.path.join(ROOT, "rust-shim", "src", "lib.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "jubjub_hip.hpp")).read()
    for name, proto in PROTOS.items():
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
        assert len(_lib._SIGS[name]) + 1 == len(proto), name                           # the context comes first
        assert name + "(" in rs and name + "(" in hpp, name
    sig = _lib._SIGS["jj_blake2b"]
    assert sig[0] is ctypes.c_size_t and sig[1] is ctypes.c_int and sig[6] is ctypes.POINTER(ctypes.c_void_p) and sig[7] is sig[8] is ctypes.POINTER(ctypes.c_size_t)
    assert ("pub fn jj_blake2b(ctx: *mut JjCtx, n: usize, digest_len: c_int, personal16: *const c_void, prefix: *const c_void, prefix_len: usize, nsrc: c_int, "
            "srcs: *const *const c_void, lens: *const usize, strides: *const usize, out: *mut c_void) -> c_int;") in ffi
    assert ("pub fn jj_ka_kdf_each(ctx: *mut JjCtx, n: usize, sk32: *const c_void, p32: *const c_void, h32: *const c_void, flags: c_uint, personal16: *const c_void, "
            "key32: *mut c_void, ok: *mut u8) -> c_int;") in ffi
    assert "pub fn blake2b(" in rs and "pub fn ka_kdf_each(" in rs and "inline KaKeys ka_kdf_each(" in hpp and " blake2b(const Context& c" in hpp
    # the .hpp wrappers are EXECUTED by tests/test_cpp_mirror_ovk.py (on the GPU)
    for name in ("blake2b", "ka_kdf_each", "note_encrypt", "ovk_open"):
        assert callable(getattr(engine.Engine, name)), name
    assert engine.SAPLING_OCK_PERSONAL == b"Zcash_Derive_ock"
    assert "CONSTANT-TIME" in engine.Engine.ka_kdf_each.__doc__ and "waits for the device" in engine.Engine.ovk_open.__doc__
    assert "knows no protocol" in engine.Engine.blake2b.__doc__ and "knows no protocol" in engine.Engine.note_encrypt.__doc__


def test_the_sapling_constant_is_in_the_python_package_only():
    from jubjub_amd import _lib

    blob = open(_lib.LIB_PATH, "rb").read()
    assert b"Zcash" not in blob and b"Derive_ock" not in blob
    for d, names in (("jubjub_amd/csrc", None), ("include", None), ("rust-shim/src", None)):
        for f in sorted(os.listdir(os.path.join(ROOT, d))):
            src = open(os.path.join(ROOT, d, f), errors="replace").read()
            assert "Derive_ock" not in src, os.path.join(d, f)
    assert "Derive_ock" in open(os.path.join(ROOT, "jubjub_amd", "engine.py")).read()


def test_a_null_context_is_refused_with_the_outputs_untouched():
    import __graft_entry__ as ge

    ge.build()
    from jubjub_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_uint8 * 256)(*([0xEE] * 256))
    p = ctypes.cast(buf, ctypes.c_void_p)
    srcs = (ctypes.c_void_p * 1)(p.value + 128)
    lens = (ctypes.c_size_t * 1)(32)
    strides = (ctypes.c_size_t * 1)(32)
    for n in (0, 1, 2):
        for digest_len in (32, 64):
            assert lib.jj_blake2b(None, n, digest_len, None, None, 0, 1, srcs, lens, strides, p) == _lib.JJ_ERR_INVALID
            assert lib.jj_blake2b(None, n, digest_len, None, None, 0, 0, None, None, None, p) == _lib.JJ_ERR_INVALID
        for flags in (0, 1 | 32 | 64):
            assert lib.jj_ka_kdf_each(None, n, p.value + 64, p.value + 128, None, flags, None, p, p.value + 192) == _lib.JJ_ERR_INVALID
    assert bytes(buf) == b"\xee" * 256
