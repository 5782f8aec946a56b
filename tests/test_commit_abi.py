"""CPU-side checks of jj_pedersen_commit_vartime's place in the C ABI: the header declares the prototype the issue fixes and its comment carries
the contract, the library exports the symbol, the Python, C++ and Rust bindings name it, the protocol's constants live in the Python package
alone, and a NULL context is refused with the output untouched.  No GPU."""
import ctypes
import os
import re

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "jubjub_hip.h")
NAME = "jj_pedersen_commit_vartime"
PROTO = ["jj_ctx*", "const jj_table* ped", "const jj_table* rbase", "size_t n", "unsigned prefix", "int prefix_bits", "int nsrc", "const void* const* srcs",
         "const size_t* strides", "int nfields", "const uint32_t* fields", "const void* r32", "unsigned flags", "void* out"]


def test_header_declares_the_prototype_and_states_the_contract():
    text = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    proto = re.search(r"int\s+%s\s*\(([^)]*)\)\s*;" % NAME, code)
    assert proto, "%s is not declared" % NAME
    assert [re.sub(r"\s+", " ", a.strip()) for a in proto.group(1).split(",")] == PROTO
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int %s" % NAME, text, re.S)
    assert m, "no comment in front of the prototype"
    words = ("VARIABLE-TIME", "CONSTANT-TIME", "JJ_ERR_INVALID", "k_pedersen_commit", "byte for byte", "jj_point_add(jj_pedersen_hash_vartime", "jj_fixedbase_mul(rbase, r)",
             "n = 0 succeeds and touches nothing", "knows no protocol", "(src, byte_offset, nbits)", "HOST array", "OUT OF SCOPE")
    comment = re.sub(r"\s*\n \*\s*", " ", m.group(1))
    assert all(w in comment for w in words), [w for w in words if w not in comment]


def test_library_exports_the_symbol_and_bindings_name_it():
    import __graft_entry__ as ge

    ge.build()
    lib = ctypes.CDLL(os.path.join(ROOT, "jubjub_amd", "lib", "libjubjub_hip.so"))
    from jubjub_amd import _lib, engine

    ffi = open(os.path.join(ROOT, "rust-shim", "src", "ffi.rs")).read()
    rs = open(os.path.join(ROOT, "rust-shim", "src", "lib.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "jubjub_hip.hpp")).read()
    assert hasattr(lib, NAME) and NAME in _lib.EXPORTS
    sig = _lib._SIGS[NAME]
    assert len(sig) + 1 == len(PROTO)                                                  # the context comes first
    assert sig[2] is ctypes.c_size_t and sig[6] is ctypes.POINTER(ctypes.c_void_p) and sig[7] is ctypes.POINTER(ctypes.c_size_t) and sig[9] is ctypes.POINTER(ctypes.c_uint32)
    assert ("pub fn jj_pedersen_commit_vartime(ctx: *mut JjCtx, ped: *const JjTable, rbase: *const JjTable, n: usize, prefix: c_uint, prefix_bits: c_int, nsrc: c_int, "
            "srcs: *const *const c_void, strides: *const usize, nfields: c_int, fields: *const u32, r32: *const c_void, flags: c_uint, out: *mut c_void) -> c_int;") in ffi
    assert NAME + "(" in rs and "pub fn commit(" in rs and NAME + "(" in hpp and "commit(" in hpp and "commit_points(" in hpp
    # the .hpp wrappers are EXECUTED by tests/test_cpp_mirror_commit.py (on the GPU)
    for name in ("pedersen_commit", "note_commit", "note_check"):
        assert callable(getattr(engine.Engine, name)), name
    assert engine.SAPLING_EXPAND_PERSONAL == b"Zcash_ExpandSeed" and (engine.SAPLING_NOTE_PREFIX, engine.SAPLING_NOTE_PREFIX_BITS) == (0b111111, 6)
    for name in ("pedersen_commit", "note_check"):
        doc = getattr(engine.Engine, name).__doc__
        assert "VARIABLE-TIME" in doc and "CONSTANT-TIME" in doc, name


def test_the_c_library_still_holds_no_protocol_string():
    from jubjub_amd import _lib

    blob = open(_lib.LIB_PATH, "rb").read()
    assert b"Zcash" not in blob and b"Sapling" not in blob and b"ExpandSeed" not in blob
    for f in ("jj_pedersen.h", "jj_abi.hip", "jj_kernels.h"):
        src = open(os.path.join(ROOT, "jubjub_amd", "csrc", f)).read()
        assert "ExpandSeed" not in src and "Zcash_" not in src, f


def test_a_null_context_is_refused_with_the_output_untouched():
    import __graft_entry__ as ge

    ge.build()
    from jubjub_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_uint8 * 96)(*([0xEE] * 96))
    p = ctypes.cast(buf, ctypes.c_void_p)
    srcs = (ctypes.c_void_p * 1)(p.value)
    strides = (ctypes.c_size_t * 1)(32)
    fields = (ctypes.c_uint32 * 3)(0, 0, 8)
    handle = ctypes.c_void_p(0x1234)                                                  # never looked at: the context is checked first
    for n in (0, 1):
        for flags in (0, 1):
            assert lib.jj_pedersen_commit_vartime(None, handle, handle, n, 5, 6, 1, srcs, strides, 1, fields, p, flags, p) == _lib.JJ_ERR_INVALID
            assert lib.jj_pedersen_commit_vartime(None, handle, None, n, 0, 0, 1, srcs, strides, 1, fields, None, flags, p) == _lib.JJ_ERR_INVALID
    assert bytes(buf) == b"\xee" * 96
