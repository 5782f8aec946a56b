"""CPU-side checks of the Pedersen entry points' place in the C ABI: the header declares the three prototypes the issue fixes, the library
exports the symbols, the Python, C++ and Rust bindings name them, the binary still holds no protocol string, and a NULL context is refused with
the output untouched.  No GPU."""
import ctypes
import os
import re

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "jubjub_hip.h")
LAYOUT = ["unsigned prefix", "int prefix_bits", "const void* rows", "size_t row_stride", "int nfields", "const uint32_t* fields"]
PROTOS = {
    "jj_pedersen_table_create": ["jj_ctx*", "int nseg", "const void* gens64", "int seg_chunks", "int window_chunks", "jj_table** out"],
    "jj_pedersen_hash_vartime": ["jj_ctx*", "const jj_table* t", "size_t n"] + LAYOUT + ["unsigned flags", "void* out"],
    "jj_pedersen_scalars": ["jj_ctx*", "int nseg", "int seg_chunks", "size_t n"] + LAYOUT + ["void* scalars32"],
}
NAMES = sorted(PROTOS)


def test_header_declares_the_prototypes():
    text = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, want in PROTOS.items():
        proto = re.search(r"int\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert proto, "%s is not declared" % name
        assert [re.sub(r"\s+", " ", a.strip()) for a in proto.group(1).split(",")] == want, name
    assert re.search(r"#define\s+JJ_PEDERSEN_POINT\s+1u", code)
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*#define JJ_PEDERSEN_POINT", text, re.S)
    assert m and all(w in m.group(1) for w in ("VARIABLE-TIME", "JJ_ERR_INVALID", "k_pedersen_gather", "k_pedersen_scalars", "torsion-free", "jj_fixedbase_table_destroy"))


def test_library_exports_the_symbols_and_bindings_name_them():
    import __graft_entry__ as ge

    ge.build()
    lib = ctypes.CDLL(os.path.join(ROOT, "jubjub_amd", "lib", "libjubjub_hip.so"))
    from jubjub_amd import _lib, engine

    ffi = open(os.path.join(ROOT, "rust-shim", "src", "ffi.rs")).read()
    rs = open(os.path.join(ROOT, "rust-shim", "src", "lib.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "jubjub_hip.hpp")).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
        assert len(_lib._SIGS[name]) + 1 == len(PROTOS[name]), name                    # the context comes first
        assert "pub fn %s(" % name in ffi and name + "(" in rs and name + "(" in hpp, name
        # the .hpp wrappers are EXECUTED by tests/test_cpp_mirror.py (group pedersen, on the GPU) and tests/test_cpp_mirror_stub_cpu.py (sizes, nseg, NULLs)
    assert ("pub fn jj_pedersen_hash_vartime(ctx: *mut JjCtx, t: *const JjTable, n: usize, prefix: c_uint, prefix_bits: c_int, rows: *const c_void, row_stride: usize, "
            "nfields: c_int, fields: *const u32, flags: c_uint, out: *mut c_void) -> c_int;") in ffi
    sig = _lib._SIGS["jj_pedersen_hash_vartime"]
    assert sig[1] is ctypes.c_size_t and sig[2] is ctypes.c_uint and sig[5] is ctypes.c_size_t and sig[7] is ctypes.POINTER(ctypes.c_uint32)
    for name in ("pedersen_table", "pedersen_hash", "pedersen_scalars", "pedersen_merkle"):
        assert callable(getattr(engine.Engine, name)), name
    assert engine.FLAG_PEDERSEN_POINT == 1


def test_the_c_library_still_holds_no_protocol_string():
    from jubjub_amd import _lib

    blob = open(_lib.LIB_PATH, "rb").read()
    assert b"RedJubjub" not in blob and b"Zcash" not in blob and b"Sapling" not in blob
    src = open(os.path.join(ROOT, "jubjub_amd", "csrc", "jj_pedersen.h")).read()
    assert "getenv" not in src and "Zcash" not in src and "Sapling" not in src


def test_a_null_context_is_refused_with_the_output_untouched():
    import __graft_entry__ as ge

    ge.build()
    from jubjub_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_uint8 * 96)(*([0xEE] * 96))
    p = ctypes.cast(buf, ctypes.c_void_p)
    fields = (ctypes.c_uint32 * 2)(0, 8)
    handle = ctypes.c_void_p(0x1234)                                                  # never looked at: the context is checked first
    out = ctypes.c_void_p(0x5678)
    for n in (0, 1):
        assert lib.jj_pedersen_hash_vartime(None, handle, n, 0, 0, p, 32, 1, fields, 0, p) == _lib.JJ_ERR_INVALID
        assert lib.jj_pedersen_hash_vartime(None, handle, n, 5, 6, p, 32, 1, fields, 1, p) == _lib.JJ_ERR_INVALID
        assert lib.jj_pedersen_scalars(None, 3, 63, n, 0, 0, p, 32, 1, fields, p) == _lib.JJ_ERR_INVALID
    assert lib.jj_pedersen_table_create(None, 1, p, 63, 0, ctypes.byref(out)) == _lib.JJ_ERR_INVALID
    assert out.value == 0x5678 and bytes(buf) == b"\xee" * 96
