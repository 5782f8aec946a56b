"""CPU-side checks of jj_blake2s' and jj_group_hash's place in the C ABI: the header declares the two prototypes, says that the library knows no
protocol's personalisation or prefix and that the calls are variable-time over public inputs, adds no flag bit, the library exports the
symbols, the Python, C++ and Rust bindings name them with the same argument lists, the protocol's constants live in the Python module and not
in the C library, and a NULL context is refused with the outputs untouched.  No GPU."""
import ctypes
import os
import re

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "jubjub_hip.h")
HASH_ARGS = ["jj_ctx*", "size_t n", "const void* personal8", "const void* prefix", "size_t prefix_len", "const void* msgs", "size_t msg_len", "size_t msg_stride"]


def _header():
    text = open(HEADER).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _args(code, name):
    proto = re.search(r"int\s+%s\s*\(([^)]*)\)\s*;" % name, code)
    assert proto, "%s is not declared" % name
    return [re.sub(r"\s+", " ", a.strip()) for a in proto.group(1).split(",")]


def test_header_declares_the_prototypes():
    text, code = _header()
    assert _args(code, "jj_blake2s") == HASH_ARGS + ["void* out32"]
    assert _args(code, "jj_group_hash") == HASH_ARGS + ["unsigned flags", "void* out64", "uint8_t* ok"]
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int jj_blake2s\(", text, re.S)
    assert m, "no comment in front of the two entry points"
    doc = re.sub(r"\s*\n \*\s*", " ", m.group(1))
    for needle in ("RFC 7693", "0x01010020", "knows NONE of a protocol's personalisations or prefixes", "VARIABLE-TIME over public inputs", "like jj_decompress", "JJ_ERR_INVALID",
                   "k_blake2s", "launch stream", "2^20", "NO fused hash-and-decode kernel", "byte for byte what jj_decompress writes", "n * msg_stride <= 2^32", "n <= 2^24",
                   "0..4096", "0..65536", "16-byte aligned", "n = 0 succeeds", "ragged message lengths", "keyed or salted", "profiles/group_hash_ab.txt"):
        assert needle in doc, needle
    # no new flag bit: the seven of the header are the seven there were
    val = lambda name: int(re.search(r"#define %s\s+(\d+)u" % name, code).group(1))      # noqa: E731
    flags = re.findall(r"#define (JJ_(?:DECOMPRESS|SIG|KA)_[A-Z0-9_]+)\s+\d+u", code)
    assert sorted(val(f) for f in flags if f not in ("JJ_SIG_OK", "JJ_SIG_REJECT", "JJ_SIG_MALFORMED")) == [1, 2, 4, 8, 16, 32, 64]


def test_library_exports_the_symbols_and_bindings_name_them():
    import __graft_entry__ as ge

    ge.build()
    lib = ctypes.CDLL(os.path.join(ROOT, "jubjub_amd", "lib", "libjubjub_hip.so"))
    assert hasattr(lib, "jj_blake2s") and hasattr(lib, "jj_group_hash")
    from jubjub_amd import _lib, engine

    assert {"jj_blake2s", "jj_group_hash"} <= set(_lib.EXPORTS)
    sig = _lib._SIGS["jj_blake2s"]
    assert len(sig) + 1 == 9 and [k for k, t in enumerate(sig) if t is ctypes.c_size_t] == [0, 3, 5, 6] and all(t is ctypes.c_void_p for k, t in enumerate(sig) if k not in (0, 3, 5, 6))
    sig = _lib._SIGS["jj_group_hash"]
    assert len(sig) + 1 == 11 and [k for k, t in enumerate(sig) if t is ctypes.c_size_t] == [0, 3, 5, 6] and sig[7] is ctypes.c_uint
    for name in ("blake2s", "group_hash", "find_group_hash"):
        assert callable(getattr(engine.Engine, name)), name
    assert engine.SAPLING_GD_PERSONAL == b"Zcash_gd" and engine.SAPLING_PH_PERSONAL == b"Zcash_PH" and engine.GROUP_HASH_FLAGS == 1 | 4 | 8
    ffi = open(os.path.join(ROOT, "rust-shim", "src", "ffi.rs")).read()
    assert ("pub fn jj_blake2s(ctx: *mut JjCtx, n: usize, personal8: *const c_void, prefix: *const c_void, prefix_len: usize, msgs: *const c_void, msg_len: usize, "
            "msg_stride: usize, out32: *mut c_void) -> c_int;") in ffi
    assert ("pub fn jj_group_hash(ctx: *mut JjCtx, n: usize, personal8: *const c_void, prefix: *const c_void, prefix_len: usize, msgs: *const c_void, msg_len: usize, "
            "msg_stride: usize, flags: c_uint, out64: *mut c_void, ok: *mut u8) -> c_int;") in ffi
    for f in (os.path.join("rust-shim", "src", "lib.rs"), os.path.join("include", "jubjub_hip.hpp")):
        src = open(os.path.join(ROOT, f)).read()
        assert "jj_blake2s(" in src and "jj_group_hash(" in src, f
        # the .hpp wrappers are EXECUTED by tests/test_cpp_mirror.py (group hash, on the GPU) and tests/test_cpp_mirror_stub_cpu.py (sizes, strides, NULLs)


def test_the_c_library_holds_no_protocol_string():
    from jubjub_amd import _lib

    blob = open(_lib.LIB_PATH, "rb").read()
    for word in (b"Zcash", b"Sapling", b"GroupHash"):
        assert word not in blob, word
    csrc = os.path.join(ROOT, "jubjub_amd", "csrc")
    src = open(os.path.join(csrc, "jj_blake2s.h")).read()
    assert "getenv" not in src and "Zcash" not in src


def test_a_null_context_is_refused_with_the_outputs_untouched():
    """a NULL context is refused before anything is looked at, whatever else is given -- valid arguments, n = 0, flags or lengths that are errors
    of their own --; the outputs stay as they were"""
    import __graft_entry__ as ge

    ge.build()
    from jubjub_amd import _lib

    lib = _lib.load()
    INVALID = _lib.JJ_ERR_INVALID
    buf = (ctypes.c_uint8 * 512)(*([0xEE] * 512))
    p = ctypes.cast(buf, ctypes.c_void_p)
    q, r = ctypes.c_void_p(p.value + 128), ctypes.c_void_p(p.value + 384)
    for n in (0, 1):
        for personal in (None, b"12345678"):
            for prefix, plen in ((None, 0), (b"x" * 64, 64), (None, 5), (b"x", 4097)):
                for mlen, stride in ((11, 12), (0, 0), (11, 10), (65537, 65537)):
                    assert lib.jj_blake2s(None, n, personal, prefix, plen, p, mlen, stride, q) == INVALID
                    for flags in (0, 13, 15, 16, 1 << 31):
                        assert lib.jj_group_hash(None, n, personal, prefix, plen, p, mlen, stride, flags, q, r) == INVALID
    assert bytes(buf) == b"\xee" * 512


def test_rows_argument_copies_what_the_library_cannot_read_in_place():
    """Engine's (n, L) argument: rows that are adjacent bytes a fixed distance apart are read where they are, every other layout is copied --
    for ONE row as well, which has no row stride but still needs adjacent bytes"""
    import numpy as np

    from jubjub_amd.engine import _Rows

    def seen(r):
        if r.len == 0 or r.n == 0:
            return b""
        return b"".join(bytes((ctypes.c_uint8 * r.len).from_address(r.ptr + i * r.stride)) for i in range(r.n))

    a = np.arange(4 * 52, dtype=np.uint8).reshape(4, 52)
    for view, in_place in ((a[:, :11], True), (a[1:3, 5:16], True), (a[2:3, 7:18], True), (a, True), (a[:1], True),
                           (a[:1, ::2], False), (a[3:4, 1:23:2], False), (a[:, ::2], False), (a[::-1, :11], False), (a[:, 10::-1], False),
                           (np.broadcast_to(a[0, :8], (3, 8)), False), (a[:1, :1], True), (a[:, 3:4], True), (a[:1, 50::-1], False)):
        r = _Rows(view)
        assert (r.n, r.len) == view.shape and seen(r) == view.tobytes(), (view.shape, view.strides)
        lo, hi = a.ctypes.data, a.ctypes.data + a.size
        assert (lo <= r.ptr < hi) == in_place, (view.shape, view.strides)
    assert _Rows(a[:1, ::2]).stride == 26 and _Rows(a[:, :11]).stride == 52 and _Rows(a[2:3, 7:18]).stride == 11
    assert _Rows(a[:, :0]).ptr is None and _Rows(a[:0]).ptr is None
