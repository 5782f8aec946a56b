"""CPU-side checks of jj_sigverify_each's place in the C ABI: the header declares the prototype and the constants the issue fixes, the flag
bit is clear of every JJ_DECOMPRESS_* bit, the library exports the symbol, the Python, C++ and Rust bindings name it with the same argument
list, and the shipped library still reads no JJ_* environment variable.  No GPU."""
import ctypes
import os
import re

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "jubjub_hip.h")


def _header():
    return open(HEADER).read()


def _defines():
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define\s+(JJ_[A-Z0-9_]+)\s+(\d+)u\b", _header(), re.M)}


def test_header_declares_the_prototype_and_constants():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    proto = re.search(r"int\s+jj_sigverify_each\s*\(([^)]*)\)\s*;", code)
    assert proto, "jj_sigverify_each is not declared"
    args = [re.sub(r"\s+", " ", a.strip()) for a in proto.group(1).split(",")]
    assert args == ["jj_ctx*", "const jj_table* t", "size_t n", "const void* r32", "const void* a32", "const void* s32", "const void* c32", "unsigned flags", "uint8_t* verdict"]
    d = _defines()
    assert (d["JJ_SIG_REJECT"], d["JJ_SIG_OK"], d["JJ_SIG_MALFORMED"], d["JJ_SIG_COFACTORLESS"]) == (0, 1, 2, 16)


def test_flag_bit_is_disjoint_from_the_decoder_flags():
    d = _defines()
    dec = [v for k, v in d.items() if k.startswith("JJ_DECOMPRESS_")]
    assert len(dec) >= 4
    for v in dec:
        assert v & d["JJ_SIG_COFACTORLESS"] == 0
    assert bin(d["JJ_SIG_COFACTORLESS"]).count("1") == 1


def test_header_says_variable_time():
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*#define JJ_SIG_REJECT", _header(), re.S)
    assert m and "VARIABLE-TIME" in m.group(1) and "public" in m.group(1)


def test_library_exports_the_symbol_and_bindings_name_it():
    import __graft_entry__ as ge

    ge.build()
    lib = ctypes.CDLL(os.path.join(ROOT, "jubjub_amd", "lib", "libjubjub_hip.so"))
    assert hasattr(lib, "jj_sigverify_each")
    from jubjub_amd import _lib, engine

    assert "jj_sigverify_each" in _lib.EXPORTS
    assert len(_lib._SIGS["jj_sigverify_each"]) + 1 == 9               # the context comes first
    assert (engine.SIG_REJECT, engine.SIG_OK, engine.SIG_MALFORMED, engine.FLAG_SIG_COFACTORLESS) == (0, 1, 2, 16)
    assert callable(engine.Engine.sigverify_each) and callable(engine.Engine.sig_locate)
    ffi = open(os.path.join(ROOT, "rust-shim", "src", "ffi.rs")).read()
    assert re.search(r"pub fn jj_sigverify_each\(ctx: \*mut JjCtx, t: \*const JjTable, n: usize,.*verdict: \*mut u8\) -> c_int;", ffi)
    assert "jj_sigverify_each(" in open(os.path.join(ROOT, "rust-shim", "src", "lib.rs")).read()
    assert "jj_sigverify_each(" in open(os.path.join(ROOT, "include", "jubjub_hip.hpp")).read()
    # the .hpp wrapper is EXECUTED by tests/test_cpp_mirror.py (group sig, on the GPU) and tests/test_cpp_mirror_stub_cpu.py (the flag bits)


def test_library_still_reads_no_jj_environment_variable():
    """the rule of tests/test_abi.py, repeated beside the new entry point: no JJ_* name in the shipped library, no getenv outside the
    experiment blocks, and the new code adds no option name either"""
    from jubjub_amd import _lib

    blob = open(_lib.LIB_PATH, "rb").read()
    names = sorted(set(m.decode() for m in re.findall(rb"JJ_[A-Z0-9_]{3,}", blob)) - {"JJ_MSM_PARTIAL_BYTES"})
    assert names == [], names
    csrc = os.path.join(ROOT, "jubjub_amd", "csrc")
    src = "".join(open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)))
    outside = re.sub(r"#ifdef JJ_EXPERIMENTS.*?#e(?:lse|ndif)", "", src, flags=re.S)
    assert re.findall(r'getenv\("(\w+)"\)', outside) == ["GPU_MAX_HW_QUEUES"]
    assert "getenv" not in open(os.path.join(csrc, "jj_sig_each.h")).read()
    assert not re.search(rb"sig_?each_[a-z_]*(chunk|route|fused)\x00", blob), "an option name for the new entry point"
