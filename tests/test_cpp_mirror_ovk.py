"""
ka_kdf_each and blake2b of include/jubjub_hip.hpp, executed on the GPU by tests/cpp/test_mirror_ovk.cpp and held to the restatements of
tests/ovk_cases.py byte for byte, the size of each returned container included: the key agreement over one wave and three rows of the planted
scalars and points under four flag sets, with and without a second hashed part; the hash at the ock shape, at one array serving two sources
with a skew, at a prefix alone and at four uneven sources, both digest lengths.  This module writes the vectors file (inputs and expected
bytes: the restatement, never the library) and runs the program in one child process.  The compile step runs without a GPU.
"""
import os
import subprocess

import pytest

from conftest import ROOT
from tests import ka_cases as KC
from tests import ovk_cases as OC
from tests.test_cpp_mirror import Vectors, printed_wrappers

SRC = os.path.join(ROOT, "tests", "cpp", "test_mirror_ovk.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "test_mirror_ovk")
WRAPPERS = ["blake2b", "ka_kdf_each"]
N = 67                                             # one wave and three units
KA_FLAGS = (KC.SAPLING_FLAGS, KC.SAPLING_FLAGS, KC.KA_COFACTOR | KC.TORSION_FREE, KC.KA_HASH_INPUT | KC.NOT_SMALL_ORDER, 0)
B2B = (("ock", 32), ("one_array_two_sources", 64), ("prefix128_total128", 32), ("four_sources_uneven", 64), ("straddle", 32))


def build_binary():
    """g++ only, against the C-ABI library; rebuilt when the source, either header or the library is newer"""
    libdir = os.path.join(ROOT, "jubjub_amd", "lib")
    deps = [SRC, os.path.join(ROOT, "include", "jubjub_hip.hpp"), os.path.join(ROOT, "include", "jubjub_hip.h"), os.path.join(libdir, "libjubjub_hip.so")]
    if os.path.exists(BIN) and all(os.path.getmtime(d) <= os.path.getmtime(BIN) for d in deps):
        return BIN
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", BIN, "-L", libdir, "-ljubjub_hip",
                           "-Wl,-rpath,$ORIGIN/../../jubjub_amd/lib", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"])
    return BIN


def write_vectors(path):
    v = Vectors()
    sks, encs = OC.ka_grid(N, shift=3)
    h = OC.hash_rows(N)
    v.put("ka.sk", sks)
    v.put("ka.p", encs)
    v.put("ka.h", h)
    v.put("ka.personal", KC.SAPLING_PERSONAL)
    v.nums("ka.flags", KA_FLAGS)
    for j, flags in enumerate(KA_FLAGS):
        keys, ok = OC.ka_each(sks, encs, flags, KC.SAPLING_PERSONAL, h if (flags & KC.KA_HASH_INPUT and j & 1) else None)
        v.put("ka.keys%d" % j, keys)
        v.put("ka.ok%d" % j, ok)
    v.put("ka.keys_null", OC.ka_each(sks, encs, KA_FLAGS[0], None)[0])
    v.nums("b2b.count", [len(B2B)])
    for k, (name, digest_len) in enumerate(B2B):
        c = OC.B2B_BY_NAME[name]
        arrays = c.arrays(N, seed=k)
        key = "b2b.%d" % k
        v.nums(key + ".params", [digest_len, N, len(c.parts)])
        v.nums(key + ".lens", c.lens)
        v.nums(key + ".strides", [c.strides[a] for a, _, _ in c.parts])
        v.nums(key + ".skews", [skew for _, skew, _ in c.parts])
        for s, (a, _, _) in enumerate(c.parts):
            v.put(key + ".array%d" % s, arrays[a])
        v.put(key + ".prefix", c.prefix())
        v.put(key + ".personal", OC.SAPLING_OCK_PERSONAL)
        v.put(key + ".want", c.want(arrays, N, digest_len, OC.SAPLING_OCK_PERSONAL, c.prefix()))
        v.put(key + ".want_null", c.want(arrays, N, digest_len, None, c.prefix()))
    v.write(path)


def test_wrappers_are_in_the_header_and_the_program_compiles():
    """CPU-side: the wrappers' C entry points are in the header the program compiles, and the program compiles against the mirror and the C ABI"""
    hpp = open(os.path.join(ROOT, "include", "jubjub_hip.hpp")).read()
    assert all("inline " in hpp and " " + w + "(const Context& c" in hpp for w in WRAPPERS) and "jj_ka_kdf_each(" in hpp and "jj_blake2b(" in hpp
    assert os.path.exists(build_binary())


@pytest.mark.gpu
def test_mirror_ovk(tmp_path):
    build_binary()
    vec = tmp_path / "vectors_ovk.txt"
    write_vectors(str(vec))
    try:
        r = subprocess.run([BIN, str(vec)], capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        pytest.fail("the child did not end within its time limit", pytrace=False)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "ALL PASSED" in r.stdout
    assert printed_wrappers(r.stdout) == sorted(WRAPPERS)
