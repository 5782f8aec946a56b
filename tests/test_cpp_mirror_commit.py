"""
PedersenTable::commit and PedersenTable::commit_points of include/jubjub_hip.hpp, executed on the GPU by tests/cpp/test_mirror_commit.cpp and
held to the restatement of tests/commit_cases.py byte for byte, the size of each returned container included: the tiny shapes (three sources
of stride 5, 3 and 9; windows with pieces of two and of three sources; a padded last chunk), blinded over the mirror's default LDS table and
in the hash-only form.  This module writes the vectors file (inputs and expected bytes: the restatement, never the library) and runs the
program in one child process.  The compile step runs without a GPU.
"""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from tests import commit_cases as CC
from tests import pedersen_cases as PC
from tests.test_cpp_mirror import Vectors, printed_wrappers

SRC = os.path.join(ROOT, "tests", "cpp", "test_mirror_commit.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "test_mirror_commit")
WRAPPERS = ["PedersenTable::commit", "PedersenTable::commit_points"]
CASE_IDS = ("tiny3_two", "tiny3_three")
N = 67                                             # one wave and three units


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
    for cid in CASE_IDS:
        c = CC.BY_ID[cid]
        want = CC.expected_points(c, N)
        hashed = np.stack([PC.point_bytes(PC.expected(CC.gens_of(c.gens), c.seg_chunks, c.bits(i))) for i in range(N)])
        v.nums(cid + ".params", [c.prefix, c.prefix_bits, N, c.seg_chunks])
        v.nums(cid + ".strides", c.strides)
        v.nums(cid + ".fields", [x for f in c.fields for x in f])
        v.put(cid + ".gens", CC.gens_bytes(c.gens))
        v.put(cid + ".rbase", PC.point_bytes(CC.bases()[c.rbase]))
        for s, a in enumerate(c.sources):
            v.put(cid + ".src%d" % s, a[:N])
        v.put(cid + ".r", c.r[:N])
        v.put(cid + ".points", want)
        v.put(cid + ".commit", want[:, :32])
        v.put(cid + ".hash_points", hashed)
        v.put(cid + ".hash", hashed[:, :32])
    v.write(path)


def test_wrappers_are_in_the_header_and_the_program_compiles():
    """CPU-side: the wrappers' C entry point is in the header the program compiles, and the program compiles against the mirror and the C ABI"""
    hpp = open(os.path.join(ROOT, "include", "jubjub_hip.hpp")).read()
    assert all(w.split("::")[-1] + "(" in hpp for w in WRAPPERS) and "jj_pedersen_commit_vartime(" in hpp
    assert os.path.exists(build_binary())


@pytest.mark.gpu
def test_mirror_commit(tmp_path):
    build_binary()
    vec = tmp_path / "vectors_commit.txt"
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
