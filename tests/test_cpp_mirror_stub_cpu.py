"""
The CPU half of the check of include/jubjub_hip.hpp: tests/cpp/test_mirror_stub.cpp calls every wrapper that tests/test_cpp_mirror.py runs on
the GPU, here against tests/cpp/abi_stub.cpp -- a recording stand-in for the C ABI that reads every input and writes every output over exactly
the extent include/jubjub_hip.h documents -- as ONE stand-alone program built with the host sanitizers.  A result container the mirror sized too
small or an input it made too short is a sanitizer report; one too large, a swapped length or stride, an inverted flag, a wrong NULL or a
wrong row order in a flattened buffer is a failed comparison in the program.  Nothing is loaded into Python and no GPU is involved.
"""
import os
import subprocess

from conftest import ROOT
from test_cpp_mirror import ALL_WRAPPERS, printed_wrappers

import pytest

CPP = os.path.join(ROOT, "tests", "cpp")
SOURCES = [os.path.join(CPP, "test_mirror_stub.cpp"), os.path.join(CPP, "abi_stub.cpp")]
BIN = os.path.join(CPP, "test_mirror_stub")
# the runtimes are linked INTO the program: it then runs the same whatever the environment preloads, and the environment stays as it is
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


def sanitizer_runtime_links(tmp_path):
    """whether g++ can link a program with the sanitizer runtimes on this machine -> (bool, the linker's words)"""
    src = tmp_path / "probe.cpp"
    src.write_text("int main() { return 0; }\n")
    r = subprocess.run(["g++", "-std=c++17"] + SANITIZE + [str(src), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    return r.returncode == 0, r.stderr[-400:]


def build_binary():
    deps = SOURCES + [os.path.join(CPP, "abi_stub.h"), os.path.join(ROOT, "include", "jubjub_hip.hpp"), os.path.join(ROOT, "include", "jubjub_hip.h")]
    if os.path.exists(BIN) and all(os.path.getmtime(d) <= os.path.getmtime(BIN) for d in deps):
        return BIN
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall"] + SANITIZE + ["-I", os.path.join(ROOT, "include")] + SOURCES + ["-o", BIN])
    return BIN


def test_mirror_against_the_recording_stub(tmp_path):
    ok, why = sanitizer_runtime_links(tmp_path)
    if not ok:
        pytest.skip("g++ cannot link the sanitizer runtimes here: " + why)
    build_binary()
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    assert r.stderr == ""
    assert "ALL PASSED" in r.stdout
    assert printed_wrappers(r.stdout) == ALL_WRAPPERS
