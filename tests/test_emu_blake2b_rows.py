"""Host emulation of the functions behind jj_blake2b (Blake2bRows of jubjub_amd/csrc/jj_blake2b.h compiled for the CPU with -DJJ_HOST_EMU into
the stand-alone program tests/cpp/emu_blake2b_rows.cpp): the host's midstate over the whole blocks of the prefix, the piece plan, and the
block loop of one lane of k_blake2b must give hashlib's digest for EVERY case of tests/ovk_cases.py (both digest lengths, every prefix length
crossed with every total, exact multiples of 128, prefixes of 128 and 256 bytes alone, sources across and up to a block boundary, four
sources, one array serving two, strides over the lengths at skews 0 and 16, the longest prefix and the longest source).  The program puts
every array into an allocation that ends with the last byte a source reads, and the test runs it twice: a plain build, and a stand-alone
build with -fsanitize=address,undefined, which would report a dword read outside a source's own bytes.  No GPU; nothing is loaded into
Python.  Test infrastructure only: the product never runs this program."""
import os
import subprocess

import pytest

from tests import ovk_cases as OC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "emu_blake2b_rows.cpp")
DEPS = [SRC] + [os.path.join(ROOT, "jubjub_amd", "csrc", f) for f in ("jj_blake2b.h", "jj_field.h", "jj_constants.h")]
BUILDS = {"plain": ("emu_blake2b_rows", ["-O2"]),
          "sanitized": ("emu_blake2b_rows_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])}
ROWS = 5


@pytest.fixture(scope="module", params=list(BUILDS))
def emu(request):
    name, flags = BUILDS[request.param]
    out = os.path.join(ROOT, "tests", "cpp", name)
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in DEPS):
        subprocess.check_call(["g++", "-std=c++17", "-Wno-unknown-pragmas"] + flags + ["-o", out, SRC])
    return out


def record(case, digest_len, personal, n, arrays):
    """the program's line for one case; every array is cut behind the last byte a source reads of its last row"""
    hx = lambda b: bytes(b).hex() if len(b) else "-"      # noqa: E731
    cols = []
    for a, st in enumerate(case.strides):
        reach = max(skew + length for arr, skew, length in case.parts if arr == a)
        cols.append("%d %s" % (st, hx(arrays[a].tobytes()[:(n - 1) * st + reach])))
    parts = " ".join("%d %d %d" % p for p in case.parts)
    return "%d %s %s %d %s %d %s %d\n" % (digest_len, hx(personal or b""), hx(case.prefix()), len(case.strides), " ".join(cols), len(case.parts), parts, n)


@pytest.fixture(scope="module")
def cases():
    """[(case, digest_len, personal, n, arrays, want)]: hashlib's digests, made once for both builds"""
    out = []
    for k, case in enumerate(OC.B2B_CASES):
        n = min(ROWS, case.nrows or ROWS)
        arrays = case.arrays(n)
        for digest_len in OC.DIGESTS:
            personal = list(OC.PERSONALS.values())[(k + digest_len // 32) % 3]
            out.append((case, digest_len, personal, n, arrays, case.want(arrays, n, digest_len, personal, case.prefix())))
    return out


def test_every_case_equals_hashlib(emu, cases):
    res = subprocess.run([emu], input="".join(record(c, d, p, n, a) for c, d, p, n, a, _ in cases), capture_output=True, text=True)
    assert res.returncode == 0, "exit status %d\n%s" % (res.returncode, res.stderr[-4000:])
    lines = res.stdout.split("\n")[:-1]
    assert len(lines) == len(cases)
    for line, (case, digest_len, personal, n, _, want) in zip(lines, cases):
        assert line == want.tobytes().hex(), (case.name, digest_len, personal)
