"""Host emulation of the multi-source Pedersen plan and bit extraction (jubjub_amd/csrc/jj_pedersen.h compiled for the CPU with -DJJ_HOST_EMU
into the stand-alone program tests/cpp/emu_commit.cpp): the plan of ped_build_plan_src with the source of every piece, the row position and
the clamp dword formed per source, the funnel shift, the window index, the sign and the choice of the sub-table.  Every case of
tests/commit_cases.py, all its rows, under every window_chunks 1 .. 4: the program prints per window (segment, window, sub-table, index,
sign), this test decodes the table entry those name, rebuilds <M_j> and compares with the restatement.  The program puts every source array at
the end of its own allocation, and the test runs it twice: a plain build, and a stand-alone build with -fsanitize=address,undefined, which
would report a dword read beyond the last one that holds a covered byte of that source.  No GPU; nothing is loaded into Python.  Test
infrastructure only: the product never runs this program."""
import os
import subprocess

import pytest

from tests import commit_cases as CC
from tests import pedersen_cases as PC
from tests.test_emu_pedersen import entry0, entry_value

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "emu_commit.cpp")
DEPS = [SRC] + [os.path.join(ROOT, "jubjub_amd", "csrc", f) for f in ("jj_pedersen.h", "jj_blake2b.h", "jj_field.h", "jj_constants.h")]
BUILDS = {"plain": ("emu_commit", ["-O2"]),
          "sanitized": ("emu_commit_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])}


@pytest.fixture(scope="module", params=list(BUILDS))
def emu(request):
    name, flags = BUILDS[request.param]
    out = os.path.join(ROOT, "tests", "cpp", name)
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in DEPS):
        subprocess.check_call(["g++", "-std=c++17", "-Wno-unknown-pragmas"] + flags + ["-o", out, SRC])
    return out


def record(case, w, n):
    strides = " ".join("%d" % s for s in case.strides)
    flat = " ".join("%d %d %d" % f for f in case.fields)
    srcs = " ".join(a[:n].tobytes().hex() for a in case.sources)
    return "%d %d %d %d %d %d %s %d %s %d %s\n" % (case.nseg, case.seg_chunks, w, case.prefix, case.prefix_bits, len(case.strides), strides, len(case.fields), flat, n, srcs)


@pytest.mark.parametrize("w", CC.WINDOWS)
def test_plan_index_and_sign_rebuild_the_segment_sums(emu, w):
    res = subprocess.run([emu], input="".join(record(c, w, c.nrows) for c in CC.CASES), capture_output=True, text=True)
    assert res.returncode == 0, "exit status %d\n%s" % (res.returncode, res.stderr[-4000:])
    lines = res.stdout.split("\n")[:-1]
    assert len(lines) == sum(c.nrows for c in CC.CASES)
    at = 0
    for case in CC.CASES:
        chunks = -(-case.bits_len // 3)
        for i in range(case.nrows):
            sums, seen = [0] * case.nseg, 0
            for tok in lines[at + i].split(";")[:-1]:
                seg, win, t, e0, idx, neg = (int(x) for x in tok.split())
                present = min(w, case.seg_chunks - win * w, chunks - seg * case.seg_chunks - win * w)      # a chunk that is not there is not in the sub-table
                assert t == present and 1 <= t and e0 == entry0(case, w, seg, win, t), (case.id, i, tok)
                sums[seg] += (-1 if neg else 1) * entry_value(t, idx) * 16 ** (win * w)
                seen += t
            assert seen == chunks, (case.id, i)
            assert sums == PC.segment_sums(case.seg_chunks, case.nseg, case.bits(i)), (case.id, w, i)
        at += case.nrows

