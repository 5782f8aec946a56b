"""Host emulation of the Pedersen hash's device functions (jubjub_amd/csrc/jj_pedersen.h compiled for the CPU with -DJJ_HOST_EMU into the
stand-alone program tests/cpp/emu_pedersen.cpp): the host-made plan, the bit extraction over aligned dwords with its funnel shift and clamp, the
window index, the sign and the choice of the sub-table.  Every case of tests/pedersen_cases.py -- all 257 rows, so every message length 0 .. 27
of the tiny shape at every start residue modulo 16 -- under every window_chunks 1 .. 4: the program prints per window (segment, window,
sub-table, index, sign), this test decodes the table entry those name, rebuilds <M_j> and compares with the restatement.  No GPU.  Test
infrastructure only: the product never runs this program.
(The same source built with -fsanitize=address,undefined and fed these records is the place for a host sanitizer run: the program puts every
row array at the end of its own allocation.)"""
import os
import subprocess

import pytest

from tests import pedersen_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "emu_pedersen.cpp")
OUT = os.path.join(ROOT, "tests", "cpp", "emu_pedersen")
DEPS = [SRC] + [os.path.join(ROOT, "jubjub_amd", "csrc", f) for f in ("jj_pedersen.h", "jj_blake2b.h", "jj_field.h", "jj_constants.h")]
SUB_OFFSET = {1: 0, 2: 4, 3: 36, 4: 292}             # sub-tables of 4, 32, 256, 2048 entries
WINDOW_ENTRIES = {1: 4, 2: 36, 3: 292, 4: 2340}


@pytest.fixture(scope="module")
def emu():
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in DEPS):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wno-unknown-pragmas", "-o", OUT, SRC])
    return OUT


def record(case, w, n):
    rows = case.rows[:n, :case.row_stride]
    flat = " ".join("%d %d" % f for f in case.fields)
    return "%d %d %d %d %d %d %d %s %d %s\n" % (case.nseg, case.seg_chunks, w, case.prefix, case.prefix_bits, case.row_stride, len(case.fields), flat, n,
                                                rows.tobytes().hex() if case.fields else "-")


def entry0(case, w, seg, win, t):
    nw = -(-case.seg_chunks // w)
    seg_entries = (nw - 1) * WINDOW_ENTRIES[w] + WINDOW_ENTRIES[case.seg_chunks - (nw - 1) * w]
    return seg * seg_entries + win * WINDOW_ENTRIES[w] + SUB_OFFSET[t]


def entry_value(t, idx):
    """sum_i e_i 16^i of entry `idx` of a sub-table of t chunks: the last chunk's sign is not in the index"""
    assert idx < 1 << (3 * t - 1)
    total = 0
    for i in range(t):
        ch = (idx >> (3 * i)) & 7
        total += PC.enc(ch & 1, (ch >> 1) & 1, (ch >> 2) & 1) * 16 ** i
    return total


@pytest.mark.parametrize("w", PC.WINDOWS)
def test_plan_index_and_sign_rebuild_the_segment_sums(emu, w):
    n = PC.NROWS
    res = subprocess.run([emu], input="".join(record(c, w, n) for c in PC.CASES), capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.split("\n")[:-1]
    assert len(lines) == n * len(PC.CASES)
    residues = set()
    for k, case in enumerate(PC.CASES):
        chunks = -(-case.bits_len // 3)
        for i in range(n):
            sums, seen = [0] * case.nseg, 0
            for tok in lines[k * n + i].split(";")[:-1]:
                seg, win, t, e0, idx, neg = (int(x) for x in tok.split())
                present = min(w, case.seg_chunks - win * w, chunks - seg * case.seg_chunks - win * w)      # a chunk that is not there is not in the sub-table
                assert t == present and 1 <= t and e0 == entry0(case, w, seg, win, t), (case.id, i, tok)
                sums[seg] += (-1 if neg else 1) * entry_value(t, idx) * 16 ** (win * w)
                seen += t
            assert seen == chunks, (case.id, i)
            assert sums == PC.segment_sums(case.seg_chunks, case.nseg, case.bits(i)), (case.id, w, i)
            if case.id.startswith("tiny") and case.fields:
                residues.add((i * case.row_stride + case.fields[0][0]) % 16)
    assert residues == set(range(16))
