"""Host emulation of the 32-bit row offsets AT the offsets the ABI accepts, 2^31 up to 2^32 (tests/cpp/emu_high_offsets.cpp: jj_blake2s.h,
jj_blake2b.h and jj_pedersen.h compiled for the CPU with -DJJ_HOST_EMU, stand-alone, with -fsanitize=address,undefined).  The row array is a
sparse anonymous mapping of 2^32 bytes between two inaccessible pages: only the rows a record uses are written, a read past 2^32 or below 0
ends the program, and an offset that lost a high bit, was sign-extended or wrapped reads other bytes and gives another result.

The layouts are those of tests/high_offset_cases.py: every row of the sparse ones; of the dense ones the last three rows and the rows at and
around 2^31.  Blake2s::finish goes against hashlib.blake2s, Blake2b::hash<PARTS> against hashlib.blake2b (two parts, and none for the ragged
layout, whose three empty messages lie at offset 2^32 itself), ped_build_plan + Pedersen::raw_bits / index against the segment sums of
tests/pedersen_cases.py.  The 64-bit row arithmetic of the ChaCha20 and Poly1305 kernels is not in an emulated header: it is held on the GPU
only (tests/test_gpu_high_offsets.py).  No GPU.  Test infrastructure only: the product never runs this program."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

from tests import high_offset_cases as HC
from tests import pedersen_cases as PC
from tests.test_emu_pedersen import entry0, entry_value

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "emu_high_offsets.cpp")
OUT = os.path.join(ROOT, "tests", "cpp", "emu_high_offsets")
DEPS = [SRC] + [os.path.join(ROOT, "jubjub_amd", "csrc", f) for f in ("jj_blake2s.h", "jj_blake2b.h", "jj_pedersen.h", "jj_field.h", "jj_constants.h")]
FLAGS = ["-std=c++17", "-O1", "-g", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.fixture(scope="module")
def emu():
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in DEPS):
        subprocess.check_call(["g++"] + FLAGS + ["-o", OUT, SRC])
    return OUT


class Job:
    """the records of one run of the program and the file of bytes they copy from"""

    def __init__(self, seed):
        self.rng, self.blob, self.size, self.lines, self.results = np.random.default_rng(seed), [], 0, [], 0

    def fill(self, offset, nbytes):
        """nbytes seeded bytes at `offset` of the array -> those bytes"""
        data = self.rng.integers(0, 256, nbytes, dtype=np.uint8).tobytes()
        if nbytes:
            self.lines.append("w %d %d %d" % (offset, self.size, nbytes))
            self.blob.append(data)
            self.size += nbytes
        return data

    def record(self, text):
        self.lines.append(text)
        self.results += 1

    def clear(self):
        self.lines.append("z")

    def run(self, emu, tmp_path):
        path = tmp_path / "rows.bin"
        path.write_bytes(b"".join(self.blob))
        res = subprocess.run([emu, str(path)], input="\n".join(self.lines) + "\n", capture_output=True, text=True)
        assert res.returncode == 0, "exit status %d\n%s" % (res.returncode, res.stderr[-4000:])
        out = res.stdout.split("\n")[:-1]
        assert len(out) == self.results
        return out


def hx(b):
    return bytes(b).hex() if b else "-"


def blake2s_job():
    job, want = Job(31001), []
    prefix = np.random.default_rng(31002).integers(0, 256, HC.B2S_PREFIX_LEN, dtype=np.uint8).tobytes()
    for L in HC.BLAKE2S:
        job.clear()
        for i in (range(L.n) if L.n <= 4 else L.top_rows()):
            msg = job.fill(L.start(i), L.length)
            job.record("s %s %s %d %d" % (hx(HC.B2S_PERSONAL), hx(prefix), L.start(i), L.length))
            want.append(("%s row %d" % (L.id, i), hashlib.blake2s(prefix + msg, digest_size=32, person=HC.B2S_PERSONAL).hexdigest()))
    return job, want


def test_blake2s_finish_at_the_real_offsets(emu, tmp_path):
    job, want = blake2s_job()
    got = job.run(emu, tmp_path)
    bad = [what for (what, w), g in zip(want, got) if g != w]
    assert not bad, bad


def blake2b_job():
    job, want = Job(32001), []
    rng = np.random.default_rng(32002)

    def one(what, off, length, msg, parts):
        p = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(parts)]
        job.record("b %s %s %s %d %d" % (hx(HC.SIG_PERSONAL), hx(p[0] if parts else b""), hx(p[1] if parts > 1 else b""), off, length))
        want.append((what, hashlib.blake2b(b"".join(p) + msg, digest_size=64, person=HC.SIG_PERSONAL).hexdigest()))

    F = HC.SIG_FIXED
    job.clear()
    for i in F.top_rows():
        one("fixed row %d, two parts" % i, F.start(i), F.length, job.fill(F.start(i), F.length), 2)
    off = HC.sig_ragged_offsets()
    n = len(off) - 1
    across = int(np.searchsorted(off, HC.T31, side="right")) - 1
    job.clear()
    for i in sorted({0, across - 1, across, across + 1} | set(range(n - HC.SIG_RAGGED_EMPTY - 3, n))):
        lo, length = int(off[i]), int(off[i + 1]) - int(off[i])
        msg = job.fill(lo, length)
        for parts in (2, 0):
            one("ragged message %d at %d, %d bytes, %d parts" % (i, lo, length, parts), lo, length, msg, parts)
    return job, want


def test_blake2b_hash_at_the_real_offsets(emu, tmp_path):
    job, want = blake2b_job()
    got = job.run(emu, tmp_path)
    bad = [what for (what, w), g in zip(want, got) if g != w]
    assert not bad, bad
    assert sum("0 bytes" in what for what, _ in want) == 2 * HC.SIG_RAGGED_EMPTY       # the empty messages at offset 2^32: pos wraps to 0, nothing is read


WINDOWS = (4, 3, 1)


def pedersen_job():
    job, want = Job(33001), []
    for P in HC.PEDERSEN:
        nseg = len(PC.generators(P.gens))
        job.clear()
        held = {}
        for i in range(P.n):
            for lo, hi in P.spans(i):
                held[(lo, hi)] = job.fill(lo, hi - lo)

        def read(lo, nbytes, held=held):
            return held[(lo, lo + nbytes)]

        flat = " ".join("%d %d" % f for f in P.fields)
        for w in WINDOWS:
            for i in range(P.n):
                job.record("p %d %d %d %d %d %d %d %s %d" % (nseg, P.seg_chunks, w, P.prefix, P.prefix_bits, P.row_stride, len(P.fields), flat, i))
                want.append((P, w, i, PC.segment_sums(P.seg_chunks, nseg, P.bits(i, read))))
    return job, want


def pedersen_mismatches(want, got):
    """the records whose windows do not rebuild the segment sums of the restatement"""
    bad = []
    for (P, w, i, sums_want), line in zip(want, got):
        nseg, chunks = len(sums_want), -(-P.bits_len // 3)
        sums, seen, ok = [0] * nseg, 0, True
        for tok in line.split(";")[:-1]:
            seg, win, t, e0, idx, neg = (int(x) for x in tok.split())
            present = min(w, P.seg_chunks - win * w, chunks - seg * P.seg_chunks - win * w)
            ok = ok and t == present and t >= 1 and e0 == entry0(P, w, seg, win, t)
            sums[seg] += (-1 if neg else 1) * entry_value(t, idx) * 16 ** (win * w)
            seen += t
        if not (ok and seen == chunks and sums == sums_want):
            bad.append("layout %s, window_chunks %d, unit %d" % (P.id, w, i))
    return bad


def test_pedersen_plan_and_bits_at_the_real_offsets(emu, tmp_path):
    """fails on a plan whose piece bytes are formed from a 32-bit bit number (every layout has a field at or beyond byte 2^29) or whose cover
    is summed in 32 bits"""
    job, want = pedersen_job()
    for P in HC.PEDERSEN:
        spans = sorted(s for i in range(P.n) for s in P.spans(i))
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), P.id    # no two fields of a layout overlap: every write is read back as written
    bad = pedersen_mismatches(want, job.run(emu, tmp_path))
    assert not bad, bad
