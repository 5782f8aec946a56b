"""Host emulation of jj_sig_challenge's device functions (jubjub_amd/csrc/jj_blake2b.h compiled for the CPU with -DJJ_HOST_EMU into the
stand-alone program tests/cpp/emu_blake2b.cpp): the BLAKE2b compression, the streaming of up to two 32-byte parts and a message that starts at
any byte address, the funnel shift over aligned dwords with its clamp and its byte masks, and the wide reduction behind it.  Every total length
0 .. 300 in every part combination that fits, at start offsets of every residue modulo 16, and the whole case table of
tests/sig_challenge_cases.py under every personalisation must give the oracle's digest (hashlib.blake2b) and the oracle's scalar
(oracle.jubjub_ref.FR.from_bytes_wide).  No GPU.  Test infrastructure only: the product never runs this program.
(The same source built with -fsanitize=address,undefined and fed these records is the place for a host sanitizer run: the program puts every
message at the end of its own allocation.)"""
import hashlib
import os
import subprocess

import pytest

from oracle.jubjub_ref import FR
from tests import sig_challenge_cases as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "emu_blake2b.cpp")
OUT = os.path.join(ROOT, "tests", "cpp", "emu_blake2b")
DEPS = [SRC] + [os.path.join(ROOT, "jubjub_amd", "csrc", f) for f in ("jj_blake2b.h", "jj_field.h", "jj_constants.h")]


@pytest.fixture(scope="module")
def emu():
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in DEPS):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wno-unknown-pragmas", "-o", OUT, SRC])
    return OUT


def records_every_length():
    """(personal, part0, part1, message, skew) for every total 0 .. 300 x every combination that fits"""
    out = []
    names = list(CC.PERSONALS)
    for total in range(301):
        for k, combo in enumerate(CC.COMBOS):
            if total < CC.PREFIX[combo]:
                continue
            R, A = CC.parts(1, combo, seed=total)
            msg = CC.fixed(1, total - CC.PREFIX[combo], seed=total)[0].tobytes()
            p = [x[0].tobytes() for x in (R, A) if x is not None]
            out.append((CC.PERSONALS[names[(total + k) % len(names)]], p[0] if p else None, p[1] if len(p) > 1 else None, msg, (total * 5 + k) % 16))
    return out


def records_case_table():
    out = []
    for pname, personal in CC.PERSONALS.items():
        for j, (total, combo, msg_len) in enumerate(CC.CASES):
            R, A = CC.parts(1, combo, seed=j)
            p = [x[0].tobytes() for x in (R, A) if x is not None]
            out.append((personal, p[0] if p else None, p[1] if len(p) > 1 else None, CC.fixed(1, msg_len, seed=j)[0].tobytes(), (3 * j + len(pname)) % 16))
    return out


def run(emu, records):
    hx = lambda b: b.hex() if b else "-"
    text = "".join("%s %s %s %s %d\n" % (hx(p), hx(a), hx(b), hx(m), skew) for p, a, b, m, skew in records)
    res = subprocess.run([emu], input=text, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.split("\n")[:-1]
    assert len(lines) == len(records)
    return [tuple(bytes.fromhex(x) for x in ln.split()) for ln in lines]


@pytest.mark.parametrize("records", [records_every_length, records_case_table], ids=["every_length_0_to_300", "case_table_every_personal"])
def test_emulation_equals_the_oracle(emu, records):
    recs = records()
    got = run(emu, recs)
    residues = set()
    for (personal, a, b, m, skew), (digest, scalar) in zip(recs, got):
        data = (a or b"") + (b or b"") + m
        want = hashlib.blake2b(data, digest_size=64, person=personal or b"").digest()
        assert digest == want, "digest of %d bytes (%d of them message at skew %d, personal %r)" % (len(data), len(m), skew, personal)
        assert scalar == FR.to_bytes(FR.from_bytes_wide(want))
        if m:
            residues.add(skew)
    assert residues == set(range(16))
