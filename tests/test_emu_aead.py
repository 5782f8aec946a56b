"""Host emulation of the device functions behind jj_poly1305, jj_aead_open and jj_aead_seal (jubjub_amd/csrc/jj_poly1305.h and jj_chacha20.h
compiled for the CPU with -DJJ_HOST_EMU into the stand-alone program tests/cpp/emu_aead.cpp): Poly1305::mac_row must give the restatement's tag
(tests/aead_cases.py, pinned by RFC 8439's vectors) for every planted key and message -- the accumulator below, at and above p before the
final reduction, the dropped carry, the clamp -- and at EVERY legal length 4, 8 .. 1024; Aead::row must give the restatement's bytes for seal
and for open at every pair of a legal length and an aad length in 0, 12, 16, 17 and 64 (1280 records each), and the zero row with ok = 0 for every tampered row.  No GPU.
Test infrastructure only: the product never runs this program.

(The same source built with -fsanitize=address,undefined and fed these records is the place for a host sanitizer run: the program puts every
row into an allocation of exactly its length, so a dword read or written outside a row is reported.  records_for_sanitizer() writes them out.)"""
import os
import subprocess

import numpy as np
import pytest

from tests import aead_cases as AC
from tests import ka_cases as KC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "emu_aead.cpp")
OUT = os.path.join(ROOT, "tests", "cpp", "emu_aead")
DEPS = [SRC] + [os.path.join(ROOT, "jubjub_amd", "csrc", f) for f in ("jj_poly1305.h", "jj_chacha20.h", "jj_field.h", "jj_constants.h")]
EMU_AADS = (0, 12, 16, 17, 64)


@pytest.fixture(scope="module")
def emu():
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in DEPS):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wno-unknown-pragmas", "-o", OUT, SRC])
    return OUT


def run(emu, lines):
    res = subprocess.run([emu], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
    assert res.returncode == 0 and not res.stderr, res.stderr[-2000:]
    out = res.stdout.split("\n")[:-1]
    assert len(out) == len(lines)
    return out


def build_mac_records():
    """(name, key, row, tag): every planted case, and every legal length with a seeded key"""
    recs = list(AC.planted())
    for j, length in enumerate(range(4, 1025, 4)):
        key, row = KC.rng_bytes(9300 + j, 32).tobytes(), KC.rng_bytes(9600 + j, length).tobytes()
        recs.append(("len %d" % length, key, row, AC.poly1305(key, row)))
    return recs


def build_aead_records():
    """(key, nonce, aad, plain, sealed): every legal length with every aad length of EMU_AADS -- 256 x 5 rows"""
    recs = []
    for j, length in enumerate(range(4, 1025, 4)):
        for a, aad_len in enumerate(EMU_AADS):
            key, nonce = KC.rng_bytes(9900 + 5 * j + a, 32).tobytes(), (AC.NONCE if (j + a) % 2 else bytes(12))
            aad, plain = KC.rng_bytes(11500 + 5 * j + a, aad_len).tobytes(), KC.rng_bytes(13100 + 5 * j + a, length).tobytes()
            recs.append((key, nonce, aad, plain, AC.seal_one(key, nonce, aad, plain)))
    return recs


@pytest.fixture(scope="module")
def mac_records():
    return build_mac_records()


@pytest.fixture(scope="module")
def aead_records():
    return build_aead_records()


hx = lambda b: b.hex() if b else "-"      # noqa: E731


def mac_lines(mac_records):
    return ["P %s %s" % (k.hex(), row.hex()) for _, k, row, _ in mac_records]


def seal_lines(aead_records):
    return ["S %s %s %s %s" % (k.hex(), nc.hex(), hx(aad), plain.hex()) for k, nc, aad, plain, _ in aead_records]


def test_mac_planted_cases_and_every_legal_length(emu, mac_records):
    assert {len(r[2]) for r in mac_records} >= set(range(4, 1025, 4)) and len(mac_records) > 270
    got = run(emu, mac_lines(mac_records))
    for (name, _, _, tag), g in zip(mac_records, got):
        assert g == tag.hex(), name


def test_seal_at_every_legal_length(emu, aead_records):
    assert {(len(r[3]), len(r[2])) for r in aead_records} == {(length, a) for length in range(4, 1025, 4) for a in EMU_AADS} and len(aead_records) == 1280
    got = run(emu, seal_lines(aead_records))
    for (_, _, aad, plain, sealed), g in zip(aead_records, got):
        assert g == sealed.hex(), (len(plain), len(aad))


def open_lines(aead_records):
    """(records, expected output lines): every sealed row, then the tampered ones"""
    lines, want = [], []
    for k, nc, aad, plain, sealed in aead_records:
        lines.append("O %s %s %s %s" % (k.hex(), nc.hex(), hx(aad), sealed.hex()))
        want.append("01 " + plain.hex())
    # tampered: every entry of the list at the lengths where a path changes; another nonce and another aad
    for k, nc, aad, plain, sealed in [r for r in aead_records if len(r[3]) in (4, 64, 68, 564, 1024) and len(r[2]) in (0, 17)]:
        length = len(plain)
        other = AC.seal_one(k, nc, aad, bytes(length))
        for name, what in AC.tamper_list(length):
            key, row = bytearray(k), bytearray(sealed)
            if what[0] == "ct":
                row[what[1]] ^= 1 << what[2]
            elif what[0] == "tag":
                row[length + what[1]] ^= 1 << what[2]
            elif what[0] == "neighbour":
                row[length:] = other[length:]
            else:
                key[what[1]] ^= 1 << what[2]
            lines.append("O %s %s %s %s" % (key.hex(), nc.hex(), hx(aad), row.hex()))
            want.append("00 " + bytes(length).hex())
        lines.append("O %s %s %s %s" % (k.hex(), bytes(11).hex() + "01", hx(aad), sealed.hex()))
        want.append("00 " + bytes(length).hex())
        lines.append("O %s %s %s %s" % (k.hex(), nc.hex(), hx(aad + b"\x00") if len(aad) < 64 else hx(aad[:-1]), sealed.hex()))
        want.append("00 " + bytes(length).hex())
    return lines, want


def records_for_sanitizer():
    """every record of this file, for the stand-alone program built with -fsanitize=address,undefined: python -m tests.test_emu_aead > records"""
    recs = build_aead_records()
    return mac_lines(build_mac_records()) + seal_lines(recs) + open_lines(recs)[0]


def test_open_at_every_legal_length_and_every_tampered_row(emu, aead_records):
    lines, want = open_lines(aead_records)
    got = run(emu, lines)
    assert len(want) > len(aead_records) + 200
    for line, w, g in zip(lines, want, got):
        assert g == w, line[:200]
    # the restatement's own open agrees with what was asked of the program
    k, nc, aad, plain, sealed = aead_records[37]
    assert AC.open_one(k, nc, aad, sealed) == (plain, 1) and AC.open_one(k, nc, aad, sealed[:-1] + bytes([sealed[-1] ^ 1])) == (bytes(len(plain)), 0)
    assert np.array_equal(AC.mac_rows(np.frombuffer(k, np.uint8).reshape(1, 32), np.frombuffer(plain, np.uint8).reshape(1, -1), len(plain))[0],
                          np.frombuffer(AC.poly1305(k, plain), np.uint8))


if __name__ == "__main__":
    print("\n".join(records_for_sanitizer()))
