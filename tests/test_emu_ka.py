"""Host emulation of the device functions behind jj_ka_kdf's hash and jj_chacha20_xor (jubjub_amd/csrc/jj_blake2b.h and jj_chacha20.h compiled
for the CPU with -DJJ_HOST_EMU into the stand-alone program tests/cpp/emu_ka.cpp): the one-compression BLAKE2b with a 32-byte digest over one
or two 32-byte parts must give hashlib's digest for every share and encoding of tests/ka_cases.py under every personalisation, and the row
cipher must give the restatement's bytes (tests/ka_cases.py, pinned by the block of RFC 8439) at EVERY legal length 4, 8 .. 1024, at every
counter of the case list and at a counter that wraps inside the row.  No GPU.  Test infrastructure only: the product never runs this program.
(The same source built with -fsanitize=address,undefined and fed these records is the place for a host sanitizer run: the program puts every
row into an allocation of exactly its length.)"""
import hashlib
import os
import subprocess

import pytest

from tests import ka_cases as KC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "emu_ka.cpp")
OUT = os.path.join(ROOT, "tests", "cpp", "emu_ka")
DEPS = [SRC] + [os.path.join(ROOT, "jubjub_amd", "csrc", f) for f in ("jj_blake2b.h", "jj_chacha20.h", "jj_field.h", "jj_constants.h")]


@pytest.fixture(scope="module")
def emu():
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in DEPS):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wno-unknown-pragmas", "-o", OUT, SRC])
    return OUT


def run(emu, lines):
    res = subprocess.run([emu], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    out = res.stdout.split("\n")[:-1]
    assert len(out) == len(lines)
    return [bytes.fromhex(x) for x in out]


def hash_records():
    """(personal, share, encoding or None): every planted share, plain and cofactored, alone and with its encoding, and the edge patterns"""
    recs = []
    names = list(KC.PERSONALS)
    k = 0
    for sk in KC.SCALARS[:4] + KC.SCALARS[-2:]:
        for _, enc in KC.points():
            p, ok = KC.decode(enc, 0)
            if not ok:
                continue
            for share in KC.shares(sk, p):
                for with_input in (False, True):
                    recs.append((KC.PERSONALS[names[k % len(names)]], share, enc if with_input else None))
                    k += 1
    for pat in (bytes(32), b"\xff" * 32, bytes(range(32))):
        for personal in KC.PERSONALS.values():
            recs += [(personal, pat, None), (personal, pat, pat[::-1])]
    return recs


def test_hash_of_32_and_64_bytes_equals_hashlib(emu):
    recs = hash_records()
    assert len(recs) > 400 and {r[2] is None for r in recs} == {True, False}
    hx = lambda b: b.hex() if b else "-"      # noqa: E731
    got = run(emu, ["H %s %s %s" % (hx(p), a.hex(), hx(b)) for p, a, b in recs])
    for (p, a, b), g in zip(recs, got):
        assert g == hashlib.blake2b(a + (b or b""), digest_size=32, person=p or b"").digest(), (p, a.hex(), hx(b))
    # BLAKE2b-256 is not BLAKE2b-512 cut short: the digest length is in the parameter word
    assert got[0] != hashlib.blake2b(recs[0][1] + (recs[0][2] or b""), digest_size=64, person=recs[0][0] or b"").digest()[:32]


def cipher_records():
    """(key, nonce, counter, row): every legal length at a counter of the case list, and rows of two and more blocks whose counter wraps"""
    recs = []
    for j, length in enumerate(range(4, 1025, 4)):
        key = KC.rng_bytes(7000 + j, 32).tobytes()
        nonce = KC.NONCE if j % 2 else bytes(12)
        recs.append((key, nonce, KC.CIPHER_COUNTERS[j % len(KC.CIPHER_COUNTERS)], KC.rng_bytes(7500 + j, length).tobytes()))
    for j, (length, counter) in enumerate(((68, (1 << 32) - 1), (128, (1 << 32) - 1), (564, (1 << 32) - 3), (1024, (1 << 32) - 15), (1024, (1 << 32) - 16))):
        recs.append((KC.rng_bytes(7900 + j, 32).tobytes(), KC.NONCE, counter, KC.rng_bytes(7950 + j, length).tobytes()))
    recs.append((bytes(range(32)), KC.NONCE, 1, bytes(64)))                      # RFC 8439 section 2.3.2: the keystream itself
    return recs


def test_cipher_at_every_legal_length_and_a_wrapping_counter(emu):
    import numpy as np

    recs = cipher_records()
    got = run(emu, ["C %s %s %d %s" % (k.hex(), nc.hex(), c, row.hex()) for k, nc, c, row in recs])
    for (k, nc, c, row), g in zip(recs, got):
        want = KC.chacha20_xor(np.frombuffer(k, dtype=np.uint8).reshape(1, 32), np.frombuffer(row, dtype=np.uint8).reshape(1, -1), len(row), nc, c)[0].tobytes()
        assert g == want, (len(row), c)
    assert {len(r[3]) for r in recs} >= set(range(4, 1025, 4))
    assert got[-1].hex() == ("10f1e7e4d13b5915500fdd1fa32071c4c7d1f4c733c068030422aa9ac3d46c4ed2826446079faa0914c2d705d98b02a2"
                             "b5129cd1de164eb9cbd083e8a2503c4e")
