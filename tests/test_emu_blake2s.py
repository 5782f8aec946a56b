"""Host emulation of the functions behind jj_blake2s and the hash of jj_group_hash (jubjub_amd/csrc/jj_blake2s.h compiled for the CPU with
-DJJ_HOST_EMU into the stand-alone program tests/cpp/emu_blake2s.cpp): the host's midstate over the whole blocks of the prefix, then one lane
of k_blake2s over the prefix's tail and its message, must give hashlib's BLAKE2s-256 digest for EVERY prefix_len 0..200 with EVERY msg_len
0..140 at row-start skews 0..3 -- every tail length, every offset of the message inside the first block, every alignment of its first and
last dword, totals of 0, 64 and 128 bytes, up to five blocks.  hashlib writes the digests to a file; the program reads it and compares.
No GPU.  Test infrastructure only: the product never runs this program.
(The same source built stand-alone with -fsanitize=address,undefined and given the same file is the place for a host sanitizer run: the
program puts every prefix into an allocation of exactly its length and every message into one that ends with the dword of its last byte.)"""
import hashlib
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "emu_blake2s.cpp")
OUT = os.path.join(ROOT, "tests", "cpp", "emu_blake2s")
DEPS = [SRC] + [os.path.join(ROOT, "jubjub_amd", "csrc", f) for f in ("jj_blake2s.h", "jj_field.h", "jj_constants.h")]
PREFIX_POOL, MSG_POOL, PREFIX_MAX, MSG_MAX = 256, 512, 200, 140


@pytest.fixture(scope="module")
def emu():
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in DEPS):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wno-unknown-pragmas", "-o", OUT, SRC])
    return OUT


def case_file():
    """the bytes of the program's input: personalisation, the two pools, hashlib's digest of every case in the program's order"""
    rng = np.random.default_rng(20251)
    personal = rng.integers(0, 256, 8, dtype=np.uint8).tobytes()
    ppool = rng.integers(0, 256, PREFIX_POOL, dtype=np.uint8).tobytes()
    mpool = rng.integers(0, 256, MSG_POOL, dtype=np.uint8).tobytes()
    parts = [personal, ppool, mpool]
    for pl in range(PREFIX_MAX + 1):
        for ml in range(MSG_MAX + 1):
            person = b"" if (pl + ml) % 5 == 0 else personal
            for skew in range(4):
                off = (3 * pl + 5 * ml + 7 * skew) % 128
                parts.append(hashlib.blake2s(ppool[:pl] + mpool[off:off + ml], digest_size=32, person=person).digest())
    return b"".join(parts)


def test_every_prefix_and_message_length_at_every_skew_equals_hashlib(emu, tmp_path):
    path = tmp_path / "blake2s_cases.bin"
    path.write_bytes(case_file())
    res = subprocess.run([emu, str(path)], capture_output=True, text=True)
    print(res.stdout, res.stderr)
    assert res.returncode == 0, res.stderr
    assert res.stdout.strip() == "%d cases, 0 mismatches" % ((PREFIX_MAX + 1) * (MSG_MAX + 1) * 4)
