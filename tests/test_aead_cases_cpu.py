"""tests/aead_cases.py, pinned without a GPU: the integer Poly1305 gives the tag of RFC 8439 section 2.5.2, the AEAD built from it and from
tests/ka_cases.py's ChaCha20 gives the ciphertext and tag of section 2.8.2 (a 114-byte plaintext: not a multiple of 4, so this vector pins the
restatement alone), the planted accumulator cases give the tags that follow from p = 2^130 - 5 by hand, and -- where the system's libcrypto
loads -- the restatement equals EVP_chacha20_poly1305 at every len in 0, 4 .. 128, 564, 1024 and every aad_len in 0, 1, 12, 16, 17, 64.  The
three buffer-discipline rows of tests/aead_buffer_row.py join the table here, and their oracles hold both verdicts."""
import ctypes
import ctypes.util

import numpy as np
import pytest

from tests import aead_buffer_row as BR
from tests import aead_cases as AC
from tests import ka_cases as KC

SUNSCREEN = b"Ladies and Gentlemen of the class of '99: If I could offer you only one tip for the future, sunscreen would be it."


def test_poly1305_rfc8439_2_5_2():
    key = bytes.fromhex("85d6be7857556d337f4452fe42d506a80103808afb0db2fd4abff6af4149f51b")
    assert AC.poly1305(key, b"Cryptographic Forum Research Group").hex() == "a8061dc1305136c6c22b8baf0c0127a9"


def test_aead_rfc8439_2_8_2():
    key, nonce, aad = bytes(range(0x80, 0xA0)), bytes.fromhex("070000004041424344454647"), bytes.fromhex("50515253c0c1c2c3c4c5c6c7")
    assert len(SUNSCREEN) == 114 and nonce == AC.NONCE
    sealed = AC.seal_one(key, nonce, aad, SUNSCREEN)
    assert sealed[-16:].hex() == "1ae10b594f09e26a7e902ecbd0600691"
    assert sealed[:16].hex() == "d31a8d34648e60db7b86afbc53ef7ec2"                                                    # section 2.8.2: the ciphertext's first bytes
    assert AC.otk(key, nonce).hex() == "7bac2b252db447af09b67a55a4e955840ae1d6731075d9eb2a9375783ed553ff"      # section 2.8.2: the Poly1305 key
    assert AC.open_one(key, nonce, aad, sealed) == (SUNSCREEN, 1)
    for j in (0, 57, 113, 114, 129):
        bad = bytearray(sealed)
        bad[j] ^= 0x10
        assert AC.open_one(key, nonce, aad, bad) == (bytes(114), 0), j
    assert AC.open_one(key, nonce, aad + b"\x00", sealed)[1] == 0 and AC.open_one(key, bytes(12), aad, sealed)[1] == 0


def test_planted_accumulator_cases():
    cases = {name: (key, msg, tag) for name, key, msg, tag in AC.planted()}
    assert len(cases) == len(AC.planted()) >= 23
    for name, (key, msg, tag) in cases.items():
        assert AC.poly1305(key, msg) == tag, name                                # the literals of the issue among them
        assert len(msg) % 4 == 0 and 4 <= len(msg) <= 1024, name                 # every case is a legal row
    assert cases["h = p - 1"][2].hex() == "fa" + "ff" * 15 and cases["h = p"][2] == bytes(16) and cases["h = p + 1"][2].hex() == "01" + "00" * 15
    assert cases["h = 2^130 - 2"][2].hex() == "03" + "00" * 15 and cases["h = 2^130 - 2, s = ff x 16"][2].hex() == "02" + "00" * 15
    # what the names say, on integers: the accumulator before the final reduction
    for name, want in (("h = p - 1", AC.P1305 - 1), ("h = p", AC.P1305), ("h = p + 1", AC.P1305 + 1), ("h = 2^130 - 2", (1 << 130) - 2)):
        msg = cases[name][1]
        assert sum(int.from_bytes(msg[i:i + 16] + b"\x01", "little") for i in (0, 16)) == want, name      # r = 1: h is the plain sum
    # the unclamped r equals its clamped twin
    a, b = cases["r at the clamp's maximum, 1024 bytes of ff"], cases["r with every bit set"]
    assert a[0] != b[0] and a[1] == b[1] and a[2] == b[2]
    assert {len(m) % 16 for _, m, _ in cases.values()} >= {0, 4, 8, 12}


def test_rows_and_tampering():
    n, length = 40, 52
    keys, plain = AC.pool_keys(n, 5, 1), KC.rng_bytes(2, n, length)
    sealed = AC.seal_rows(keys, plain, length, AC.NONCE, b"aad")
    for i in (0, 7, 39):
        assert sealed[i].tobytes() == AC.seal_one(keys[i].tobytes(), AC.NONCE, b"aad", plain[i].tobytes())
    got, ok = AC.open_rows(keys, sealed, length, AC.NONCE, b"aad")
    assert ok.all() and np.array_equal(got, plain)
    victims = list(range(1, n, 2))
    assert len(victims) == len(AC.tamper_list(length))                             # every entry of the list once
    tk, tr, names = AC.tamper(keys, sealed, length, victims)
    got, ok = AC.open_rows(tk, tr, length, AC.NONCE, b"aad")
    for i in range(n):
        if i in names:
            assert ok[i] == 0 and not got[i].any(), names[i]
        else:
            assert ok[i] == 1 and np.array_equal(got[i], plain[i]), i
    assert not AC.open_rows(keys, sealed, length, None, b"aad")[1].any() and not AC.open_rows(keys, sealed, length, AC.NONCE, b"aae")[1].any()


def test_buffer_rows_join_the_table():
    import buffer_cases as BC

    ids = {c.id for c in BC.CASES}
    assert {"jj_poly1305", "jj_aead_seal", "jj_aead_open"} <= ids
    # the rows are keyed to entry points the header declares (the table's coverage pin reads the same prototypes)
    import os
    import re

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "jubjub_hip.h")).read()
    for fn in ("jj_poly1305", "jj_aead_seal", "jj_aead_open"):
        assert re.search(r"^int\s+%s\s*\(jj_ctx\*" % fn, header, re.M), "%s is not declared in include/jubjub_hip.h" % fn
    assert (BR.LEN, BR.STRIDE, BR.OPEN_STRIDE) == (52, 56, 72)
    for n in (1, 5, 65):
        ins, outs = BR.ROW_OPEN.data(n)
        ok = outs["ok"].reshape(-1)
        assert outs["out"].shape == (n * 13, 4) and ok.shape == (n,)
        assert n < 3 or (0 < int(ok.sum()) < n)
        assert not outs["out"].reshape(n, 52)[ok == 0].any()
        ins, outs = BR.ROW_SEAL.data(n)
        assert outs["out"].shape == (n * 17, 4) and BR.ROW_MAC.data(n)[1]["tag"].shape == (n * 4, 4)


def _libcrypto():
    name = ctypes.util.find_library("crypto")
    if not name:
        return None
    try:
        lib = ctypes.CDLL(name)
        for fn in ("EVP_CIPHER_CTX_new", "EVP_chacha20_poly1305"):
            getattr(lib, fn).restype = ctypes.c_void_p
        for fn in ("EVP_EncryptInit_ex", "EVP_CIPHER_CTX_ctrl", "EVP_EncryptUpdate", "EVP_EncryptFinal_ex"):
            getattr(lib, fn).restype = ctypes.c_int
        lib.EVP_EncryptInit_ex.argtypes = [ctypes.c_void_p] * 5
        lib.EVP_CIPHER_CTX_ctrl.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        lib.EVP_EncryptUpdate.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.c_void_p, ctypes.c_int]
        lib.EVP_EncryptFinal_ex.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
        lib.EVP_CIPHER_CTX_free.argtypes = [ctypes.c_void_p]
        return lib
    except (OSError, AttributeError):
        return None


def evp_seal(lib, key, nonce, aad, plain):
    ctx = lib.EVP_CIPHER_CTX_new()
    try:
        outl = ctypes.c_int(0)
        out, tag = ctypes.create_string_buffer(len(plain) + 16), ctypes.create_string_buffer(16)
        assert lib.EVP_EncryptInit_ex(ctx, lib.EVP_chacha20_poly1305(), None, None, None) == 1
        assert lib.EVP_CIPHER_CTX_ctrl(ctx, 0x9, 12, None) == 1                   # EVP_CTRL_AEAD_SET_IVLEN
        assert lib.EVP_EncryptInit_ex(ctx, None, None, key, nonce) == 1
        if aad:
            assert lib.EVP_EncryptUpdate(ctx, None, ctypes.byref(outl), aad, len(aad)) == 1
        total = 0
        if plain:
            assert lib.EVP_EncryptUpdate(ctx, out, ctypes.byref(outl), plain, len(plain)) == 1
            total = outl.value
        assert lib.EVP_EncryptFinal_ex(ctx, ctypes.byref(out, total), ctypes.byref(outl)) == 1
        assert total + outl.value == len(plain)
        assert lib.EVP_CIPHER_CTX_ctrl(ctx, 0x10, 16, tag) == 1                   # EVP_CTRL_AEAD_GET_TAG
        return out.raw[:len(plain)] + tag.raw
    finally:
        lib.EVP_CIPHER_CTX_free(ctx)


def test_restatement_equals_libcrypto():
    lib = _libcrypto()
    if lib is None:
        pytest.skip("the system's libcrypto does not load")
    key, nonce, aad = bytes(range(0x80, 0xA0)), AC.NONCE, bytes.fromhex("50515253c0c1c2c3c4c5c6c7")
    assert evp_seal(lib, key, nonce, aad, SUNSCREEN) == AC.seal_one(key, nonce, aad, SUNSCREEN)
    count = 0
    for length in [0] + list(range(4, 129, 4)) + [564, 1024]:
        for aad_len in (0, 1, 12, 16, 17, 64):
            key, nonce = KC.rng_bytes(12000 + count, 32).tobytes(), (bytes(12) if count % 3 == 0 else KC.rng_bytes(12500 + count, 12).tobytes())
            aad, plain = KC.rng_bytes(13000 + count, aad_len).tobytes(), KC.rng_bytes(13500 + count, length).tobytes()
            assert evp_seal(lib, key, nonce, aad, plain) == AC.seal_one(key, nonce, aad, plain), (length, aad_len)
            count += 1
    assert count == 35 * 6
