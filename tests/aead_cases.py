"""Restatement and cases of jj_poly1305, jj_aead_open and jj_aead_seal (the CPU tests, the host emulation and the GPU tests share them):
Poly1305 on Python integers (RFC 8439 section 2.5) and the ChaCha20-Poly1305 AEAD of section 2.8 built from it and from the ChaCha20 of
tests/ka_cases.py (chacha20_block, keystream).  tests/test_aead_cases_cpu.py pins both with the RFC's own vectors and, where the system's
libcrypto loads, against EVP_chacha20_poly1305.  Test infrastructure only.

PLANTED: one-time keys and messages at which a Poly1305 implementation goes wrong -- the accumulator just below, at and just above
p = 2^130 - 5 and at 2^130 - 2 before the final reduction (an incomplete reduction leaves h in [p, 2^130) as it is), the carry out of 2^128
when s is added, r at the clamp's maximum over the longest row, r with every unclamped bit set (which must equal its clamped twin), r = 0, and
last blocks of 4, 8 and 12 bytes."""
import struct

import numpy as np

from tests import ka_cases as KC

P1305 = (1 << 130) - 5
CLAMP = 0x0ffffffc0ffffffc0ffffffc0fffffff
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1025)            # wave edges, workgroup edges, the tail block of the grid
MAC_LENS = (4, 8, 12, 16, 20, 60, 64, 68, 564, 1024)
SEAL_LENS = (4, 12, 16, 20, 52, 60, 64, 68, 128, 564, 1024)
AAD_LENS = (0, 1, 12, 16, 17, 63, 64)
NONCE = bytes.fromhex("070000004041424344454647")          # the nonce of RFC 8439 section 2.8.2


def poly1305(key, msg):
    """the 16-byte tag of `msg` under the 32-byte one-time key (r = key[:16], clamped; s = key[16:])"""
    key, msg = bytes(key), bytes(msg)
    r = int.from_bytes(key[:16], "little") & CLAMP
    s = int.from_bytes(key[16:], "little")
    h = 0
    for i in range(0, len(msg), 16):
        h = (h + int.from_bytes(msg[i:i + 16] + b"\x01", "little")) * r % P1305
    return ((h + s) & ((1 << 128) - 1)).to_bytes(16, "little")


def pad16(x):
    return bytes(-len(x) % 16)


def mac_data(aad, ct):
    return aad + pad16(aad) + ct + pad16(ct) + struct.pack("<QQ", len(aad), len(ct))


def otk(key, nonce):
    return KC.chacha20_block(key, 0, bytes(12) if nonce is None else bytes(nonce))[:32]


def seal_one(key, nonce, aad, plain):
    """ciphertext || tag"""
    ct = bytes(a ^ b for a, b in zip(plain, KC.keystream(key, 1, nonce, len(plain))))
    return ct + poly1305(otk(key, nonce), mac_data(bytes(aad), ct))


def open_one(key, nonce, aad, row):
    """(plaintext, 1), or (zeros, 0) where the tag does not verify; row = ciphertext || tag"""
    ct, tag = bytes(row[:-16]), bytes(row[-16:])
    if poly1305(otk(key, nonce), mac_data(bytes(aad), ct)) != tag:
        return bytes(len(ct)), 0
    return bytes(a ^ b for a, b in zip(ct, KC.keystream(key, 1, nonce, len(ct)))), 1


# ---------------------------------------------------------------------------------------------------- whole arrays (a key's streams are made once)
def mac_rows(keys, data, length):
    """keys (n, 32), data (n, stride) -> (n, 16)"""
    out = np.zeros((len(keys), 16), np.uint8)
    for i in range(len(keys)):
        out[i] = np.frombuffer(poly1305(keys[i].tobytes(), data[i, :length].tobytes()), dtype=np.uint8)
    return out


def _streams(cache, key, nonce, length):
    if key not in cache:
        cache[key] = (otk(key, nonce), np.frombuffer(KC.keystream(key, 1, nonce, length), dtype=np.uint8))
    return cache[key]


def seal_rows(keys, data, length, nonce=None, aad=b""):
    """keys (n, 32), data (n, stride) -> (n, length + 16)"""
    out = np.zeros((len(keys), length + 16), np.uint8)
    cache = {}
    for i in range(len(keys)):
        one_time, ks = _streams(cache, keys[i].tobytes(), nonce, length)
        out[i, :length] = data[i, :length] ^ ks
        out[i, length:] = np.frombuffer(poly1305(one_time, mac_data(bytes(aad), out[i, :length].tobytes())), dtype=np.uint8)
    return out


def open_rows(keys, data, length, nonce=None, aad=b""):
    """keys (n, 32), data (n, stride >= length + 16) -> (plain (n, length), ok (n,)): zero rows where the tag does not verify"""
    plain, ok = np.zeros((len(keys), length), np.uint8), np.zeros(len(keys), np.uint8)
    cache = {}
    for i in range(len(keys)):
        one_time, ks = _streams(cache, keys[i].tobytes(), nonce, length)
        if poly1305(one_time, mac_data(bytes(aad), data[i, :length].tobytes())) == data[i, length:length + 16].tobytes():
            plain[i], ok[i] = data[i, :length] ^ ks, 1
    return plain, ok


def pool_keys(n, nkeys, seed):
    """n keys drawn from a pool of nkeys: the restatement makes a key's streams once"""
    pool = KC.rng_bytes(seed, max(nkeys, 1), 32)
    return np.ascontiguousarray(pool[np.arange(n) % max(nkeys, 1)])


# ---------------------------------------------------------------------------------------------------- planted Poly1305 cases
def _key(r, s):
    return int(r).to_bytes(16, "little") + int(s).to_bytes(16, "little")


FF16 = b"\xff" * 16
ALL = (1 << 128) - 1


def planted():
    """[(name, key, message, expected tag or None)]: the tags the issue states are held here as literals, the rest come from poly1305()"""
    le = lambda v: int(v).to_bytes(16, "little")      # noqa: E731
    cases = [
        ("h = p - 1", _key(1, 0), FF16 + le((1 << 128) - 5), bytes([0xFA]) + b"\xff" * 15),
        ("h = p", _key(1, 0), FF16 + le((1 << 128) - 4), bytes(16)),
        ("h = p + 1", _key(1, 0), FF16 + le((1 << 128) - 3), bytes([1]) + bytes(15)),
        ("h = 2^130 - 2", _key(1, 0), FF16 + FF16, bytes([3]) + bytes(15)),
        ("h = 2^130 - 2, s = ff x 16", _key(1, ALL), FF16 + FF16, bytes([2]) + bytes(15)),
        ("r at the clamp's maximum, 1024 bytes of ff", _key(CLAMP, 0x0123456789abcdef0123456789abcdef), b"\xff" * 1024, None),
        ("r with every bit set", _key(ALL, 0x0123456789abcdef0123456789abcdef), b"\xff" * 1024, None),
        ("r = 0", _key(0, 0xfedcba9876543210fedcba9876543210), bytes(range(64)), None),
        ("r = 0, s = 0", _key(0, 0), b"\xff" * 32, bytes(16)),
    ]
    for j, length in enumerate((4, 8, 12, 20, 24, 28, 564 + 4, 564 + 8, 1020)):                # 4, 8 and 12 bytes in the last block
        cases.append(("last block of %d bytes (len %d)" % (length % 16, length), KC.rng_bytes(9100 + j, 32).tobytes(), KC.rng_bytes(9150 + j, length).tobytes(), None))
    for j, length in enumerate((16, 64, 564, 1024)):                                           # seeded random rows
        cases.append(("random row of %d bytes" % length, KC.rng_bytes(9200 + j, 32).tobytes(), KC.rng_bytes(9250 + j, length).tobytes(), None))
    # the high bytes of every limb set in r and in the data: the widest products the clamp allows, a last block of 12 bytes behind them
    cases.append(("wide limbs, 12 bytes in the last block", _key(CLAMP, ALL), b"\xff" * 1020, None))
    return [(name, key, msg, poly1305(key, msg) if tag is None else tag) for name, key, msg, tag in cases]


# ---------------------------------------------------------------------------------------------------- tampered rows
def tamper_list(length):
    """[(name, what)]: what = ("ct", byte, bit) | ("tag", byte, bit) | ("neighbour",) | ("key", byte, bit)"""
    t = [("first ciphertext byte", ("ct", 0, 0)), ("last ciphertext byte", ("ct", length - 1, 7))]
    t += [("tag byte %d" % b, ("tag", b, (3 * b) % 8)) for b in range(16)]
    t += [("the neighbour's tag", ("neighbour",)), ("one bit of the key", ("key", 13, 5))]
    return t


def tamper(keys, rows, length, victims):
    """copies of keys and rows with the tamper list applied to the rows `victims` in turn -> (keys, rows, {row: name})"""
    keys, rows = keys.copy(), rows.copy()
    names = {}
    todo = tamper_list(length)
    for k, i in enumerate(victims):
        name, what = todo[k % len(todo)]
        if what[0] == "ct":
            rows[i, what[1]] ^= 1 << what[2]
        elif what[0] == "tag":
            rows[i, length + what[1]] ^= 1 << what[2]
        elif what[0] == "neighbour":
            rows[i, length:length + 16] = rows[(i + 1) % len(rows), length:length + 16]
        else:
            keys[i, what[1]] ^= 1 << what[2]
        names[i] = name
    return keys, rows, names
