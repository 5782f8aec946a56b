"""Cases of jj_sig_challenge (Schnorr challenges hashed on the device): c = Fr::from_bytes_wide(BLAKE2b-512(personal; R || A || M)) as 32
canonical bytes.  The oracle is hashlib.blake2b(data, digest_size=64, person=personal) followed by oracle.jubjub_ref.FR.from_bytes_wide; nothing
here runs the library.  Everything is seeded and small.  Test infrastructure only.

TOTALS are the hashed lengths (parts plus message) the tests must reach: the empty input, one byte, and the lengths around one, two and three
128-byte blocks (a block's last byte, its exact end, one byte into the next); 32 is one part and an empty message; 384 ends exactly on the
third block.  CASES crosses them with the
four part combinations wherever the parts fit into the total.  ragged() plants, inside one wave, a three-block message among empty ones, empty
messages at both ends, neighbours straddling the block edges, and start offsets of every residue modulo 16."""
import hashlib

import numpy as np

from oracle.jubjub_ref import FR

TOTALS = (0, 1, 32, 63, 64, 65, 127, 128, 129, 255, 256, 257, 384)
COMBOS = ("both", "r", "a", "none")
PREFIX = {"both": 64, "r": 32, "a": 32, "none": 0}
REDJUBJUB = b"Zcash_RedJubjubH"
PERSONALS = {"null": None, "zeros": bytes(16), "redjubjub": REDJUBJUB, "ones": b"\xff" * 16}
SIZES = (1, 63, 64, 65, 257)
# (total hashed length, combination, message length)
CASES = [(t, c, t - PREFIX[c]) for t in TOTALS for c in COMBOS if t >= PREFIX[c]]


def rng_bytes(seed, *shape):
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


def challenge(personal, data):
    """the oracle: 32 canonical little-endian bytes"""
    d = hashlib.blake2b(bytes(data), digest_size=64, person=personal or b"").digest()
    return np.frombuffer(FR.to_bytes(FR.from_bytes_wide(d)), dtype=np.uint8)


def expected(personal, R, A, msgs):
    """R, A: (n, 32) arrays or None; msgs: n byte strings"""
    out = np.zeros((len(msgs), 32), np.uint8)
    for i, m in enumerate(msgs):
        out[i] = challenge(personal, (bytes(R[i]) if R is not None else b"") + (bytes(A[i]) if A is not None else b"") + bytes(m))
    return out


def parts(n, combo, seed=1):
    """(R, A) of a combination: seeded (n, 32) arrays or None.  The bytes are hashed as given; nothing has to decode."""
    R = rng_bytes(1000 + seed, n, 32) if combo in ("both", "r") else None
    A = rng_bytes(2000 + seed, n, 32) if combo in ("both", "a") else None
    return R, A


def fixed(n, msg_len, seed=1):
    """(n, msg_len) message bytes"""
    return rng_bytes(3000 + 7 * seed + msg_len, n, msg_len)


def pack(msgs):
    """byte strings -> (flat uint8 array, offsets uint64 of len(msgs) + 1)"""
    offsets = np.zeros(len(msgs) + 1, np.uint64)
    offsets[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
    flat = np.frombuffer(b"".join(bytes(m) for m in msgs), dtype=np.uint8).copy() if int(offsets[-1]) else np.zeros(0, np.uint8)
    return flat, offsets


RAGGED_N = 300


def ragged_lengths(prefix):
    """message lengths of RAGGED_N units for a given parts length: unit 0 and the last are empty; units 1..63 (one wave with unit 0) hold a
    three-block message among empty ones and, in neighbouring lanes, the totals 63/64/65 and 127/128/129; the rest are short lengths whose running
    sum takes the start offsets through every residue modulo 16."""
    L = [0] * RAGGED_N
    L[3] = 384 - prefix                                   # three blocks with the parts, among the empty units 0..2 and 4..7
    for k, t in enumerate((63, 64, 65, 127, 128, 129)):
        L[8 + k] = max(0, t - prefix)
    for k, t in enumerate((63, 64, 65, 127, 128, 129)):    # the message alone at the block edges
        L[16 + k] = t
    for i in range(24, RAGGED_N - 1):
        L[i] = (i * 7 + 3) % 41                             # 0 .. 40: odd and even steps
    L[40] = 0
    L[RAGGED_N - 1] = 0
    return L


def ragged(prefix, seed=5, reverse=False):
    """the messages of the ragged case as byte strings"""
    L = ragged_lengths(prefix)
    blob = rng_bytes(4000 + seed, sum(L)).tobytes()
    msgs, o = [], 0
    for n in L:
        msgs.append(blob[o:o + n])
        o += n
    return msgs[::-1] if reverse else msgs


def start_residues(msgs):
    """the residues modulo 16 at which the non-empty messages start in the packed array"""
    _, off = pack(msgs)
    return {int(off[i]) % 16 for i in range(len(msgs)) if len(msgs[i])}
