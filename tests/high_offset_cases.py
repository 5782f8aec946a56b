"""Layouts that put the rows of one call at byte offsets from 2^31 up to 2^32: the range in which the kernels' 32-bit row offsets (`u32 pos` in
k_sig_challenge, k_blake2s and k_pedersen_*) and the 64-bit products i * in_stride of the cipher kernels have a set bit 31, a carry out of it,
or end at the very top.  Every entry point takes up to 2^32 bytes of rows per call, so every layout here is a call the ABI promises to accept;
tests/test_high_offset_cases_cpu.py checks that arithmetic, tests/test_emu_high_offsets.py runs the device functions at these offsets on the
CPU and tests/test_gpu_high_offsets.py the kernels.  Nothing here runs the library or holds data: a layout is numbers only.  Test
infrastructure only.

n * stride <= 2^32 is the bound, so a row can END at 2^32 only where rows are dense (stride = the row's bytes); sparse layouts with a huge
stride reach the other offsets with a handful of rows."""
import numpy as np

T31, T32 = 1 << 31, 1 << 32
SEEDED_OTHERS = 64


class Layout:
    """n rows, row i at byte i * stride of the call's array, `rowbytes` of it read (length, plus the tag where there is one)."""

    def __init__(self, id, n, stride, length, rowbytes=None, out_row=None):
        self.id, self.n, self.stride, self.length = id, n, stride, length
        self.rowbytes = length if rowbytes is None else rowbytes
        self.out_row = out_row
        self.dense = self.stride == self.rowbytes

    def start(self, i):
        return i * self.stride

    def end(self, i):
        return i * self.stride + self.rowbytes

    @property
    def span(self):
        """bytes from the array's first byte to the last byte any row reads"""
        return self.end(self.n - 1)

    def touching(self, lo, hi):
        """the rows with a byte in [lo, hi)"""
        first = max(0, (lo - self.rowbytes) // self.stride + 1) if lo >= self.rowbytes else 0
        return [i for i in range(first, min(self.n, -(-hi // self.stride))) if self.start(i) < hi and self.end(i) > lo]

    def named_rows(self):
        """what the GPU test holds to the oracle byte for byte: rows 0 and 1, every row that touches [2^31 - 2 rowbytes, 2^31 + 2 rowbytes), the
        last three rows and 64 seeded others; every row of a layout that has no more than those"""
        if self.n <= SEEDED_OTHERS:
            return list(range(self.n))
        rows = {0, 1, self.n - 3, self.n - 2, self.n - 1} | set(self.touching(T31 - 2 * self.rowbytes, T31 + 2 * self.rowbytes))
        rng = np.random.default_rng(0x48494F46 + self.n + self.stride)
        rows |= {int(x) for x in rng.integers(0, self.n, SEEDED_OTHERS)}
        return sorted(rows)

    def top_rows(self):
        """what the CPU emulation takes of a dense layout: the last three rows, the row across (or at) 2^31 and its two neighbours"""
        mid = T31 // self.stride
        return sorted({mid - 1, mid, mid + 1, self.n - 3, self.n - 2, self.n - 1})

    def split_row(self):
        """k for the two-halves call: base + k * stride 16-byte aligned, k * stride about 2^31"""
        k = T31 // self.stride
        while (k * self.stride) % 16:
            k -= 1
        return k


def classes(layouts, end_at_top=True):
    """which of the dangerous positions a set of layouts reaches: {"row0", "below", "straddle", "at", "top"}"""
    seen = set()
    for L in layouts:
        seen.add("row0")
        for i in L.touching(T31 - L.rowbytes, T31 + L.rowbytes):
            s, e = L.start(i), L.end(i)
            if T31 - 16 < e <= T31:
                seen.add("below")
            if s < T31 < e:
                seen.add("straddle")
            if s == T31:
                seen.add("at")
        if L.span == T32:
            seen.add("top")
    return seen


ALL_CLASSES = {"row0", "below", "straddle", "at", "top"}

# ---- jj_chacha20_xor, jj_poly1305, jj_aead_seal, jj_aead_open: rows of aligned dwords, len <= 1024
CIPHER_SPARSE = Layout("sparse", 4, (1 << 30) - 256, 1024)                       # row 2 starts at 2^31 - 512; 4 * stride = 2^32 - 1024
CIPHER_DENSE = Layout("dense", 1 << 22, 1024, 1024)                              # ends at 2^32
CHACHA20 = POLY1305 = (CIPHER_SPARSE, CIPHER_DENSE)
SEAL_DENSE = Layout("dense", 1 << 22, 1008, 1008, out_row=1024)                  # the OUTPUT of n x 1024 bytes ends at 2^32
AEAD_SEAL = (Layout("sparse", 4, (1 << 30) - 256, 1024, out_row=1040), SEAL_DENSE)
OPEN_DENSE = Layout("dense", 1 << 22, 1024, 1008, rowbytes=1024)                 # the last row's tag ends at 2^32
AEAD_OPEN = (Layout("sparse", 4, (1 << 30) - 256, 1008, rowbytes=1024), OPEN_DENSE)

# ---- jj_blake2s, jj_group_hash: rows at any byte, msg_len <= 65536.  The prefix leaves a tail (75 = one whole block and 11 bytes), so that
# `at` > 0 in the first block and the virtual start pos - at of row 0 is negative
B2S_SPARSE = Layout("sparse", 4, (1 << 30) - 3, 150)                             # rows at residues 0, 1, 2, 3 mod 4; row 2 starts at 2^31 - 6
B2S_DENSE = Layout("dense", 1 << 16, 1 << 16, 1 << 16)                           # ends at 2^32
B2S_ODD = Layout("odd_dense", 65551, 65521, 65521)                               # every residue mod 4, a row across 2^31, 225 bytes short of 2^32
BLAKE2S = GROUP_HASH = (B2S_SPARSE, B2S_DENSE, B2S_ODD)
B2S_PREFIX_LEN = 75
B2S_PERSONAL = b"JJ_hioff"

# ---- jj_sig_challenge: dense by definition (fixed msg_len, or CSR offsets)
SIG_FIXED = Layout("fixed", 1 << 16, 1 << 16, 1 << 16)
SIG_RAGGED_N, SIG_RAGGED_EMPTY = (1 << 16) + 3, 3
SIG_PERSONAL = b"JJ_hioff_sigchal"


def sig_ragged_offsets():
    """n + 1 = 2^16 + 4 offsets: 2^16 seeded lengths within +-4096 of 2^16, adjusted so that one message straddles 2^31 from an odd offset and the
    total is exactly 2^32; three empty messages follow, whose offsets are 2^32 itself"""
    m = 1 << 16
    rng = np.random.default_rng(0x5349474F)
    lens = (m + rng.integers(-4000, 4001, m)).astype(np.int64)
    h = m // 2

    def settle(lo, hi, total):
        """spread what the lengths lo .. hi - 1 miss of `total` evenly over them (a few dozen bytes each), the remainder one byte each"""
        miss = total - int(lens[lo:hi].sum())
        q, r = divmod(miss, hi - lo)
        lens[lo:hi] += q
        lens[lo:lo + r] += 1

    settle(0, h, T31 - 4097)                                                     # message h starts at an odd offset and (>= 61440 bytes) reaches past 2^31
    settle(h, m, T32 - (T31 - 4097))
    assert (abs(lens - m) <= 4096).all()
    off = np.zeros(m + 1, np.int64)
    off[1:] = np.cumsum(lens)
    return np.concatenate([off, np.full(SIG_RAGGED_EMPTY, T32, np.int64)]).astype(np.uint64)


def sig_ragged_named(offsets):
    """the messages held to the oracle: 0 and 1, the one across 2^31 with two neighbours on each side, the last three with bytes, the empty
    ones and 64 seeded others"""
    n = len(offsets) - 1
    j = int(np.searchsorted(offsets, T31, side="right")) - 1
    rows = {0, 1} | set(range(j - 2, j + 3)) | set(range(n - SIG_RAGGED_EMPTY - 3, n))
    rows |= {int(x) for x in np.random.default_rng(0x5349474F + 1).integers(0, n, SEEDED_OTHERS)}
    return sorted(rows)


# ---- jj_pedersen_hash_vartime, jj_pedersen_scalars: the small generator sets of tests/pedersen_cases.py; no dense case (the unit is far heavier
# and the sparse cases reach the same offsets).  `ends` is what the fields cover of a row.
class PedLayout:
    def __init__(self, id, n, row_stride, fields, gens="three", seg_chunks=63, prefix=0, prefix_bits=0):
        self.id, self.n, self.row_stride, self.fields, self.gens, self.seg_chunks, self.prefix, self.prefix_bits = id, n, row_stride, tuple(fields), gens, seg_chunks, prefix, prefix_bits
        self.cover = max(off + (nb + 7) // 8 for off, nb in self.fields)
        self.bits_len = prefix_bits + sum(nb for _, nb in self.fields)

    def spans(self, i):
        """(first byte, one past the last byte) of every field of row i, as offsets into the call's array"""
        return [(i * self.row_stride + off, i * self.row_stride + off + (nb + 7) // 8) for off, nb in self.fields]

    def bits(self, i, read):
        """the message bits of unit i; read(offset, nbytes) -> the bytes of the call's array"""
        out = [(self.prefix >> k) & 1 for k in range(self.prefix_bits)]
        for (lo, hi), (_, nb) in zip(self.spans(i), self.fields):
            b = read(lo, hi - lo)
            out += [(b[k >> 3] >> (k & 7)) & 1 for k in range(nb)]
        return out


P29, P30 = 1 << 29, 1 << 30
PED_A = PedLayout("a", 4, P30, ((0, 61), (P29 - 3, 40), (P30 - 9, 72)), prefix=0b100101, prefix_bits=6)      # a field across byte 2^29; the last row ends at 2^32
# rows at three residues; the issue's fields at 0 and 2^29 + 5, and one more that lies across 2^31 in row 1 (2^31 - 4 - row_stride)
PED_B = PedLayout("b", 3, 1431655765, ((0, 33), (P29 + 5, 50), (T31 - 4 - 1431655765, 61)), gens="two", seg_chunks=63)
PED_C = PedLayout("c", 2, T31, ((3, 13), (T31 - 12, 95)), gens="one", seg_chunks=63)                          # a field that ends at the row's end
PED_D = PedLayout("d", 1, T32, ((1, 20), (T32 - 9, 72)), gens="two", seg_chunks=20)                           # cover = 2^32: accepted, see jj_pedersen.h
PEDERSEN = (PED_A, PED_B, PED_C, PED_D)
PED_WINDOWS = (0, 3)                                                                                           # the default (4) and one narrower table
