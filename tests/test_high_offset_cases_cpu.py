"""The arithmetic of tests/high_offset_cases.py: every layout satisfies every documented limit of its entry point (include/jubjub_hip.h), and
the layouts of an entry point together put a row at each dangerous position -- row 0, a row that ends at 2^31, a row across 2^31, a row that
starts at 2^31, and a last row that ends exactly at 2^32.  No GPU, nothing large: a layout is numbers only."""
import numpy as np
import pytest

from tests import high_offset_cases as HC

T31, T32 = HC.T31, HC.T32


@pytest.mark.parametrize("name,layouts,tail", [("chacha20", HC.CHACHA20, 0), ("poly1305", HC.POLY1305, 0), ("aead_seal", HC.AEAD_SEAL, 0), ("aead_open", HC.AEAD_OPEN, 16)])
def test_cipher_layouts_keep_the_limits_and_reach_every_position(name, layouts, tail):
    for L in layouts:
        assert 4 <= L.length <= 1024 and L.length % 4 == 0 and L.stride % 4 == 0 and L.stride >= L.length + tail, (name, L.id)
        assert L.rowbytes == L.length + tail and L.n * L.stride <= T32, (name, L.id)
    sparse, dense = layouts
    assert sparse.n == 4 and sparse.start(2) == T31 - 512 and 4 * sparse.stride == T32 - 1024
    assert dense.n == 1 << 22 and dense.dense
    if name == "aead_seal":
        assert dense.span == dense.n * 1008 and dense.n * dense.out_row == T32 and dense.out_row == dense.length + 16      # the output ends at 2^32
        assert {"row0", "straddle"} <= HC.classes(layouts)                          # the input of 2^22 x 1008 bytes stays below 2^32 ...
        assert (T31 // dense.out_row) * dense.out_row == T31                         # ... and an output row starts at 2^31
    else:
        assert dense.span == T32 and HC.classes(layouts) == HC.ALL_CLASSES
    if name == "aead_open":
        assert dense.end(dense.n - 1) == T32 and dense.start(dense.n - 1) + dense.length == T32 - 16                        # the last row's tag ends at 2^32


def test_blake2s_layouts():
    sparse, dense, odd = HC.BLAKE2S
    for L in HC.BLAKE2S:
        assert L.length <= 65536 and L.stride >= L.length and L.n <= 1 << 24 and L.n * L.stride <= T32
    assert [sparse.start(i) % 4 for i in range(4)] == [0, 1, 2, 3] and sparse.start(2) == T31 - 6 and sparse.end(2) > T31
    assert dense.span == T32 and dense.start(1 << 15) == T31 and dense.end((1 << 15) - 1) == T31
    assert odd.span == T32 - 225 and {odd.start(i) % 4 for i in range(8)} == {0, 1, 2, 3}
    (j,) = [i for i in odd.touching(T31 - 1, T31 + 1) if odd.start(i) < T31 < odd.end(i)]
    assert j in odd.top_rows() and j in odd.named_rows()
    assert HC.classes(HC.BLAKE2S) == HC.ALL_CLASSES
    # the prefix leaves a tail: the message starts inside the first block and the virtual start of row 0 is negative
    assert 0 < HC.B2S_PREFIX_LEN % 64 and HC.B2S_PREFIX_LEN <= 4096 and len(HC.B2S_PERSONAL) == 8


def test_sig_challenge_layouts():
    f = HC.SIG_FIXED
    assert f.n <= 1 << 24 and f.n * f.length == T32 and HC.classes([f]) == {"row0", "below", "at", "top"}
    off = HC.sig_ragged_offsets()
    n = len(off) - 1
    assert n == HC.SIG_RAGGED_N == (1 << 16) + 3 and off.dtype == np.uint64 and off[0] == 0 and int(off[-1]) == T32
    lens = np.diff(off.astype(np.int64))
    assert (lens >= 0).all() and (lens[-3:] == 0).all() and (off[-4:] == T32).all()                 # three empty messages at offset 2^32 itself
    assert (abs(lens[:-3] - (1 << 16)) <= 4096).all()
    across = [i for i in range(n) if int(off[i]) < T31 < int(off[i + 1])]
    assert len(across) == 1 and int(off[across[0]]) % 2 == 1                                         # one message straddles 2^31 from an odd offset
    assert {int(o) % 4 for o in off[:64]} == {0, 1, 2, 3}
    named = HC.sig_ragged_named(off)
    assert set(range(across[0] - 2, across[0] + 3)) <= set(named) and {0, 1, n - 1, n - 4} <= set(named)
    assert np.array_equal(off, HC.sig_ragged_offsets())                                              # seeded: the same in every process


def test_pedersen_layouts():
    from tests import pedersen_cases as PC

    for P in HC.PEDERSEN:
        nseg = len(PC.generators(P.gens))
        assert 1 <= len(P.fields) <= 4 and 0 <= P.prefix_bits <= 32 and P.bits_len <= 3 * P.seg_chunks * nseg, P.id
        assert all(nb >= 1 and off < T32 and off + (nb + 7) // 8 <= P.row_stride for off, nb in P.fields), P.id
        assert P.row_stride <= T32 and P.n * P.row_stride <= T32, P.id
    a, b, c, d = HC.PEDERSEN
    assert a.n == 4 and a.row_stride == 1 << 30 and a.fields[1] == ((1 << 29) - 3, 40) and a.fields[2] == ((1 << 30) - 9, 72)
    assert a.spans(1)[1][0] < (1 << 30) + (1 << 29) < a.spans(1)[1][1] and a.spans(3)[2][1] == T32 and a.spans(1)[2][1] == T31 and a.spans(2)[0][0] == T31
    assert b.n == 3 and b.row_stride == 1431655765 and {b.row_stride * i % 4 for i in range(3)} == {0, 1, 2} and b.fields[1][0] == (1 << 29) + 5
    assert b.spans(1)[2][0] < T31 < b.spans(1)[2][1]                                                 # a field across 2^31
    assert c.n == 2 and c.row_stride == T31 and c.spans(0)[1][1] == T31 and c.spans(1)[1][1] == T32
    assert d.n == 1 and d.row_stride == T32 and d.fields[1] == (T32 - 9, 72) and d.cover == T32
    assert any(8 * off >= T32 for P in HC.PEDERSEN for off, _ in P.fields)                           # a bit number that does not fit 32 bits


def test_named_rows_and_the_split():
    for L in (HC.CIPHER_DENSE, HC.SEAL_DENSE, HC.OPEN_DENSE, HC.B2S_DENSE, HC.B2S_ODD, HC.SIG_FIXED):
        named = L.named_rows()
        assert {0, 1, L.n - 3, L.n - 2, L.n - 1} <= set(named) and len(named) <= 5 + 6 + HC.SEEDED_OTHERS and named == sorted(set(named))
        want = [i for i in range(max(0, T31 // L.stride - 4), T31 // L.stride + 5) if L.start(i) < T31 + 2 * L.rowbytes and L.end(i) > T31 - 2 * L.rowbytes]
        assert set(want) <= set(named) and len(want) >= 4
        assert named == L.named_rows()
        k = L.split_row()
        assert (k * L.stride) % 16 == 0 and 0 < k < L.n and abs(k * L.stride - T31) <= 16 * L.stride
        assert L.end(k - 1) <= T31 + L.stride and (L.n - k) * L.stride <= T31 + 16 * L.stride + L.stride    # both halves run (about) below 2^31
        tops = L.top_rows()
        assert {L.n - 3, L.n - 2, L.n - 1} <= set(tops) and any(L.start(i) <= T31 < L.end(i) or L.start(i) == T31 for i in tops)
    for L in (HC.CIPHER_SPARSE, HC.B2S_SPARSE):
        assert L.named_rows() == [0, 1, 2, 3]
