"""tests/commit_cases.py, pinned without a GPU: the two formulations of the windowed Pedersen commitment agree over the whole case table, the
cases hold what they say (strides, residues, arrays that end mid-dword, windows with pieces of two and of three sources, the padded last
chunk, the reordered and overlapping fields, the planted identity and doubling, the edge values of r), and the entry point's
buffer-discipline row joins the table."""
import numpy as np

from oracle import jubjub_ref as J
from tests import commit_buffer_row as BR  # joins buffer_cases.CASES at collection, before the table's coverage pin runs
from tests import commit_cases as CC
from tests import pedersen_cases as PC


def test_the_two_formulations_agree_on_the_whole_table():
    for c in CC.CASES:
        want = CC.expected_points(c, c.nrows)
        step = 1 if c.nrows <= 65 else 4                                           # by_chunks is the slow one: every unit of the short tables, every
        for i in sorted(set(range(0, c.nrows, step)) | set(range(8))):             # fourth of the long ones, and always the edge rows 0..7
            assert (PC.point_bytes(CC.by_chunks(c, i)) == want[i]).all(), (c.id, i)


def sources_per_window(c, w):
    """for every table window of w chunks that the message reaches: the set of sources its bits come from"""
    owner = [None] * c.prefix_bits
    for s, _, nb in c.fields:
        owner += [s] * nb
    out = []
    chunks = -(-c.bits_len // 3)
    for j in range(c.nseg):
        for k in range(0, c.seg_chunks, w):
            c0 = j * c.seg_chunks + k
            if c0 >= chunks:
                break
            t = min(w, c.seg_chunks - k, chunks - c0)
            out.append({s for s in owner[3 * c0:3 * (c0 + t)] if s is not None})
    return out


def test_case_table_holds_what_it_must():
    ids = [c.id for c in CC.CASES]
    assert ids == ["note", "tiny3_two", "tiny3_three", "tiny3_padded", "reordered", "twin", "hash_only", "one_source"]
    n = CC.BY_ID["note"]
    assert (n.nseg, n.seg_chunks, n.strides, n.fields, n.prefix, n.prefix_bits, n.bits_len) == (4, 63, (52, 32, 32), ((0, 12, 64), (1, 0, 256), (2, 0, 256)), 0b111111, 6, 582)
    assert -(-n.bits_len // 3) == 194 and 194 - 3 * 63 == 5 and n.nrows == 65 and n.sizes == (1, 63, 64, 65)
    for cid in ("tiny3_two", "tiny3_three", "tiny3_padded"):
        c = CC.BY_ID[cid]
        assert (c.nseg, c.seg_chunks, c.strides, tuple(off for _, off, _ in c.fields)) == (3, 3, (5, 3, 9), (1, 0, 2))
        for (s, off, _), st in zip(c.fields, c.strides):
            assert {(i * st + off) % 4 for i in range(4)} == {0, 1, 2, 3}           # the rows start at every residue modulo 4
            assert all((m * st) % 4 for m in c.sizes if m % 4)                       # ... and the array ends mid-dword at every size but the multiples of 4
        assert c.sizes == CC.SIZES
    assert CC.BY_ID["tiny3_two"].bits_len == 27 and any(len(s) == 2 for s in sources_per_window(CC.BY_ID["tiny3_two"], 4))
    assert any(len(s) == 2 for s in sources_per_window(CC.BY_ID["tiny3_two"], 1))  # even a window of one chunk straddles two sources there
    assert {0, 1, 2} in sources_per_window(CC.BY_ID["tiny3_three"], 3) and {0, 1, 2} in sources_per_window(CC.BY_ID["tiny3_three"], 4)
    assert CC.BY_ID["tiny3_three"].bits_len % 3 == 1 and CC.BY_ID["tiny3_padded"].bits_len % 3 == 2          # two padding bits, one padding bit
    r = CC.BY_ID["reordered"]
    assert [s for s, _, _ in r.fields] == [1, 0, 1]
    (_, o1, n1), _, (_, o2, n2) = r.fields
    assert o1 < o2 + (n2 + 7) // 8 and o2 < o1 + (n1 + 7) // 8                        # the two fields of source 1 share a byte
    assert CC.BY_ID["hash_only"].rbase is None and CC.BY_ID["one_source"].rbase is None and len(CC.BY_ID["one_source"].strides) == 1
    assert CC.SIZES == (1, 63, 64, 65, 257) and CC.WINDOWS == (1, 2, 3, 4)
    for c in CC.CASES:
        assert all(not a[0].any() and (a[1] == 0xFF).all() and not a.flags.writeable for a in c.sources)
        got = [int.from_bytes(c.r[i].tobytes(), "little") for i in range(min(6, c.nrows))]
        assert got == list(CC.R_EDGES) and not c.r.flags.writeable
        assert [c.r_int(i) for i in range(6)] == [0, 1, J.R_MOD - 1, J.R_MOD, (1 << 252) - 1, (1 << 252) - 1]
    assert J.R_MOD < 1 << 252 < 2 * J.R_MOD                                         # r and 2^252 - 1 are past the order: [r]R is the identity


def test_planted_identity_and_doubling():
    c = CC.BY_ID["twin"]
    p0 = CC.bases()["P0"]
    assert CC.gens_of("one") == (p0,) and c.rbase == "P0"
    m = PC.segment_sums(63, 1, c.bits(CC.TWIN_CANCEL_ROW))[0]
    assert m and c.r_int(CC.TWIN_CANCEL_ROW) == (-m) % J.R_MOD
    assert CC.expected(c, CC.TWIN_CANCEL_ROW) == J.AFFINE_IDENTITY and not CC.expected_points(c, 8)[CC.TWIN_CANCEL_ROW][:32].any()      # u = 0
    m = PC.segment_sums(63, 1, c.bits(CC.TWIN_EQUAL_ROW))[0]
    assert m and c.r_int(CC.TWIN_EQUAL_ROW) == m % J.R_MOD
    half = J.affine_to_extended(PC._mul(p0, m))
    assert CC.expected(c, CC.TWIN_EQUAL_ROW) == J.ext_to_affine(J.ext_double(half))
    # r = r (unit 3): the blinding term is the identity and the commitment is the hash
    assert CC.expected(c, 3) == PC.expected((p0,), 63, c.bits(3))


def test_packed_rows_carry_the_same_message():
    for c in CC.CASES:
        rows, pairs = c.packed(5)
        for i in range(5):
            bits = [(c.prefix >> k) & 1 for k in range(c.prefix_bits)]
            for off, nb in pairs:
                bits += [(int(rows[i][off + (k >> 3)]) >> (k & 7)) & 1 for k in range(nb)]
            assert bits == c.bits(i), (c.id, i)


def test_buffer_row_joins_the_table():
    import buffer_cases as BC

    assert BR.ROW in BC.CASES and BR.ROW.covers == ("jj_pedersen_commit_vartime",)
    assert BR.ROW.ins == [("a", 9), ("b", 5), ("c", 3), ("r", 32)] and BR.ROW.outs == [("out", 32)]
    assert BR.PREFIX_BITS + sum(nb for _, _, nb in BR.FIELDS) == 3 * BR.SEG_CHUNKS * BR.NSEG
    ins, outs = BR.ROW.data(9)
    assert [ins[k].shape for k in "abcr"] == [(9, 9), (9, 5), (9, 3), (9, 32)] and outs["out"].shape == (9, 32)
    assert ins["r"][8, 8:].any() and not ins["r"][7, 8:].any()
    assert bytes(outs["out"][8]) == BR._point(ins, 8)[0].to_bytes(32, "little")
    assert BR.ROW.data(0)[1]["out"].size == 0
