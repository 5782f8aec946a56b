"""tests/pedersen_cases.py, pinned without a GPU: the two formulations of the windowed Pedersen hash agree over the whole case table, enc is the
specification's table, the segment sums stay below (r - 1) / 2, short messages encode injectively, the planted rows are what they say, and the
entry points' buffer-discipline rows join the table."""
import itertools

import numpy as np

from oracle import jubjub_ref as J
from tests import pedersen_buffer_row as BR  # joins buffer_cases.CASES at collection, before the table's coverage pin runs
from tests import pedersen_cases as PC


def test_enc_is_the_specifications_table():
    assert {s: PC.enc(*s) for s in itertools.product((0, 1), repeat=3)} == PC.ENC_TABLE
    assert sorted(PC.ENC_TABLE.values()) == [-4, -3, -2, -1, 1, 2, 3, 4]
    assert PC.enc(0, 0, 0) == 1 and PC.enc(1, 1, 1) == -4                          # all zero bits: every chunk +1; all one bits: every chunk -4
    assert PC.chunks_of([]) == [] and PC.chunks_of([1]) == [2] and PC.chunks_of([0, 1]) == [3] and PC.chunks_of([0, 0, 1, 1]) == [-1, 2]      # padded with zero bits


def test_segment_sums_stay_below_half_the_group_order():
    worst = PC.segment_sums(63, 1, [1] * 189)[0]
    assert worst == -4 * (16 ** 63 - 1) // 15 and abs(worst) < (J.R_MOD - 1) // 2
    assert PC.segment_sums(63, 1, [0] * 189)[0] == (16 ** 63 - 1) // 15
    assert abs(worst) * 16 > (J.R_MOD - 1) // 2                                    # a 64th chunk would not fit: 63 is the limit the entry point sets


def test_short_messages_encode_injectively():
    seen = set()
    for length in range(10):
        for bits in itertools.product((0, 1), repeat=length):
            key = tuple(PC.segment_sums(3, 3, bits)) + (length,)
            assert key not in seen
            seen.add(key)
    assert len(seen) == 2 ** 10 - 1
    assert PC.segment_sums(3, 3, []) == [0, 0, 0]                                  # the empty message: no chunk at all, not the chunk 000


def test_the_two_formulations_agree_on_the_whole_table():
    for c in PC.CASES:
        gs = PC.generators(c.gens)
        want = PC.expected_points(c, PC.NROWS)
        for i in range(PC.NROWS):
            assert (PC.point_bytes(PC.by_chunks(gs, c.seg_chunks, c.bits(i))) == want[i]).all(), (c.id, i)


def test_case_table_holds_what_it_must():
    ids = {c.id for c in PC.CASES}
    assert {"merkle", "twin", "one_field_stride9", "overlap", "five_pieces", "prefix_only", "empty"} <= ids and {"tiny_%02d" % L for L in range(28)} <= ids
    m = PC.BY_ID["merkle"]
    assert (m.nseg, m.seg_chunks, m.row_stride, m.fields, m.prefix_bits, m.bits_len) == (3, 63, 64, ((0, 255), (32, 255)), 6, 516)
    for L, c in enumerate(PC.TINY):
        assert (c.nseg, c.seg_chunks, c.bits_len) == (3, 3, L)
    assert PC.TINY[27].bits_len == 3 * 3 * 3                                       # exactly at capacity
    assert {L % 3 for L in range(28)} == {0, 1, 2}                                 # no padding, two zero bits, one zero bit
    assert {(i * PC.TINY_STRIDE + PC.TINY_OFFSET) % 16 for i in range(PC.NROWS)} == set(range(16))
    o = PC.BY_ID["one_field_stride9"]
    assert (o.row_stride, o.fields[0][0]) == (9, 1) and {(i * 9 + 1) % 4 for i in range(4)} == {0, 1, 2, 3} and (PC.NROWS * 9) % 4
    v = PC.BY_ID["overlap"]
    assert v.bits_len == 3 * v.seg_chunks * v.nseg and v.fields[0][0] == v.fields[2][0]          # at capacity, and two fields read the same bytes
    assert PC.SIZES == (1, 63, 64, 65, 257) and PC.WINDOWS == (1, 2, 3, 4)
    for c in PC.CASES:
        if c.fields:
            assert set(PC.chunks_of(c.bits(0)[c.prefix_bits:])[:-1]) <= {1} and all(b == 1 for b in c.bits(1)[c.prefix_bits:])
        assert not c.rows.flags.writeable


def test_planted_identity_and_doubling():
    c = PC.BY_ID["twin"]
    gs = PC.generators("twin")
    assert gs[0] == gs[1] and J.ext_is_torsion_free(J.affine_to_extended(gs[0]))
    s = PC.segment_sums(63, 2, c.bits(PC.TWIN_CANCEL_ROW))
    assert s[0] == -s[1] != 0
    assert PC.expected(gs, 63, c.bits(PC.TWIN_CANCEL_ROW)) == J.AFFINE_IDENTITY and not PC.expected_points(c, 4)[PC.TWIN_CANCEL_ROW][:32].any()      # u = 0
    s = PC.segment_sums(63, 2, c.bits(PC.TWIN_EQUAL_ROW))
    assert s[0] == s[1] != 0
    half = J.affine_to_extended(PC._mul(gs[0], s[0]))
    assert PC.expected(gs, 63, c.bits(PC.TWIN_EQUAL_ROW)) == J.ext_to_affine(J.ext_double(half))
    assert PC.expected(PC.generators("three"), 63, []) == J.AFFINE_IDENTITY


def test_expected_scalars_are_the_sums_mod_r():
    c = PC.BY_ID["merkle"]
    s = PC.expected_scalars(c, 3)
    assert s.shape == (3, 3, 32)
    sums = PC.segment_sums(63, 3, c.bits(1))
    assert all(v < 0 for v in sums) and [int.from_bytes(bytes(s[j, 1]), "little") for j in range(3)] == [J.R_MOD + v for v in sums]
    assert not PC.expected_scalars(PC.BY_ID["tiny_09"], 2)[1:].any()               # a segment the message does not reach gets 0


def test_buffer_rows_join_the_table():
    import buffer_cases as BC

    assert BR.ROW_HASH in BC.CASES and BR.ROW_SCALARS in BC.CASES
    assert BR.ROW_HASH.covers == ("jj_pedersen_hash_vartime",) and BR.ROW_SCALARS.covers == ("jj_pedersen_scalars",)
    assert BR.ROW_HASH.ins == [("m", 9)] and BR.ROW_HASH.outs == [("out", 32)] and BR.ROW_SCALARS.outs == [("s", 32)] and BR.ROW_SCALARS.nrows("s", 5) == 15
    assert BR.PREFIX_BITS + sum(nb for _, nb in BR.FIELDS) == 3 * BR.SEG_CHUNKS * BR.NSEG
    ins, outs = BR.ROW_HASH.data(5)
    assert ins["m"].shape == (5, 9) and outs["out"].shape == (5, 32)
    want = PC.expected(PC.generators(BR.GENS), BR.SEG_CHUNKS, BR._bits(ins["m"][4]))
    assert bytes(outs["out"][4]) == want[0].to_bytes(32, "little")
    ins, outs = BR.ROW_SCALARS.data(5)
    assert outs["s"].shape == (15, 32)
    assert BR.ROW_HASH.data(0)[1]["out"].size == 0 and BR.ROW_SCALARS.data(0)[1]["s"].size == 0
