"""tests/group_hash_cases.py, pinned without a GPU: hashlib's BLAKE2s gives the values of RFC 7693, the restatement hashes prefix || message
under the personalisation, the case matrix holds every prefix length, message length and stride it must and the totals 0, 64 and 128, every
shape's seed gives rows that decode and rows that are refused under every flag set, TORSION_FREE and CLEAR_COFACTOR each change a result in
every case that sets them, and the two buffer-discipline rows stand in the table with the restatement's bytes."""
import hashlib

import numpy as np
import pytest

from oracle import jubjub_ref as J
from tests import group_hash_buffer_row as BR  # joins buffer_cases.CASES at collection, before the table's coverage pin runs
from tests import group_hash_cases as GC


def test_blake2s_of_the_restatement_is_rfc_7693():
    assert hashlib.blake2s(b"abc").hexdigest() == "508c5e8c327c14e2e1a72ba34eeb452f37458b209ed63a294d999b4c86675982"      # RFC 7693 appendix B
    assert hashlib.blake2s(b"").hexdigest() == "69217a3079908094e11121d042354a7c1f55b6482ca1a51e1b250dfd1ed0eef9"
    abc = np.frombuffer(b"abc", dtype=np.uint8).reshape(1, 3)
    assert GC.digests(None, b"", abc)[0].tobytes().hex() == "508c5e8c327c14e2e1a72ba34eeb452f37458b209ed63a294d999b4c86675982"
    assert GC.digests(None, b"ab", abc[:, 2:])[0].tobytes() == GC.digests(None, b"", abc)[0].tobytes()              # the prefix is hashed in front of the row
    assert GC.digests(None, b"", np.zeros((1, 0), np.uint8))[0].tobytes().hex() == "69217a3079908094e11121d042354a7c1f55b6482ca1a51e1b250dfd1ed0eef9"
    assert GC.digests(b"JJ_gh_t0", b"", abc)[0].tobytes() == hashlib.blake2s(b"abc", person=b"JJ_gh_t0").digest() != hashlib.blake2s(b"abc").digest()
    assert GC.digests(bytes(8), b"", abc)[0].tobytes() == hashlib.blake2s(b"abc").digest()                           # no personalisation = eight zero bytes


def test_the_matrix_holds_what_it_must():
    assert GC.PREFIX_LENS == (0, 1, 11, 63, 64, 65, 128, 200) and GC.MSG_LENS == (0, 1, 3, 4, 11, 32, 55, 56, 63, 64, 65, 128, 129)
    assert {p for p, _ in GC.SHAPES} == set(GC.PREFIX_LENS) and {m for _, m in GC.SHAPES} == set(GC.MSG_LENS) and len(set(GC.SHAPES)) == len(GC.SHAPES)
    assert len(GC.PAIRS) == 8 * 13 == len(set(GC.PAIRS)) and set(GC.SHAPES) <= set(GC.PAIRS) and all(GC.personal_of(s) in GC.PERSONALS for s in GC.PAIRS)
    totals = {p + m for p, m in GC.SHAPES}
    assert {0, 64, 128} <= totals
    # an exact block end with the boundary inside the prefix, at its end and inside the message; the empty input; a prefix of whole blocks alone
    assert {(63, 1), (0, 64), (64, 0), (64, 64), (128, 0), (63, 65), (65, 63), (0, 128), (0, 0)} <= set(GC.SHAPES) and GC.MAIN in GC.SHAPES
    assert GC.ROWS == 96 and GC.PAD == (0, 1, 5)
    for L in GC.MSG_LENS:                                            # the three strides between them put rows at every residue mod 4
        assert {(i * (L + pad)) % 4 for pad in GC.PAD for i in range(GC.ROWS)} == {0, 1, 2, 3}, L
    assert GC.FLAG_SETS == (0, 1, 1 | 4 | 8, 2, 1 | 2 | 4 | 8) and GC.SAPLING_SHAPED == 13
    assert set(GC.SEEDS) == {s for s in GC.SHAPES if s[1]}
    assert None in GC.PERSONALS and all(p is None or len(p) == 8 for p in GC.PERSONALS) and {GC.personal_of(s) for s in GC.SHAPES} == set(GC.PERSONALS)
    msgs = GC.messages(GC.MAIN)
    buf, view = GC.layout(msgs, 5)
    assert view.shape == (96, 11) and view.strides == (16, 1) and np.array_equal(view, msgs) and (buf.reshape(96, 16)[:, 11:] == 0xA5).all()
    assert np.array_equal(GC.messages(GC.MAIN, 257)[:96], msgs)


@pytest.mark.parametrize("shape", [s for s in GC.SHAPES if s[1]], ids=lambda s: "%d+%d" % s)
def test_the_seed_of_every_shape_serves(shape):
    """at least 8 rows decode and 8 are refused under every flag set; TORSION_FREE changes an ok byte, CLEAR_COFACTOR a point"""
    assert GC.conditions(shape) == []
    for flags in GC.FLAG_SETS:
        pts, ok = GC.case_expected(shape, flags)
        assert pts.shape == (96, 64) and ok.shape == (96,) and set(ok.tolist()) == {0, 1}
        assert not pts[ok == 0].any()                                                   # a refused row is (0, 0)


def test_the_shapes_without_a_message_are_one_digest():
    """msg_len = 0: every row hashes the prefix alone, so the 96 rows are one digest and one verdict -- these shapes cannot have rows of both kinds"""
    for shape in (s for s in GC.SHAPES if s[1] == 0):
        assert GC.messages(shape).shape == (96, 0)
        d = GC.digests(GC.personal_of(shape), GC.prefix_of(shape), GC.messages(shape))
        assert (d == d[0]).all() and d[0].tobytes() == hashlib.blake2s(GC.prefix_of(shape), person=GC.personal_of(shape) or b"").digest()
        for flags in GC.FLAG_SETS:
            pts, ok = GC.case_expected(shape, flags)
            assert (ok == ok[0]).all() and (pts == pts[0]).all()


def test_the_restatement_decodes_as_the_oracle_does():
    pts, ok = GC.case_expected(GC.MAIN, 0)
    plain, _ = GC.case_expected(GC.MAIN, GC.ZIP216)
    cleared, ok13 = GC.case_expected(GC.MAIN, GC.SAPLING_SHAPED)
    d = GC.digests(GC.personal_of(GC.MAIN), GC.prefix_of(GC.MAIN), GC.messages(GC.MAIN))
    seen = 0
    for i in range(GC.ROWS):
        p, good = J.affine_from_bytes(d[i].tobytes(), zip216=True)
        assert bool(good) == bool(ok13[i])                                              # no small-order point comes out of a hash
        if good:
            assert plain[i].tobytes() == p[0].to_bytes(32, "little") + p[1].to_bytes(32, "little") and J.affine_is_on_curve(p)
            e = J.ext_mul_by_cofactor(J.affine_to_extended(p))
            q = J.ext_to_affine(e)
            assert cleared[i].tobytes() == q[0].to_bytes(32, "little") + q[1].to_bytes(32, "little") and J.ext_is_torsion_free(e)
            seen += 1
    assert seen >= 8 and np.array_equal(pts, plain) and np.array_equal(ok, ok13)
    # the loop of find_group_hash: the first counter with a point, and no earlier one
    b, i = GC.find_group_hash(b"JJ_gh_t0", GC.PREFIX_POOL[:64], b"generator", GC.SAPLING_SHAPED)
    assert GC.decode_digest(hashlib.blake2s(GC.PREFIX_POOL[:64] + b"generator" + bytes([i]), person=b"JJ_gh_t0").digest(), GC.SAPLING_SHAPED) == (b, 1)
    assert all(not GC.decode_digest(hashlib.blake2s(GC.PREFIX_POOL[:64] + b"generator" + bytes([j]), person=b"JJ_gh_t0").digest(), GC.SAPLING_SHAPED)[1] for j in range(i))


def test_buffer_rows_join_the_table():
    import buffer_cases as BC

    ids = {c.id for c in BC.CASES}
    assert {"jj_blake2s", "jj_group_hash"} <= ids and BR.ROW_HASH.covers == ("jj_blake2s",) and BR.ROW_GROUP.covers == ("jj_group_hash",)
    assert (BR.LEN, BR.STRIDE) == (11, 12) and dict(BR.ROW_HASH.ins)["m"] == 12 and dict(BR.ROW_GROUP.ins)["m"] == 12 and len(BR.PREFIX) == 64
    assert BR.ROW_HASH.out_bytes(5) == {"out": 160} and BR.ROW_GROUP.out_bytes(5) == {"pt": 320, "ok": 5}
    ins, outs = BR.ROW_HASH.data(65)
    assert ins["m"].shape == (65, 12) and outs["out"].shape == (65, 32)
    assert outs["out"][7].tobytes() == hashlib.blake2s(BR.PREFIX + ins["m"][7, :11].tobytes(), person=BR.PERSONAL).digest()
    ins, outs = BR.ROW_GROUP.data(65)
    assert outs["pt"].shape == (65, 64) and outs["ok"].shape == (65, 1) and 0 < int(outs["ok"].sum()) < 65
