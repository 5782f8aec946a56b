"""tests/sig_challenge_cases.py, pinned without a GPU: the oracle is the RFC's BLAKE2b (hashlib) with its personalisation, the case table reaches
every hashed length it must in every part combination that fits, the ragged case plants what it says, and the entry point's buffer-discipline
row joins the table."""
import hashlib

import numpy as np

from oracle.jubjub_ref import FR, R_MOD
from tests import sig_challenge_buffer_row as BR  # joins buffer_cases.CASES at collection, before the table's coverage pin runs
from tests import sig_challenge_cases as CC

RFC7693_ABC = ("ba80a53f981c4d0d6a2797b69f12f6e94c212f14685ac4b74b12bb6fdbffa2d17d87c5392aab792dc252d5de4533cc9518d38aa8dbf1925ab92386edd4009923")


def test_oracle_is_rfc7693_blake2b():
    assert hashlib.blake2b(b"abc").hexdigest() == RFC7693_ABC                      # RFC 7693, appendix A
    assert hashlib.blake2b(b"abc", digest_size=64, person=b"").hexdigest() == RFC7693_ABC


def test_personalisation_changes_the_digest_and_zeros_do_not():
    plain = hashlib.blake2b(b"abc", digest_size=64).digest()
    assert hashlib.blake2b(b"abc", digest_size=64, person=bytes(16)).digest() == plain
    assert hashlib.blake2b(b"abc", digest_size=64, person=CC.REDJUBJUB).digest() != plain
    assert hashlib.blake2b(b"abc", digest_size=64, person=b"\xff" * 16).digest() != plain
    assert (CC.challenge(None, b"abc") == CC.challenge(bytes(16), b"abc")).all() and (CC.challenge(None, b"abc") != CC.challenge(CC.REDJUBJUB, b"abc")).any()
    assert len(CC.REDJUBJUB) == 16 and CC.PERSONALS["null"] is None and CC.PERSONALS["zeros"] == bytes(16)
    from jubjub_amd.engine import REDJUBJUB_PERSONAL
    assert REDJUBJUB_PERSONAL == CC.REDJUBJUB == b"Zcash_RedJubjubH"


def test_challenge_is_the_wide_reduction_of_the_digest():
    d = hashlib.blake2b(b"abc", digest_size=64, person=CC.REDJUBJUB).digest()
    c = CC.challenge(CC.REDJUBJUB, b"abc")
    assert int.from_bytes(bytes(c), "little") == int.from_bytes(d, "little") % R_MOD == FR.from_bytes_wide(d) and c.shape == (32,)


def test_case_table_coverage():
    assert set(CC.TOTALS) >= {0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 384}
    have = {(t, c) for t, c, _ in CC.CASES}
    for t in CC.TOTALS:
        for combo in CC.COMBOS:
            assert ((t, combo) in have) == (t >= CC.PREFIX[combo]), (t, combo)           # wherever the length allows
    for t, combo, msg_len in CC.CASES:
        assert CC.PREFIX[combo] + msg_len == t and msg_len >= 0
    assert {c for t, c, _ in CC.CASES if t == 0} == {"none"} and {c for t, c, _ in CC.CASES if t == 63} == {"r", "a", "none"}
    assert {c for t, c, m in CC.CASES if m == 0} == set(CC.COMBOS)                        # an empty message behind every combination
    assert CC.SIZES == (1, 63, 64, 65, 257)


def test_expected_uses_the_parts_in_order():
    R, A = CC.parts(3, "both")
    msgs = [b"", b"x", b"yz" * 70]
    e = CC.expected(CC.REDJUBJUB, R, A, msgs)
    for i in range(3):
        assert (e[i] == CC.challenge(CC.REDJUBJUB, bytes(R[i]) + bytes(A[i]) + msgs[i])).all()
    assert (CC.expected(None, None, A, msgs)[2] == CC.challenge(None, bytes(A[2]) + msgs[2])).all()
    assert (CC.expected(None, R, None, msgs)[1] != CC.expected(None, None, R, msgs)[1]).sum() == 0       # one part is one part, whichever argument


def test_ragged_case_plants_what_it_says():
    for prefix in (0, 32, 64):
        L = CC.ragged_lengths(prefix)
        assert len(L) == CC.RAGGED_N == 300 and L[0] == 0 and L[-1] == 0
        assert L[3] + prefix == 384 and all(L[i] == 0 for i in (0, 1, 2, 4, 5, 6, 7))      # three blocks among empty lanes of the first wave
        assert [L[8 + k] + prefix for k in range(6)] == [max(prefix, t) for t in (63, 64, 65, 127, 128, 129)]
        assert [L[16 + k] for k in range(6)] == [63, 64, 65, 127, 128, 129]
        for reverse in (False, True):
            msgs = CC.ragged(prefix, reverse=reverse)
            assert [len(m) for m in msgs] == (L[::-1] if reverse else L)
            assert CC.start_residues(msgs) == set(range(16))
            flat, off = CC.pack(msgs)
            assert off[0] == 0 and int(off[-1]) == flat.size == sum(L) and all(bytes(flat[int(off[i]):int(off[i + 1])]) == msgs[i] for i in range(len(msgs)))
    assert CC.ragged(64) == CC.ragged(64)[:] and CC.ragged(64, reverse=True) == CC.ragged(64)[::-1]


def test_buffer_row_joins_the_table():
    import buffer_cases as BC

    assert BR.ROW in BC.CASES and BR.ROW.covers == ("jj_sig_challenge",) and BR.MSG_LEN == 33
    assert [k for k, _ in BR.ROW.ins] == ["r", "a", "m"] and BR.ROW.outs == [("c", 32)]
    ins, outs = BR.ROW.data(5)
    assert ins["m"].shape == (5, 33) and outs["c"].shape == (5, 32)
    assert (outs["c"][4] == CC.challenge(CC.REDJUBJUB, bytes(ins["r"][4]) + bytes(ins["a"][4]) + bytes(ins["m"][4]))).all()
    assert BR.ROW.data(0)[1]["c"].size == 0
