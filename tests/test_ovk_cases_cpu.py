"""The restatements of tests/ovk_cases.py, pinned without a GPU: the hash by the RFC 7693 "abc" digest and by a second way of cutting the same
string; the per-row key agreement by equality with tests/ka_cases.py's own keys when every row carries the same scalar and h32 is absent;
the case table by what the issue asks of it; the two compositions by a round trip through each other and through ka_cases / aead_cases."""
import hashlib

import numpy as np

from tests import aead_cases as AC
from tests import ka_cases as KC
from tests import ovk_buffer_row as BR  # joins buffer_cases.CASES at collection, before the table's coverage pin runs
from tests import ovk_cases as OC


def test_hash_restatement_is_rfc_7693():
    abc = np.frombuffer(b"abc\0", dtype=np.uint8)[None, :]
    assert hashlib.blake2b(b"abc").digest() == OC.RFC7693_ABC
    # the restatement cuts strings into prefix and sources; the same bytes cut another way give the same digest
    rows = KC.rng_bytes(1, 7, 96)
    whole = OC.digests([rows], 7, 64, None, b"abc")
    assert (OC.digests([rows[:, :32], rows[:, 32:36], rows[:, 36:]], 7, 64, None, b"abc") == whole).all()
    assert (OC.digests([rows[:, 1:]], 7, 64, None, b"abc" + rows[0, :1].tobytes())[0] == whole[0]).all()
    assert bytes(OC.digests([abc[:, :0]], 1, 64, None, b"abc")[0]) == OC.RFC7693_ABC
    # BLAKE2b-256 is its own hash, and the personalisation enters
    assert bytes(OC.digests([], 1, 32, None, b"abc")[0]) == hashlib.blake2b(b"abc", digest_size=32).digest() != OC.RFC7693_ABC[:32]
    assert bytes(OC.digests([], 1, 32, OC.SAPLING_OCK_PERSONAL, b"abc")[0]) == hashlib.blake2b(b"abc", digest_size=32, person=b"Zcash_Derive_ock").digest()


def test_case_table_holds_what_it_promises():
    by = OC.B2B_BY_NAME
    for pl in OC.PREFIX_LENS:
        for total in OC.TOTALS:
            assert (total < pl) or by["prefix%d_total%d" % (pl, total)].total == total
    totals = {c.total for c in OC.B2B_CASES}
    assert set(OC.TOTALS) <= totals
    assert any(c.total % 128 == 0 and c.total and c.parts for c in OC.B2B_CASES)                       # the last block is final
    assert by["prefix128_total128"].parts == () and by["prefix256_total256"].parts == ()              # the prefix alone: its last block is the final one
    assert any(len(c.parts) == 4 for c in OC.B2B_CASES)
    assert len({a for a, _, _ in by["one_array_two_sources"].parts}) == 1 and len(by["one_array_two_sources"].parts) == 2
    assert {c.parts[0][1] for c in (by["stride_over_len_skew0"], by["stride_over_len_skew16"])} == {0, 16}
    assert by["ock"].prefix_len == 32 and by["ock"].lens == [32, 32, 32]

    def spans(c):
        at, out = c.prefix_len, []
        for _, _, length in c.parts:
            out.append((at, at + length))
            at += length
        return out

    assert any(lo // 128 != (hi - 1) // 128 for c in OC.B2B_CASES for lo, hi in spans(c))              # a source across a block boundary
    assert any(hi % 128 == 0 and hi < c.total for c in OC.B2B_CASES for lo, hi in spans(c))            # a piece that ends on one, with more behind it
    assert by["longest_prefix"].prefix_len == 4096 and by["longest_source"].lens == [65536]
    for c in OC.B2B_CASES:                                                                           # the views are what the parts say
        arrays = c.arrays(3)
        for v, (a, skew, length) in zip(c.views(arrays), c.parts):
            assert v.shape == (3, length) and v.strides == (c.strides[a], 1) and (v == arrays[a][:, skew:skew + length]).all()


def test_ka_each_with_one_scalar_repeated_is_ka_cases():
    encs = KC.encodings()
    n = len(encs)
    for flags in KC.FLAGS:
        for k, sk in enumerate(KC.SCALARS[:4] + KC.SCALARS[8:10]):
            sks = np.repeat(np.frombuffer(sk, dtype=np.uint8)[None, :], n, axis=0)
            personal = list(KC.PERSONALS.values())[(flags + k) % 3]
            keys, ok = OC.ka_each(sks, encs, flags, personal)
            want_keys, want_ok = KC.expected(sk, encs, flags, personal)
            assert (keys == want_keys).all() and (ok == want_ok).all(), (flags, k)


def test_ka_each_grid_and_hash_rows():
    assert OC.GRID == len(KC.SCALARS) * len(KC.points())
    sks, encs = OC.ka_grid(OC.GRID)
    pairs = {(bytes(s), bytes(e)) for s, e in zip(sks, encs)}
    assert len(pairs) == len(set(KC.SCALARS)) * len({e for _, e in KC.points()})     # (two of the torsion points are also planted by name)
    flags, personal = KC.SAPLING_FLAGS, KC.SAPLING_PERSONAL
    h = OC.hash_rows(OC.GRID)
    with_h, ok_h = OC.ka_each(sks, encs, flags, personal, h)
    without, ok = OC.ka_each(sks, encs, flags, personal)
    assert (ok_h == ok).all() and ok.any() and not ok.all()
    assert ((with_h != without).any(axis=1) == (ok == 1)).all()                      # h32 enters every key that exists, and only the hash
    same, _ = OC.ka_each(sks, encs, flags, personal, encs)
    assert (same == without).all()                                                   # h32 = p32 is the NULL form
    plain, _ = OC.ka_each(sks, encs, flags & ~KC.KA_HASH_INPUT, personal, h)
    plain2, _ = OC.ka_each(sks, encs, flags & ~KC.KA_HASH_INPUT, personal)
    assert (plain == plain2).all()                                                   # without the flag nothing second is hashed
    i, j = KC.HIGH_PAIR                                                              # bits 252..255 of a scalar are not read
    assert OC.ka_one(KC.SCALARS[i], encs[-1], flags, personal) == OC.ka_one(KC.SCALARS[j], encs[-1], flags, personal)


def test_note_encrypt_and_ovk_open_round_trip():
    b = OC.planted_batch()
    kdf, ockp = KC.SAPLING_PERSONAL, OC.SAPLING_OCK_PERSONAL
    epk, c_enc, c_out = OC.note_encrypt(b["esk"], b["gd64"], b["pkd"], b["plain"], b["ovk"], b["cv"], b["cmu"], kdf, ockp)
    assert epk.shape == (OC.PLANTED_ROWS, 32) and c_enc.shape == (OC.PLANTED_ROWS, OC.NOTE_LEN + 16) and c_out.shape == (OC.PLANTED_ROWS, 80)
    # the recipient's side: ka_cases' key agreement with ivk against epk gives the key the sender sealed with
    clean = [i for i in range(OC.PLANTED_ROWS) if i not in OC.PLANT]
    keys, ok = KC.expected(b["ivk"], epk[clean], KC.SAPLING_FLAGS, kdf)
    assert ok.all()
    got, tag_ok = AC.open_rows(keys, c_enc[clean], OC.NOTE_LEN)
    assert tag_ok.all() and (got == b["plain"][clean]).all()
    # the sender's side
    c_enc_t, c_out_t = OC.tamper(c_enc, c_out)
    plain, op, ok, verdicts = OC.ovk_open(b["ovk"], b["cv"], b["cmu"], epk, c_out_t, c_enc_t, kdf, ockp, OC.OPEN_FLAGS)
    want = {"c_out tag": (0, 0, 0, 0), "c_enc tag": (1, 1, 1, 0), "esk >= r": (1, 0, 1, 1), "pk_d does not decode": (1, 1, 0, None), "pk_d of small order": (1, 1, 0, None)}
    for i in range(OC.PLANTED_ROWS):
        if i in OC.PLANT:
            assert ok[i] == 0 and not plain[i].any() and not op[i].any(), (i, OC.PLANT[i])
            for got_v, want_v in zip(verdicts[i], want[OC.PLANT[i]]):
                assert want_v is None or got_v == want_v, (i, OC.PLANT[i], verdicts[i])
        else:
            assert ok[i] == 1 and (plain[i] == b["plain"][i]).all() and bytes(op[i]) == bytes(b["pkd"][i]) + bytes(b["esk"][i]), i
    assert sorted(set(OC.PLANT.values())) == sorted(want)
    # another ovk opens nothing
    other = np.array(b["ovk"]) ^ 1
    assert not OC.ovk_open(other, b["cv"], b["cmu"], epk, c_out, c_enc, kdf, ockp)[2].any()


def test_buffer_rows_join_the_table():
    import buffer_cases as BC

    assert BR.ROW_B2B in BC.CASES and BR.ROW_EACH in BC.CASES
    assert BR.ROW_B2B.covers == ("jj_blake2b",) and BR.ROW_EACH.covers == ("jj_ka_kdf_each",)
    assert BR.ROW_B2B.ins == [("a", 36), ("b", 32), ("c", 44)] and BR.ROW_B2B.outs == [("out", 32)]
    assert BR.ROW_EACH.ins == [("sk", 32), ("p", 32), ("h", 32)] and BR.ROW_EACH.outs == [("key", 32), ("ok", 1)]
    assert all(BR.LENS[k] % 4 == 0 and BR.STRIDES[k] % 4 == 0 and BR.LENS[k] <= BR.STRIDES[k] for k in "abc") and BR.LENS["a"] < BR.STRIDES["a"]
    assert (len(BR.PREFIX) + sum(BR.LENS.values())) > 128                          # two blocks
    ins, outs = BR.ROW_B2B.data(9)
    assert [ins[k].shape for k in "abc"] == [(9, 36), (9, 32), (9, 44)] and outs["out"].shape == (9, 32)
    msg = BR.PREFIX + bytes(ins["a"][8, :32]) + bytes(ins["b"][8]) + bytes(ins["c"][8, :40])
    assert bytes(outs["out"][8]) == hashlib.blake2b(msg, digest_size=32, person=BR.PERSONAL).digest()
    ins, outs = BR.ROW_EACH.data(257)
    assert outs["key"].shape == (257, 32) and outs["ok"].shape == (257, 1) and 0 < int(outs["ok"].sum()) < 257
    assert BR.ROW_B2B.data(0)[1]["out"].size == 0 and BR.ROW_EACH.data(0)[1]["key"].size == 0
