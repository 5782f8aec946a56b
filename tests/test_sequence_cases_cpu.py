"""
Pins tests/sequence_cases.py without a GPU: the walks hold every ordered pair once, every size lands on the path its kind names (by the
thresholds parsed from jj_msm.hip / jj_engine.h: moving one fails here instead of silently losing a path), the planted decoder rows are what
they claim, and the expected values of every kind agree between two routes through the oracle wherever there are two.
"""
import collections

import numpy as np
import pytest

import sequence_cases as SC
from oracle import c_oracle as O
from oracle import jubjub_ref as J
from util import Q, to_int, to_pt

K = SC.source_constants()


@pytest.fixture(scope="module")
def km():
    return SC.kinds_m(K)


@pytest.fixture(scope="module")
def kw():
    return SC.kinds_w(K)


# ------------------------------------------------------------------------------------------------------------------ walks
@pytest.mark.parametrize("k", [1, 2, 3, 13, 19, 32])
def test_walk_holds_every_ordered_pair_once(k):
    w = SC.euler_walk(k)
    assert len(w) == k * k + 1 and w[0] == w[-1] and set(w) == set(range(k))
    pairs = collections.Counter(zip(w[:-1], w[1:]))
    assert len(pairs) == k * k and set(pairs.values()) == {1}
    assert set(pairs) == {(a, b) for a in range(k) for b in range(k)}
    assert SC.euler_walk(k) == w                                        # fixed: a failure names a position that means the same next time
    if k > 3:
        assert SC.euler_walk(k, seed=SC.WALK_SEED + 1) != w


def test_groups_and_cycle(km, kw):
    assert len(km) == 13 and len(kw) == 19
    assert [k.name.split(":")[0] for k in km] == ["M%d" % i for i in range(1, 14)]
    assert [k.name.split(":")[0] for k in kw] == ["W%d" % i for i in range(1, 20)]
    assert sorted(SC.one_cycle(32)) == list(range(32)) and SC.one_cycle(32) == SC.one_cycle(32)
    # the unit count (the SoA stride) changes at every step of the walk of group W but the 19 loops and the three pairs of kinds of one size
    n = [40001, 5, 3000, 1000, 700, 4097, 300, 513, 100, 1000, 3, 2049, 7, 777, 4097, 5000, 600, 300, 65]
    assert [len(k.args["p"]) if k.name[:3] == "W16" else k.want()[0].shape[0] for k in kw] == n
    w = SC.euler_walk(19)
    assert sum(1 for a, b in zip(w[:-1], w[1:]) if n[a] != n[b]) == 19 * 19 - 19 - 6


# ------------------------------------------------------------------------------------------------------------------ paths
def test_constants_are_the_documented_ones():
    """the values the issue's sizes were written against; a moved threshold shows here first"""
    assert K["MSM_LARGE_MIN"] == 9 << 14 and K["msm_small_max"] == 1 << 14 and K["MSM_BATCH_MAX"] == 1 << 13
    assert K["vb_quad_max"] == 32768 and K["WIDE_LOG2"] == 18 and (K["W_WIDE"], K["W_LARGE"], K["W_MID"]) == (16, 17, 23)
    assert K["msm_segments"] == -1 and K["msm_lanes"] == 3 and K["HOST_OUT_SLOTS"] == 8


def test_msm_sizes_reach_their_paths(km):
    by = {k.name.split(":")[0]: k for k in km}
    for name, n in (("M1", 700), ("M2", 20000), ("M3", K["MSM_LARGE_MIN"] + 5), ("M4", (1 << 18) + 3), ("M11", 20000), ("M12", 20000), ("M13", 20000)):
        k = by[name]
        assert len(k.args["s"]) == n == len(k.args["p"]), name
        assert SC.msm_path(n, K) == k.path, (name, SC.msm_path(n, K))
    assert by["M1"].path == "small" and by["M2"].path == (23, "one-pass", "chunks")
    assert by["M3"].path == (17, "two-pass", "segments") and by["M4"].path == (16, "two-pass", "segments")
    # the three paths' neighbours lie on other paths: the sizes are not on a plateau by accident
    assert SC.msm_path(K["msm_small_max"], K) == "small" != SC.msm_path(K["msm_small_max"] + 1, K)
    assert SC.msm_path(K["MSM_LARGE_MIN"] - 1, K) == (23, "one-pass", "chunks") and SC.msm_path((1 << 18) - 1, K) == (17, "two-pass", "segments")


def test_batch_ragged_and_basis_sizes_reach_their_paths(km):
    by = {k.name.split(":")[0]: k for k in km}
    bmax = K["MSM_BATCH_MAX"]
    B, n, _ = by["M5"].args["s"].shape
    assert (B, n) == (2, 4000) and by["M5"].args["p"].shape == (n, 64) and n <= bmax and SC.batch_slices(B, n, K) > 1       # slices, arrival counters
    B, n, _ = by["M6"].args["s"].shape
    assert (B, n) == (50, 20) and by["M6"].args["p"].shape == (B, n, 64) and SC.batch_slices(B, n, K) == 1                  # one slice per row
    B, n, _ = by["M7"].args["s"].shape
    assert (B, n) == (3, bmax + 1) and n > bmax                                                                             # the jobs route
    off = by["M8"].args["offsets"]
    lengths = np.diff(off.astype(np.int64)).tolist()
    assert lengths == [0, 1, 17, 5000, bmax + 7, 0, 300] and off.dtype == np.uint64 and int(off[-1]) == len(by["M8"].args["s"])
    assert sum(1 for x in lengths if x > bmax) == 1 and sum(1 for x in lengths if x == 0) == 2
    assert SC.msm_path(bmax + 7, K) == "small"                                                                              # the long segment's job
    _, m, nb = by["M9"].path
    assert by["M9"].args["s"].shape == (3, m, 32) and len(by["M9"].args["basis"]) == nb and m < nb <= bmax                  # rows over the resident tables
    _, m, nb = by["M10"].path
    assert by["M10"].args["s"].shape == (m, 32) and len(by["M10"].args["basis"]) == nb and bmax < m < nb                    # one row over the window table


def test_varbase_sizes_reach_their_paths(kw):
    by = {k.name.split(":")[0]: k for k in kw}
    assert len(by["W1"].args["s"]) == K["vb_quad_max"] + 7233 == 40001 and by["W1"].path == "ladder"
    assert len(by["W2"].args["s"]) == 5 <= K["vb_quad_max"] and by["W2"].path == "quad"
    sizes = {"W3": 3000, "W4": 1000, "W5": 700, "W10": 1000, "W11": 3, "W14": 777, "W16": 5000, "W17": 600, "W19": 65}
    for name, n in sizes.items():
        assert len(by[name].args["p"]) == n, name
    assert len(by["W6"].args["s"]) == 4097 and len(by["W7"].args["s"]) == 300 and by["W8"].args["s"].shape == (2, 513, 32)
    assert by["W9"].args["s"].shape == (3, 100, 32) and len(by["W12"].args["enc"]) == 2049 and len(by["W13"].args["enc"]) == 7
    assert len(by["W15"].args["ext"]) == 4097 and len(by["W18"].args["a"]) == 300


# ------------------------------------------------------------------------------------------------------------------ planted rows
def test_pool_and_torsion():
    p = SC.pool()
    assert p.shape == (1 << 14, 64) and len({bytes(r) for r in p}) == len(p)
    assert O.predicate("is_on_curve", p).all()
    tf = O.predicate("is_torsion_free", p)
    assert tf[0::2].all() and not tf[1::2].all()                       # even rows: prime order; odd rows: anywhere in the group
    t = SC.torsion()
    assert (t[0] == SC.IDENTITY).all() and len({bytes(r) for r in t}) == 8
    assert O.predicate("is_small_order", t).all() and O.predicate("is_on_curve", t).all()
    assert [J.ext_is_small_order(J.affine_to_extended(to_pt(r))) for r in t] == [True] * 8


def test_planted_decoder_rows_are_what_they_claim():
    enc, where = SC.decoder_rows(2049, 212)
    assert all(len(where[k]) >= 30 for k in SC.DEC_PLANTS)
    planted = sorted(i for v in where.values() for i in v)
    assert planted == list(range(0, 2049, 9))
    o0, k0 = O.decompress(enc, 0)
    o1, k1 = O.decompress(enc, 1)
    o15, k15 = O.decompress(enc, 15)
    plain = np.setdiff1d(np.arange(2049), planted)
    assert k0[plain].all() and k1[plain].all() and (o1[plain] == SC.points_for(2049, offset=212)[plain]).all()
    for i in where["v>=q"]:
        assert to_int(enc[i]) & ((1 << 255) - 1) >= Q and not k0[i] and not k1[i]          # non-canonical: refused whatever the flags
    for i in where["nonsquare"]:
        assert not k0[i] and not k1[i] and not J.affine_from_bytes(bytes(enc[i]), zip216=False)[1]
    for name, v in (("u=0,sign,v=1", 1), ("u=0,sign,v=q-1", Q - 1)):
        for i in where[name]:
            assert k0[i] and not k1[i] and to_pt(o0[i]) == (0, v)                           # ZIP-216 alone refuses them
    for i in where["small-order"]:
        assert k1[i] and O.predicate("is_small_order", o1[i][None])[0] and not k15[i]
    for i in where["coset"]:
        assert k1[i] and not O.predicate("is_torsion_free", o1[i][None])[0] and not O.predicate("is_small_order", o1[i][None])[0] and not k15[i]
    junk_ok = [bool(k0[i]) for i in where["junk"]]
    assert True in junk_ok and False in junk_ok                                              # raw bytes: some decode, some do not
    # flags 15 on the plain rows: odd pool rows lie outside the subgroup -> refused; the accepted ones come back times the cofactor
    acc = plain[k15[plain] == 1]
    assert 0 < len(acc) < len(plain)
    assert (o15[acc] == O.point_op("mul_by_cofactor", o1[acc])).all()
    enc7, where7 = SC.decoder_rows(7, 213)
    assert where7["v>=q"] == [0] and O.decompress(enc7, 0)[1].tolist() == [0, 1, 1, 1, 1, 1, 1]


def test_planted_rows_of_the_other_kinds(kw):
    by = {k.name.split(":")[0]: k for k in kw}
    ext = by["W15"].args["ext"]
    z = [to_int(r[64:96]) for r in ext]
    assert z[2048] == 0 and sum(1 for x in z if x == 0) == 1 and all(x != 1 for x in z)
    assert (by["W15"].want()[0][2048] == 0).all()
    tf = by["W17"].want()[0]
    assert tf.tolist() == [1 if i * 5 % 8 == 0 else 0 for i in range(600)]                  # all eight cosets, the subgroup among them
    root, ok = by["W18"].want()
    assert ok[:101].all() and 0 < int(ok[101:].sum()) < 199


# ------------------------------------------------------------------------------------------------------------------ two routes
def _rows(n, count=6):
    return sorted({0, n - 1} | {int(i) for i in np.linspace(0, n - 1, count)})


def test_msm_expected_values_two_routes(km):
    by = {k.name.split(":")[0]: k for k in km}
    for name in ("M1", "M2", "M11", "M12", "M13"):
        a, want = by[name].args, by[name].want()[0]
        assert (O.msm(a["s"], a["p"]) == want).all() and (O.msm_pippenger(a["s"], a["p"], 11) == want).all(), name
    for name in ("M3", "M4"):
        # the sum of a head by the Straus oracle and of the tail by buckets of another width
        a, want = by[name].args, by[name].want()[0]
        cut = 3001
        parts = np.stack([O.msm(a["s"][:cut], a["p"][:cut]), O.msm_pippenger(a["s"][cut:], a["p"][cut:], 11)])
        assert (O.point_sum(parts) == want).all(), name
    for name in ("M5", "M6", "M7"):
        a, want = by[name].args, by[name].want()[0]
        assert want.shape == (a["s"].shape[0], 64)
        for b in range(a["s"].shape[0]):
            assert (O.msm_pippenger(a["s"][b], a["p"] if a["p"].ndim == 2 else a["p"][b], 9) == want[b]).all(), (name, b)
    a, want = by["M8"].args, by["M8"].want()[0]
    o = a["offsets"].astype(np.int64)
    for k in range(len(o) - 1):
        assert (O.msm_pippenger(a["s"][o[k]:o[k + 1]], a["p"][o[k]:o[k + 1]], 9) == want[k]).all(), k
    assert (want[0] == SC.IDENTITY).all() and (want[5] == SC.IDENTITY).all()
    assert (want[1] == O.varbase_mul(a["s"][:1], a["p"][:1])[0]).all()
    a, want = by["M9"].args, by["M9"].want()[0]
    for b in range(3):
        assert (O.msm_pippenger(a["s"][b], a["basis"][:a["s"].shape[1]], 9) == want[b]).all()
    a, want = by["M10"].args, by["M10"].want()[0]
    assert (O.msm(a["s"], a["basis"][:len(a["s"])]) == want).all()


def test_workset_expected_values_two_routes(kw):
    by = {k.name.split(":")[0]: k for k in kw}

    def bigint_mul(s, p):
        return J.ext_to_affine(J.ext_multiply(J.affine_to_extended(to_pt(p)), bytes(s)))

    for name in ("W1", "W2", "W3"):
        a, want = by[name].args, by[name].want()[0]
        for i in _rows(len(want), 4):
            assert to_pt(want[i]) == bigint_mul(a["s"][i], a["p"][i]), (name, i)
    a, want = by["W4"].args, by["W4"].want()[0]
    for i in _rows(1000, 3):
        assert to_pt(want[i]) == J.affine_add_fast(bigint_mul(a["a"][i], a["p"][i]), bigint_mul(a["b"][i], a["q"][i])), i
    a, want = by["W5"].args, by["W5"].want()[0]
    for i in _rows(700, 3):
        assert to_pt(want[i]) == bigint_mul(a["k"], a["p"][i]), i
    g = np.repeat(np.frombuffer(J.GENERATOR[0].to_bytes(32, "little") + J.GENERATOR[1].to_bytes(32, "little"), np.uint8)[None], 4097, axis=0)
    assert (O.varbase_mul(by["W6"].args["s"], g) == by["W6"].want()[0]).all()
    b2 = np.repeat(np.array(SC.pool()[5])[None], 513, axis=0)
    assert (O.varbase_mul(by["W7"].args["s"], b2[:300]) == by["W7"].want()[0]).all()
    s8 = by["W8"].args["s"]
    assert (O.point_op("add", O.varbase_mul(s8[0], g[:513]), O.varbase_mul(s8[1], b2)) == by["W8"].want()[0]).all()
    s9, want = by["W9"].args["s"], by["W9"].want()[0]
    for i in _rows(100, 3):
        terms = np.stack([s9[b, i] for b in range(3)])
        terms[:, 8:] = 0                                                                   # 64 bits of each scalar
        assert (O.msm(terms, np.array(SC.pool()[10:13])) == want[i]).all(), i
    a, want = by["W10"].args, by["W10"].want()[0]
    for i in _rows(1000):
        assert to_pt(want[i]) == J.affine_add_fast(to_pt(a["p"][i]), to_pt(a["q"][i])), i
    a, want = by["W11"].args, by["W11"].want()[0]
    assert (O.varbase_mul(np.repeat(np.frombuffer((8).to_bytes(32, "little"), np.uint8)[None], 3, axis=0), a["p"]) == want).all()
    for name, flags in (("W12", 15), ("W13", 0)):
        enc, (out, ok) = by[name].args["enc"], by[name].want()
        for i in sorted(set(range(0, len(enc), 9)) | set(_rows(len(enc), 12))):
            p, good = J.affine_from_bytes(bytes(enc[i]), zip216=bool(flags & 1))
            p = p if good else None
            if p is not None and flags & 2 and not J.ext_is_torsion_free(J.affine_to_extended(p)):
                p = None
            if p is not None and flags & 4 and J.ext_is_small_order(J.affine_to_extended(p)):
                p = None
            assert bool(ok[i]) == (p is not None), (name, i)
            if p is not None:
                if flags & 8:
                    p = J.ext_to_affine(J.ext_mul_by_cofactor(J.affine_to_extended(p)))
                assert to_pt(out[i]) == p, (name, i)
    a, want = by["W14"].args, by["W14"].want()[0]
    for i in _rows(777):
        assert bytes(want[i]) == J.affine_to_bytes(to_pt(a["p"][i])), i
    assert (O.decompress(want, 1)[0] == a["p"]).all()
    ext, want = by["W15"].args["ext"], by["W15"].want()[0]
    sub = _rows(4097, 8) + [2048]
    _, aff = J.batch_normalize([tuple(to_int(ext[i][32 * k:32 * k + 32]) for k in range(5)) for i in sub])
    assert [to_pt(want[i]) for i in sub] == list(aff)
    a, want = by["W16"].args, by["W16"].want()[0]
    assert (O.msm_pippenger(np.repeat(np.frombuffer((1).to_bytes(32, "little"), np.uint8)[None], 5000, axis=0), a["p"], 9) == want).all()
    a, want = by["W17"].args, by["W17"].want()[0]
    for i in range(0, 600, 37):
        assert bool(want[i]) == J.ext_is_torsion_free(J.affine_to_extended(to_pt(a["p"][i]))), i
    a, (root, ok) = by["W18"].args["a"], by["W18"].want()
    sq = O.field_op(O.FQ, "square", root)[0]
    canon = O.field_op(O.FQ, "add", a, np.zeros_like(a))[0]                                 # a mod q
    assert (sq[ok == 1] == canon[ok == 1]).all()
    for i in np.flatnonzero(ok == 0)[:20]:
        assert pow(to_int(canon[i]), (Q - 1) // 2, Q) == Q - 1, i                           # refused: a non-residue
    a, want = by["W19"].args, by["W19"].want()[0]
    for i in _rows(65):
        nl = J.affine_to_niels(to_pt(a["p"][i]))
        assert tuple(to_int(want[i][32 * k:32 * k + 32]) for k in range(3)) == tuple(x % Q for x in nl), i


def test_empty_record_combines_to_the_identity():
    import ctypes as C

    from jubjub_amd import _lib

    lib = _lib.load()
    for n in (0, 1, 12):
        rec = SC.empty_record(n)
        out = np.zeros(64, np.uint8)
        assert lib.jj_msm_combine(C.c_size_t(1), rec.ctypes.data, out.ctypes.data) == 0
        assert (out == SC.IDENTITY).all() and (out == O.msm(np.zeros((0, 32), np.uint8), np.zeros((0, 64), np.uint8))).all()
