"""
jj_sigbatch_ragged without a GPU: every case of tests/sig_seg_cases.py is pinned to the oracle -- each segment's slice of the concatenated arrays
through sig_batch_cases.full_evaluation (the definition of jj_sigbatch_begin's bytes); the cofactor-cleared formulation the device uses gives the
same 64 bytes, torsion components included; the term offsets and head slots follow their formulas (a brute-force model of k_sig_seg_terms' lanes);
the bisection of Engine.sigbatch_locate, run over an oracle verdict function, finds exactly the planted signatures in the calls it may take; the
symbol is exported, declared and bound with one signature in the header, jubjub_amd/_lib.py and the Rust shim; its argument checks need no device;
its buffer-discipline row (tests/sig_seg_buffer_row.py) stands in the table of tests/buffer_cases.py and its expected rows are the oracle's.
"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from tests import sig_batch_cases as SC
from tests import sig_seg_buffer_row as BR
from tests import sig_seg_cases as GC

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
SMALL = 600                     # segments up to this size are evaluated term by term; the 4095 / 4096 ones rely on the closed forms plus one evaluation each


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from jubjub_amd import _lib

    ge.build()
    return _lib.load()


def test_case_list_is_what_the_tests_rely_on():
    cases = GC.all_cases()
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    shapes = {tuple(c.sizes()) for c in cases}
    for want in ([5], [63, 1, 64, 65], [255, 257], [256, 256], [600], [1] * 300, [0, 7, 0, 0, 9, 0], [0, 0, 0], [4095, 3], [3, 4096, 2], list(GC.geometric_sizes())):
        assert tuple(want) in shapes, want
    g = GC.geometric_sizes()
    assert len(g) == 64 and 0 in g and max(g) > 16 and 6 <= sum(g) / 64 <= 10
    assert 2 * 4095 + 1 == GC.JOB_TERMS - 1 and 2 * 4096 + 1 == GC.JOB_TERMS + 1
    planted = {v for c in cases for p in c.parts for v in [p.name.split(" n=")[0]]}
    assert planted >= {"valid", "order8r", "c_plus_r", "torsion_r", "bad_s", "bad_r", "s_plus_r", "off_curve_r", "noncanonical_a_zip216", "noncanonical_a"}
    assert set(GC.POSITIONED) == {v for v, k in SC.variants(130) if k is not None}
    assert {c.flags for c in cases} == {0, SC.ZIP216}
    rows = {bytes(r) for c in cases for r in c.expected}
    assert bytes(SC.IDENTITY) in rows and bytes(SC.MALFORMED) in rows and len(rows) > 10
    # a planted segment's neighbours are valid: a verdict that leaks shows as a wrong identity row
    for c in cases:
        if "of the middle segment" in c.name:
            assert bytes(c.expected[0]) == bytes(c.expected[2]) == bytes(SC.IDENTITY) and int(c.offsets[1]) == 7, c.name
    lo = int(GC.layout("p", GC.PLANT).offsets[1])
    assert [lo + k for k in GC.PLANT_POSITIONS] == [7, 63, 64, 136]


def test_every_small_segment_equals_the_whole_sum_of_its_slice():
    seen = set()
    for c in GC.all_cases():
        for g in range(c.S):
            b = c.slice(g)
            key = (bytes(c.base), b.r.tobytes(), b.a.tobytes(), b.s.tobytes(), b.c.tobytes(), b.z.tobytes(), c.flags)
            if b.n > SMALL or key in seen:
                continue
            seen.add(key)
            assert bytes(SC.full_evaluation(b)) == bytes(c.expected[g]), "%s, segment %d" % (c.name, g)
    assert len(seen) > 60


def test_the_long_segments_one_evaluation_each():
    by_name = {c.name: c for c in GC.all_cases()}
    c = by_name["[4095, 3], bad s at the long segment's end"]
    assert bytes(SC.full_evaluation(c.slice(0))) == bytes(c.expected[0]) and bytes(c.expected[0]) not in (bytes(SC.IDENTITY), bytes(SC.MALFORMED))
    c = by_name["valid [3, 4096, 2]"]
    assert bytes(SC.full_evaluation(c.slice(1))) == bytes(SC.IDENTITY) == bytes(c.expected[1])


def test_the_cofactor_cleared_formulation_gives_the_same_bytes():
    """decode, [8] on every point and on B, one sum, no doublings: the terms lie in the prime-order subgroup and an affine point has one encoding"""
    picks = [SC.batch(70, v, k) for v, k in SC.variants(70)] + [SC.batch(1, v, 0) for v in GC.POSITIONED] + [SC.batch(5, "order8r"), SC.batch(0), GC.two_in_one(70, 3, 66)]
    assert {"torsion_r", "order8r"} <= {b.name.split(" n=")[0] for b in picks}
    for b in picks:
        assert bytes(GC.cleared_evaluation(b)) == bytes(SC.full_evaluation(b)) == bytes(b.expected), b.name
    # the torsion component is really there: the planted R is not in the subgroup, and the order8r base is not either
    t = SC.batch(70, "torsion_r", 63)
    from oracle import c_oracle as O

    pts, ok = O.decompress(t.r, 0)
    assert ok.all() and not O.predicate("is_torsion_free", pts[63:64])[0] and not O.predicate("is_torsion_free", SC.bases()["order8r"][None])[0]


def lanes_model(offsets, zs):
    """k_sig_seg_terms lane by lane: the segment of every signature by a linear scan, the heads, and the segmented butterfly over the waves with
    Python integers -> ({head index: the sum it holds}, [segment of i])"""
    o = [int(x) for x in offsets]
    n, S = o[-1], len(o) - 1
    seg = [g for g in range(S) for _ in range(o[g + 1] - o[g])]
    held = {}
    for w0 in range(0, n, 64):
        lanes = list(range(w0, min(w0 + 64, n)))
        key = [seg[i] for i in lanes] + [None] * (64 - len(lanes))
        t = [zs[i] for i in lanes] + [0] * (64 - len(lanes))
        m = 1
        while m <= 32:
            t = [(t[l] + t[l + m]) % GC.R if l + m < 64 and key[l + m] == key[l] and key[l] is not None else t[l] for l in range(64)]
            m <<= 1
        for l, i in enumerate(lanes):
            if l == 0 or o[seg[i]] == i:
                held[i] = t[l]
    return held, seg


def test_term_offsets_and_head_slots_against_a_brute_force_model():
    rng = np.random.default_rng(7)
    layouts = [c.sizes() for c in GC.all_cases() if c.n <= 700] + [[64] * 3, [1, 62, 1, 64, 129, 0, 5], [130], [0, 0, 200, 0]]
    for sizes in layouts:
        offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        n, S = int(offsets[-1]), len(sizes)
        # terms: R terms, A terms, the term of B, segment after segment
        pos, r_at, a_at, b_at = 0, {}, {}, {}
        for g in range(S):
            lo, hi = int(offsets[g]), int(offsets[g + 1])
            for i in range(lo, hi):
                r_at[i] = pos + (i - lo)
                a_at[i] = pos + (hi - lo) + (i - lo)
            b_at[g] = pos + 2 * (hi - lo)
            pos = b_at[g] + 1
        toff = GC.term_offsets(offsets)
        assert toff[-1] == pos == 2 * n + S and toff == sorted(toff) and all(b > a for a, b in zip(toff[:-1], toff[1:]))
        zs = [int(x) for x in rng.integers(1, 1 << 62, n)]
        held, seg = lanes_model(offsets, zs)
        for i in range(n):
            g, lo = seg[i], int(offsets[seg[i]])
            assert r_at[i] == toff[g] + (i - lo) and a_at[i] == toff[g] + int(offsets[g + 1]) - lo + (i - lo)
        assert all(b_at[g] == toff[g + 1] - 1 for g in range(S))
        hs = GC.heads(offsets)
        assert sorted(h for g in hs for h in g) == sorted(held)
        for g in range(S):
            lo, hi = int(offsets[g]), int(offsets[g + 1])
            assert len(hs[g]) == (1 + ((hi - 1) >> 6) - (lo >> 6) if hi > lo else 0)
            assert sum(held[h] for h in hs[g]) % GC.R == sum(zs[lo:hi]) % GC.R, (sizes, g)


def oracle_verdicts(batch, calls):
    base, r, a, s, c, z, _ = batch

    def verdicts_of(index, offsets):
        calls.append(len(offsets) - 1)
        idx = np.arange(len(r)) if index is None else np.asarray(index, np.int64)
        out = []
        for lo, hi in zip(offsets[:-1], offsets[1:]):
            k = idx[lo:hi]
            out.append(GC.verdict(SC.full_evaluation(SC.Batch("slice", base, r[k], a[k], s[k], c[k], z[k], 0, None))))
        return out

    return verdicts_of


def test_locate_model_finds_exactly_the_planted_signatures():
    from jubjub_amd.engine import _locate_cut, _sigbatch_locate

    assert _locate_cut(0, 1000, 16)[:3] == [0, 63, 126] and _locate_cut(5, 8, 16) == [5, 6, 7, 8] and _locate_cut(0, 7, 2) == [0, 4, 7]
    planted = GC.locate_batch()
    assert [k for k, _ in planted[6]] == [0, 63, 64, 511, 999] and [v for _, v in planted[6]].count("malformed") == 1
    for fanout in (2, 16):
        calls = []
        assert _sigbatch_locate(GC.LOCATE_N, fanout, oracle_verdicts(planted, calls)) == planted[6]
        assert calls[0] == fanout and len(calls) <= 1 + math.ceil(math.log(GC.LOCATE_N, fanout))
        calls = []
        assert _sigbatch_locate(GC.LOCATE_N, fanout, oracle_verdicts(GC.locate_batch(valid=True), calls)) == [] and calls == [fanout]
    assert _sigbatch_locate(0, 16, None) == []
    with pytest.raises(ValueError):
        _sigbatch_locate(10, 1, None)


def test_engine_shape_checks_raise_before_any_c_call():
    from jubjub_amd.engine import _sigbatch_ragged_args

    c = GC.layout("checks", [3, 4])
    S, n, o, args = _sigbatch_ragged_args(c.base, c.offsets, *c.arrays())
    assert (S, n, len(args)) == (2, 7, 6) and o.dtype == np.uint64
    assert _sigbatch_ragged_args(c.base, [0, 3, 7], c.r, c.a, c.s, c.c, None)[3][5].n == 7
    for bad in ([0, 3, 6], [1, 3, 7], [0, 8, 7], []):
        with pytest.raises(ValueError):
            _sigbatch_ragged_args(c.base, bad, *c.arrays())
    with pytest.raises(ValueError):
        _sigbatch_ragged_args(c.base[:63], c.offsets, *c.arrays())
    with pytest.raises(ValueError):
        _sigbatch_ragged_args(c.base, c.offsets, c.r, c.a[:6], c.s, c.c, c.z)
    with pytest.raises(ValueError):
        _sigbatch_ragged_args(c.base, c.offsets, c.r, c.a, c.s, c.c, c.z[:, :15])


def test_symbol_is_exported_declared_and_bound(lib):
    assert hasattr(lib, "jj_sigbatch_ragged")
    header = open(os.path.join(ROOT, "include", "jubjub_hip.h")).read()
    m = re.search(r"int jj_sigbatch_ragged\(([^;]*)\);", header)
    assert m and len(m.group(1).split(",")) == 11
    from jubjub_amd import _lib

    assert len(_lib._SIGS["jj_sigbatch_ragged"]) == 10                  # (the context comes first in every binding and is not listed)
    ffi = open(os.path.join(ROOT, "rust-shim", "src", "ffi.rs")).read()
    assert re.search(r"pub fn jj_sigbatch_ragged\(ctx: \*mut JjCtx, base64: \*const c_void, S: usize, offsets: \*const u64,", ffi)
    assert "jj_sigbatch_ragged" in open(os.path.join(ROOT, "rust-shim", "src", "lib.rs")).read()
    assert "jj_sigbatch_ragged" in open(os.path.join(ROOT, "include", "jubjub_hip.hpp")).read()
    assert "jj_sig_seg_kernels.h" in open(os.path.join(ROOT, "jubjub_amd", "build.py")).read()


def test_argument_checks_that_need_no_device(lib):
    """a NULL context is refused whatever S is"""
    from jubjub_amd import _lib

    out = (C.c_uint8 * 64)()
    base = (C.c_uint8 * 64)()
    offs = np.zeros(2, np.uint64)
    assert lib.jj_sigbatch_ragged(None, base, 1, C.c_void_p(offs.ctypes.data), None, None, None, None, None, 0, out) == _lib.JJ_ERR_INVALID
    assert lib.jj_sigbatch_ragged(None, base, 0, None, None, None, None, None, None, 0, None) == _lib.JJ_ERR_INVALID


def test_the_buffer_row_is_in_the_table_and_pinned_to_the_oracle():
    """the row names every pointer parameter of the prototype in order, builds at every size of the table, and at the small sizes every result row is
    the whole sum of its segment"""
    BC = BR.BC
    assert BR.ROW in BC.CASES and [c.id for c in BC.CASES].count(BR.ROW_ID) == 1 and "jj_sigbatch_ragged" not in BC.EXEMPT
    header = open(os.path.join(ROOT, "include", "jubjub_hip.h")).read()
    params = [p.strip() for p in re.search(r"int jj_sigbatch_ragged\(([^;]*)\);", header).group(1).split(",")]
    names = [p.split()[-1].lstrip("*") for p in params]
    assert names == ["jj_ctx*", "base64", "S", "offsets", "r32", "a32", "s32", "c32", "z16", "flags", "out64"]
    assert [a for a in BR.ROW.args if isinstance(a, str)] == ["ctx", "base", "n", "offsets", "r", "a", "s", "c", "z", "out"] and len(BR.ROW.args) == len(params)
    verdicts = set()
    for S in BC.SIZES + (0,):
        ins, outs = BR.ROW.data(S)
        lens = BC.ragged_lengths(S)
        assert ins["offsets"].shape == (S + 1, 8) and ins["z"].shape == (sum(lens), 16) and outs["out"].shape == (S, 64)
        off = np.frombuffer(ins["offsets"].tobytes(), "<u8")
        assert [int(x) for x in np.diff(off.astype(np.int64))] == lens
        verdicts |= {GC.verdict(r) for r in outs["out"]}
        if S <= 65:
            for g in range(S):
                lo, hi = int(off[g]), int(off[g + 1])
                b = SC.Batch("row", ins["base"].reshape(64), ins["r"][lo:hi], ins["a"][lo:hi], ins["s"][lo:hi], ins["c"][lo:hi], ins["z"][lo:hi], 0, None)
                assert bytes(SC.full_evaluation(b)) == bytes(outs["out"][g]), (S, g)
    assert verdicts == {"ok", "reject", "malformed"}
