"""CPU checks of jj_msm_ragged and its planner (jj_plan_msm_ragged, jj_plan_msm_ragged_items): exported and declared, arguments refused before
any device is touched, the planner's properties over a matrix of length lists and parameters, Engine.msm_ragged's shape checks, and a C++
caller of jubjub_hip.hpp's msm_ragged compiles and links."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

MAX = 8192                 # MSM_BATCH_MAX: longer segments take the jobs route
NAMES = ("jj_msm_ragged", "jj_plan_msm_ragged", "jj_plan_msm_ragged_items")


def lib():
    from jubjub_amd import _lib

    return _lib.load(), _lib


def offsets_of(lens):
    return np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.uint64))]).astype(np.uint64)


def test_symbols_exported_and_declared():
    import __graft_entry__ as ge

    ge.build()
    so = ctypes.CDLL(os.path.join(ROOT, "jubjub_amd", "lib", "libjubjub_hip.so"))
    header = open(os.path.join(ROOT, "include", "jubjub_hip.h")).read()
    for name in NAMES:
        assert hasattr(so, name), name
        assert name + "(" in header, name


def test_refuses_bad_arguments_without_a_device():
    L, _lib = lib()
    INVALID = _lib.JJ_ERR_INVALID
    out = (ctypes.c_uint8 * 256)()
    buf = (ctypes.c_uint8 * 256)()
    good = offsets_of([1, 2])
    # no context, whatever else: also with S = 0, like jj_msm_batch(NULL, 0, ...)
    assert L.jj_msm_ragged(None, 2, good.ctypes.data, buf, buf, out) == INVALID
    assert L.jj_msm_ragged(None, 0, None, None, None, None) == INVALID
    assert L.jj_msm_ragged(None, 2, None, buf, buf, out) == INVALID
    assert L.jj_msm_ragged(None, 2, np.array([1, 2, 3], np.uint64).ctypes.data, buf, buf, out) == INVALID
    assert L.jj_msm_ragged(None, 2, np.array([0, 2, 1], np.uint64).ctypes.data, buf, buf, out) == INVALID
    assert L.jj_msm_ragged(None, 1 << 60, good.ctypes.data, buf, buf, out) == INVALID
    # the planner is the code that refuses offsets for the call: the same cases, here decided by the offsets themselves
    out4 = (ctypes.c_int64 * 4)()
    count = ctypes.c_size_t(77)
    for fn in (lambda S, o: L.jj_plan_msm_ragged(S, o, 0, 0, 0, out4), lambda S, o: L.jj_plan_msm_ragged_items(S, o, 0, 0, 0, None, 0, ctypes.byref(count))):
        assert fn(2, good.ctypes.data) == 0
        assert fn(0, None) == 0
        assert fn(2, None) == INVALID                                                   # NULL offsets with S > 0
        assert fn(2, np.array([1, 2, 3], np.uint64).ctypes.data) == INVALID              # offsets[0] != 0
        assert fn(2, np.array([0, 2, 1], np.uint64).ctypes.data) == INVALID              # a decreasing pair
        assert fn(2, np.array([0, 1, 1 << 62], np.uint64).ctypes.data) == INVALID        # N * 64 beyond size_t
        assert fn(1 << 60, good.ctypes.data) == INVALID                                  # S * 64 beyond size_t (refused before offsets is read)
    assert L.jj_plan_msm_ragged(2, good.ctypes.data, 0, 0, 0, None) == INVALID
    assert L.jj_plan_msm_ragged(2, good.ctypes.data, -1, 0, 0, out4) == INVALID
    assert L.jj_plan_msm_ragged(2, good.ctypes.data, 0, -1, 0, out4) == INVALID
    assert L.jj_plan_msm_ragged_items(2, good.ctypes.data, 0, 0, 0, None, 0, None) == INVALID
    assert L.jj_plan_msm_ragged_items(2, good.ctypes.data, 0, 0, 0, None, 5, ctypes.byref(count)) == INVALID      # room claimed, no array


def _length_lists():
    rng = np.random.default_rng(20240)
    big = [int(x) for x in rng.integers(0, 300, size=99)]
    big.append(20000 - sum(big))
    assert 0 < big[-1] <= MAX and sum(big) == 20000
    return [
        ([0], 0), ([1], 0), ([0, 0, 0], 0), ([0, 1, 0, 17, 16, 15, 33, 0], 0), ([8192, 8193, 1], 0),
        ([int(x) for x in np.random.default_rng(7).integers(0, 201, size=300)], 0),
        (big, 4096),
        ([0, 1, 0, 17, 16, 15, 33, 0], 20),        # rounds of a few segments, one segment (33) above round_terms
    ]


def plan(lens, slice_min, waves, round_terms):
    L, _lib = lib()
    off = offsets_of(lens)
    S = len(lens)
    out4 = (ctypes.c_int64 * 4)()
    assert L.jj_plan_msm_ragged(S, off.ctypes.data, slice_min, waves, round_terms, out4) == 0
    count = ctypes.c_size_t(1 << 40)
    assert L.jj_plan_msm_ragged_items(S, off.ctypes.data, slice_min, waves, round_terms, None, 0, ctypes.byref(count)) == 0      # the count only
    assert count.value == out4[2]
    items = np.full((count.value + 1, 4), 0xEE, dtype=np.uint64)
    n = ctypes.c_size_t(1 << 40)
    assert L.jj_plan_msm_ragged_items(S, off.ctypes.data, slice_min, waves, round_terms, items.ctypes.data, count.value, ctypes.byref(n)) == 0
    assert n.value == count.value and (items[count.value] == 0xEE).all()                     # nothing written past cap
    if count.value:
        small = np.zeros((count.value, 4), dtype=np.uint64)
        m = ctypes.c_size_t(1 << 40)
        assert L.jj_plan_msm_ragged_items(S, off.ctypes.data, slice_min, waves, round_terms, small.ctypes.data, count.value - 1, ctypes.byref(m)) == _lib.JJ_ERR_INVALID
        assert m.value == count.value                                                         # count is set all the same
    return off, list(out4), items[:count.value]


@pytest.mark.parametrize("waves", [1, 64, 2048])
@pytest.mark.parametrize("slice_min", [1, 16, 64])
def test_planner_properties(slice_min, waves):
    for lens, round_terms in _length_lists():
        off, out4, items = plan(lens, slice_min, waves, round_terms)
        rt = round_terms or (1 << 18)
        n_short = sum(x for x in lens if x <= MAX)
        t = max(slice_min, -(-n_short // waves), 1)
        by_seg = {}
        for r, s, first, end in items.tolist():
            by_seg.setdefault(s, []).append((r, first, end))
        # order: items come segment by segment, in input order, rounds never decrease
        assert [int(x) for x in items[:, 1]] == sorted(int(x) for x in items[:, 1])
        assert [int(x) for x in items[:, 0]] == sorted(int(x) for x in items[:, 0])
        n_short_segs = n_long = 0
        round_segs = {}
        for s, ln in enumerate(lens):
            if ln == 0 or ln > MAX:
                assert s not in by_seg, (lens, s)                         # empty and long segments have no item
                n_long += ln > MAX
                continue
            n_short_segs += 1
            sl = by_seg[s]
            assert len(sl) == -(-ln // t), (lens, s, t)
            assert sl[0][1] == off[s] and sl[-1][2] == off[s + 1]
            for k, (r, first, end) in enumerate(sl):                      # the slices tile the segment exactly, in order, 1 .. t terms each
                assert 1 <= end - first <= t
                assert r == sl[0][0]                                      # a segment is whole in one round
                if k:
                    assert first == sl[k - 1][2]
            sizes = [e - f for _, f, e in sl]
            assert max(sizes) - min(sizes) <= 1                           # near-equal
            round_segs.setdefault(sl[0][0], []).append(s)
        rounds = sorted(round_segs)
        assert rounds == list(range(len(rounds)))                         # consecutive, from 0
        for r in rounds:
            segs = round_segs[r]
            terms = sum(lens[s] for s in segs)
            assert terms <= rt or len(segs) == 1, (lens, r)
            # consecutive in input order: nothing but empty segments between the round's first and last segment
            assert all(lens[s] == 0 or s in segs for s in range(segs[0], segs[-1] + 1)), (lens, r)
            if r:
                # a round is not closed early: the next segment did not fit, or a long segment lies between
                prev = round_segs[r - 1]
                between_long = any(lens[s] > MAX for s in range(prev[-1], segs[0]))
                assert between_long or sum(lens[s] for s in prev) + lens[segs[0]] > rt, (lens, r)
        assert out4 == [n_short_segs, n_long, len(items), len(rounds)], (lens, out4)


def test_planner_defaults_are_the_batched_constants():
    """0 for slice_min / waves / round_terms means 16 / 2048 / 2^18"""
    for lens in ([100] * 50, [5000, 3, 8000, 77] * 40):
        a = plan(lens, 0, 0, 0)
        b = plan(lens, 16, 2048, 1 << 18)
        assert a[1] == b[1] and (a[2] == b[2]).all()


def test_engine_shape_checks():
    import threading

    from jubjub_amd import Engine
    from jubjub_amd.engine import _msm_ragged_shapes as shapes

    s, p = np.zeros((6, 32), np.uint8), np.zeros((6, 64), np.uint8)
    assert shapes(s, p, [0, 6]) == (1, 6)
    assert shapes(s, p, [0, 0, 2, 2, 6, 6]) == (5, 6)
    assert shapes(s, p, np.array([0, 1, 6], np.int32)) == (2, 6)
    assert shapes(s, p, (0, 3, 6)) == (2, 6)
    assert shapes(s[:0], p[:0], [0]) == (0, 0)
    assert shapes(s[:0], p[:0], [0, 0, 0]) == (2, 0)
    bad = [(s, p, []), (s, p, [1, 6]), (s, p, [0, 4, 3, 6]), (s, p, [0, 5]), (s, p, [0, 7]), (s, p, [0.0, 6.0]), (s, p, [[0, 6]]), (s, p, [0, -1, 6]),
           (s.reshape(2, 3, 32), p, [0, 6]), (s[:, :31], p, [0, 6]), (s, p[:5], [0, 6]), (s, p[:, :32], [0, 6]), (s, s, [0, 6])]
    for a, b, o in bad:
        with pytest.raises(ValueError):
            shapes(a, b, o)
    # the public method checks shapes and offsets before it touches a context
    e = object.__new__(Engine)
    e._mu = threading.RLock()
    for a, b, o in bad:
        with pytest.raises(ValueError):
            e.msm_ragged(a, b, o)
    # the planner front-end needs no context at all
    got = e.plan_msm_ragged([0, 1, 18, 18, 9000], items=True)
    assert (got["short"], got["long"], got["items"], got["rounds"]) == (2, 1, 3, 1)
    assert got["list"].tolist() == [[0, 0, 0, 1], [0, 1, 1, 10], [0, 1, 10, 18]]
    with pytest.raises(ValueError):
        e.plan_msm_ragged([1, 2])


def test_cpp_caller_compiles(tmp_path):
    src = tmp_path / "msm_ragged.cpp"
    src.write_text(r'''
#include "jubjub_hip.hpp"
int main() {
  try {
    jubjub::Context c(0);
    jubjub::AffineBatch pts = jubjub::AffineBatch::identity(c, 4);
    std::vector<jubjub::FrBatch> rows;
    jubjub::AffineBatch four = jubjub::msm_batch(c, pts, rows);
    jubjub::FrBatch scalars = jubjub::FrBatch::random(c, 4, 1);
    std::vector<uint64_t> offsets = {0, 1, 1, 4};
    jubjub::AffineBatch three = jubjub::msm_ragged(c, pts, scalars, offsets);
    return (int)(four.len() + three.len());
  } catch (const jubjub::Error& e) {
    return 1;
  }
}
''')
    lib_dir = os.path.join(ROOT, "jubjub_amd", "lib")
    out = tmp_path / "msm_ragged"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-L", lib_dir, "-ljubjub_hip",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", str(out)])
    assert out.exists()
