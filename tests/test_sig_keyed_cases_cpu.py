"""
jj_sigbatch_keyed_begin without a GPU: every case of tests/sig_keyed_cases.py is pinned to the oracle -- expanded (a32[k] repeated over its group)
through sig_batch_cases.full_evaluation, and as the n + K + 1 term sum itself (keyed_evaluation), which is what pins the cases with keys that
have no signatures; the layouts have the boundaries they claim; Engine.group_by_key is a stable grouping; the symbol is exported, declared and
bound with one signature in the header, jubjub_amd/_lib.py and the Rust shim; its argument checks come before any device work.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import sig_batch_cases as SC
from tests import sig_keyed_cases as KC

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
SMALL = 305                     # (300 and the five signatures of sizes [0, 5, 0, 0, 300, 0]) cases up to this size are evaluated term by term; above it the closed forms stand (-[8 z delta] B, the identity)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from jubjub_amd import _lib

    ge.build()
    return _lib.load()


def small_cases():
    return [c for c in KC.all_cases() if c.n <= SMALL]


def test_case_list_is_what_the_tests_rely_on():
    cases = KC.all_cases()
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    assert max(c.n for c in cases) == KC.LARGE and sum(1 for c in cases if c.n > SMALL) == 2
    variants = {v for n in KC.SIZES for v, _ in SC.variants(n)}
    assert variants == {"valid", "order8r", "c_plus_r", "torsion_r", "bad_s", "bad_r", "s_plus_r", "off_curve_r", "noncanonical_a_zip216", "noncanonical_a"}
    assert len(KC.regrouped_cases()) == sum(len(SC.variants(n)) for n in KC.SIZES)
    verdicts = {bytes(c.expected) for c in cases}
    assert bytes(SC.IDENTITY) in verdicts and bytes(SC.MALFORMED) in verdicts and len(verdicts) > 10
    assert any(c.has_empty_group() for c in cases) and any(c.K == 0 for c in cases) and any(c.K == c.n > 64 for c in cases)


def test_every_small_case_expanded_equals_the_whole_sum():
    """a32[k] repeated over its group, through the evaluation tests/test_sig_batch_cpu.py uses for jj_sigbatch_begin.  A key without signatures
    drops out of the expansion: a valid one keeps the verdict, an undecodable one does not (keyed_evaluation below pins those)."""
    for c in small_cases():
        undecodable_empty = c.has_empty_group() and bytes(c.expected) == bytes(SC.MALFORMED)
        got = SC.full_evaluation(c.expanded())
        if undecodable_empty:
            assert bytes(got) == bytes(SC.IDENTITY), c.name
        else:
            assert bytes(got) == bytes(c.expected), c.name


def test_every_small_case_equals_the_n_plus_k_plus_1_term_sum():
    for c in small_cases():
        assert bytes(KC.keyed_evaluation(c)) == bytes(c.expected), c.name


def test_empty_groups_are_pinned_by_the_direct_sum():
    empty = [c for c in KC.all_cases() if c.has_empty_group()]
    assert len(empty) >= 8
    by_name = {c.name: c for c in empty}
    for name in ("empty group first", "empty group last", "empty group between"):
        assert bytes(KC.keyed_evaluation(by_name[name])) == bytes(SC.IDENTITY)
    bad = by_name["empty group between, bad s after it"]
    assert bytes(KC.keyed_evaluation(bad)) == bytes(bad.expected) and bytes(bad.expected) not in (bytes(SC.IDENTITY), bytes(SC.MALFORMED))
    for name in ("off-curve key without signatures", "off-curve key without signatures, last"):
        c = by_name[name]
        k = [i for i, row in enumerate(c.keys) if bytes(row) == bytes(SC.off_curve_encoding())]
        assert len(k) == 1 and c.sizes()[k[0]] == 0
        assert bytes(KC.keyed_evaluation(c)) == bytes(SC.MALFORMED) == bytes(c.expected)
    nothing = by_name["three keys (one off-curve), no signatures: nothing is read"]
    assert nothing.n == 0 and bytes(nothing.expected) == bytes(SC.IDENTITY)


def test_regrouped_cases_are_stable_groupings_of_their_batches():
    for n in KC.SIZES:
        for v, k in SC.variants(n):
            b, c = SC.batch(n, v, k), KC.regrouped(n, v, k)
            keys, offsets, order = KC.group(b.a)
            assert len({bytes(r) for r in c.keys}) == c.K == len({bytes(r) for r in b.a}) and not c.has_empty_group()
            assert (c.expanded().a == b.a[order]).all() and (c.r == b.r[order]).all() and (c.z == b.z[order]).all()
            for lo, hi in zip(offsets[:-1], offsets[1:]):
                assert (np.diff(order[int(lo):int(hi)]) > 0).all()                   # stable: a group keeps the batch's order
            if v.startswith("noncanonical_a"):
                g = [i for i, row in enumerate(c.keys) if bytes(row) == bytes(SC.NONCANONICAL_IDENTITY)]
                assert len(g) == 1 and c.sizes()[g[0]] == 1                          # a group of one


def test_layouts_have_the_boundaries_they_claim():
    by_name = {c.name: c for c in KC.all_cases()}
    tri = by_name["sizes 1, 2, 3, ..., 23"]
    assert tri.n == 276 >= 257 and tri.K == 23
    starts = {int(o) % 64 for o in tri.offsets[:-1]}
    assert len(starts) == 23 and {0, 1, 3, 6, 10, 15, 21, 28, 36, 45, 55, 2, 14, 27, 41, 56, 8, 25, 43, 62, 18, 39, 61} == starts
    threes = by_name["90 groups of three"]
    assert threes.n == 270 >= 257 and {int(o) % 64 for o in threes.offsets[:-1]} == set(range(64))      # a group starts at EVERY residue mod 64
    assert any(int(lo) < 64 * w < int(hi) for w in (1, 2, 3, 4) for lo, hi in zip(threes.offsets[:-1], threes.offsets[1:]))
    assert any(int(lo) < 256 < int(hi) for lo, hi in zip(tri.offsets[:-1], tri.offsets[1:]))              # a group straddles the workgroup edge
    assert [len(h) for h in KC.heads(by_name["sizes [63, 1]"].offsets)] == [1, 1]
    assert KC.heads(by_name["sizes [64, 64]"].offsets) == [[0], [64]]
    assert KC.heads(by_name["sizes [65]"].offsets) == [[0, 64]]
    assert KC.heads(by_name["sizes [0, 5, 0, 0, 300, 0]"].offsets) == [[], [0], [], [], [5, 64, 128, 192, 256], []]
    assert KC.heads([0, 63, 65]) == [[0], [63, 64]] and KC.heads([0, 64]) == [[0]] and KC.heads([0, 0]) == [[]]
    big = by_name["one group of %d, bad s in its last wave" % KC.LARGE]
    h = KC.heads(big.offsets)[0]
    assert len(h) == 66 > 64 and h[-1] == 4160                                       # more heads than lanes: the close kernel's lane loop wraps
    valid_big = by_name["one group of %d" % KC.LARGE]
    changed = [i for i in range(big.n) if bytes(big.s[i]) != bytes(valid_big.s[i])]
    assert changed == [KC.LARGE - 10] and changed[0] >= h[-1]                        # the tampered signature lies in the last wave
    one = by_name["every group of one"]
    assert one.K == one.n == 130 and len({bytes(k) for k in one.keys}) == SC.NKEYS   # keys repeat: each listing is a group of its own
    twice = by_name["one key listed twice, its signatures split"]
    assert bytes(twice.keys[0]) == bytes(twice.keys[2]) != bytes(twice.keys[1])


def test_heads_are_exactly_the_run_starts_of_a_wave_wise_segmented_sum():
    """heads(): lane i starts a run exactly when i == offsets[k] or i % 64 == 0 -- compared with a direct simulation"""
    for c in KC.all_cases():
        if c.n == 0 or c.n > 1000:
            continue
        key_of = np.repeat(np.arange(c.K), c.sizes())
        runs = [i for i in range(c.n) if i % 64 == 0 or key_of[i] != key_of[i - 1]]
        assert sorted(h for hs in KC.heads(c.offsets) for h in hs) == runs, c.name


def test_group_by_key_is_a_stable_grouping_and_round_trips():
    from jubjub_amd.engine import Engine

    rng = np.random.default_rng(0x6B01)
    pool = rng.integers(0, 256, size=(7, 32), dtype=np.uint8)
    pool[1, :31] = pool[0, :31]                                                      # two keys that differ in the last byte only
    for n in (0, 1, 2, 64, 500):
        A = pool[rng.integers(0, 7, n)]
        keys, offsets, order = Engine.group_by_key(A)
        assert keys.dtype == np.uint8 and keys.shape == (len({bytes(r) for r in A}), 32) and offsets.dtype == np.uint64 and offsets.shape == (len(keys) + 1,)
        assert int(offsets[0]) == 0 and int(offsets[-1]) == n and (np.diff(offsets.astype(np.int64)) > 0).all()
        assert sorted(order.tolist()) == list(range(n))
        assert (np.repeat(keys, np.diff(offsets.astype(np.int64)), axis=0) == A[order]).all()
        for lo, hi in zip(offsets[:-1], offsets[1:]):
            assert (np.diff(order[int(lo):int(hi)]) > 0).all()                       # stable
        back = np.empty_like(A)
        back[order] = np.repeat(keys, np.diff(offsets.astype(np.int64)), axis=0)
        assert (back == A).all()
        k2, o2, order2 = KC.group(A)
        assert (k2 == keys).all() and (o2 == offsets).all() and (order2 == order).all()
    with pytest.raises(ValueError):
        Engine.group_by_key(np.zeros((3, 64), np.uint8))


def test_symbol_is_exported_declared_and_bound_with_one_signature(lib):
    from jubjub_amd import _lib
    from tests import test_rust_shim_signatures as RS

    name = "jj_sigbatch_keyed_begin"
    assert name in _lib.EXPORTS and hasattr(lib, name) and hasattr(C.CDLL(_lib.LIB_PATH), name)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jubjub_hip.h")).read(), flags=re.S)
    m = re.search(r"int\s+%s\s*\(([^;]*?)\)\s*;" % name, header)
    assert m, "%s is not declared in include/jubjub_hip.h" % name
    params = [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]
    assert params == ["jj_ctx*", "const void* base64", "size_t K", "const void* a32", "const uint64_t* offsets", "const void* r32", "const void* s32", "const void* c32",
                      "const void* z16", "unsigned flags", "jj_msm_job** job"]
    sig = _lib._SIGS[name]                                                            # the context comes first
    assert len(sig) == len(params) - 1 and sig[1] is C.c_size_t and sig[8] is C.c_uint and sig[9] == C.POINTER(C.c_void_p)
    assert all(t is C.c_void_p for i, t in enumerate(sig) if i not in (1, 8, 9))
    h, r = RS.header_prototypes()[name], RS.rust_declarations()[name]
    assert h == r and len(h[1]) == 11 and h[1][4] == ("ptr", True, 1) and r[1][10] == ("ptr", False, 2)
    ffi = open(os.path.join(ROOT, "rust-shim", "src", "ffi.rs")).read()
    assert "offsets: *const u64" in re.search(r"pub fn %s\(([^)]*)\)" % name, ffi).group(1)
    # the only non-const pointer is the job slot: no row of tests/buffer_cases.py is needed
    assert [p for p in params[1:] if "*" in p and not p.startswith("const ")] == ["jj_msm_job** job"]


def test_argument_checks_come_before_any_device_work(lib):
    """JJ_ERR_INVALID with *job = NULL.  The checks read no field of the context: a block of zero bytes stands in for it (no GPU here)."""
    from jubjub_amd import _lib

    fake_ctx = C.create_string_buffer(1 << 16)
    buf = C.create_string_buffer(64)
    ctx, p = C.cast(fake_ctx, C.c_void_p), C.cast(buf, C.c_void_p)

    def offs(*v):
        a = np.array(v, dtype=np.uint64)
        return a, C.c_void_p(a.ctypes.data)

    def refused(*args):
        job = C.c_void_p(0xDEAD)
        rc = lib.jj_sigbatch_keyed_begin(*args, C.byref(job))
        return rc == _lib.JJ_ERR_INVALID and not job.value

    k1, o1 = offs(0, 1)
    k0, o0 = offs(0, 0)
    assert refused(None, p, 1, p, o1, p, p, p, p, 0)                                  # no context
    assert lib.jj_sigbatch_keyed_begin(ctx, p, 1, p, o1, p, p, p, p, 0, None) == _lib.JJ_ERR_INVALID      # no job slot
    assert refused(ctx, None, 1, p, o1, p, p, p, p, 0)                                # no base
    for flags in (2, 3, 4, 8, 16, 1 << 31):
        assert refused(ctx, p, 1, p, o0, None, None, None, None, flags), flags        # only 0 and JJ_DECOMPRESS_ZIP216
    assert refused(ctx, p, 1, p, None, p, p, p, p, 0)                                 # NULL offsets with K > 0
    for missing in range(5):
        arrays = [p] * 5
        arrays[missing] = None
        a32, rest = arrays[0], arrays[1:]
        assert refused(ctx, p, 1, a32, o1, *rest, 0), missing                         # a NULL array with n > 0
    a, o = offs(1, 2)
    assert refused(ctx, p, 1, p, o, p, p, p, p, 0)                                    # offsets[0] != 0
    a, o = offs(0, 5, 4, 6)
    assert refused(ctx, p, 3, p, o, p, p, p, p, 0)                                    # a decreasing pair
    a, o = offs(0, (1 << 24) - 1)
    assert refused(ctx, p, 1, p, o, p, p, p, p, 0)                                    # n + K + 1 = 2^24 + 1
    a, o = offs(0, (1 << 64) - 1)
    assert refused(ctx, p, 1, p, o, p, p, p, p, 1)                                    # no wrap-around
    assert refused(ctx, p, 1 << 24, p, o, p, p, p, p, 0)                              # K alone is too large: offsets are not read
    assert refused(ctx, p, (1 << 64) - 1, p, o, p, p, p, p, 0)


def test_engine_checks_shapes_before_any_c_call():
    from jubjub_amd.engine import _sigbatch_keyed_args

    n, K = 5, 2
    base, keys, x32, z = np.zeros(64, np.uint8), np.zeros((K, 32), np.uint8), np.zeros((n, 32), np.uint8), np.ones((n, 16), np.uint8)
    gk, gn, o, args = _sigbatch_keyed_args(base, keys, [0, 2, 5], x32, x32, x32, z)
    assert (gk, gn) == (K, n) and o.dtype == np.uint64 and o.tolist() == [0, 2, 5] and [a.n for a in args] == [1, K, n, n, n, n]
    assert _sigbatch_keyed_args(base, keys, [0, 2, 5], x32, x32, x32, None)[3][5].keep.shape == (n, 16)
    bad = [
        (np.zeros(32, np.uint8), keys, [0, 2, 5], x32, x32, x32, z),
        (base, np.zeros((K, 64), np.uint8), [0, 2, 5], x32, x32, x32, z),
        (base, keys, [0, 2], x32, x32, x32, z),                                       # K + 1 offsets
        (base, keys, [0, 2, 4], x32, x32, x32, z),                                    # offsets[-1] != n
        (base, keys, [1, 2, 5], x32, x32, x32, z),
        (base, keys, [0, 3, 2], x32[:2], x32[:2], x32[:2], z[:2]),
        (base, keys, [0, 2, 5], x32, x32[:-1], x32, z),
        (base, keys, [0, 2, 5], x32, x32, x32, np.ones((n, 32), np.uint8)),
        (base, keys, [0.0, 2.0, 5.0], x32, x32, x32, z),
    ]
    for a in bad:
        with pytest.raises(ValueError):
            _sigbatch_keyed_args(*a)


CPP_CALLER = r"""
#include "jubjub_hip.hpp"
int main(int argc, char**) {
  if (argc < 1000) return 0;                 // links the entry point; runs it only where a device exists
  jubjub::Context ctx(0);
  jubjub::Bytes64 base{};
  std::vector<jubjub::Bytes32> keys(2), r(3), s(3), c(3);
  std::vector<jubjub::Bytes16> z(3);
  std::vector<uint64_t> offsets = {0, 1, 3};
  auto job = jubjub::sigbatch_keyed_begin(ctx, base, keys, offsets, r, s, c, z, true);
  const jubjub::SigVerdict v = jubjub::sigbatch_verdict(job->finish());
  return v == jubjub::SigVerdict::Ok ? 0 : jubjub::sigbatch_keyed_verify(ctx, base, keys, offsets, r, s, c, z) == jubjub::SigVerdict::Malformed ? 2 : 1;
}
"""


def test_cpp_caller_compiles_and_links(lib, tmp_path):
    import subprocess

    src, out = tmp_path / "sig_keyed_caller.cpp", tmp_path / "sig_keyed_caller"
    src.write_text(CPP_CALLER)
    libdir = os.path.join(ROOT, "jubjub_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(out), "-L", libdir, "-ljubjub_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"])
    assert subprocess.run([str(out)], timeout=60).returncode == 0
