"""
jj_sigbatch_begin without a GPU: the symbol is exported, declared and bound; its argument checks come before any device work; Engine's shape
checks raise before any C call; a C++ caller of include/jubjub_hip.hpp compiles and links; and every planted case of tests/sig_batch_cases.py is
pinned to the oracle's evaluation of the whole sum (O.msm over the 2n + 1 terms plus three doublings) at n <= 65.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import c_oracle as O
from tests import sig_batch_cases as SC

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
SIZES = (1, 2, 63, 64, 65)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from jubjub_amd import _lib

    ge.build()
    return _lib.load()


def test_symbol_is_exported_declared_and_bound(lib):
    from jubjub_amd import _lib

    assert "jj_sigbatch_begin" in _lib.EXPORTS and hasattr(lib, "jj_sigbatch_begin")
    header = open(os.path.join(ROOT, "include", "jubjub_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"int\s+jj_sigbatch_begin\s*\(([^;]*?)\)\s*;", header)
    assert m, "jj_sigbatch_begin is not declared in include/jubjub_hip.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 10 and params[0].startswith("jj_ctx") and params[-1].replace(" ", "") == "jj_msm_job**job"
    assert len(_lib._SIGS["jj_sigbatch_begin"]) == 9                      # the context comes first
    assert hasattr(C.CDLL(_lib.LIB_PATH), "jj_sigbatch_begin")             # a default-visibility export of the shared object itself


def test_argument_checks_come_before_any_device_work(lib):
    """JJ_ERR_INVALID with *job = NULL.  The checks read no field of the context: where a context is needed to reach a check, a block of zero bytes
    stands in for it (no GPU here)."""
    from jubjub_amd import _lib

    fake_ctx = C.create_string_buffer(1 << 16)
    buf = C.create_string_buffer(64)
    ctx, p = C.cast(fake_ctx, C.c_void_p), C.cast(buf, C.c_void_p)

    def refused(*args):
        job = C.c_void_p(0xDEAD)
        rc = lib.jj_sigbatch_begin(*args, C.byref(job))
        return rc == _lib.JJ_ERR_INVALID and not job.value

    assert refused(None, p, 0, None, None, None, None, None, 0)                          # no context
    assert lib.jj_sigbatch_begin(ctx, p, 0, None, None, None, None, None, 0, None) == _lib.JJ_ERR_INVALID      # no job slot
    assert refused(ctx, None, 0, None, None, None, None, None, 0)                        # no base
    for flags in (2, 3, 4, 8, 16, 1 << 31):
        assert refused(ctx, p, 0, None, None, None, None, None, flags), flags             # only 0 and JJ_DECOMPRESS_ZIP216
    for missing in range(5):
        arrays = [p] * 5
        arrays[missing] = None
        assert refused(ctx, p, 1, *arrays, 0), missing                                    # a NULL array with n > 0
    assert refused(ctx, p, 1 << 23, p, p, p, p, p, 0)                                     # 2n + 1 > 2^24
    assert refused(ctx, p, (1 << 64) - 1, p, p, p, p, p, 1)


def test_engine_checks_shapes_before_any_c_call():
    from jubjub_amd.engine import SIGBATCH_IDENTITY, SIGBATCH_MALFORMED, _sigbatch_args, _sigbatch_z

    n = 5
    base, x32, z = np.zeros(64, np.uint8), np.zeros((n, 32), np.uint8), np.ones((n, 16), np.uint8)
    got_n, args = _sigbatch_args(base, x32, x32, x32, x32, z)
    assert got_n == n and [a.n for a in args] == [1, n, n, n, n, n]
    assert _sigbatch_args(base, x32, x32, x32, x32, None)[1][5].keep.shape == (n, 16)
    bad = [
        (np.zeros(32, np.uint8), x32, x32, x32, x32, z),
        (np.zeros((2, 64), np.uint8), x32, x32, x32, x32, z),
        (base, np.zeros((n, 64), np.uint8), x32, x32, x32, z),
        (base, np.zeros(n * 32, np.uint8), x32, x32, x32, z),
        (base, x32, x32[:-1], x32, x32, z),
        (base, x32, x32, np.zeros((n, 16), np.uint8), x32, z),
        (base, x32, x32, x32, x32[1:], z),
        (base, x32, x32, x32, x32, np.ones((n, 32), np.uint8)),
        (base, x32, x32, x32, x32, np.ones((n - 1, 16), np.uint8)),
        (base, x32, x32, x32, x32, [1] * 16 * n),
    ]
    for args in bad:
        with pytest.raises(ValueError):
            _sigbatch_args(*args)
    with pytest.raises(TypeError):
        _sigbatch_args(base, x32.astype(np.int32), x32, x32, x32, z)
    with pytest.raises(ValueError):
        big = np.broadcast_to(np.zeros((1, 32), np.uint8), (1 << 23, 32))
        _sigbatch_args(base, big, big, big, big, np.broadcast_to(np.ones((1, 16), np.uint8), (1 << 23, 16)))
    drawn = _sigbatch_z(4096)
    assert drawn.shape == (4096, 16) and drawn.dtype == np.uint8 and drawn.any(axis=1).all() and len({bytes(r) for r in drawn}) == 4096
    assert SIGBATCH_IDENTITY == bytes(SC.IDENTITY) and SIGBATCH_MALFORMED == bytes(SC.MALFORMED)


CPP_CALLER = r"""
#include "jubjub_hip.hpp"
int main(int argc, char**) {
  if (argc < 1000) return 0;                 // links the entry points; runs them only where a device exists
  jubjub::Context ctx(0);
  jubjub::Bytes64 base{};
  std::vector<jubjub::Bytes32> r(2), a(2), s(2), c(2);
  std::vector<jubjub::Bytes16> z(2);
  auto job = jubjub::sigbatch_begin(ctx, base, r, a, s, c, z, true);
  const jubjub::SigVerdict v = jubjub::sigbatch_verdict(job->finish());
  return v == jubjub::SigVerdict::Ok ? 0 : jubjub::sigbatch_verify(ctx, base, r, a, s, c, z) == jubjub::SigVerdict::Malformed ? 2 : 1;
}
"""


def test_cpp_caller_compiles_and_links(lib, tmp_path):
    src, out = tmp_path / "sig_caller.cpp", tmp_path / "sig_caller"
    src.write_text(CPP_CALLER)
    libdir = os.path.join(ROOT, "jubjub_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(out), "-L", libdir, "-ljubjub_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"])
    assert subprocess.run([str(out)], timeout=60).returncode == 0


def test_cases_are_what_they_claim():
    ident = SC.IDENTITY[None]
    t = SC.T8[None]
    assert not (O.point_op("double", O.point_op("double", t)) == ident).all() and (O.point_op("mul_by_cofactor", t) == ident).all()      # order 8
    b = SC.bases()
    assert O.predicate("is_prime_order", b["prime"][None])[0] == 1 and O.predicate("is_torsion_free", b["order8r"][None])[0] == 0
    enc = SC.NONCANONICAL_IDENTITY[None]
    assert O.decompress(enc, 0)[1][0] == 1 and (O.decompress(enc, 0)[0] == ident).all() and O.decompress(enc, SC.ZIP216)[1][0] == 0
    assert O.decompress(SC.off_curve_encoding()[None], 0)[1][0] == 0
    assert SC.positions(257) == [0, 63, 64, 128, 256] and SC.positions(1) == [0] and SC.positions(64) == [0, 32, 63]
    names = {v for v, _ in SC.variants(65)}
    assert names == {"valid", "order8r", "c_plus_r", "torsion_r", "bad_s", "bad_r", "s_plus_r", "off_curve_r", "noncanonical_a_zip216", "noncanonical_a"}
    v = SC.batch(65, "valid")
    assert v.z.any(axis=1).all() and all(SC.to_int(x) < SC.R for x in v.s) and all(SC.to_int(x) < SC.R for x in v.c)
    u = SC.batch(65, "c_plus_r")
    assert all(SC.to_int(x) >= SC.R for x in u.c) and all(SC.to_int(x) - SC.R == SC.to_int(y) for x, y in zip(u.c, v.c))
    # the order-8r base: valid under the cofactored check only -- [s]B - R - [c]A is a non-trivial torsion point for some signature
    w = SC.batch(65, "order8r")
    rp, ap = O.decompress(w.r, 0)[0], O.decompress(w.a, 0)[0]
    lhs = O.varbase_mul(w.s, np.tile(w.base, (65, 1)))
    rhs = O.point_op("add", rp, O.varbase_mul(w.c, ap))
    diff = O.point_op("sub", lhs, rhs)
    assert (diff != SC.IDENTITY).any() and (O.point_op("mul_by_cofactor", diff) == SC.IDENTITY).all()


@pytest.mark.parametrize("n", SIZES)
def test_every_planted_case_equals_the_whole_sum(n):
    """the expected bytes (closed forms: -[8 z_k delta] B, [8 z_k] D, the identity, the sentinel) against O.msm over all 2n + 1 terms + 3 doublings"""
    for variant, k in SC.variants(n):
        b = SC.batch(n, variant, k)
        got = SC.full_evaluation(b)
        assert bytes(got) == bytes(b.expected), b.name
        if variant in ("bad_s", "bad_r"):
            assert bytes(b.expected) not in (bytes(SC.IDENTITY), bytes(SC.MALFORMED)), b.name
        if variant == "c_plus_r":
            assert bytes(b.expected) == bytes(SC.batch(n, "valid").expected)


def test_the_empty_batch_is_the_identity():
    b = SC.batch(0, "valid")
    assert b.n == 0 and bytes(SC.full_evaluation(b)) == bytes(SC.IDENTITY)
