"""
The field and point entry points on the edge matrix of tests/field_cases.py (shown to be what it says, and to execute both zero
representations of Field::to_plain / is_zero, by tests/test_field_cases_cpu.py), bit for bit, every unit compared.

Field entry points of both fields on host arrays and on device tensors: add / sub / mul on the cross product of the fixed values and the
relation pairs (a + b = 0, a - b = 0, a b = +-1, two byte strings of one residue), the unary ones on every value that appears, pow on
bases x exponents (the lowest and the highest bit of every exponent word), from_bytes_wide on its own list.  Expected values are Python
integers; sqrt is the oracle's root, and a root.
Field::invert_divsteps on the device, on the list the emulator inverts (field_cases.inversion_values): through k_normalize<4> and
k_normalize<16> with one planted Z per lane and through k_varbase_mont_x1 with one planted denominator per lane.
Point ops on all ordered pairs of the torsion points, +-G, a prime-order point and its torsion cosets; the exact ladder on edge scalars x
those points, all five coordinates.
"""
import functools

import numpy as np
import pytest

import backend_cases as B
import field_cases as F
from oracle import c_oracle as O
from util import EDGE_SCALARS, arr32, to_int

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NAMES = ("fq", "fr")
KINDS = ("host", "device")


@pytest.fixture(scope="module")
def eng():
    from jubjub_amd import Engine

    e = Engine(0)
    yield e
    e.close()


def _to(kind, *arrays):
    if kind == "host":
        return arrays
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


def _np(x):
    if isinstance(x, tuple):
        return tuple(_np(y) for y in x)
    return x.cpu().numpy() if hasattr(x, "cpu") else x


def _same(got, want, what, rows=None):
    got = _np(got)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).reshape(len(want), -1).any(axis=1))
    if len(bad):
        i = int(bad[0])
        detail = " (%s)" % rows(i) if rows else ""
        pytest.fail("%s: %d of %d rows differ, first at row %d%s: got %s, want %s" % (what, len(bad), len(want), i, detail, bytes(got[i]).hex(), bytes(want[i]).hex()))


@functools.lru_cache(maxsize=None)
def _binary_want(name):
    A, Bb = F.pairs(name)
    return {op: F.expect_binary(name, op, A, Bb) for op in F.BINARY}


@functools.lru_cache(maxsize=None)
def _unary_want(name):
    U = F.unary_values(name)
    want = {op: F.expect_unary(name, op, U) for op in F.UNARY}
    want["invert"] = F.expect_invert(name, U)
    want["from_bytes"] = F.expect_from_bytes(name, U)
    want["sqrt"] = O.field_op(F.FIELDS[name][0], "sqrt", U)
    want["bits"] = F.expect_bits(name, U)
    return want


# ------------------------------------------------------------------------------------------------------ field entry points
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_field_binary_on_all_pairs(eng, name, kind):
    A, Bb = F.pairs(name)
    a, b = _to(kind, A, Bb)
    pair = lambda i: "a = %#x, b = %#x" % (to_int(A[i]), to_int(Bb[i]))
    for op, want in _binary_want(name).items():
        _same(eng.field_binary(name, op, a, b), want, "jj_%s_%s, %s" % (name, op, kind), pair)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_field_unary_on_every_value(eng, name, kind):
    p = F.FIELDS[name][1]
    U = F.unary_values(name)
    (a,) = _to(kind, U)
    want = _unary_want(name)
    val = lambda i: "a = %#x" % to_int(U[i])
    for op in F.UNARY:
        _same(eng.field_unary(name, op, a), want[op], "jj_%s_%s, %s" % (name, op, kind), val)
    for op in ("invert", "from_bytes", "sqrt"):
        out, ok = eng.field_unary_ok(name, op, a)
        _same(ok, want[op][1], "jj_%s_%s ok, %s" % (name, op, kind), val)
        _same(out, want[op][0], "jj_%s_%s, %s" % (name, op, kind), val)
        if op == "sqrt":
            for x, r, k in zip(U, _np(out), _np(ok)):                                # a root, whichever the oracle names
                if k:
                    assert to_int(r) < p and to_int(r) ** 2 % p == to_int(x) % p, hex(to_int(x))
    _same(eng.to_le_bits(name, a), want["bits"], "jj_%s_to_le_bits, %s" % (name, kind), val)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_field_pow_matrix(eng, name, kind):
    A, E = F.pow_matrix(name)
    a, e = _to(kind, A, E)
    _same(eng.field_binary(name, "pow", a, e), F.expect_pow(name, A, E), "jj_%s_pow, %s" % (name, kind),
          lambda i: "a = %#x, e = %#x" % (to_int(A[i]), to_int(E[i])))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_from_bytes_wide_list(eng, name, kind):
    (w,) = _to(kind, F.wide_bytes(name))
    _same(eng.from_bytes_wide(name, w), F.expect_wide(name), "jj_%s_from_bytes_wide, %s" % (name, kind), lambda i: "%#x" % F.wide_values(name)[i])


# ------------------------------------------------------------------------------------------- invert_divsteps on the device
def test_inversion_list_through_k_normalize_4(eng):
    """n = 4 |X|: T = |X|, lane t holds rows t, t + T, t + 2T, t + 3T and inverts X[t] * 1 * 1 * 1"""
    X = F.inversion_values("fq")
    m = len(X)
    lanes = eng.device_info()["cus"] * B.LANES_PER_CU
    assert B.norm_chunk(4 * m, lanes) == 4
    ext, want = F.norm_plant(4 * m)
    for kind in KINDS:
        (e,) = _to(kind, ext)
        _same(eng.batch_normalize(e), want, "jj_batch_normalize, k_normalize<4>, %s" % kind,
              lambda i: "lane %d, position %d%s" % (i % m, i // m, ", Z = %#x" % X[i] if i < m else ""))


def test_inversion_list_through_k_normalize_16(eng):
    """the smallest n that takes k_normalize<16>: 4 x lanes rows, T = n / 16, lane t < |X| inverts X[t] * 1^15"""
    X = F.inversion_values("fq")
    lanes = eng.device_info()["cus"] * B.LANES_PER_CU
    n = 4 * lanes
    assert B.norm_chunk(n, lanes) == 16 and B.norm_chunk(n - 1, lanes) == 4 and n // 16 >= len(X)
    ext, want = F.norm_plant(n)
    T = n // 16
    _same(eng.batch_normalize(torch.from_numpy(ext).cuda()), want, "jj_batch_normalize, k_normalize<16>, n = %d" % n,
          lambda i: "lane %d, position %d%s" % (i % T, i // T, ", Z = %#x" % X[i] if i < len(X) else ""))


def test_inversion_list_through_k_varbase_mont_x1():
    """every x of X that is 1 - v of a curve point, alone in its lane of k_varbase_mont_x1 (the identity at the lane's other fifteen units):
    the default ladder above vb_quad_max, affine and compressed"""
    from jubjub_amd import Engine

    S, P, units = F.mont_plant()
    want = O.varbase_mul(S, P)
    e = Engine(0, options={"vb_quad_max": 0})
    try:
        where = lambda i: "unit %d (wave %d, lane %d, step %d)%s" % (i, i // 1024, i % 64, i % 1024 // 64, ", planted" if i in set(units.tolist()) else "")
        _same(e.varbase_mul(S, P), want, "jj_varbase_mul through k_varbase_mont_x1", where)
        _same(e.varbase_mul_compressed(S, P), O.compress(want), "jj_varbase_mul_compressed through k_varbase_mont_x1", where)
        s, p = _to("device", S, P)
        _same(e.varbase_mul(s, p), want, "jj_varbase_mul through k_varbase_mont_x1, device", where)
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------------------------ points
@pytest.mark.parametrize("kind", KINDS)
def test_point_add_sub_on_all_ordered_pairs(eng, kind):
    P, Qq = F.point_pairs()
    p, q = _to(kind, P, Qq)
    n = len(F.points())
    pair = lambda i: "A[%d], A[%d]" % (i // n, i % n)
    _same(eng.point_add(p, q), O.point_op("add", P, Qq), "jj_point_add, %s" % kind, pair)
    _same(eng.point_sub(p, q), O.point_op("sub", P, Qq), "jj_point_sub, %s" % kind, pair)


@pytest.mark.parametrize("kind", KINDS)
def test_point_unary_ops_and_predicates(eng, kind):
    A = F.points()
    (a,) = _to(kind, A)
    _same(eng.point_double(a), O.point_op("double", A), "jj_point_double, %s" % kind)
    _same(eng.point_neg(a), O.point_op("neg", A), "jj_point_neg, %s" % kind)
    _same(eng.mul_by_cofactor(a), O.point_op("mul_by_cofactor", A), "jj_point_mul_by_cofactor, %s" % kind)
    _same(eng.to_niels(a), O.to_niels(A), "jj_point_to_niels, %s" % kind)
    for pred in ("is_identity", "is_small_order", "is_on_curve", "is_torsion_free", "is_prime_order"):
        _same(eng.predicate(pred, a), O.predicate(pred, A), "jj_%s, %s" % (pred, kind))


def test_exact_ladder_on_edge_scalars_and_special_points(eng):
    """jj_varbase_mul_exact promises the reference's projective coordinates: all five, on the torsion points and the cosets too"""
    A = F.points()
    S = np.repeat(arr32(EDGE_SCALARS), len(A), axis=0)
    P = np.tile(A, (len(EDGE_SCALARS), 1))
    want = O.varbase_mul_ext(S, P)
    where = lambda i: "scalar %#x, A[%d]" % (EDGE_SCALARS[i // len(A)], i % len(A))
    _same(eng.varbase_mul_exact(S, P), want, "jj_varbase_mul_exact", where)
    s, p = _to("device", S, P)
    _same(eng.varbase_mul_exact(s, p), want, "jj_varbase_mul_exact, device", where)
