"""
The edge matrix of tests/field_cases.py is what it says (CPU only), and it executes the branches it was built for.

Every relation class occurs per field and the expected values agree by two routes (Python integers, the C oracle).  The whole matrix goes
through the host emulation of jj_field.h (tests/cpp/emu_field.cpp, every accumulator shadowed in 128 bits): the emulator and the GPU
(tests/test_gpu_field_matrix.py) see one matrix.  emu_plain_product_class names the class of the product Field::to_plain and is_zero form --
digits 0, digits of -p, other -- and the matrix must reach a zero in both representations (or field_cases.UNREACHED says what was searched),
where field_inputs of tests/test_gpu_parity.py, the GPU's only field inputs until now, reaches the digits of -p never.  emu_normalize_lane
mirrors a lane of k_normalize and counts the conditional additions of q in canon_plain_product over the normaliser plant.  The two plant
layouts are pinned against normalize_launch, MONT_X1_UNITS and the unit indexing of k_varbase_mont_x1.
"""
import collections
import ctypes
import os
import re

import numpy as np
import pytest

import backend_cases as B
import field_cases as F
from oracle import c_oracle as O
from oracle import jubjub_ref as J
from test_backend_cases_cpu import _body, parse_normalize_launch
from test_emu_field import _buf, _in, emu  # noqa: F401  (the emulator fixture: built on demand, zero shadow overflows at teardown)
from util import EDGE_SCALARS, Q, R, arr32, b32, to_int, to_pt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fq", "fr")


# ------------------------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("name", NAMES)
def test_values_and_relation_classes(name):
    which, p = F.FIELDS[name]
    fixed, V = F.fixed_values(name), F.values(name)
    assert all(0 <= v <= F.M256 for v in V) and len(set(V)) == len(V) == len(fixed) + 32
    must = [0, 1, 2, 3, p - 1, p - 2, p - 3, (p - 1) // 2, (p + 1) // 2, (1 << 29) - 1, 1 << 29, 1 << 58, (1 << 232) - 1, 1 << 232,
            (1 << 252) - 1, 1 << 252, (1 << 255) - 1, 1 << 255, F.M256]
    multiples = F.M256 // p
    assert multiples == (2 if name == "fq" else 17)
    for k in range(1, multiples + 1):
        must += [k * p - 1, k * p] + ([k * p + 1] if k * p + 1 <= F.M256 else [])
    assert set(must) <= set(fixed)
    forms = {v * F.MONT_R % p for v in fixed}
    assert {1, p - 1, 1 << 232, (F.MONT_R - 1) % p} <= forms
    rel = F.relation_pairs(name)
    count = collections.Counter(r for r, _, _ in rel)
    assert set(count) == set(F.RELATIONS) and count["v,v"] == count["v,p-v"] == len(V)
    checks = {"v,v": lambda a, b: a == b, "v,p-v": lambda a, b: (a + b) % p == 0 and 0 < b <= p, "v,2p-v": lambda a, b: (a + b) % p == 0 and p < b,
              "v,1/v": lambda a, b: a * b % p == 1, "v,-1/v": lambda a, b: a * b % p == p - 1, "v,v+1": lambda a, b: b == a + 1,
              "v,v+p": lambda a, b: b == a + p}
    for r, a, b in rel:
        assert 0 <= b <= F.M256 and checks[r](a, b), (r, hex(a), hex(b))
    # what the old inputs never held: a + b = 0 with a != 0, a - b = 0 beyond (p, p), a b = +-1, two byte strings of one residue
    assert any(a % p and (a + b) % p == 0 for _, a, b in rel) and any(a != b and a % p == b % p for _, a, b in rel)
    A, Bb = F.pairs(name)
    assert len(A) == len(Bb) == len(fixed) ** 2 + len(rel)
    U = F.unary_values(name)
    have = {bytes(r) for r in U}
    assert len(have) == len(U) and all(bytes(r) in have for r in A) and all(bytes(r) in have for r in Bb)


@pytest.mark.parametrize("name", NAMES)
def test_expected_values_by_both_routes(name):
    which, p = F.FIELDS[name]
    A, Bb = F.pairs(name)
    for op in F.BINARY:
        assert (F.expect_binary(name, op, A, Bb) == O.field_op(which, op, A, Bb)[0]).all(), op
    U = F.unary_values(name)
    for op in F.UNARY:
        assert (F.expect_unary(name, op, U) == O.field_op(which, op, U)[0]).all(), op
    inv, ok = F.expect_invert(name, U)
    oi, ook = O.field_op(which, "invert", U)
    assert (inv == oi).all() and (ok == ook).all() and 0 < ok.sum() < len(ok)
    dec, ok = F.expect_from_bytes(name, U)
    od, ook = O.from_bytes(which, U)
    assert (dec == od).all() and (ok == ook).all() and 0 < ok.sum() < len(ok)
    assert (F.expect_wide(name) == O.from_bytes_wide(which, F.wide_bytes(name))).all()
    root, ok = O.field_op(which, "sqrt", U)
    for a, r, k in zip(U, root, ok):
        a, r = to_int(a) % p, to_int(r)
        assert k == (1 if a == 0 or pow(a, (p - 1) // 2, p) == 1 else 0)
        if k:
            assert r < p and r * r % p == a
    assert 0 < ok.sum() < len(ok)


@pytest.mark.parametrize("name", NAMES)
def test_pow_and_wide_lists(name):
    which, p = F.FIELDS[name]
    A, E = F.pow_matrix(name)
    bases, exps = {to_int(a) for a in A}, {to_int(e) for e in E}
    assert len(A) == len(bases) * len(exps)
    assert {0, 1, 2, p - 1, p, p + 1, F.M256, F.GENERATORS[name]} <= bases and len(bases) == 13
    assert pow(F.GENERATORS[name], (p - 1) // 2, p) == p - 1
    assert {0, 1, 2, 3, p - 2, p - 1, p, p + 1, (p - 1) // 2, F.M256} <= exps
    assert all(1 << (32 * w) in exps and 1 << (32 * w + 31) in exps for w in range(8)) and all(1 << k in exps for k in (33, 63, 64, 224, 255))
    src = open(os.path.join(ROOT, "jubjub_amd", "csrc", "jj_kernels.h")).read()
    assert "word = ((bit >> 5) == w) ? we[w] : word;" in src                        # the word select the word powers aim at
    want = F.expect_pow(name, A, E)
    fld = J.FQ if name == "fq" else J.FR
    for a, e, w in list(zip(A, E, want))[::7]:
        assert fld.pow(to_int(a) % p, to_int(e)) == to_int(w)
    W = F.wide_values(name)
    top = ((1 << 512) - 1) // p * p
    assert {p << 256, (p << 256) - 1, top, top - 1, top + 1, (1 << 512) - 1, F.M256 | (F.M256 << 256), p | (p << 256)} <= set(W)
    assert top % p == 0 and top + p >= 1 << 512 and len(W) == 81 + 3          # p 2^256, p 2^256 - 1 and 2^512 - 1 are in the cross product already


def test_inversion_list_and_points():
    for name in NAMES:
        p = F.FIELDS[name][1]
        X = F.inversion_values(name)
        assert len({x % p for x in X}) == len(X) and all(x % p for x in X) and max(X) < 1 << 255
        assert {1, 2, 3, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2} <= set(X) and all(1 << k in X for k in range(255))
        assert len(X) >= 4 + 2 * 255 - 4 + 3 + 64 - 2
    assert max(F.inversion_values("fq")) < Q                                        # canonical: a Z, and 1 - v, as they stand
    A = F.points()
    pts = [to_pt(r) for r in A]
    assert len(set(pts)) == len(pts) == 8 + 2 + 1 + 7 + 2 and all(J.affine_is_on_curve(pt) for pt in pts)
    assert O.predicate("is_on_curve", A).all()
    small, free = O.predicate("is_small_order", A), O.predicate("is_torsion_free", A)
    assert small[:8].all() and not small[8:].any()
    assert free[0] and not free[1:10].any() and free[10] and not free[11:18].any()    # the identity and S; G generates the full group of order 8 r
    assert pts[8] == J.GENERATOR and pts[9] == J.affine_neg(J.GENERATOR)
    P, Qq = F.point_pairs()
    assert len(P) == len(A) ** 2 and len({bytes(a) + bytes(b) for a, b in zip(P, Qq)}) == len(P)


# ------------------------------------------------------------------------------------------------- through the emulator
@pytest.mark.parametrize("name", NAMES)
def test_matrix_through_the_emulator(emu, name):  # noqa: F811
    which, p = F.FIELDS[name]
    fn = emu.emu_fq_op if name == "fq" else emu.emu_fr_op
    out, ok = _buf(32), _buf(1)
    A, Bb = F.pairs(name)
    want = {op: F.expect_binary(name, op, A, Bb) for op in F.BINARY}
    for i, (a, b) in enumerate(zip(A, Bb)):
        ia, ib = _in(a), _in(b)
        for op in F.BINARY:
            fn(F.EMU_OPS[op], ia, ib, out, ok)
            assert bytes(out) == bytes(want[op][i]), (name, op, hex(to_int(a)), hex(to_int(b)))
        fn(F.EMU_OPS["eq"], ia, ib, out, ok)
        assert ok[0] == (1 if to_int(a) % p == to_int(b) % p else 0)
    U = F.unary_values(name)
    want = {op: F.expect_unary(name, op, U) for op in F.UNARY}
    inv, inv_ok = F.expect_invert(name, U)
    dec, dec_ok = F.expect_from_bytes(name, U)
    for i, a in enumerate(U):
        ia = _in(a)
        for op in F.UNARY:
            fn(F.EMU_OPS[op], ia, ia, out, ok)
            assert bytes(out) == bytes(want[op][i]), (name, op, hex(to_int(a)))
        fn(F.EMU_OPS["invert"], ia, ia, out, ok)
        assert bytes(out) == bytes(inv[i]) and ok[0] == inv_ok[i]
        emu.emu_from_bytes(which, ia, out, ok)
        assert bytes(out) == bytes(dec[i]) and ok[0] == dec_ok[i]
    for w, x in zip(F.wide_bytes(name), F.expect_wide(name)):
        emu.emu_from_wide(which, _in(w), out)
        assert bytes(out) == bytes(x)
    assert emu.emu_overflow_count() == 0


def _classes(emu, which, op, A, Bb):  # noqa: F811
    """{class: count} over the pairs whose result is 0 mod p; class 0: digits 0, 1: digits of -p"""
    p = (Q, R)[which]
    f = {0: lambda a, b: a + b, 1: lambda a, b: a - b, 2: lambda a, b: a * b}[op]
    count = collections.Counter()
    for a, b in zip(A, Bb):
        cls = emu.emu_plain_product_class(which, op, _in(a), _in(b))
        zero = f(to_int(a), to_int(b)) % p == 0
        assert (cls != 2) == zero, (which, op, hex(to_int(a)), hex(to_int(b)))
        if zero:
            count[cls] += 1
    return count


def _old_field_inputs(p, seed, n=1000):
    """field_inputs of tests/test_gpu_parity.py, copied (that module needs a GPU marker and the engine to import)"""
    rng = np.random.default_rng(seed)
    edge = [0, 1, 2, p - 1, p - 2, p, p + 1, (p - 1) // 2, (1 << 255) - 1, (1 << 256) - 1, 1 << 255, 3 * p]
    edge = [e for e in edge if e < (1 << 256)]
    a = np.concatenate([arr32(edge), rng.integers(0, 256, size=(n, 32), dtype=np.uint8)])
    b = np.concatenate([arr32(list(reversed(edge))), rng.integers(0, 256, size=(n, 32), dtype=np.uint8)])
    return a, b


def test_old_field_inputs_is_the_copy():
    src = open(os.path.join(ROOT, "tests", "test_gpu_parity.py")).read()
    body = src[src.index("def field_inputs("):src.index("@pytest.mark.parametrize", src.index("def field_inputs("))]
    import inspect

    mine = inspect.getsource(_old_field_inputs)
    strip = lambda s: [ln.strip() for ln in s.splitlines()[1:] if ln.strip() and not ln.strip().startswith('"""')]
    assert strip(body) == strip(mine)
    assert "a, b = field_inputs(p, 11 + which)" in src


@pytest.mark.parametrize("name", NAMES)
def test_matrix_reaches_both_zero_representations_and_the_old_inputs_do_not(emu, name):  # noqa: F811
    """to_plain and is_zero see a zero as the digits 0 or as the digits of -p; only the second makes to_plain add p and carry through every limb"""
    which, p = F.FIELDS[name]
    A, Bb = F.pairs(name)
    seen = {}
    for opname, op in (("add", 0), ("sub", 1), ("mul", 2)):
        c = _classes(emu, which, op, A, Bb)
        seen[opname] = c
        print("%s %s: %d zero results, %d as digits 0, %d as digits of -p" % (name, opname, c[0] + c[1], c[0], c[1]))
        assert c[0] > 0, (name, opname)
        key = "%s %s: zero as -p" % (name, opname)
        if key in F.UNREACHED:
            assert c[1] == 0, "%s is reached %d times: take it out of UNREACHED" % (key, c[1])
        else:
            assert c[1] > 0, "%s: no pair of the matrix leaves the digits of -p" % key
    assert seen["add"][1] > 0                                                        # never in UNREACHED: the reason this matrix exists
    old_a, old_b = _old_field_inputs(p, 11 + which)
    for opname, op in (("add", 0), ("sub", 1), ("mul", 2)):
        c = _classes(emu, which, op, old_a, old_b)
        print("%s %s, field_inputs: %d zero results, %d as digits 0, %d as digits of -p" % (name, opname, c[0] + c[1], c[0], c[1]))
        assert c[0] > 0 and c[1] == 0, (name, opname, c)
    assert all(k.split()[0].rstrip(":") in NAMES + ("normaliser",) for k in F.UNREACHED) and all(v.strip() for v in F.UNREACHED.values())


# ------------------------------------------------------------------------------------------------------- the two plants
def _lane(emu, rows):  # noqa: F811
    chunk = len(rows)
    out = _buf(64 * chunk)
    adds = (ctypes.c_int * (2 * chunk))()
    emu.emu_normalize_lane(chunk, _in(np.ascontiguousarray(rows[:, :96]).tobytes()), out, adds)
    return np.frombuffer(bytes(out), np.uint8).reshape(chunk, 64), list(adds)


def test_normaliser_plant_through_the_emulated_lane(emu):  # noqa: F811
    """lane t of k_normalize<4> on the plant: rows t, t + m, t + 2m, t + 3m.  The planted row's result is (U / x, V / x), the others are their own
    bytes, and the plant hits every number of additions of q in canon_plain_product that X x a seeded set of (U, V) can produce."""
    X = F.inversion_values("fq")
    m = len(X)
    ext, want = F.norm_plant(4 * m)
    assert (ext[m:, 64:96] == b32(1)).all() and (ext[:m, 64:96] == arr32(X)).all()
    assert (want[m:] == ext[m:, :64]).all() and (O.batch_normalize(ext[:m]) == want[:m]).all()
    hit = collections.Counter()
    for t in range(m):
        rows = ext[[t, t + m, t + 2 * m, t + 3 * m]]
        got, adds = _lane(emu, rows)
        assert (got == want[[t, t + m, t + 2 * m, t + 3 * m]]).all(), (t, hex(X[t]))
        hit.update(adds[:2])                                                         # the planted row
    print("normaliser plant: additions of q in canon_plain_product over the planted rows: %s" % dict(sorted(hit.items())))
    rng = np.random.default_rng(0x5345454B)
    possible = collections.Counter()
    uv = [b32(v) for v in (0, 1, Q - 1, (Q - 1) // 2, 2, Q - 2, (Q + 1) // 2, (1 << 254) - 1)] + [r for r in F._canonical_rows(rng, 8)]
    row = np.zeros((1, 96), np.uint8)
    for x in X:
        row[0, 64:96] = b32(x)
        for a in range(0, len(uv), 2):
            row[0, :32], row[0, 32:64] = uv[a], uv[a + 1]
            possible.update(_lane(emu, row)[1])
    print("normaliser search (every x of X, sixteen U / V): %s" % dict(sorted(possible.items())))
    assert set(hit) <= {0, 1, 2}
    for count in (0, 1, 2):
        key = "normaliser: %d additions of q" % count
        if count in possible or count in hit:
            assert count in hit, "%s occurs in the search and not in the plant" % key
            assert key not in F.UNREACHED
        else:
            assert key in F.UNREACHED, key
    assert emu.emu_overflow_count() == 0


def test_normaliser_plant_layout_is_normalize_launch():
    lanes_per_cu, table, last = parse_normalize_launch(_body("normalize_launch"))
    assert last == 4 and (4, 16) in table and min(mult for mult, _ in table) == 4 and lanes_per_cu == B.LANES_PER_CU
    kern = open(os.path.join(ROOT, "jubjub_amd", "csrc", "jj_kernels.h")).read()
    body = kern[kern.index("k_normalize(size_t n, size_t T"):kern.index("k_is_identity_ext")]
    assert "const size_t i = t + (size_t)j * T;" in body and "Fq::invert_divsteps(acc)" in body      # element j of lane t is row t + j T
    m = len(F.inversion_values("fq"))
    for cus in (64, 256, 304):
        lanes = cus * lanes_per_cu
        assert B.norm_chunk(4 * m, lanes) == 4 and (4 * m + 3) // 4 == m                              # T = m: lane t < m holds rows t + j m
        n16 = 4 * lanes
        assert B.norm_chunk(n16, lanes) == 16 and B.norm_chunk(n16 - 1, lanes) == 4 and (n16 + 15) // 16 >= m


def test_mont_plant_layout_is_k_varbase_mont_x1():
    mont = open(os.path.join(ROOT, "jubjub_amd", "csrc", "jj_mont.h")).read()
    assert int(re.search(r"constexpr int MONT_X1_UNITS = (\d+);", mont).group(1)) == F.MONT_X1_UNITS
    assert "const Fe d = Fq::sub(Fq::one(), v);" in mont and "return Fq::select(d, Fq::one(), 0u - (u32)Fq::is_zero(d));" in mont
    kern = open(os.path.join(ROOT, "jubjub_amd", "csrc", "jj_kernels.h")).read()
    body = kern[kern.index("k_varbase_mont_x1(size_t n"):kern.index("k_varbase_mont(size_t n")]
    assert "const size_t first = (t >> 6) * (size_t)(64 * MONT_X1_UNITS) + (t & 63u);" in body
    assert body.count("const size_t i = first + (size_t)s * 64;") == 2 and "Fq::invert_divsteps(acc)" in body
    pts = F.mont_points()
    X = F.inversion_values("fq")
    assert len(pts) >= len(X) // 3 and {x for x, _ in pts} <= set(X)
    for j, (x, (u, v)) in enumerate(pts):
        assert J.affine_is_on_curve((u, v)) and (1 - v) % Q == x and u
    assert len({u & 1 for _, (u, _) in pts}) == 2
    S, P, units = F.mont_plant()
    n = len(P)
    assert n % F.MONT_WAVE_UNITS == 0 and len(S) == n and n // F.MONT_WAVE_UNITS == (len(pts) + 63) // 64
    assert O.predicate("is_on_curve", P).all()
    ident = O.predicate("is_identity", P)
    for j, i in enumerate(units):
        w, l = divmod(j, 64)
        assert i == w * 1024 + l and to_pt(P[i]) == pts[j][1]
        assert all(ident[i + 64 * s] for s in range(1, 16))
    assert int((~ident.astype(bool)).sum()) == len(pts) + 16 * (64 * (n // F.MONT_WAVE_UNITS) - len(pts))
    heads = {to_int(s) for s in S[:4]}
    assert {1, 2, R - 1} <= heads and to_int(S[3]) >> 252


def test_exact_ladder_rows():
    assert len(EDGE_SCALARS) * len(F.points()) == 22 * 20
