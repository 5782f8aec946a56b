"""
The cases of tests/backend_cases.py are what they say (CPU only): the variant table of k_normalize and the fold width of the sum tree
are the ones in jj_abi.hip, the oracle agrees with the Python big-int reference on every planted row, sum layout and root pattern, and
every root pattern has an encoding that brings it to the decoder.
"""
import os
import re

import numpy as np
import pytest

import backend_cases as B
from oracle import c_oracle as O
from oracle import jubjub_ref as J
from util import Q, arr32, b32, pt64, to_int, to_pt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ABI = os.path.join(ROOT, "jubjub_amd", "csrc", "jj_abi.hip")


def _body(name):
    src = open(ABI).read()
    m = re.search(r"^static int %s\([^)]*\) \{\n(.*?)^\}\n" % name, src, re.S | re.M)
    assert m, name
    return m.group(1)


def parse_normalize_launch(body):
    """(lanes per CU, [(multiplier, CHUNK)] in the order of the branches, CHUNK of the final else)"""
    m = re.search(r"lanes_wanted = \(size_t\)c->cus((?: \* \d+)+);", body)
    lanes = int(np.prod([int(x) for x in re.findall(r"\d+", m.group(1))]))
    launch = r"\{ size_t T = \(n \+ (\d+)\) / (\d+); hipLaunchKernelGGL\(\(k_normalize<(\d+)>\)"
    pairs = []
    for mult, add, div, chunk in re.findall(r"if \(n >= lanes_wanted \* (\d+)\) " + launch, body):
        assert int(add) + 1 == int(div) == int(chunk), (mult, add, div, chunk)
        pairs.append((int(mult), int(chunk)))
    add, div, chunk = re.search(r"\n\s*else " + launch, body).groups()
    assert int(add) + 1 == int(div) == int(chunk)
    assert len(re.findall(r"k_normalize<", body)) == len(pairs) + 1                        # no branch the patterns above missed
    return lanes, pairs, int(chunk)


def test_norm_chunk_is_normalize_launch():
    lanes_per_cu, pairs, last = parse_normalize_launch(_body("normalize_launch"))
    assert lanes_per_cu == B.LANES_PER_CU
    assert tuple(pairs) == B.NORM_TABLE and last == 4
    assert [m for m, _ in pairs] == sorted((m for m, _ in pairs), reverse=True)           # first match = largest threshold
    for cus in (1, 64, 256, 304):
        lanes = cus * lanes_per_cu
        for (chunk, mult, off), n in zip(B.NORM_SPECS, B.norm_sizes(lanes)):
            want = next((c for m, c in pairs if n >= m * lanes), last)
            assert B.norm_chunk(n, lanes) == want == chunk, (cus, n)
        for chunk, mult, off in B.NORM_RAGGED:
            n = mult * lanes + off
            assert B.norm_chunk(n, lanes) == chunk and n % chunk, (cus, n)
    assert {c for c, _, _ in B.NORM_RAGGED} == {4, 16, 32, 64}


def test_parse_normalize_launch_sees_a_moved_threshold():
    """the parser reads the numbers, so a changed multiplier cannot pass as the old one"""
    body = _body("normalize_launch").replace("lanes_wanted * 32)", "lanes_wanted * 64)")
    assert tuple(parse_normalize_launch(body)[1]) != B.NORM_TABLE


def test_sum_fold_is_sum_reduce():
    body = _body("sum_reduce")
    assert int(re.search(r"constexpr int FOLD = (\d+);", body).group(1)) == B.SUM_FOLD
    assert "const size_t T = (m + FOLD - 1) / FOLD;" in body and "k_sum_pass<FOLD>" in body
    assert B.sum_passes(1048577) == [1048577, 32769, 1025, 33, 2]                         # five passes, ragged at every level
    assert all(m % B.SUM_FOLD for m in B.sum_passes(1048577))


# ------------------------------------------------------------------------------------------------------------- normaliser
def test_plant_positions_cover_the_groups():
    for n, chunk in ((70001, 4), (524297, 16), (1025, 4), (4194321, 32), (16777249, 64)):
        T = (n + chunk - 1) // chunk
        idx, kind, ext, groups = B.norm_plant(n, T, chunk, n)
        assert len(set(idx.tolist())) == len(idx) and idx.min() >= 0 and idx.max() < n
        lane = {t: sorted(int(i) // T for i in idx if i % T == t) for t in (0, 3, T // 3, T - 1)}
        assert lane[0] == sorted({0, chunk // 2, chunk - 1})
        assert lane[3] == list(range(chunk)) == lane[T // 3]
        assert 0 < len(lane[T - 1]) < chunk and lane[T - 1] == list(range(len(lane[T - 1])))     # the ragged lane, whole
        zero = np.array([B.norm_kinds[k][1] for k in kind])
        assert zero[idx % T == groups["all-zero"]].all()
        assert (~zero[idx % T == groups["one-nonzero"]]).sum() == 1
        assert set(kind.tolist()) == set(range(len(B.norm_kinds)))                        # every kind occurs


def test_oracle_and_bigint_agree_on_planted_rows():
    n, chunk = 70001, 4
    idx, kind, ext, _ = B.norm_plant(n, (n + chunk - 1) // chunk, chunk, 1)
    got = O.batch_normalize(ext)
    rows = [B.ext160_to_ints(r) for r in ext]
    _, want = J.batch_normalize([tuple(x % Q for x in r) for r in rows])
    for a, (r, w) in enumerate(zip(rows, want)):
        name, zero, _ = B.norm_kinds[kind[a]]
        assert to_pt(got[a]) == w, (name, a)
        assert zero == (r[2] % Q == 0) and (not zero or w == (0, 0)), (name, a)
    by_name = {B.norm_kinds[k][0]: rows[a] for a, k in enumerate(kind)}
    assert by_name["Z=q"][2] == Q and by_name["Z=q+1"][2] == Q + 1 and by_name["Z=q-1"][2] == Q - 1
    assert by_name["U+q,V+q"][0] >= Q and by_name["U+q,V+q"][1] >= Q
    assert by_name["all-ones"][:3] == (B.M256,) * 3
    for a, k in enumerate(kind):
        if B.norm_kinds[k][0] == "(0,z,z)":
            assert to_pt(got[a]) == J.AFFINE_IDENTITY
        if B.norm_kinds[k][0] == "(0,-z,z)":
            assert to_pt(got[a]) == (0, Q - 1)
    # one shared inversion on the oracle's side too: a row's answer does not depend on its neighbours
    for sub in (np.arange(0, len(ext), 3), np.arange(len(ext))[::-1], np.nonzero([B.norm_kinds[k][1] for k in kind])[0]):
        assert (O.batch_normalize(ext[sub]) == got[sub]).all()


# --------------------------------------------------------------------------------------------------------------- sum tree
def _bigint_sum(P):
    return J.ext_to_affine(J.ext_sum([J.affine_to_extended(to_pt(r)) for r in P]))


@pytest.mark.parametrize("layout", B.SUM_LAYOUTS)
def test_sum_layout_oracle_vs_bigint(layout):
    for n in B.sum_sizes:
        P = B.sum_layout(n, layout)
        assert P.shape == (n, 64)
        if n > 32769:
            continue
        got = to_pt(O.point_sum(P))
        assert got == _bigint_sum(P), (layout, n)
        if layout in ("to-identity", "all-identity"):
            assert got == J.AFFINE_IDENTITY, (layout, n)
        if layout == "same-point":
            assert got == J.scalar_mul_fast(to_pt(P[0]), n), (layout, n)


def test_sum_layout_plants_what_it_says():
    ident = pt64(J.AFFINE_IDENTITY)
    tors = {bytes(r) for r in B.torsion_points()}
    for n in (1025, 32769, 1048577):
        P = B.sum_layout(n, "planted")
        T = (n + 31) // 32
        for i in (0, n - 1, T - 1, T, 31 * T - 1, 31 * T):
            assert bytes(P[i]) in tors, (n, i)
        assert (P == ident).all(axis=1).sum() >= 2 * 64 // 9                              # 66 spots, two of every nine the identity
        i = T // 2
        assert (O.point_op("neg", P[i: i + 1]) == P[i + T]).all() and bytes(P[i]) not in tors    # lane i: P - P in rows 0 and 1
        assert to_pt(O.point_sum(P[[i, i + T]])) == J.AFFINE_IDENTITY


# ---------------------------------------------------------------------------------------------------------------- Fq root
def test_sqrt_patterns_are_real():
    pats = B.sqrt_patterns()
    assert len(pats) >= 1020 + 16 and len(set(pats)) == len(pats)
    for want in (0, 1, 1 << 31, (1 << 32) - 2, (1 << 32) - 1, 0x100, 0x00FF00FE):
        assert want in pats
    cases = B.sqrt_cases()
    assert [e for e, _, _ in cases] == list(pats)
    A, E = B.sqrt_inputs()
    out, ok = O.field_op(O.FQ, "sqrt", A)
    for k, (e, a, enc) in enumerate(cases):
        assert 0 < a < Q and pow(a, B.FQ_T, Q) == pow(B.FQ_G, e, Q), hex(e)
        x, xok = J.fq_sqrt(a)
        assert xok == ok[k] == (e % 2 == 0), hex(e)
        assert to_int(out[k]) == (x if xok else 0), hex(e)
        assert not xok or x * x % Q == a


def test_every_sqrt_pattern_reaches_the_decoder():
    cases = B.sqrt_cases()
    missing = [hex(e) for e, _, enc in cases if enc is None]
    assert not missing, "no encoding found for the logs %s" % missing
    A, E = B.sqrt_inputs()
    assert len(E) == len(cases)
    for flags in (0, 1):
        out, ok = O.decompress(E, flags)
        for k, (e, a, enc) in enumerate(cases):
            pt, pok = J.affine_from_bytes(bytes(b32(enc)), zip216=bool(flags))
            assert pok == ok[k] == (e % 2 == 0), (hex(e), flags)
            assert to_pt(out[k]) == pt, (hex(e), flags)
            if pok:
                assert pt[0] * pt[0] % Q == a and pt[1] == enc & ((1 << 255) - 1)           # the decoder took the root of exactly a
