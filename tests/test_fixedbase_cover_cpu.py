"""
CPU checks of tests/fixedbase_cover.py, the plain model of the fixed-base recodings that tests/test_gpu_fixedbase_matrix.py runs on the GPU:
every model gives back the integer it recodes, every cover set selects every reachable table entry of its kernel, and the composite
partition rule matches the cases the GPU test expects to be accepted or refused.  No GPU and no native library of the package.
"""
import os
import random
import re
import sys

import pytest

import fixedbase_cover as C
from util import EDGE_SCALARS, rand_scalars, to_int

M252 = (1 << 252) - 1
KINDS = [("comb", None), ("lds6", None)] + [("gather", w) for w in C.GATHER_WIDTHS]


def _sample_scalars():
    rnd = random.Random(2024)
    full = [to_int(r) for r in rand_scalars(5, 300, full_width=True)]
    below = [to_int(r) for r in rand_scalars(6, 300)]
    return list(EDGE_SCALARS) + full + below + [rnd.getrandbits(256) for _ in range(100)]


@pytest.mark.parametrize("kind,w", KINDS, ids=[k if w is None else "%s%d" % (k, w) for k, w in KINDS])
def test_model_gives_back_the_integer(kind, w):
    for k in _sample_scalars() + C.cover_scalars(kind, w)[::97]:
        e = C.entries_of(kind, k, w)
        if kind == "comb":
            assert len(e) == C.K["FBC_SPACING"]
            assert C.comb_value(e) == k & M252, hex(k)
            continue
        ww = w if kind == "gather" else C.K["FB_W"]
        assert C.window_value(e, ww) == k & M252, hex(k)
        E = C.gather_layout(w)[1] if kind == "gather" else C.K["FB_ENT"] - 1
        assert all(0 <= j <= E and s in (1, -1) and (j or s == 1) for _, j, s in e)
        assert all(j < E or s == -1 for i, j, s in e[:-1])     # a signed digit is in [-E, E - 1]


def test_comb_even_scalars_take_the_extra_tables():
    blocks = C.K["FBC_BLOCKS"]
    for k in _sample_scalars():
        col0 = C.comb_digits(k)[0]
        if k & 1:
            assert col0[1] == 0
        else:
            assert col0[1] == (blocks if col0[3] > 0 else blocks + 1)
        assert C.comb_entry_value(blocks, 5) == C.comb_entry_value(0, 5) - 1
        assert C.comb_entry_value(blocks + 1, 5) == C.comb_entry_value(0, 5) + 1


def test_lds6_recoding_constant_matches_the_kernel():
    nwin, E, recode, top = C.lds6_layout()
    assert recode == C.recode6_words()
    assert (nwin, E, top) == (42, 32, 252)
    assert C.K["FB_ENTRIES"] == nwin * C.K["FB_ENT"] + 1


def test_window_counts_match_the_library():
    text = open(os.path.join(C.CSRC, "jj_abi.hip")).read()
    assert re.search(r"fp\.W\s*=\s*\(253\s*\+\s*window_bits\s*-\s*1\)\s*/\s*window_bits", text)
    for w in C.GATHER_WIDTHS:
        W, E, recode = C.gather_layout(w)
        assert W == -(-253 // w) and w * W >= 253 and w * (W - 1) <= 252, w
        assert E == 1 << (w - 1)
        assert recode == sum(1 << (w * i + w - 1) for i in range(W - 1))


@pytest.mark.parametrize("kind,w", KINDS, ids=[k if w is None else "%s%d" % (k, w) for k, w in KINDS])
def test_cover_set_selects_every_reachable_entry(kind, w):
    scalars = C.cover_scalars(kind, w)
    assert all(0 <= k <= M252 for k in scalars)
    reach, got = C.reachable(kind, w), C.covered(kind, w)
    assert got <= reach, sorted(got - reach)[:5]              # the model never selects an entry the constraints rule out
    assert reach <= got, sorted(reach - got)[:5]
    # not larger than it must be: a signed window (a comb column) holds 2^w (2^8) pairs (index, sign) and one scalar selects one
    # of them, plus the top values the main set misses
    per = 2 << C.K["FBC_TEETH"] if kind == "comb" else 1 << (w or C.K["FB_W"])
    assert len(scalars) <= per + (C.top_digit_max(kind, w) + 1 if kind != "comb" else 0)


def test_reachable_extremes():
    for w in C.GATHER_WIDTHS:
        W, E, _ = C.gather_layout(w)
        reach = C.reachable("gather", w)
        top = C.top_digit_max("gather", w)
        assert top <= E, w                                           # the top digit never runs past the last entry of its window
        assert top == ((1 << 252) - 1 + C.gather_layout(w)[2]) >> (w * (W - 1))
        for i in range(W - 1):
            assert {(i, 0, 1), (i, E, -1), (i, E - 1, 1), (i, E - 1, -1), (i, 1, 1), (i, 1, -1)} <= reach, (w, i)
            assert (i, E, 1) not in reach and (i, 0, -1) not in reach
    assert C.top_digit_max("gather", 11) == C.gather_layout(11)[1]    # 11 divides 253: the top digit reaches E exactly
    assert C.top_digit_max("gather", 9) == 1                          # top window of one bit at bit 252 (Q = 2 * 2^251 B)
    assert C.top_digit_max("lds6") == 1
    assert len([e for e in C.reachable("comb") if e[1] >= C.K["FBC_BLOCKS"]]) == 2 * C.K["FBC_TENT"]
    tables = {(t, s) for _, t, _, s in C.reachable("comb")}
    blocks = C.K["FBC_BLOCKS"]
    assert tables == {(t, s) for t in range(blocks) for s in (1, -1)} | {(blocks, 1), (blocks + 1, -1)}


def test_coverage_report_lists_every_kind():
    rep = C.coverage_report()
    assert "MISSING" not in rep
    assert len(rep.splitlines()) == 1 + 2 + len(C.GATHER_WIDTHS)
    for line in rep.splitlines()[1:]:
        f = line.split()
        assert f[3] == f[4], line


@pytest.mark.parametrize("bits,ok,why", C.composite_cases(), ids=[c[2] for c in C.composite_cases()])
def test_composite_rule_and_packing(bits, ok, why):
    off = C.composite_slots(bits)
    assert (off is not None) == ok, why
    if not ok:
        return
    nwin, E, _, _ = C.lds6_layout()
    vals = [C.composite_field_values(b) for b in bits]
    for b, v in zip(bits, vals):
        assert 0 in v and (1 << b) - 1 in v and (1 << (b - 1)) in v, b
    slots = [-(-(b + 2) // C.K["FB_W"]) for b in bits]
    rows = max(len(v) for v in vals)
    for r in range(rows):
        field = [v[(r + j) % len(v)] for j, v in enumerate(vals)]
        garbage = [f | (random.Random(r * 31 + j).getrandbits(256) >> b << b) for j, (f, b) in enumerate(zip(field, bits))]
        virt = C.pack_composite(garbage, bits)
        assert virt < 1 << 250
        d = C.lds6_digits(virt)
        assert d[nwin] == (nwin, 0, 1)                                # no carry out of the last field
        for j, (o, s) in enumerate(zip(off, slots)):                  # each field's digits give back the field: no carry between fields
            assert C.window_value([(i - o, jj, sg) for i, jj, sg in d[o:o + s]], C.K["FB_W"]) == field[j], (why, j)
        assert all(d[i][1] == 0 for i in range(off[-1] + slots[-1], nwin))
    # the field values put digit -32, digit 31 and 0 into each window of the field below its top wherever a field value can
    for b, v in zip(bits, vals):
        s = -(-(b + 2) // C.K["FB_W"])
        seen = {(i, jj, sg) for x in v for i, jj, sg in C.lds6_digits(x)[:s - 1]}
        want = {(i, jj, sg) for i in range(s - 1) for jj, sg in ((E, -1), (E - 1, 1), (0, 1))}
        if b <= 16:
            want &= {(i, jj, sg) for x in range(1 << b) for i, jj, sg in C.lds6_digits(x)[:s - 1]}
        assert want <= seen, (b, sorted(want - seen))


def test_module_imports_no_native_library():
    assert "jubjub_amd._lib" not in sys.modules or not hasattr(C, "_lib")
    src = open(C.__file__).read()
    assert "jubjub_amd" not in re.sub(r'"""[\s\S]*?"""', "", src).replace("jubjub_amd\", \"csrc", "")
