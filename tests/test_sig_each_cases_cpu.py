"""Every expected verdict byte of tests/sig_each_cases.py, held to the oracle's term-by-term evaluation (decode, its fixed-base and variable-base
ladders, its point subtraction, its cofactor operation, its identity test) in both modes at n in {1, 65, 300}; the two modes must differ
exactly on the units with a torsion component.  No GPU."""
import numpy as np
import pytest

from oracle import c_oracle as O
from tests import sig_batch_cases as SC
from tests import sig_each_buffer_row as BR  # joins buffer_cases.CASES at collection, before the table's coverage pin runs
from tests import sig_each_cases as EC

SIZES = (1, 65, 300)


def test_constants_and_building_blocks():
    assert (EC.REJECT, EC.OK, EC.MALFORMED, EC.COFACTORLESS) == (0, 1, 2, 16)
    assert O.predicate("is_small_order", SC.T8[None])[0] and not O.predicate("is_identity", O.point_op("double", O.point_op("double", SC.T8[None])))[0]      # T8 has order 8
    assert O.predicate("is_prime_order", SC.bases()["prime"][None])[0]
    names = [k for k, _, _ in EC.KINDS]
    assert len(set(names)) == len(names) and abs(names.index("noncanonical_a") - names.index("noncanonical_a_zip216")) >= 5
    assert EC.TORSION_KINDS == {"torsion_r", "torsion_a_odd_c", "r_order2"}


@pytest.mark.parametrize("n", SIZES)
def test_every_expected_byte_is_the_oracles(n):
    kinds_seen = set()
    for b in EC.batches(n):
        assert b.n == n
        for cofactored in (True, False):
            got = EC.full_evaluation(b, cofactored)
            bad = np.nonzero(got != b.expect[cofactored])[0]
            assert not len(bad), "%s %s: unit %d expected %d, the oracle gives %d (planted %r)" % (
                b.name, "cofactored" if cofactored else "cofactorless", bad[0], b.expect[cofactored][bad[0]], got[bad[0]], b.planted)
        kinds_seen |= {k for _, k in b.planted}
    assert kinds_seen == {k for k, _, _ in EC.KINDS}


@pytest.mark.parametrize("n", SIZES)
def test_modes_differ_exactly_on_the_torsion_units(n):
    for b in EC.batches(n):
        want = np.zeros(n, bool)
        for k, kind in b.planted:
            want[k] = kind in EC.TORSION_KINDS
        if b.base_name == "order8r":
            # [s]G - [c]A - R = [-w r]G with w the wrap of k + c sk: a torsion component unless 8 | w
            sB = O.fixedbase_mul(b.s, b.base)
            cA = O.varbase_mul(b.c, O.decompress(b.a, 0)[0])
            d = O.point_op("sub", O.point_op("sub", sB, cA), O.decompress(b.r, 0)[0])
            want = O.predicate("is_identity", d) == 0
            assert O.predicate("is_small_order", d).all()
        assert np.array_equal(b.torsion, want), b.name
        assert ((b.expect[True] == EC.MALFORMED) == (b.expect[False] == EC.MALFORMED)).all()


def test_whole_batches():
    bs = {b.name.split(" ", 1)[1]: b for b in EC.batches(65)}
    assert (bs["all_fail"].expect[True] == EC.REJECT).all() and (bs["all_fail"].expect[False] == EC.REJECT).all()
    assert (bs["all_malformed"].expect[True] == EC.MALFORMED).all()
    assert (bs["valid"].expect[True] == EC.OK).all() and (bs["valid"].expect[False] == EC.OK).all()
    assert bs["valid"].failing() == [] and len(bs["all_fail"].failing()) == 65 and bs["all_malformed"].failing()[0] == (0, "malformed")


def test_large_batch_is_the_pool_repeated():
    """the closed forms of the large sizes: a batch beyond the pool repeats it (held to the oracle on the units around the planted ones and on
    one period), with every kind but one planted and a few dozen failing units at most"""
    n = 3 * EC.POOL + 77
    b = EC.large_batch(n)
    assert {k for _, k in b.planted} == {k for k, _, _ in EC.KINDS} - {"noncanonical_a"}
    assert 0 < len(b.failing()) <= 48
    idx = sorted({min(n - 1, max(0, k + d)) for k, _ in b.planted for d in (-1, 0, 1)} | set(range(EC.POOL, EC.POOL + 40)))
    sub = EC.Batch("sub", b.base_name, b.r[idx], b.a[idx], b.s[idx], b.c[idx], b.flags, b.expect[True][idx], b.expect[False][idx], [])
    for cofactored in (True, False):
        assert np.array_equal(EC.full_evaluation(sub, cofactored), sub.expect[cofactored])


def test_buffer_row_joins_the_table_and_holds_every_verdict():
    """tests/sig_each_buffer_row.py: imported by this module so that the table's coverage pin finds the row in a run without a GPU; its expected bytes are
    the oracle's evaluation and hold all three values"""
    import buffer_cases as BC

    assert BR.ROW in BC.CASES and BR.ROW.covers == ("jj_sigverify_each",)
    ins, outs = BR.ROW.data(65)
    v = outs["verdict"].reshape(-1)
    assert set(v.tolist()) == {EC.REJECT, EC.OK, EC.MALFORMED} and v[2] == EC.REJECT and v[5] == EC.MALFORMED and v[0] == EC.OK
    assert BR.ROW.data(0)[1]["verdict"].size == 0
