"""Machine-checks the lazy-reduction bounds of the Montgomery-form ladder (jubjub_amd/csrc/jj_mont.h, tools/bounds_check.py check_mont_ladder)."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import bounds_check  # noqa: E402


def test_mont_ladder_bounds():
    st, x1, res = bounds_check.check_mont_ladder(verbose=False)
    for v in (st, x1, res):
        assert v.vlo > -2 * bounds_check.Q and v.vhi < bounds_check.Q


def test_squared_sums_need_their_carry():
    """without the carry step the squares of x2 + z2 and DA + CB could overflow a column accumulator: the checker must say so"""
    st, _, _ = bounds_check.check_mont_ladder(verbose=False)
    F = bounds_check.FieldModel(bounds_check.Q)
    try:
        F.sqr(F.add(st, st), "uncarried")
    except AssertionError:
        return
    raise AssertionError("the square of an uncarried sum passed the checker")
