"""The buffer-discipline row of jj_sigverify_each (tests/buffer_cases.py holds the table and says what a row is): the call's regions carved into
guarded arenas at every size and skew, the n verdict bytes equal to the oracle, guards and inputs untouched.  The row lives here, beside the entry
point's other cases, and joins buffer_cases.CASES when this module is imported (tests/test_sig_each_cases_cpu.py and
tests/test_gpu_sigverify_each.py import it): the table's coverage pin (tests/test_buffer_cases_cpu.py) then finds a row for the entry point, and
tests/test_gpu_sigverify_each.py runs the row through the arenas with the runner of tests/test_gpu_buffers.py.  Test infrastructure only.

Valid signatures of tests/sig_each_cases.py over the table's base (buffer_cases.fixed_base(0), the generator: order 8r, so the cofactored mode
the row runs accepts them all); every seventh unit has a bad s, every seventh an off-curve R, so that the verdict bytes hold all three values.
Both ladders: the default engine (the quad ladder at these sizes) and vb_quad_max = 0 (k_varbase_fixed on the gathered table)."""
import ctypes as C

import buffer_cases as BC  # by the name tests/test_buffer_cases_cpu.py and tests/test_gpu_buffers.py import it: one module, one table
import numpy as np

from tests import sig_batch_cases as SC
from tests import sig_each_cases as EC

ROW_ID = "jj_sigverify_each"
TABLE_BITS = 8


def build(n):
    r, a, s, c, _, _, _ = EC.valid(n, "order8r")
    for k in range(2, n, 7):
        s[k] = SC.b32((SC.to_int(s[k]) + 5) % SC.R)
    for k in range(5, n, 7):
        r[k] = SC.off_curve_encoding()
    return {"r": r, "a": a, "s": s, "c": c}


def oracle(i, n):
    if n == 0:
        return {"verdict": np.zeros((0, 1), np.uint8)}
    b = EC.Batch("row", "order8r", i["r"], i["a"], i["s"], i["c"], 0, None, None, [])
    return {"verdict": BC._memo("sig_each", (i["r"], i["a"], i["s"], i["c"]), lambda: EC.full_evaluation(b, True)).reshape(n, 1)}


def row():
    """the row, added to the table on first use"""
    assert np.array_equal(BC.fixed_base(0), SC.bases()["order8r"])
    for c in BC.CASES:
        if c.id == ROW_ID:
            return c
    return BC._add("jj_sigverify_each", [("r", 32), ("a", 32), ("s", 32), ("c", 32)], [("verdict", 1)],
                   ["ctx", ("handle", ("table", 0, TABLE_BITS)), "n", "r", "a", "s", "c", (C.c_uint, 0), "verdict"], build, oracle,
                   options=({}, {"vb_quad_max": 0}))


ROW = row()
