"""The buffer-discipline row of jj_sigbatch_ragged (tests/buffer_cases.py holds the table and says what a row is): the call's regions carved into
guarded arenas at every size and skew, outputs equal to the oracle, guards and inputs untouched.  The row lives here, beside the entry point's
other cases, and joins buffer_cases.CASES when this module is imported (tests/test_sig_seg_cases_cpu.py and tests/test_gpu_sig_seg.py import it):
the table's coverage pin (tests/test_buffer_cases_cpu.py) then finds a row for the entry point, and tests/test_gpu_sig_seg.py runs the row through
the arenas with the runner of tests/test_gpu_buffers.py.  Test infrastructure only.

Segments of buffer_cases.ragged_lengths(S) signatures (empty ones at the front, in the middle and at the end) taken from tests/sig_batch_cases.py;
every seventh non-empty segment has a bad s or an off-curve R at its last position, so that the result rows hold the identity, other points and
the (0, -1) sentinel."""
import ctypes as C

import buffer_cases as BC  # by the name tests/test_buffer_cases_cpu.py and tests/test_gpu_buffers.py import it: one module, one table
import numpy as np

from tests import sig_batch_cases as SC

ROW_ID = "jj_sigbatch_ragged"


def parts(S):
    out, k = [], 0
    for L in BC.ragged_lengths(S):
        planted = L and k % 7 in (2, 5)
        out.append(SC.batch(L, ("bad_s", "off_curve_r")[k % 7 == 5], L - 1) if planted else SC.batch(L))
        k += 1 if L else 0
    return out


def build(S):
    ps = parts(S)
    cat = lambda f, w: np.concatenate([getattr(p, f) for p in ps]) if sum(p.n for p in ps) else np.zeros((0, w), np.uint8)      # noqa: E731
    return {"base": SC.bases()["prime"], "offsets": np.concatenate([[0], np.cumsum(BC.ragged_lengths(S))]).astype("<u8").view(np.uint8),
            "r": cat("r", 32), "a": cat("a", 32), "s": cat("s", 32), "c": cat("c", 32), "z": cat("z", 16)}


def oracle(i, S):
    return {"out": BC._rows(np.stack([p.expected for p in parts(S)]), 64) if S else np.zeros((0, 64), np.uint8)}


def row():
    """the row, added to the table on first use"""
    for c in BC.CASES:
        if c.id == ROW_ID:
            return c
    per_sig = lambda S: sum(BC.ragged_lengths(S))      # noqa: E731
    return BC._add("jj_sigbatch_ragged", [("base", 64), ("offsets", 8), ("r", 32), ("a", 32), ("s", 32), ("c", 32), ("z", 16)], [("out", 64)],
                   ["ctx", "base", "n", "offsets", "r", "a", "s", "c", "z", (C.c_uint, 0), "out"], build, oracle,
                   rows={"base": BC.ONE, "offsets": lambda S: S + 1, "r": per_sig, "a": per_sig, "s": per_sig, "c": per_sig, "z": per_sig}, host=("offsets",))


ROW = row()
