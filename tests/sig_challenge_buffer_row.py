"""The buffer-discipline row of jj_sig_challenge (tests/buffer_cases.py holds the table and says what a row is): the call's regions carved into
guarded arenas at every size and skew, the n x 32 challenge bytes equal to the oracle, guards and inputs untouched.  The row lives here, beside
the entry point's other cases, and joins buffer_cases.CASES when this module is imported (tests/test_sig_challenge_cases_cpu.py and
tests/test_gpu_sig_challenge.py import it): the table's coverage pin (tests/test_buffer_cases_cpu.py) then finds a row for the entry point, and
tests/test_gpu_sig_challenge.py runs the row through the arenas with the runner of tests/test_gpu_buffers.py.  Test infrastructure only.

Regions r, a (32 bytes per unit) and m with a fixed msg_len of 33 -- odd on purpose: the messages start at every residue modulo 4 and the m
region ends in the middle of a dword, directly in front of its guard --; the output is c, 32 bytes per unit.  The personalisation (host memory,
RedJubjub's) and the NULL offsets are no regions, so the row makes the call itself."""
import ctypes as C

import buffer_cases as BC  # by the name tests/test_buffer_cases_cpu.py and tests/test_gpu_buffers.py import it: one module, one table
import numpy as np

from tests import sig_challenge_cases as CC

ROW_ID = "jj_sig_challenge"
MSG_LEN = 33
PERSONAL = CC.REDJUBJUB


def build(n):
    R, A = CC.parts(n, "both", seed=77)
    return {"r": R, "a": A, "m": CC.fixed(n, MSG_LEN, seed=77)}


def oracle(i, n):
    if n == 0:
        return {"c": np.zeros((0, 32), np.uint8)}
    return {"c": BC._memo("sig_challenge", (i["r"], i["a"], i["m"]), lambda: CC.expected(PERSONAL, i["r"], i["a"], [bytes(x) for x in i["m"]]))}


def call(run, lib, ctx, env):
    return lib.jj_sig_challenge(ctx, C.c_size_t(run.n), PERSONAL, C.c_void_p(run.ptr("r")), C.c_void_p(run.ptr("a")), C.c_void_p(run.ptr("m")), C.c_size_t(MSG_LEN), None,
                                C.c_void_p(run.ptr("c")))


def row():
    """the row, added to the table on first use"""
    for c in BC.CASES:
        if c.id == ROW_ID:
            return c
    return BC._add("jj_sig_challenge", [("r", 32), ("a", 32), ("m", MSG_LEN)], [("c", 32)],
                   ["ctx", "n", (C.c_void_p, None), "r", "a", "m", (C.c_size_t, MSG_LEN), (C.c_void_p, None), "c"], build, oracle, call=call)


ROW = row()
