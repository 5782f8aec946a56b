"""The buffer-discipline rows of jj_poly1305, jj_aead_seal and jj_aead_open (tests/buffer_cases.py holds the table and says what a row is): the
call's regions carved into guarded arenas at every size and skew, the output bytes equal to the restatement of tests/aead_cases.py, guards and
inputs untouched.  The rows live here, beside the entry points' other cases, and join buffer_cases.CASES when this module is imported
(tests/test_aead_cases_cpu.py and tests/test_gpu_aead.py import it): the table's coverage pin (tests/test_buffer_cases_cpu.py) then finds a row
for each entry point, and tests/test_gpu_aead.py runs them through the arenas with the runner of tests/test_gpu_buffers.py.  Test
infrastructure only.

jj_poly1305 and jj_aead_seal: regions k (32 per unit) and c, rows of len = 52 bytes in a stride of 56: a row ends 4 bytes in front of the
next, and the bytes between belong to the input region, which must come back unchanged like the rest of it.  Outputs: n x 16 tags; n x 68 of
ciphertext and tag, dense.
jj_aead_open: rows of 52 ciphertext bytes and the 16 tag bytes in a stride of 72; every third row is tampered (the entries of
aead_cases.tamper_list in turn), so both verdicts and the zero rows are compared byte for byte; outputs n x 52 and n verdict bytes.
Nonce, aad and the lengths are no regions, so the rows make the calls themselves."""
import ctypes as C

import buffer_cases as BC  # by the name tests/test_buffer_cases_cpu.py and tests/test_gpu_buffers.py import it: one module, one table
import numpy as np

from tests import aead_cases as AC
from tests import ka_cases as KC

LEN, STRIDE, OPEN_STRIDE, NONCE, AAD = 52, 56, 72, AC.NONCE, bytes.fromhex("50515253c0c1c2c3c4c5c6c7")


def build_rows(n):
    return {"k": AC.pool_keys(n, 7, 11300 + n), "c": KC.rng_bytes(11400 + n, n, STRIDE)}


def oracle_mac(i, n):
    return {"tag": AC.mac_rows(i["k"], i["c"], LEN).reshape(-1, 4)}


def call_mac(run, lib, ctx, env):
    return lib.jj_poly1305(ctx, C.c_size_t(run.n), C.c_void_p(run.ptr("k")), C.c_void_p(run.ptr("c")), C.c_size_t(LEN), C.c_size_t(STRIDE), C.c_void_p(run.ptr("tag")))


def oracle_seal(i, n):
    return {"out": AC.seal_rows(i["k"], i["c"], LEN, NONCE, AAD).reshape(-1, 4)}


def call_seal(run, lib, ctx, env):
    return lib.jj_aead_seal(ctx, C.c_size_t(run.n), C.c_void_p(run.ptr("k")), NONCE, AAD, C.c_size_t(len(AAD)), C.c_void_p(run.ptr("c")), C.c_size_t(LEN), C.c_size_t(STRIDE),
                            C.c_void_p(run.ptr("out")))


def build_open(n):
    keys = AC.pool_keys(n, 7, 11500 + n)
    rows = KC.rng_bytes(11600 + n, n, OPEN_STRIDE)                                # the four bytes behind each tag stay random
    rows[:, :LEN + 16] = AC.seal_rows(keys, KC.rng_bytes(11700 + n, n, LEN), LEN, NONCE, AAD)
    keys, rows, _ = AC.tamper(keys, rows, LEN, range(1, n, 3))
    return {"k": keys, "c": rows}


def oracle_open(i, n):
    plain, ok = AC.open_rows(i["k"], i["c"], LEN, NONCE, AAD)
    assert n < 3 or (0 < int(ok.sum()) < n and not plain[ok == 0].any())           # both verdicts among the rows
    return {"out": plain.reshape(-1, 4), "ok": ok.reshape(-1, 1)}


def call_open(run, lib, ctx, env):
    return lib.jj_aead_open(ctx, C.c_size_t(run.n), C.c_void_p(run.ptr("k")), NONCE, AAD, C.c_size_t(len(AAD)), C.c_void_p(run.ptr("c")), C.c_size_t(LEN), C.c_size_t(OPEN_STRIDE),
                            C.c_void_p(run.ptr("out")), C.c_void_p(run.ptr("ok")))


def rows():
    """the three rows, added to the table on first use"""
    have = {c.id: c for c in BC.CASES}
    if "jj_poly1305" not in have:
        # the dense outputs are declared as rows of 4 bytes, the dwords the kernels store: the table's pin of the output widths stays as it is
        BC._add("jj_poly1305", [("k", 32), ("c", STRIDE)], [("tag", 4)], [], build_rows, oracle_mac, call=call_mac, rows={"tag": lambda n: 4 * n})
        BC._add("jj_aead_seal", [("k", 32), ("c", STRIDE)], [("out", 4)], [], build_rows, oracle_seal, call=call_seal, rows={"out": lambda n: n * ((LEN + 16) // 4)})
        BC._add("jj_aead_open", [("k", 32), ("c", OPEN_STRIDE)], [("out", 4), ("ok", 1)], [], build_open, oracle_open, call=call_open, rows={"out": lambda n: n * (LEN // 4)})
        have = {c.id: c for c in BC.CASES}
    return have["jj_poly1305"], have["jj_aead_seal"], have["jj_aead_open"]


ROW_MAC, ROW_SEAL, ROW_OPEN = rows()
