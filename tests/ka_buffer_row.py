"""The buffer-discipline rows of jj_ka_kdf and jj_chacha20_xor (tests/buffer_cases.py holds the table and says what a row is): the call's
regions carved into guarded arenas at every size and skew, the output bytes equal to the restatement of tests/ka_cases.py, guards and inputs
untouched.  The rows live here, beside the entry points' other cases, and join buffer_cases.CASES when this module is imported
(tests/test_ka_cases_cpu.py and tests/test_gpu_ka.py import it): the table's coverage pin (tests/test_buffer_cases_cpu.py) then finds a row
for each entry point, and tests/test_gpu_ka.py runs them through the arenas with the runner of tests/test_gpu_buffers.py.  Test infrastructure only.

jj_ka_kdf: regions sk (ONE row of 32 bytes, whatever n is) and p (32 bytes per unit: the planted encodings of tests/ka_cases.py repeated, the
ones that do not decode among them); outputs key (32 per unit) and ok (1 per unit).  The Sapling recipient's flags and personalisation.
jj_chacha20_xor: regions k (32 per unit) and c, rows of len = 52 bytes in a stride of 56: a row ends 4 bytes in front of the next, and the
bytes between belong to the input region, which must come back unchanged like the rest of it; the output is n x 52, dense.  Counter 1, the
nonce of RFC 8439's example.  Flags, personalisation, nonce and counter are no regions, so the rows make the calls themselves."""
import ctypes as C

import buffer_cases as BC  # by the name tests/test_buffer_cases_cpu.py and tests/test_gpu_buffers.py import it: one module, one table
import numpy as np

from tests import ka_cases as KC

SK = KC.SCALARS[-1]
FLAGS, PERSONAL = KC.SAPLING_FLAGS, KC.SAPLING_PERSONAL
LEN, STRIDE, COUNTER, NONCE = 52, 56, 1, KC.NONCE


def build_kdf(n):
    return {"sk": np.frombuffer(SK, dtype=np.uint8).reshape(1, 32), "p": KC.tiled(n, shift=n)}


def oracle_kdf(i, n):
    keys, ok = KC.expected(bytes(i["sk"][0]), i["p"], FLAGS, PERSONAL)
    return {"key": keys, "ok": ok.reshape(-1, 1)}


def call_kdf(run, lib, ctx, env):
    return lib.jj_ka_kdf(ctx, C.c_size_t(run.n), C.c_void_p(run.ptr("sk")), C.c_void_p(run.ptr("p")), C.c_uint(FLAGS), PERSONAL, C.c_void_p(run.ptr("key")),
                         C.c_void_p(run.ptr("ok")))


def build_cipher(n):
    return {"k": KC.rng_bytes(8300 + n, n, 32), "c": KC.rng_bytes(8400 + n, n, STRIDE)}


def oracle_cipher(i, n):
    return {"out": KC.chacha20_xor(i["k"], i["c"], LEN, NONCE, COUNTER).reshape(-1, 4)}


def call_cipher(run, lib, ctx, env):
    return lib.jj_chacha20_xor(ctx, C.c_size_t(run.n), C.c_void_p(run.ptr("k")), NONCE, C.c_uint(COUNTER), C.c_void_p(run.ptr("c")), C.c_size_t(LEN), C.c_size_t(STRIDE),
                               C.c_void_p(run.ptr("out")))


def rows():
    """the two rows, added to the table on first use"""
    have = {c.id: c for c in BC.CASES}
    if "jj_ka_kdf" not in have:
        BC._add("jj_ka_kdf", [("sk", 32), ("p", 32)], [("key", 32), ("ok", 1)], [], build_kdf, oracle_kdf, call=call_kdf, rows={"sk": BC.ONE})
        # the output is declared as 13 n rows of 4 bytes, the dwords the kernel stores: the table's pin of the output widths stays as it is
        BC._add("jj_chacha20_xor", [("k", 32), ("c", STRIDE)], [("out", 4)], [], build_cipher, oracle_cipher, call=call_cipher, rows={"out": lambda n: n * (LEN // 4)})
        have = {c.id: c for c in BC.CASES}
    return have["jj_ka_kdf"], have["jj_chacha20_xor"]


ROW_KDF, ROW_CIPHER = rows()
