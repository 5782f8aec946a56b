"""The buffer-discipline rows of jj_blake2b and jj_ka_kdf_each (tests/buffer_cases.py holds the table and says what a row is): the call's regions
carved into guarded arenas at every size and skew, the output bytes equal to the restatement of tests/ovk_cases.py, guards and inputs
untouched.  The rows join buffer_cases.CASES when this module is imported (tests/test_ovk_cases_cpu.py and tests/test_gpu_ovk_buffers.py import
it): the table's coverage pin (tests/test_buffer_cases_cpu.py) then finds a row for each entry point, and tests/test_gpu_ovk_buffers.py runs
them through the arenas with the runner of tests/test_gpu_buffers.py.  Test infrastructure only.

jj_blake2b: three source regions a, b, c in rows of 36, 32 and 44 bytes of which 32, 32 and 40 are hashed -- the bytes between two rows of a
and of c belong to the input regions and must come back unchanged, and the last row of a and of c ends 4 bytes in front of the guard, which a
dword read past a row's len would enter --, a 32-byte prefix and a personalisation: the ock shape with one longer source, 136 bytes, two
blocks.  The output is n x 32, dense.
jj_ka_kdf_each: regions sk (32 bytes per unit: ka_cases' planted scalars, one per row), p (the planted encodings, the ones that do not decode
among them) and h (32 bytes per unit); outputs key and ok.  The Sapling flags and personalisation.
Prefix, personalisation, flags and the host arrays (srcs, lens, strides) are no regions, so the rows make the calls themselves."""
import ctypes as C

import buffer_cases as BC  # by the name tests/test_buffer_cases_cpu.py and tests/test_gpu_buffers.py import it: one module, one table

from tests import ka_cases as KC
from tests import ovk_cases as OC

STRIDES = {"a": 36, "b": 32, "c": 44}
LENS = {"a": 32, "b": 32, "c": 40}
DIGEST = 32
PREFIX = KC.rng_bytes(8350, 32).tobytes()
PERSONAL = OC.SAPLING_OCK_PERSONAL
FLAGS, KDF_PERSONAL = KC.SAPLING_FLAGS, KC.SAPLING_PERSONAL


def build_b2b(n):
    return {k: KC.rng_bytes(8360 + 3 * n + j, n, w) for j, (k, w) in enumerate(STRIDES.items())}


def oracle_b2b(i, n):
    return {"out": OC.digests([i[k][:, :LENS[k]] for k in "abc"], n, DIGEST, PERSONAL, PREFIX)}


def call_b2b(run, lib, ctx, env):
    srcs = (C.c_void_p * 3)(*[run.ptr(k) for k in "abc"])
    lens = (C.c_size_t * 3)(*[LENS[k] for k in "abc"])
    strides = (C.c_size_t * 3)(*[STRIDES[k] for k in "abc"])
    return lib.jj_blake2b(ctx, C.c_size_t(run.n), C.c_int(DIGEST), PERSONAL, PREFIX, C.c_size_t(len(PREFIX)), C.c_int(3), srcs, lens, strides, C.c_void_p(run.ptr("out")))


def build_each(n):
    sks, encs = OC.ka_grid(n, shift=n)
    return {"sk": sks, "p": encs, "h": OC.hash_rows(n, seed=n)}


def oracle_each(i, n):
    keys, ok = OC.ka_each(i["sk"], i["p"], FLAGS, KDF_PERSONAL, i["h"])
    return {"key": keys, "ok": ok.reshape(-1, 1)}


def call_each(run, lib, ctx, env):
    return lib.jj_ka_kdf_each(ctx, C.c_size_t(run.n), C.c_void_p(run.ptr("sk")), C.c_void_p(run.ptr("p")), C.c_void_p(run.ptr("h")), C.c_uint(FLAGS), KDF_PERSONAL,
                              C.c_void_p(run.ptr("key")), C.c_void_p(run.ptr("ok")))


def rows():
    """the two rows, added to the table on first use"""
    have = {c.id: c for c in BC.CASES}
    if "jj_blake2b" not in have:
        BC._add("jj_blake2b", [(k, w) for k, w in STRIDES.items()], [("out", DIGEST)], [], build_b2b, oracle_b2b, call=call_b2b)
        BC._add("jj_ka_kdf_each", [("sk", 32), ("p", 32), ("h", 32)], [("key", 32), ("ok", 1)], [], build_each, oracle_each, call=call_each)
        have = {c.id: c for c in BC.CASES}
    return have["jj_blake2b"], have["jj_ka_kdf_each"]


ROW_B2B, ROW_EACH = rows()
