"""The buffer-discipline rows of jj_blake2s and jj_group_hash (tests/buffer_cases.py holds the table and says what a row is): the call's
regions carved into guarded arenas at every size and skew, the output bytes equal to the restatement of tests/group_hash_cases.py, guards and
inputs untouched.  The rows live here, beside the entry points' other cases, and join buffer_cases.CASES when this module is imported
(tests/test_group_hash_cases_cpu.py and tests/test_gpu_group_hash.py import it): the table's coverage pin (tests/test_buffer_cases_cpu.py) then
finds a row for each entry point, and tests/test_gpu_group_hash.py runs them through the arenas with the runner of tests/test_gpu_buffers.py.
Test infrastructure only.

Both rows: one input region m, message rows of 11 bytes in a stride of 12 -- a row ends one byte in front of the next, every row starts at
another address residue mod 4, the last row's twelfth byte is the region's last byte and is never read, and all of it must come back
unchanged --, behind a 64-byte prefix (one whole block for the host's midstate, no tail).  jj_blake2s writes out (32 per unit); jj_group_hash
writes pt (64 per unit) and ok (1 per unit) under the flags of the group hash of the Zcash specification.  Personalisation, prefix, lengths
and flags are no regions, so the rows make the calls themselves."""
import ctypes as C

import buffer_cases as BC  # by the name tests/test_buffer_cases_cpu.py and tests/test_gpu_buffers.py import it: one module, one table
import numpy as np

from tests import group_hash_cases as GC

LEN, STRIDE = 11, 12
PERSONAL, PREFIX, FLAGS = b"JJ_gh_br", GC.PREFIX_POOL[:64], GC.SAPLING_SHAPED


POOL = GC.KC.rng_bytes(9300, 128, STRIDE)           # 128 distinct rows, repeated: the restatement decodes each digest once


def build(n):
    return {"m": np.ascontiguousarray(POOL[(np.arange(n) + n) % len(POOL)])}


def oracle_hash(i, n):
    return {"out": GC.digests(PERSONAL, PREFIX, i["m"][:, :LEN])}


def oracle_group(i, n):
    pts, ok = GC.expected(PERSONAL, PREFIX, i["m"][:, :LEN], FLAGS)
    return {"pt": pts, "ok": ok.reshape(-1, 1)}


def call_hash(run, lib, ctx, env):
    return lib.jj_blake2s(ctx, C.c_size_t(run.n), PERSONAL, PREFIX, C.c_size_t(len(PREFIX)), C.c_void_p(run.ptr("m")), C.c_size_t(LEN), C.c_size_t(STRIDE), C.c_void_p(run.ptr("out")))


def call_group(run, lib, ctx, env):
    return lib.jj_group_hash(ctx, C.c_size_t(run.n), PERSONAL, PREFIX, C.c_size_t(len(PREFIX)), C.c_void_p(run.ptr("m")), C.c_size_t(LEN), C.c_size_t(STRIDE), C.c_uint(FLAGS),
                             C.c_void_p(run.ptr("pt")), C.c_void_p(run.ptr("ok")))


def rows():
    """the two rows, added to the table on first use"""
    have = {c.id: c for c in BC.CASES}
    if "jj_blake2s" not in have:
        BC._add("jj_blake2s", [("m", STRIDE)], [("out", 32)], [], build, oracle_hash, call=call_hash)
        BC._add("jj_group_hash", [("m", STRIDE)], [("pt", 64), ("ok", 1)], [], build, oracle_group, call=call_group)
        have = {c.id: c for c in BC.CASES}
    return have["jj_blake2s"], have["jj_group_hash"]


ROW_HASH, ROW_GROUP = rows()
