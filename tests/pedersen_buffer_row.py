"""The buffer-discipline rows of jj_pedersen_hash_vartime and jj_pedersen_scalars (tests/buffer_cases.py holds the table and says what a row
is): the call's regions carved into guarded arenas at every size and skew, the output bytes equal to the restatement of
tests/pedersen_cases.py, guards and inputs untouched.  The rows live here, beside the entry points' other cases, and join buffer_cases.CASES when
this module is imported (tests/test_pedersen_cases_cpu.py and tests/test_gpu_pedersen.py import it): the table's coverage pin
(tests/test_buffer_cases_cpu.py) then finds a row for each entry point, and tests/test_gpu_pedersen.py runs them through the arenas with the
runner of tests/test_gpu_buffers.py.  Test infrastructure only.

One region m of 9 bytes per unit, read as one field of 61 bits from byte 1 behind a 2-bit prefix: the rows start at every residue modulo 4
and the region ends in the middle of a dword, directly in front of its guard.  Three segments of 7 chunks (63 bits: the message is exactly
at capacity) keep the oracle's scalars short at the table's 1025 units.  The hash row writes n x 32 bytes (the u-coordinates); the scalars row
writes (3, n, 32).  The table handle, the prefix and the host array of fields are no regions, so the rows make the calls themselves."""
import ctypes as C

import buffer_cases as BC  # by the name tests/test_buffer_cases_cpu.py and tests/test_gpu_buffers.py import it: one module, one table
import numpy as np

from tests import pedersen_cases as PC

STRIDE, FIELDS, PREFIX, PREFIX_BITS, SEG_CHUNKS, GENS = 9, ((1, 61),), 0b10, 2, 7, "three"
NSEG = 3
KEY = ("pedersen", GENS, SEG_CHUNKS)


def build(n):
    return {"m": np.random.default_rng(8100 + n).integers(0, 256, size=(n, STRIDE), dtype=np.uint8)}


def _bits(row):
    out = [(PREFIX >> k) & 1 for k in range(PREFIX_BITS)]
    for off, nb in FIELDS:
        out += [(int(row[off + (k >> 3)]) >> (k & 7)) & 1 for k in range(nb)]
    return out


def _points(m):
    return np.stack([PC.point_bytes(PC.expected(PC.generators(GENS), SEG_CHUNKS, _bits(r))) for r in m]) if len(m) else np.zeros((0, 64), np.uint8)


def oracle_hash(i, n):
    return {"out": BC._memo("pedersen_hash", (i["m"],), lambda: np.ascontiguousarray(_points(i["m"])[:, :32]))}


def oracle_scalars(i, n):
    def f():
        out = np.zeros((NSEG, n, 32), np.uint8)
        for u, r in enumerate(i["m"]):
            for j, v in enumerate(PC.segment_sums(SEG_CHUNKS, NSEG, _bits(r))):
                out[j, u] = np.frombuffer((v % PC.J.R_MOD).to_bytes(32, "little"), dtype=np.uint8)
        return out.reshape(-1, 32)
    return {"s": BC._memo("pedersen_scalars", (i["m"],), f)}


def _fields():
    return (C.c_uint32 * (2 * len(FIELDS)))(*[v for f in FIELDS for v in f])


def _table(env):
    if KEY not in env.handles:
        t = env.eng0.pedersen_table(PC.gens_bytes(GENS), SEG_CHUNKS, 0)
        env.eng0.sync()                                   # built on eng0's stream, used from every context
        env.keep.append(t)
        env.handles[KEY] = t._h
    return env.handles[KEY]


def call_hash(run, lib, ctx, env):
    return lib.jj_pedersen_hash_vartime(ctx, _table(env), C.c_size_t(run.n), C.c_uint(PREFIX), C.c_int(PREFIX_BITS), C.c_void_p(run.ptr("m")), C.c_size_t(STRIDE),
                                        C.c_int(len(FIELDS)), _fields(), C.c_uint(0), C.c_void_p(run.ptr("out")))


def call_scalars(run, lib, ctx, env):
    return lib.jj_pedersen_scalars(ctx, C.c_int(NSEG), C.c_int(SEG_CHUNKS), C.c_size_t(run.n), C.c_uint(PREFIX), C.c_int(PREFIX_BITS), C.c_void_p(run.ptr("m")),
                                   C.c_size_t(STRIDE), C.c_int(len(FIELDS)), _fields(), C.c_void_p(run.ptr("s")))


def rows():
    """the two rows, added to the table on first use"""
    have = {c.id: c for c in BC.CASES}
    if "jj_pedersen_hash_vartime" not in have:
        BC._add("jj_pedersen_hash_vartime", [("m", STRIDE)], [("out", 32)], [], build, oracle_hash, call=call_hash)
        BC._add("jj_pedersen_scalars", [("m", STRIDE)], [("s", 32)], [], build, oracle_scalars, call=call_scalars, rows={"s": lambda n: NSEG * n})
        have = {c.id: c for c in BC.CASES}
    return have["jj_pedersen_hash_vartime"], have["jj_pedersen_scalars"]


ROW_HASH, ROW_SCALARS = rows()
