"""The buffer-discipline row of jj_pedersen_commit_vartime (tests/buffer_cases.py holds the table and says what a row is): the call's regions
carved into guarded arenas at every size and skew, the output bytes equal to the restatement of tests/commit_cases.py, guards and inputs
untouched.  The row joins buffer_cases.CASES when this module is imported (tests/test_commit_cases_cpu.py and tests/test_gpu_commit.py import
it): the table's coverage pin (tests/test_buffer_cases_cpu.py) then finds it, and tests/test_gpu_commit.py runs it through the arenas with the
runner of tests/test_gpu_buffers.py.  Test infrastructure only.

Three source regions a, b, c of 9, 5 and 3 bytes per unit, read from byte 1, 0 and 1 as fields of 37, 21 and 3 bits in the order b, a, c
behind a 2-bit prefix: every region's rows start at every residue modulo 4 and every region ends in the middle of a dword, directly in front
of its guard.  Three segments of 7 chunks (63 bits: the message is exactly at capacity) keep the oracle's scalars short at the table's 1025
units; r is 32 raw bytes, all of them random in every eighth unit and the upper 24 zero in the others, so that the restatement's ladders
for [r mod 2^252] R stay short for most of the 1025 units.  R's table is a gathered one (window_bits 8).  The table handles, the prefix and the host arrays (srcs, strides, fields) are no regions, so the row
makes the call itself."""
import ctypes as C

import buffer_cases as BC  # by the name tests/test_buffer_cases_cpu.py and tests/test_gpu_buffers.py import it: one module, one table
import numpy as np

from oracle import jubjub_ref as J
from tests import commit_cases as CC
from tests import pedersen_cases as PC

STRIDES = {"a": 9, "b": 5, "c": 3}
FIELDS = ((1, 0, 21), (0, 1, 37), (2, 1, 3))                # (src, byte_offset, nbits); sources in the order a, b, c
PREFIX, PREFIX_BITS, SEG_CHUNKS, GENS, NSEG = 0b01, 2, 7, "three", 3
KEY, RKEY = ("pedersen_commit", GENS, SEG_CHUNKS), ("pedersen_commit_rbase", 8)
LONG_EVERY = 8                                              # one unit in eight has a full-length r


def build(n):
    rng = np.random.default_rng(8300 + n)
    ins = {k: rng.integers(0, 256, size=(n, w), dtype=np.uint8) for k, w in STRIDES.items()}
    r = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    r[np.arange(n) % LONG_EVERY != 0, 8:] = 0
    ins["r"] = r
    return ins


def _bits(i, u):
    out = [(PREFIX >> k) & 1 for k in range(PREFIX_BITS)]
    for s, off, nb in FIELDS:
        row = i["abc"[s]][u]
        out += [(int(row[off + (k >> 3)]) >> (k & 7)) & 1 for k in range(nb)]
    return out


def _point(i, u):
    h = J.affine_to_extended(PC.expected(CC.gens_of(GENS), SEG_CHUNKS, _bits(i, u)))
    k = int.from_bytes(i["r"][u].tobytes(), "little") & ((1 << 252) - 1)
    return J.ext_to_affine(J.ext_add(h, J.affine_to_extended(J.scalar_mul_fast(CC.bases()["R"], k))))


def oracle(i, n):
    def f():
        return np.stack([PC.point_bytes(_point(i, u))[:32] for u in range(n)]) if n else np.zeros((0, 32), np.uint8)
    return {"out": BC._memo("pedersen_commit", (i["a"], i["b"], i["c"], i["r"]), f)}


def _tables(env):
    if KEY not in env.handles:
        t = env.eng0.pedersen_table(CC.gens_bytes(GENS), SEG_CHUNKS, 0)
        rt = env.eng0.fixedbase_table(PC.point_bytes(CC.bases()["R"]).copy(), RKEY[1])
        env.eng0.sync()                                   # built on eng0's stream, used from every context
        env.keep += [t, rt]
        env.handles[KEY], env.handles[RKEY] = t._h, rt._h
    return env.handles[KEY], env.handles[RKEY]


def call(run, lib, ctx, env):
    ped, rbase = _tables(env)
    srcs = (C.c_void_p * 3)(*[run.ptr(k) for k in "abc"])
    strides = (C.c_size_t * 3)(*[STRIDES[k] for k in "abc"])
    fields = (C.c_uint32 * (3 * len(FIELDS)))(*[v for f in FIELDS for v in f])
    return lib.jj_pedersen_commit_vartime(ctx, ped, rbase, C.c_size_t(run.n), C.c_uint(PREFIX), C.c_int(PREFIX_BITS), C.c_int(3), srcs, strides,
                                          C.c_int(len(FIELDS)), fields, C.c_void_p(run.ptr("r")), C.c_uint(0), C.c_void_p(run.ptr("out")))


def row():
    """the row, added to the table on first use"""
    have = {c.id: c for c in BC.CASES}
    if "jj_pedersen_commit_vartime" not in have:
        return BC._add("jj_pedersen_commit_vartime", [(k, w) for k, w in STRIDES.items()] + [("r", 32)], [("out", 32)], [], build, oracle, call=call)
    return have["jj_pedersen_commit_vartime"]


ROW = row()
