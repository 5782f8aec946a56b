"""Every batch entry point against its buffers, byte for byte (tests/buffer_cases.py: the arena, the table of entry points, the sizes).

Each call runs through the raw C ABI on pointers into a guarded arena and must (1) return 0, (2) leave every output region equal to the oracle's
bytes, (3) leave every guard byte and every input byte as it was.  Device arenas: every row x every size x every skew, all regions of a call in
ONE torch tensor.  Host arenas (pageable, one jj_host_alloc block, mixed with device memory), the chunked host pipeline, n = 0, and one positive
control that makes a real kernel store land in a guard.  The module prints how much it checked when it finishes."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import buffer_cases as BC  # noqa: E402
from buffer_cases import ANY, CASES, HOST_SIZES, SIZES, SKEWS, K, Run  # noqa: E402
from oracle import c_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

STATS = {"calls": 0, "out_bytes": 0, "guard_bytes": 0}
GPU_CASES = [c for c in CASES if not c.host_only]
ROWS = [(c, o) for c in GPU_CASES for o in c.options]
ROW_IDS = ["%s%s" % (c.id, "".join("-%s=%d" % kv for kv in sorted(o.items()))) for c, o in ROWS]


class Env:
    """contexts per option set, and the handles the rows name (tables, bases: they serve every context of the device)"""

    def __init__(self):
        import torch

        from jubjub_amd import Engine, _lib

        self.torch, self.Engine, self.lib = torch, Engine, _lib.load()
        self.engines, self.handles, self.keep, self.multi = {}, {}, [], None
        self.eng0 = self.engine({})

    def engine(self, options):
        key = tuple(sorted(options.items()))
        if key not in self.engines:
            e = self.Engine(0, options=options)
            assert self.lib.jj_ctx_use_own_stream(e._ctx) == 0          # the context's own stream, whatever the arena is made of
            self.engines[key] = e
        return self.engines[key]

    def multi_engine(self):
        if self.multi is None:
            from jubjub_amd.engine import MultiEngine

            self.multi = MultiEngine([0, 0, 0])
        return self.multi

    def ctx(self, case, eng):
        return self.multi_engine()._h if case.ctx == "multi" else eng._ctx

    def handle(self, key):
        if key not in self.handles:
            e = self.eng0
            if key[0] == "table":
                obj = e.fixedbase_table(BC.fixed_base(key[1]), key[2])
            elif key[0] == "composite":
                obj = e.fixedbase_composite_table(np.stack([BC.fixed_base(k) for k in range(3)]), BC.COMPOSITE_BITS)
            elif key[0] == "basis":
                obj = e.msm_basis(BC.points(BC.BASIS_POINTS, 707), mode={1: "points", 2: "windows"}[key[1]])
            else:
                assert key[0] == "mtable"
                self.handles[key] = self.multi_engine().fixedbase_table(BC.fixed_base(key[1]), key[2])
                return self.handles[key]
            e.sync()                                                      # built on eng0's stream, used from every context
            self.keep.append(obj)
            self.handles[key] = obj._h
        return self.handles[key]

    def allocs(self):
        return {"dev": lambda nb: self.torch.empty(nb, dtype=self.torch.uint8, device="cuda:0"), "host": None, "pinned": lambda nb: self.eng0.host_alloc(nb)}

    def close(self):
        for obj in self.keep:
            obj.close()
        if self.multi is not None:
            self.multi.close()
        for e in self.engines.values():
            e.close()


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.close()
    print("\nbuffer discipline: %d calls checked; %d output bytes compared with the oracle; %d guard bytes verified"
          % (STATS["calls"], STATS["out_bytes"], STATS["guard_bytes"]))


def checked_call(env, case, options, n, place, skew, data=None):
    """one call of a row through the raw ABI: return code 0, outputs equal to the oracle, guards and inputs untouched; returns the Run"""
    eng = env.engine(options)
    run = Run(case, n, place, skew, env.allocs(), data=data)
    env.torch.cuda.synchronize()                       # the arena was filled on torch's stream; the context runs on its own
    rc = run.call(env.lib, env.ctx(case, eng), env)
    where = (case.id, options, n, sorted((k, a.ptr(k) % BC.ALIGN) for k, a in run.where.items()))
    assert rc == (case.rc(n) if case.rc else 0), (where, rc, env.lib.jj_last_error(eng._ctx))
    assert env.lib.jj_ctx_sync(eng._ctx) == 0, where
    problems = run.problems(env.lib)
    assert problems == [], (where, problems)
    STATS["calls"] += 1
    STATS["out_bytes"] += sum(w * case.nrows(k, n) for k, w in case.outs if run.expected[k] is not ANY and run.expected[k] is not None)
    STATS["guard_bytes"] += run.counts()[1]
    return run


def placement(case, ins, outs):
    """regions in the arena named for their role, except those the row pins to one side"""
    def place(name, role):
        if name in case.device:
            return "dev"
        if name in case.host:
            return "host"
        return ins if role == "in" else outs
    return place


# every skew for all regions alike, and one placement in which the regions of a call differ: inputs at 16, outputs at 496
SKEW_SETS = [lambda name, role, s=s: s for s in SKEWS] + [lambda name, role: 16 if role == "in" else 496]
MIXED_SKEW = SKEW_SETS[-1]


@pytest.mark.parametrize("case,options", ROWS, ids=ROW_IDS)
def test_device_arena(env, case, options):
    """every size x every skew, all regions of the call in one device tensor"""
    if case.ctx == "multi":
        sizes, place = SIZES, placement(case, "host", "host")         # jj_multi_* take host pointers only: the same sizes in a pageable arena
    else:
        sizes, place = SIZES, placement(case, "dev", "dev")
    for n in sizes if case.sized else (1,):
        for skew in SKEW_SETS:
            checked_call(env, case, options, n, place, skew)


@pytest.mark.parametrize("case,options", ROWS, ids=ROW_IDS)
def test_host_arenas(env, case, options):
    """a pageable arena, an arena carved from one jj_host_alloc block, device inputs with host outputs and the reverse"""
    places = [placement(case, "host", "host"), placement(case, "pinned", "pinned")]
    if case.ctx != "multi":
        places += [placement(case, "dev", "host"), placement(case, "host", "dev"), placement(case, "dev", "pinned")]
    for n in HOST_SIZES:
        for place in places:
            checked_call(env, case, options, n, place, MIXED_SKEW)


@pytest.mark.parametrize("case", GPU_CASES, ids=[c.id for c in GPU_CASES])
def test_zero_units(env, case):
    """n = 0 with valid pointers: return code 0 and nothing written anywhere -- but for the result row the header promises of the MSM family
    (the identity), which is one of the row's outputs and is compared like any other"""
    ins, outs = case.data(0)
    for name, w in case.outs:
        assert case.nrows(name, 0) in (0, 1) and (case.nrows(name, 0) == 0 or case.fn.startswith(("jj_msm", "jj_multi_msm", "jj_point_sum")))
    for where in ("host",) if case.ctx == "multi" else ("dev", "host"):
        for skew in (SKEW_SETS[1], MIXED_SKEW):
            checked_call(env, case, case.options[-1], 0, placement(case, where, where), skew)


# ---- the host pipeline
PIPELINED = [c for c in GPU_CASES if c.pipelined]
PIPE_N = 5 * 1024 + 77


def chunk_sample(n, chunk):
    """the first and last 3 rows of every chunk of `chunk` units"""
    idx = set()
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        idx |= set(range(lo, min(hi, lo + 3))) | set(range(max(lo, hi - 3), hi))
    return np.array(sorted(idx))


def pipeline_check(env, case, options, n, chunk):
    """the same call on a device arena and on both host arenas: the whole outputs agree, and a sample that holds the edges of every chunk
    equals the oracle (the small sizes tie every row to the oracle in full)"""
    ins = {k: BC._rows(v, dict(case.ins)[k]) for k, v in case.build(n).items()}
    dev = checked_call(env, case, options, n, placement(case, "dev", "dev"), MIXED_SKEW, data=(ins, {k: ANY for k, _ in case.outs}))
    got = {k: BC._rows(dev.where[k].read(k), w) for k, w in case.outs}
    idx = chunk_sample(n, chunk)
    per_unit = {k for k, _ in case.ins if case.nrows(k, n) == n}
    want = case.oracle({k: np.ascontiguousarray(v[idx]) if k in per_unit else v for k, v in ins.items()}, len(idx))
    for k, w in case.outs:
        assert (got[k][idx] == BC._rows(want[k], w)).all(), (case.id, n, k, "device arena against the oracle on the chunk edges")
        STATS["out_bytes"] += len(idx) * w
    for where in ("host", "pinned"):
        checked_call(env, case, options, n, placement(case, where, where), MIXED_SKEW, data=(ins, got))


@pytest.mark.parametrize("case", PIPELINED, ids=[c.id for c in PIPELINED])
def test_host_pipeline_chunks(env, case):
    """chunks of 2^10 units (option pipe_chunk_log2), five whole chunks and a tail of 77"""
    assert len({c.fn for c in PIPELINED}) == 13
    opts = dict(case.options[-1], pipe_chunk_log2=10)
    pipeline_check(env, case, opts, PIPE_N, 1 << 10)


@pytest.mark.parametrize("case", PIPELINED, ids=[c.id for c in PIPELINED])
def test_host_arrays_at_the_bounce_threshold(env, case):
    """the first n whose output reaches BOUNCE_THRESHOLD: a pageable array of that size goes through the context's page-locked staging slots
    when the call stages it whole, and through the chunks' slots when it is pipelined"""
    w = max(w for _, w in case.outs)
    n = -(-K["bounce_threshold"] // w)
    assert n * w >= K["bounce_threshold"] > (n - 1) * w
    pipeline_check(env, case, case.options[0], n, 1 << 10)
    pipeline_check(env, case, dict(case.options[0], pipe_chunk_log2=10), n, 1 << 10)


# ---- one positive control, no modified kernel
def test_positive_control_one_row_too_many(env):
    """An arena carved for n rows, jj_fq_add called with n + 1: row n of both inputs is guard, and the kernel's store of row n of the result
    lands in the 32 guard bytes behind `out`.  Every byte involved lies inside the arena: an ordinary call.  The checker must report exactly
    those 32 bytes -- the device-side comparison sees a real kernel store."""
    case = next(c for c in CASES if c.id == "jj_fq_add")
    n = 65
    run = Run(case, n, placement(case, "dev", "dev"), MIXED_SKEW, env.allocs())
    env.torch.cuda.synchronize()
    assert run.call(env.lib, env.eng0._ctx, env, n=n + 1) == 0 and env.lib.jj_ctx_sync(env.eng0._ctx) == 0
    a = run.where["out"]
    guard_row = lambda name: a.view[a.region(name).off + 32 * n:a.region(name).off + 32 * n + 32].cpu().numpy()       # noqa: E731
    written = O.field_op(O.FQ, "add", guard_row("a"), guard_row("b"))[0].reshape(-1)                       # what the kernel put behind `out`
    r = a.region("out")
    before = BC._images(np, a.total)[0][r.off + 32 * n:r.off + 32 * n + 32]
    assert (written != before).all(), "pick another n: a byte of the stray row equals the guard's"
    assert (guard_row("out") == written).all()
    assert run.problems(env.lib) == ["dev arena: %r" % {"kind": "guard", "region": "out", "side": "behind", "distance": 0, "count": 32}]
    STATS["calls"] += 1


# ---- what an entry point answers to a pointer it cannot use
def _abi_entry_points():
    abi = open(os.path.join(BC.CSRC, "jj_abi.hip")).read()
    return set(re.findall(r"^JJ_API int (jj_\w+)\(", abi, flags=re.M)) | set(re.findall(r"\bFIELD_(?:BIN|UN|UN_OK)\((jj_\w+),", abi))


ABI_CASES = [c for c in GPU_CASES if c.call is None and c.fn in _abi_entry_points()]
OPTIONAL = {("jj_random_points", "attempts")}                  # may be NULL: the one optional array of these entry points


def refusals(case):
    """(position, argument, kind) of every call the row is refused with: each pointer argument as NULL, and every per-unit array (the ones
    stage_in / stage_out resolve before any launch) also as a device pointer 8 bytes past a 16-byte boundary.  A single 32- or 64-byte
    scalar argument is copied as it is and has no alignment rule: NULL only."""
    out = []
    for i, a in enumerate(case.args):
        if a == "ctx" or (isinstance(a, tuple) and a[0] in ("handle", "handles")):
            out.append((i, a if a == "ctx" else a[0], "null"))
        elif isinstance(a, str) and a != "n" and (case.fn, a) not in OPTIONAL:
            out.append((i, a, "null"))
            if case.nrows(a, 2) == 2 * case.nrows(a, 1):
                out.append((i, a, "misaligned"))
    return out


@pytest.mark.parametrize("case", ABI_CASES, ids=[c.id for c in ABI_CASES])
def test_refused_arguments(env, case):
    """One unit on a device arena, one argument at a time made unusable (refusals): the call returns JJ_ERR_INVALID and leaves every output
    region and every guard byte as it was, and the unmodified call that follows on the same context (checked_call) equals the oracle.
    The expectations were recorded with the library of the commit before the entry points got their common front end, which refused every
    one of these calls (profiles/abi_front_end_ab.txt)."""
    assert len(ABI_CASES) >= 60 and {"jj_fq_add", "jj_decompress", "jj_point_sum", "jj_random_points", "jj_fixedvar_mul_vartime"} <= {c.fn for c in ABI_CASES}
    options, place = case.options[0], placement(case, "dev", "dev")
    eng = env.engine(options)
    todo = refusals(case)
    assert len(todo) >= 3 and todo[0] == (0, "ctx", "null")
    for i, name, kind in todo:
        run = Run(case, 1, place, MIXED_SKEW, env.allocs())
        env.torch.cuda.synchronize()
        if kind == "misaligned":
            assert run.where[name].torch and run.ptr(name) % 16 == 0
        rc = run.call(env.lib, env.ctx(case, eng), env, swap={i: None if kind == "null" else run.ptr(name) + 8})
        print("refused %s %s %s: rc %d" % (case.id, name, kind, rc))
        assert rc == BC.INVALID, (case.id, name, kind, rc)
        assert env.lib.jj_ctx_sync(eng._ctx) == 0
        assert all(run.where[k].untouched(k) for k, _ in case.outs), (case.id, name, kind, "an output was written")
        assert [v for a in run.arenas.values() for v in a.violations()] == [], (case.id, name, kind)
        STATS["calls"] += 1
        STATS["guard_bytes"] += run.counts()[1]
        checked_call(env, case, options, 1, place, MIXED_SKEW)


# ---- host and device arrays within one call
from tests import group_hash_buffer_row, ka_buffer_row  # noqa: E402,F401  (their rows join CASES; ROWS above stays as it was)

MIXED_KINDS = ("jj_fq_add", "jj_varbase_mul2_vartime", "jj_fixedvar_mul_vartime", "jj_decompress", "jj_ka_kdf", "jj_chacha20_xor", "jj_group_hash")


@pytest.mark.parametrize("fn", MIXED_KINDS)
def test_host_and_device_arrays_within_one_call(env, fn):
    """the arrays of one call alternately in device and in host memory, inputs and outputs alike, starting with either: every array is staged or
    passed through by its own kind, whatever its neighbours are (the placements of test_host_arenas keep all inputs, and all outputs, on one side)"""
    case = next(c for c in CASES if c.fn == fn)
    names = [k for k, _ in case.ins + case.outs]
    assert len(names) >= 3
    for first in (0, 1):
        side = {k: ("dev", "host")[(i + first) % 2] for i, k in enumerate(names)}
        place = lambda name, role: "dev" if name in case.device else "host" if name in case.host else side[name]      # noqa: E731
        for n in HOST_SIZES:
            checked_call(env, case, case.options[0], n, place, MIXED_SKEW)
