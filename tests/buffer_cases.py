"""What a batch entry point may touch, as data (test infrastructure only; CPU side: tests/test_buffer_cases_cpu.py, GPU side:
tests/test_gpu_buffers.py).

The parity suite checks what a call RETURNS.  This module is about what a call writes BESIDE its result and whether it leaves its inputs alone:

  Arena   one flat uint8 buffer (numpy, a jj_host_alloc block, or a torch CUDA tensor) cut into regions with a guard band in front of the
          first, between all and behind the last.  A region starts `skew` bytes past a 512-byte boundary (16 is all include/jubjub_hip.h
          asks of a device pointer) and ends at exactly its byte length, so the guard begins at the very next byte.  Guards carry one
          position-dependent pattern, output regions a second one that differs from it at every offset: a kernel that writes a constant or
          a shifted copy of its neighbourhood is seen, and an output row that is never written cannot equal the oracle's.
  CASES   one row per C-ABI entry point that takes array pointers: argument order, input builder, widths, option sets, oracle.
  SIZES   the smallest sizes at which a guard can fail, derived from the launch constants in the kernels' source.
"""
import ctypes as C
import json
import os
import re

import numpy as np

from oracle import c_oracle as O
from oracle import jubjub_ref as J
from util import EDGE_SCALARS, MSM_PARTIAL_BYTES, arr32, arr64, b32, oracle_msm_record, pt64, rand_points, rand_scalars, to_int

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jubjub_amd", "csrc")
Q, R = J.Q, J.R_MOD
ALIGN = 512                     # what a fresh torch allocation is aligned to: the alignment the rest of the suite hands over by accident
SKEWS = (0, 16, 496)            # offsets modulo ALIGN a region starts at; 16 is the documented minimum and nothing more
INVALID = -1                    # JJ_ERR_INVALID


# ---------------------------------------------------------------------------------------------------- constants read out of the source
def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _one(pattern, text, what):
    m = re.search(pattern, text)
    assert m, "buffer_cases: %s not found in the source" % what
    return int(m.group(1))


def source_constants():
    """the launch constants SIZES and GUARD are derived from, found by regex (tests/test_buffer_cases_cpu.py pins them)"""
    abi, msmk = _src("jj_abi.hip"), _src("jj_msm_kernels.h")
    blocks = {int(x) for x in re.findall(r"dim3\(blocks_for\(.*?\)\), dim3\((\d+)\)", abi)}
    assert blocks, "buffer_cases: no elementwise launch found in jj_abi.hip"
    shift = _one(r"constexpr size_t BOUNCE_THRESHOLD = \(size_t\)1 << (\d+);", _src("jj_engine.h"), "BOUNCE_THRESHOLD")
    with open(os.path.join(ROOT, "include", "jubjub_hip.h")) as f:
        partial = _one(r"#define JJ_MSM_PARTIAL_BYTES (\d+)u", f.read(), "JJ_MSM_PARTIAL_BYTES")
    return {
        "block": max(blocks),                                                                       # threads per workgroup of the elementwise kernels
        "wave": _one(r"__launch_bounds__\((\d+)\) k_msm_batch_finish", msmk, "the finish kernels' wave"),
        "quad": _one(r"k_varbase_ct_quad, dim3\(blocks_for\((\d+) \* n\)\)", abi, "lanes per unit of the quad ladders"),
        "mont_x1_units": _one(r"constexpr int MONT_X1_UNITS = (\d+);", _src("jj_mont.h"), "MONT_X1_UNITS"),
        "finish_rows": _one(r"constexpr int MSM_BATCH_FINISH_ROWS = (\d+);", msmk, "MSM_BATCH_FINISH_ROWS"),
        "bounce_threshold": 1 << shift,
        "msm_partial_bytes": partial,
    }


K = source_constants()
assert K["msm_partial_bytes"] == MSM_PARTIAL_BYTES


def derive_sizes(k):
    """1, 3 and one below / at / one above every count of units after which a kernel starts another quad, wave, workgroup or lane round"""
    s = {1, 3}
    for c in (k["quad"], k["finish_rows"], k["wave"], k["block"], k["wave"] * k["mont_x1_units"]):
        s |= {c - 1, c, c + 1}
    return tuple(sorted(s))


SIZES = derive_sizes(K)
HOST_SIZES = (1, K["wave"] + 1, K["block"] + 1)          # the host-arena placements of tests/test_gpu_buffers.py


# ---------------------------------------------------------------------------------------------------- the arena
def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _images(xp, total, device=None):
    """(guard, fill) patterns over offsets 0 .. total - 1.  guard = (167 o + 13) mod 256; fill = guard ^ m with m = 0x55 | ((o >> 3) & 0x2A), never
    zero, so the two differ at EVERY offset; a fill byte of 0 or 1 (what an `ok` byte may be) is flipped to 0xFE / 0xFF, which guard (then below
    0x80) cannot be either."""
    o = xp.arange(total, dtype=xp.int64, device=device) if device is not None else xp.arange(total, dtype=xp.int64)
    g = (o * 167 + 13) & 0xFF
    f = g ^ (0x55 | ((o >> 3) & 0x2A))
    f = xp.where(f < 2, f ^ 0xFE, f)
    return g.to(xp.uint8) if device is not None else g.astype(xp.uint8), f.to(xp.uint8) if device is not None else f.astype(xp.uint8)


class Region:
    __slots__ = ("name", "role", "off", "nbytes")

    def __init__(self, name, role, off, nbytes):
        self.name, self.role, self.off, self.nbytes = name, role, off, nbytes


class Arena:
    """carve() every region, commit() once (allocates, fills), hand ptr(name) to the call, then violations() / read() / untouched()."""

    def __init__(self, guard=None):
        self.guard = GUARD if guard is None else int(guard)
        self.regions, self._end, self.buf, self._inputs = [], 0, None, {}

    def carve(self, nbytes, skew, role="in", name=None):
        assert self.buf is None and role in ("in", "out") and 0 <= skew < ALIGN and skew % 16 == 0
        lo = self._end + self.guard
        off = lo + ((skew - lo) % ALIGN)
        r = Region(name or "r%d" % len(self.regions), role, off, int(nbytes))
        assert all(r.name != x.name for x in self.regions)
        self.regions.append(r)
        self._end = off + r.nbytes
        return r

    @property
    def total(self):
        return self._end + self.guard

    def region(self, name):
        return next(r for r in self.regions if r.name == name)

    def commit(self, alloc=None, inputs=None):
        """alloc(nbytes) -> a flat uint8 numpy array or torch CUDA tensor (default: a fresh pageable numpy array); inputs: {name: bytes-like}"""
        buf = np.empty(self.total + ALIGN, np.uint8) if alloc is None else alloc(self.total + ALIGN)
        self.torch = _is_torch(buf)
        addr = buf.data_ptr() if self.torch else buf.ctypes.data
        pad = (-addr) % ALIGN
        self.buf, self.base, self.view = buf, addr + pad, buf[pad:pad + self.total]
        self._inputs = {k: np.ascontiguousarray(v, dtype=np.uint8).reshape(-1).copy() for k, v in (inputs or {}).items()}
        self.view[:] = self._expected(fill_outputs=True)
        return self

    def _xp(self):
        if self.torch:
            import torch

            return torch, self.buf.device
        return np, None

    def _expected(self, fill_outputs):
        """what the arena holds when nothing but the outputs was written (fill_outputs: and not even those)"""
        xp, dev = self._xp()
        g, f = _images(xp, self.total, dev)
        for r in self.regions:
            if r.role == "out":
                if fill_outputs:
                    g[r.off:r.off + r.nbytes] = f[r.off:r.off + r.nbytes]
            else:
                src = self._inputs[r.name]
                assert src.size == r.nbytes, (r.name, src.size, r.nbytes)
                g[r.off:r.off + r.nbytes] = xp.from_numpy(src).to(dev) if self.torch else src
        return g

    def ptr(self, name):
        return self.base + self.region(name).off

    def read(self, name):
        r = self.region(name)
        v = self.view[r.off:r.off + r.nbytes]
        return v.cpu().numpy() if self.torch else v.copy()

    def fill(self, name):
        """the bytes an output region was filled with, on the host"""
        r = self.region(name)
        return _images(np, self.total)[1][r.off:r.off + r.nbytes]

    def untouched(self, name):
        """an output region still holds its fill pattern, every byte"""
        r = self.region(name)
        xp, dev = self._xp()
        f = _images(xp, self.total, dev)[1][r.off:r.off + r.nbytes]
        return bool((self.view[r.off:r.off + r.nbytes] == f).all())

    def _mismatches(self):
        """offsets outside the output regions that differ from the regenerated image; the comparison runs where the arena lives, only the
        positions come back"""
        bad = self.view != self._expected(fill_outputs=False)
        for r in self.regions:
            if r.role == "out":
                bad[r.off:r.off + r.nbytes] = False
        if self.torch:
            return bad.nonzero().reshape(-1).cpu().numpy()
        return np.flatnonzero(bad)

    def violations(self):
        """one finding per run of changed bytes: {"kind": "guard" | "input", "region", "side": "behind" | "front" | "inside", "distance", "count"}.
        distance: behind -- bytes past the region's end (0 = the very next byte); front -- bytes before its start (1 = the byte directly in front);
        inside (inputs) -- offset from the region's start."""
        idx = self._mismatches()
        out = []
        if idx.size == 0:
            return out
        cuts = np.flatnonzero(np.diff(idx) != 1) + 1
        for run in np.split(idx, cuts):
            x, count = int(run[0]), int(run.size)
            inside = [r for r in self.regions if r.role == "in" and r.off <= x < r.off + r.nbytes]
            if inside:
                out.append({"kind": "input", "region": inside[0].name, "side": "inside", "distance": x - inside[0].off, "count": count})
                continue
            before = [r for r in self.regions if r.off + r.nbytes <= x]
            after = [r for r in self.regions if r.off > x]
            cand = []
            if before:
                r = max(before, key=lambda r: r.off + r.nbytes)
                cand.append((x - (r.off + r.nbytes), "behind", r))
            if after:
                r = min(after, key=lambda r: r.off)
                cand.append((r.off - (x + count - 1), "front", r))
            d, side, r = min(cand, key=lambda c: c[0])
            out.append({"kind": "guard", "region": r.name, "side": side, "distance": d, "count": count})
        return out

    def guard_bytes(self):
        return self.total - sum(r.nbytes for r in self.regions)


# ---------------------------------------------------------------------------------------------------- inputs (host numpy, seeded)
_POOL = {}


def _golden():
    if "golden" not in _POOL:
        with open(os.path.join(ROOT, "tests", "golden", "reference_vectors.json")) as f:
            _POOL["golden"] = json.load(f)
    return _POOL["golden"]


def _plant(base, specials):
    """ordinary rows with the special ones at the odd indices: n = 3 already holds one, n = 1 none"""
    for k, sp in enumerate(specials):
        if 2 * k + 1 < len(base):
            base[2 * k + 1] = sp
    return base


POOL_ROWS = 4096                 # distinct random points per seed; longer arrays repeat them


def _point_pool(seed, n):
    m = 16
    while m < min(n, POOL_ROWS):
        m *= 2
    if ("pts", seed, m) not in _POOL:
        _POOL["pts", seed, m] = rand_points(seed, m, subgroup=(seed % 2 == 0))
    return _POOL["pts", seed, m]


def special_points():
    g = _golden()
    tors = [(sum(int(h, 16) << (64 * i) for i, h in enumerate(p["u"])), sum(int(h, 16) << (64 * i) for i, h in enumerate(p["v"])))
            for p in g["EIGHT_TORSION_raw"]["points"]]
    return arr64([J.AFFINE_IDENTITY, (0, Q - 1)] + tors)


def points(n, seed):
    """n curve points: full-group (odd seed) or subgroup points with the identity, (0, -1) and the 8-torsion among them"""
    return _plant(np.resize(_point_pool(seed, n), (n, 64)), special_points())


def scalars(n, seed):
    """n raw 32-byte patterns (top bits set) with EDGE_SCALARS among them"""
    return _plant(rand_scalars(seed, n, full_width=True), arr32(EDGE_SCALARS))


def felems(n, seed, p):
    """n 32-byte integers, unreduced (the entry points reduce like from_raw), with 0, 1, p - 1, p, p + 1, 2^256 - 1 among them"""
    return _plant(rand_scalars(seed, n, full_width=True), arr32([0, 1, p - 1, p, p + 1, (1 << 256) - 1, 2, (p - 1) // 2]))


def encodings(n, seed):
    """compressed points (the special ones included) with undecodable bytes, the two non-canonical encodings of ZIP 216 and v >= q among them"""
    enc = O.compress(points(n, seed)) if n else np.zeros((0, 32), np.uint8)
    junk = rand_scalars(seed + 17, n, full_width=True)
    for i in range(n):
        if i % 5 == 2:
            enc[i] = junk[i]
        elif i % 7 == 3:
            enc[i] = b32((1 if i % 2 else Q - 1) | (1 << 255))       # u = 0 with the sign bit set
        elif i % 11 == 4:
            enc[i] = b32(Q + i)
    return enc


def off_curve(n, seed):
    p = points(n, seed)
    p[2::4, 0] ^= 1
    return p


def ext_points(n, seed):
    """projective (U, V, Z, T1, T2) rows with Z != 1, some with Z = 0"""
    e = O.varbase_mul_ext(scalars(n, seed), points(n, seed + 1)) if n else np.zeros((0, 160), np.uint8)
    e[1::6, 64:96] = 0
    return e


def _memo(tag, arrays, fn):
    """fn() once per distinct input bytes: rows that share inputs share the ladder"""
    key = (tag,) + tuple(hash(np.ascontiguousarray(a).tobytes()) for a in arrays)
    if key not in _POOL:
        _POOL[key] = fn()
    return _POOL[key]


def _rows(a, w):
    return np.ascontiguousarray(a, dtype=np.uint8).reshape(-1, w)


# ---------------------------------------------------------------------------------------------------- the table
class Case:
    """fn        the C-ABI entry point (covers: every prototype this row answers for)
    variant   distinguishes rows of one entry point (table kind, flags, mode)
    ins/outs  [(name, bytes per row)]; rows per region: rows[name](n), n by default
    args      the call's arguments in order: "ctx", "n", a region's name, (ctype, value) or ("handle", key) / ("handles", [keys]) -- handles come
              from the environment the test provides (tables, bases, ...)
    build     n -> {input name: (rows, width) uint8}; oracle: (inputs, n) -> {output name: array | None}, None = the region must stay untouched
    options   the option sets (jj_ctx_set_option) under which the row runs
    device / host: regions that must live in device / host memory whatever the placement; host_only: runs without a GPU
    pipelined the entry point cuts large all-host batches into chunks (it hands run_batch in jj_abi.hip a chunk length from pipe_chunk_for)
    rc        n -> the return code the header promises; call: replaces the plain call (two-step entry points); verify: replaces the byte
              comparison of an output whose bytes are not canonical (name -> fn(got, inputs, n, lib) -> problem or None)"""

    def __init__(self, fn, ins, outs, args, build, oracle, variant="", options=({},), rows=None, covers=None, device=(), host=(), host_only=False,
                 ctx="ctx", rc=None, call=None, verify=None, sized=True, share=None, pipelined=False):
        self.fn, self.variant, self.ins, self.outs, self.args, self.build, self.oracle = fn, variant, list(ins), list(outs), list(args), build, oracle
        self.options, self.rows, self.covers = [dict(o) for o in options], dict(rows or {}), tuple(covers or (fn,))
        self.device, self.host, self.host_only, self.ctx, self.rc, self.call, self.verify = tuple(device), tuple(host), host_only, ctx, rc, call, dict(verify or {})
        self.sized, self.share, self.pipelined = sized, share, pipelined
        self.id = fn + ("[%s]" % variant if variant else "")

    def nrows(self, name, n):
        return self.rows[name](n) if name in self.rows else n

    def out_bytes(self, n):
        return {name: w * self.nrows(name, n) for name, w in self.outs}

    def data(self, n):
        """(inputs, expected outputs) at size n, built once per (row or share key, n)"""
        key = ("data", self.share or self.id, n)
        if key not in _POOL:
            ins = {k: _rows(v, dict(self.ins)[k]) for k, v in self.build(n).items()}
            outs = self.oracle(ins, n)
            _POOL[key] = (ins, {k: None if outs[k] is None else _rows(outs[k], w) for k, w in self.outs})
        return _POOL[key]


CASES = []


def _add(*a, **k):
    c = Case(*a, **k)
    assert all(c.id != x.id for x in CASES), c.id
    CASES.append(c)
    return c


ONE = lambda n: 1          # noqa: E731


# ---- fields
def _field_rows():
    for f, which, p in (("fq", O.FQ, Q), ("fr", O.FR, R)):
        sd = 100 * (which + 1)
        for op in ("add", "sub", "mul"):
            _add("jj_%s_%s" % (f, op), [("a", 32), ("b", 32)], [("out", 32)], ["ctx", "n", "a", "b", "out"],
                 lambda n, sd=sd, p=p: {"a": felems(n, sd, p), "b": felems(n, sd + 1, p)[::-1]},
                 lambda i, n, which=which, op=op: {"out": O.field_op(which, op, i["a"], i["b"])[0]})
        for op in ("neg", "square", "double"):
            _add("jj_%s_%s" % (f, op), [("a", 32)], [("out", 32)], ["ctx", "n", "a", "out"],
                 lambda n, sd=sd, p=p: {"a": felems(n, sd + 2, p)},
                 lambda i, n, which=which, op=op: {"out": O.field_op(which, op, i["a"])[0]})
        for op in ("invert", "sqrt"):
            _add("jj_%s_%s" % (f, op), [("a", 32)], [("out", 32), ("ok", 1)], ["ctx", "n", "a", "out", "ok"],
                 lambda n, sd=sd, p=p: {"a": felems(n, sd + 3, p)},
                 lambda i, n, which=which, op=op: dict(zip(("out", "ok"), O.field_op(which, op, i["a"]))))
        _add("jj_%s_pow" % f, [("a", 32), ("e", 32)], [("out", 32)], ["ctx", "n", "a", "e", "out"],
             lambda n, sd=sd, p=p: {"a": felems(n, sd + 4, p), "e": scalars(n, sd + 5)},
             lambda i, n, p=p: {"out": _rows(arr32([pow(to_int(a) % p, to_int(e), p) for a, e in zip(i["a"], i["e"])]), 32)})
        _add("jj_%s_from_bytes" % f, [("a", 32)], [("out", 32), ("ok", 1)], ["ctx", "n", "a", "out", "ok"],
             lambda n, sd=sd, p=p: {"a": felems(n, sd + 6, p)},
             lambda i, n, which=which: dict(zip(("out", "ok"), O.from_bytes(which, i["a"]))))
        _add("jj_%s_from_bytes_wide" % f, [("a", 64)], [("out", 32)], ["ctx", "n", "a", "out"],
             lambda n, sd=sd, p=p: {"a": np.concatenate([felems(n, sd + 7, p), felems(n, sd + 8, p)[::-1]], axis=1)},
             lambda i, n, which=which: {"out": O.from_bytes_wide(which, i["a"])})
        _add("jj_%s_to_le_bits" % f, [("a", 32)], [("out", 256)], ["ctx", "n", "a", "out"],
             lambda n, sd=sd, p=p: {"a": felems(n, sd + 9, p)},
             lambda i, n, p=p: {"out": np.unpackbits(_rows(arr32([to_int(a) % p for a in i["a"]]), 32), axis=1, bitorder="little")})


_field_rows()


# ---- points
def _point_rows():
    for op in ("double", "neg", "mul_by_cofactor"):
        _add("jj_point_" + op, [("p", 64)], [("out", 64)], ["ctx", "n", "p", "out"],
             lambda n: {"p": points(n, 301)}, lambda i, n, op=op: {"out": O.point_op(op, i["p"])})
    for op in ("add", "sub"):
        _add("jj_point_" + op, [("p", 64), ("q", 64)], [("out", 64)], ["ctx", "n", "p", "q", "out"],
             lambda n: {"p": points(n, 301), "q": points(n, 303)[::-1]}, lambda i, n, op=op: {"out": O.point_op(op, i["p"], i["q"])})
    _add("jj_point_to_niels", [("p", 64)], [("out", 96)], ["ctx", "n", "p", "out"],
         lambda n: {"p": points(n, 301)}, lambda i, n: {"out": O.to_niels(i["p"])})
    for pred in ("is_identity", "is_small_order", "is_torsion_free", "is_prime_order", "is_on_curve"):
        _add("jj_" + pred, [("p", 64)], [("out", 1)], ["ctx", "n", "p", "out"],
             (lambda n: {"p": off_curve(n, 305)}) if pred == "is_on_curve" else (lambda n: {"p": points(n, 305)}),
             lambda i, n, pred=pred: {"out": O.predicate(pred, i["p"])})
    _add("jj_point_sum", [("p", 64)], [("out", 64)], ["ctx", "n", "p", "out"], lambda n: {"p": points(n, 307)},
         lambda i, n: {"out": O.point_sum(i["p"])}, rows={"out": ONE})


_point_rows()


# ---- variable-base ladders
VB_OPTIONS = ({}, {"vb_quad_max": 1}, {"vb_ct_window": 3, "vb_quad_max": 1}, {"vb_ct_window": 2, "vb_quad_max": 1})


def _vb_build(n):
    return {"s": scalars(n, 401), "p": points(n, 403)}


def _vb_oracle(kind):
    def f(i, n):
        if kind == "exact":
            return {"out": O.varbase_mul_ext(i["s"], i["p"])}
        out = _memo("vb", (i["s"], i["p"]), lambda: O.varbase_mul(i["s"], i["p"]))        # one ladder for the rows that share these inputs
        return {"out": O.compress(out) if kind == "compressed" else out}
    return f


def _varbase_rows():
    for fn, kind, w in (("jj_varbase_mul", "affine", 64), ("jj_varbase_mul_compressed", "compressed", 32), ("jj_varbase_mul_ct", "affine", 64),
                        ("jj_varbase_mul_vartime", "affine", 64), ("jj_varbase_mul_vartime_compressed", "compressed", 32), ("jj_varbase_mul_exact", "exact", 160)):
        _add(fn, [("s", 32), ("p", 64)], [("out", w)], ["ctx", "n", "s", "p", "out"], _vb_build, _vb_oracle(kind), options=VB_OPTIONS,
             pipelined=fn in ("jj_varbase_mul", "jj_varbase_mul_compressed", "jj_varbase_mul_ct", "jj_varbase_mul_vartime", "jj_varbase_mul_vartime_compressed"))
    _add("jj_varbase_mul_scalar", [("s", 32), ("p", 64)], [("out", 64)], ["ctx", "n", "s", "p", "out"],
         lambda n: {"s": arr32([EDGE_SCALARS[-1]]), "p": points(n, 403)},
         lambda i, n: {"out": O.varbase_mul(np.repeat(i["s"], n, axis=0), i["p"])}, rows={"s": ONE}, options=VB_OPTIONS)
    m2 = ({"vb_mul2_window": 4}, {"vb_mul2_window": 5})

    def mul2(i, n):
        return _memo("mul2", (i["a"], i["p"], i["b"], i["q"]), lambda: O.point_op("add", O.varbase_mul(i["a"], i["p"]), O.varbase_mul(i["b"], i["q"])))

    build2 = lambda n: {"a": scalars(n, 411), "p": points(n, 413), "b": scalars(n, 415)[::-1], "q": points(n, 416)[::-1]}     # noqa: E731
    _add("jj_varbase_mul2_vartime", [("a", 32), ("p", 64), ("b", 32), ("q", 64)], [("out", 64)], ["ctx", "n", "a", "p", "b", "q", "out"], build2,
         lambda i, n: {"out": mul2(i, n)}, options=m2, pipelined=True)
    _add("jj_varbase_mul2_vartime_compressed", [("a", 32), ("p", 64), ("b", 32), ("q", 64)], [("out", 32)], ["ctx", "n", "a", "p", "b", "q", "out"], build2,
         lambda i, n: {"out": O.compress(mul2(i, n))}, options=m2, pipelined=True)
    _add("jj_varbase_mul2_scalars", [("ab", 64), ("p", 64), ("q", 64)], [("out", 64)], ["ctx", "n", "ab", "p", "q", "out"],
         lambda n: {"ab": arr32([EDGE_SCALARS[-2], EDGE_SCALARS[-5]]).reshape(1, 64), "p": points(n, 413), "q": points(n, 416)[::-1]},
         lambda i, n: {"out": O.point_op("add", O.varbase_mul(np.repeat(i["ab"][:, :32], n, axis=0), i["p"]),
                                         O.varbase_mul(np.repeat(i["ab"][:, 32:], n, axis=0), i["q"]))}, rows={"ab": ONE}, options=m2, pipelined=True)


_varbase_rows()


# ---- fixed base
def fixed_base(k):
    """base k of the fixed-base rows: the generator, a full-group point, (0, -1)'s neighbour in the torsion"""
    if ("base", k) not in _POOL:
        _POOL["base", k] = [pt64(J.GENERATOR), points(16, 501)[6], points(16, 502)[8]][k]
    return _POOL["base", k]


COMPOSITE_BITS = (64, 100, 61)


def _fixed_rows():
    def fb(i, n):
        return _memo("fb", (i["s"],), lambda: O.fixedbase_mul(i["s"], fixed_base(0)))

    for w in (7, 6, 8, 13):
        _add("jj_fixedbase_mul", [("s", 32)], [("out", 64)], ["ctx", ("handle", ("table", 0, w)), "n", "s", "out"], lambda n: {"s": scalars(n, 501)},
             lambda i, n: {"out": fb(i, n)}, variant="w%d" % w, pipelined=True)
        _add("jj_fixedbase_mul_compressed", [("s", 32)], [("out", 32)], ["ctx", ("handle", ("table", 0, w)), "n", "s", "out"], lambda n: {"s": scalars(n, 501)},
             lambda i, n: {"out": O.compress(fb(i, n))}, variant="w%d" % w, pipelined=True)
    tabs = [("table", 0, 7), ("table", 1, 8), ("table", 2, 6)]

    def multi(i, n, bits=None):
        s = i["s"].reshape(3, n, 32)
        acc = None
        for k in range(3):
            sk = s[k] if bits is None else _rows(arr32([to_int(x) & ((1 << bits[k]) - 1) for x in s[k]]), 32)
            t = O.fixedbase_mul(sk, fixed_base(k))
            acc = t if acc is None else O.point_op("add", acc, t)
        return acc

    _add("jj_fixedbase_multi_mul", [("s", 32)], [("out", 64)], ["ctx", ("handles", tabs), (C.c_int, 3), "n", "s", "out"],
         lambda n: {"s": scalars(3 * n, 503)}, lambda i, n: {"out": multi(i, n)}, rows={"s": lambda n: 3 * n})
    _add("jj_fixedbase_composite_mul", [("s", 32)], [("out", 64)], ["ctx", ("handle", ("composite",)), "n", "s", "out"],
         lambda n: {"s": scalars(3 * n, 505)}, lambda i, n: {"out": multi(i, n, COMPOSITE_BITS)}, rows={"s": lambda n: 3 * n})
    for w in (7, 8):
        def fv(i, n, w=w):
            return _memo("fv", (i["a"], i["b"], i["q"]), lambda: O.point_op("add", O.fixedbase_mul(i["a"], fixed_base(0)), O.varbase_mul(i["b"], i["q"])))
        build = lambda n: {"a": scalars(n, 507), "b": scalars(n, 509)[::-1], "q": points(n, 511)}     # noqa: E731
        quad = ({}, {"vb_quad_max": 1})                   # n <= vb_quad_max: the quad-of-lanes route; above: one unit per lane
        _add("jj_fixedvar_mul_vartime", [("a", 32), ("b", 32), ("q", 64)], [("out", 64)], ["ctx", ("handle", ("table", 0, w)), "n", "a", "b", "q", "out"],
             build, lambda i, n, fv=fv: {"out": fv(i, n)}, variant="w%d" % w, options=quad, pipelined=True)
        _add("jj_fixedvar_mul_vartime_compressed", [("a", 32), ("b", 32), ("q", 64)], [("out", 32)], ["ctx", ("handle", ("table", 0, w)), "n", "a", "b", "q", "out"],
             build, lambda i, n, fv=fv: {"out": O.compress(fv(i, n))}, variant="w%d" % w, options=quad, pipelined=True)


_fixed_rows()


# ---- codec and generators
def _codec_rows():
    for flags in (0, 1, 1 | 2, 1 | 4 | 8):
        _add("jj_decompress", [("enc", 32)], [("out", 64), ("ok", 1)], ["ctx", "n", "enc", (C.c_uint, flags), "out", "ok"], lambda n: {"enc": encodings(n, 601)},
             lambda i, n, flags=flags: dict(zip(("out", "ok"), O.decompress(i["enc"], flags))), variant="flags%d" % flags, pipelined=True)
    _add("jj_compress", [("p", 64)], [("out", 32)], ["ctx", "n", "p", "out"], lambda n: {"p": points(n, 603)}, lambda i, n: {"out": O.compress(i["p"])})
    _add("jj_batch_normalize", [("e", 160)], [("out", 64)], ["ctx", "n", "e", "out"], lambda n: {"e": ext_points(n, 605)},
         lambda i, n: {"out": O.batch_normalize(i["e"])})
    seed, first = 0x5EED0BEEF, 12345
    _add("jj_synth_scalars", [], [("out", 32)], ["ctx", "n", (C.c_uint64, seed), (C.c_uint64, first), "out"], lambda n: {},
         lambda i, n: {"out": _rows(arr32([J.synth_scalar(first + k, seed) for k in range(n)]), 32)})
    _add("jj_synth_bytes32", [], [("out", 32)], ["ctx", "n", (C.c_uint64, seed), (C.c_uint64, first), "out"], lambda n: {},
         lambda i, n: {"out": _rows(np.frombuffer(b"".join(J.synth_bytes32(first + k, seed) for k in range(n)), np.uint8), 32)})
    for sub in (0, 1):
        def rp(i, n, sub=sub):
            got = [J.synth_point(first + k, seed, subgroup=bool(sub)) for k in range(n)]
            return {"out": _rows(arr64([g[0] for g in got]), 64), "attempts": _rows(np.array([g[1] for g in got], dtype="<u4").view(np.uint8), 4)}
        _add("jj_random_points", [], [("out", 64), ("attempts", 4)], ["ctx", "n", (C.c_uint64, seed), (C.c_uint64, first), (C.c_int, sub), "out", "attempts"],
             lambda n: {}, rp, variant="subgroup%d" % sub)


_codec_rows()


# ---- the MSM family
MSM_TERMS = 3                    # terms per row of the batched rows: the size parameter is the number of ROWS there


def _msm_rows_oracle(S, P, B, t, shared):
    S = S.reshape(B, t, 32)
    P = None if shared else P.reshape(B, t, 64)
    return _rows(np.stack([O.msm(S[b], P[b] if P is not None else PSHARED(t)) for b in range(B)]) if B else np.zeros((0, 64), np.uint8), 64)


def PSHARED(t):
    return points(t, 707)


def ragged_lengths(S):
    """segment lengths with empty segments at the front, in the middle and at the end"""
    lens = [(0, 2, 1, 3, 0, 1)[s % 6] for s in range(S)]
    if S:
        lens[0] = lens[S // 2] = lens[S - 1] = 0
    return lens


def _begin_finish(run, lib, ctx, env):
    job = C.c_void_p()
    rc = lib.jj_msm_begin(ctx, C.c_size_t(run.n), C.c_void_p(run.ptr("s")), C.c_void_p(run.ptr("p")), C.byref(job))
    return rc or lib.jj_msm_finish(job, C.c_void_p(run.ptr("out")))


def _record_sum(got, ins, n, lib):
    """a record's window sums are projective, so its bytes are not canonical: the header fields, the zeroed rest and the point the record sums to
    (jj_msm_combine, host only) are what the oracle pins"""
    rec = np.ascontiguousarray(got)
    hdr = np.frombuffer(rec[:32].tobytes(), "<u4")
    W = int(hdr[2])
    if int(hdr[0]) != 0x504D4A4A or not 1 <= W <= 64 or int(hdr[6]) | (int(hdr[7]) << 32) != n:
        return "record header %r" % (hdr.tolist(),)
    if rec[32:64].any() or rec[64 + 128 * W:].any():
        return "unused space of the record is not zeroed"
    out = np.zeros(64, np.uint8)
    rc = lib.jj_msm_combine(C.c_size_t(1), C.c_void_p(rec.ctypes.data), C.c_void_p(out.ctypes.data))
    want = O.msm(ins["s"], ins["p"])
    return None if rc == 0 and (out == want).all() else "the record sums to another point (rc %d)" % rc


def record_pool():
    """four records of the small-batch layout (64 windows) and the points they sum to"""
    if "recs" not in _POOL:
        s, p = scalars(8, 731), points(8, 733)
        cut = [(0, 1), (1, 4), (4, 4), (4, 8)]              # one term, three, none, four
        _POOL["recs"] = (np.stack([oracle_msm_record(s[a:b], p[a:b]) for a, b in cut]), np.stack([O.msm(s[a:b], p[a:b]) for a, b in cut]))
    return _POOL["recs"]


def _records(n):
    return record_pool()[0][np.arange(n) % 4] if n else np.zeros((0, MSM_PARTIAL_BYTES), np.uint8)


def _records_sum(n):
    return _rows(O.point_sum(record_pool()[1][np.arange(n) % 4]) if n else pt64(J.AFFINE_IDENTITY), 64)


def _msm_family():
    build = lambda n: {"s": scalars(n, 701), "p": points(n, 703)}       # noqa: E731
    one = lambda i, n: {"out": _rows(O.msm(i["s"], i["p"]), 64)}         # noqa: E731
    sp = [("s", 32), ("p", 64)]
    _add("jj_msm", sp, [("out", 64)], ["ctx", "n", "s", "p", "out"], build, one, rows={"out": ONE}, options=({}, {"msm_small_max": 0}), share="msm")
    _add("jj_msm_dev", sp, [("out", 64)], ["ctx", "n", "s", "p", "out"], build, one, rows={"out": ONE}, device=("out",), share="msm")
    _add("jj_msm_begin", sp, [("out", 64)], [], build, one, rows={"out": ONE}, covers=("jj_msm_begin", "jj_msm_finish"), call=_begin_finish, share="msm")
    _add("jj_msm_partial", sp, [("record", MSM_PARTIAL_BYTES)], ["ctx", "n", "s", "p", (C.c_int, 0), (C.c_int, 1), "record"], build,
         lambda i, n: {"record": np.zeros((1, MSM_PARTIAL_BYTES), np.uint8)}, rows={"record": ONE}, verify={"record": _record_sum})
    t = MSM_TERMS
    for shared in (1, 0):
        _add("jj_msm_batch", sp, [("out", 64)], ["ctx", "n", (C.c_size_t, t), "s", "p", (C.c_int, shared), "out"],
             lambda n, shared=shared: {"s": scalars(n * t, 705), "p": PSHARED(t) if shared else points(n * t, 709)},
             lambda i, n, shared=shared: {"out": _msm_rows_oracle(i["s"], i["p"], n, t, shared)}, variant="shared" if shared else "distinct",
             rows={"s": lambda n: n * t, "p": (lambda n: t) if shared else (lambda n: n * t)})

    def ragged_build(S):
        lens = ragged_lengths(S)
        N = sum(lens)
        return {"offsets": np.concatenate([[0], np.cumsum(lens)]).astype("<u8").view(np.uint8), "s": scalars(N, 711), "p": points(N, 713)}

    def ragged_oracle(i, S):
        off = np.frombuffer(i["offsets"].tobytes(), "<u8")
        return {"out": _rows(np.stack([O.msm(i["s"][off[k]:off[k + 1]], i["p"][off[k]:off[k + 1]]) for k in range(S)]) if S else np.zeros((0, 64), np.uint8), 64)}

    _add("jj_msm_ragged", [("offsets", 8), ("s", 32), ("p", 64)], [("out", 64)], ["ctx", "n", "offsets", "s", "p", "out"], ragged_build, ragged_oracle,
         rows={"offsets": lambda S: S + 1, "s": lambda S: sum(ragged_lengths(S)), "p": lambda S: sum(ragged_lengths(S))}, host=("offsets",))
    for mode in (1, 2):
        _add("jj_msm_basis_mul", [("s", 32)], [("out", 64)], ["ctx", ("handle", ("basis", mode)), "n", (C.c_size_t, t), "s", "out"],
             lambda n: {"s": scalars(n * t, 715)}, lambda i, n: {"out": _msm_rows_oracle(i["s"], None, n, t, True)}, variant="mode%d" % mode,
             rows={"s": lambda n: n * t}, share="basis_mul")
    _add("jj_msm_combine_dev", [("records", MSM_PARTIAL_BYTES)], [("out", 64)], ["ctx", "n", "records", "out"], lambda n: {"records": _records(n)},
         lambda i, n: {"out": _records_sum(n)}, rows={"out": ONE}, device=("records",))


BASIS_POINTS = 5                 # the bases of jj_msm_basis_mul hold PSHARED(5); the rows use the first MSM_TERMS of them
_msm_family()


# ---- host-only functions (no context, no device)
def _plan_chunks_expected(n, chunk):
    return list(range(0, n, chunk)) + [n]                 # ramp = 0, quantum = 0: jj_plan_host_chunks' chunks tile [0, n), the last one the remainder


def _host_only():
    _add("jj_msm_combine", [("records", MSM_PARTIAL_BYTES)], [("out", 64)], ["n", "records", "out"], lambda n: {"records": _records(n)},
         lambda i, n: {"out": _records_sum(n)}, rows={"out": ONE}, host_only=True)
    _add("jj_msm_fold_partials", [("parts", 64)], [("out", 64)], ["n", "parts", "out"], lambda n: {"parts": points(n, 801)},
         lambda i, n: {"out": _rows(O.point_sum(i["parts"]), 64)}, rows={"out": ONE}, host_only=True)
    _add("jj_fr_char_le_bits", [], [("out", 256)], ["out"], lambda n: {},
         lambda i, n: {"out": np.unpackbits(_rows(b32(R), 32), axis=1, bitorder="little")}, rows={"out": ONE}, host_only=True, sized=False)
    # the capped writers: the size parameter is the batch; `cap` entries of room -- fewer than, exactly and more than the plan needs
    chunk = 7
    for name, delta in (("small", -1), ("exact", 0), ("large", 2)):
        need = lambda n: len(_plan_chunks_expected(n, chunk))       # noqa: E731
        cap = lambda n, delta=delta, need=need: need(n) + delta     # noqa: E731

        def chunks(i, n, delta=delta, need=need):
            # too little room: nothing written but the count; room to spare: the entries past the count stay as they were (Run.problems)
            want = _rows(np.array(_plan_chunks_expected(n, chunk), "<u8").view(np.uint8), 8)
            return {"bounds": None if delta < 0 else want, "count": _rows(np.array([need(n)], "<u8").view(np.uint8), 8)}

        _add("jj_plan_host_chunks", [], [("bounds", 8), ("count", 8)],
             [(C.c_size_t, lambda n: n), (C.c_size_t, chunk), (C.c_size_t, 0), (C.c_int, 0), "bounds", (C.c_size_t, cap), "count"], lambda n: {}, chunks,
             variant="cap_" + name, rows={"bounds": cap, "count": ONE}, host_only=True, rc=(lambda n, delta=delta: INVALID if delta < 0 else 0))

        def items_of(S):
            off = np.concatenate([[0], np.cumsum(ragged_lengths(S))])
            return [(0, s, int(off[s]), int(off[s + 1])) for s in range(S) if off[s + 1] > off[s]]      # at most 3 terms per segment, slices of 16: one item each, one round

        icap = lambda S, delta=delta: max(0, len(items_of(S)) + delta)     # noqa: E731

        def items(i, S, icap=icap, items_of=items_of):
            need = len(items_of(S))
            want = _rows(np.array(items_of(S), "<u8").reshape(-1, 4).view(np.uint8), 32)
            return {"items": None if icap(S) < need else want, "count": _rows(np.array([need], "<u8").view(np.uint8), 8)}

        _add("jj_plan_msm_ragged_items", [("offsets", 8)], [("items", 32), ("count", 8)],
             ["n", "offsets", (C.c_int, 0), (C.c_int, 0), (C.c_uint64, 0), "items", (C.c_size_t, icap), "count"],
             lambda S: {"offsets": np.concatenate([[0], np.cumsum(ragged_lengths(S))]).astype("<u8").view(np.uint8)}, items, variant="cap_" + name,
             rows={"offsets": lambda S: S + 1, "items": icap, "count": ONE}, host_only=True,
             rc=(lambda S, icap=icap, items_of=items_of: INVALID if icap(S) < len(items_of(S)) else 0))

    def ragged_plan(i, S):
        lens = ragged_lengths(S)
        k = sum(1 for x in lens if x)
        return {"out": _rows(np.array([k, 0, k, 1 if k else 0], "<i8").view(np.uint8), 32)}

    _add("jj_plan_msm_ragged", [("offsets", 8)], [("out", 32)], ["n", "offsets", (C.c_int, 0), (C.c_int, 0), (C.c_uint64, 0), "out"],
         lambda S: {"offsets": np.concatenate([[0], np.cumsum(ragged_lengths(S))]).astype("<u8").view(np.uint8)}, ragged_plan,
         rows={"offsets": lambda S: S + 1, "out": ONE}, host_only=True)
    # jj_plan_msm_host_passes: below 2^19 terms one pass of 2^pass_log2 terms at most (tests/test_abi.py restates the split above that)
    _add("jj_plan_msm_host_passes", [], [("terms", 8), ("passes", 8)], [(C.c_size_t, lambda n: n), (C.c_int, 10), (C.c_int, 1), "terms", "passes"], lambda n: {},
         lambda i, n: {"terms": _rows(np.array([1 << 10], "<u8").view(np.uint8), 8), "passes": _rows(np.array([-(-n // (1 << 10))], "<u8").view(np.uint8), 8)},
         rows={"terms": ONE, "passes": ONE}, host_only=True)
    # jj_plan_msm_basis at up to 8192 points: the mode asked for (1 for auto), 64 windows, the small tables (1296 bytes per point), route 0
    # (tests/test_msm_basis_cpu.py test_plan_properties)
    for mode in (0, 1, 2):
        _add("jj_plan_msm_basis", [], [("out", 32)], [(C.c_size_t, lambda n: n), (C.c_int, mode), (C.c_int, 0), (C.c_uint64, 1 << 40), "out"], lambda n: {},
             lambda i, n, mode=mode: {"out": _rows(np.array([mode or 1, 64, 1296 * n, 0], "<i8").view(np.uint8), 32)}, variant="mode%d" % mode,
             rows={"out": ONE}, host_only=True)


_host_only()


# ---- several devices of one node: shards of the single-device calls on HOST pointers (the GPU test lists device 0 three times)
def _multi_rows():
    by = {c.id: c for c in CASES}
    for fn, src, args in (("jj_multi_varbase_mul", "jj_varbase_mul", ["ctx", "n", "s", "p", "out"]),
                          ("jj_multi_fixedbase_mul", "jj_fixedbase_mul[w7]", ["ctx", ("handle", ("mtable", 0, 7)), "n", "s", "out"]),
                          ("jj_multi_decompress", "jj_decompress[flags3]", ["ctx", "n", "enc", (C.c_uint, 3), "out", "ok"]),
                          ("jj_multi_msm", "jj_msm", ["ctx", "n", "s", "p", "out"]),
                          ("jj_multi_msm_batch", "jj_msm_batch[distinct]", ["ctx", "n", (C.c_size_t, MSM_TERMS), "s", "p", (C.c_int, 0), "out"])):
        s = by[src]
        _add(fn, s.ins, s.outs, args, s.build, s.oracle, rows=s.rows, ctx="multi", share=s.share or s.id)


_multi_rows()

# entry points with a non-const pointer parameter that get no row, each with its reason (tests/test_buffer_cases_cpu.py: the coverage pin)
EXEMPT = {
    "jj_ctx_get_option": "one long long through a scalar out-parameter, no array",
    "jj_device_info": "a fixed int64[4] of device properties, no batch",
    "jj_ctx_profile_read": "drains the timing log of a profiling session, capped by `max`; measurement plumbing",
    "jj_peak_imad32": "one double: a measurement",
    "jj_peak_imad32_samples": "`count` doubles: a measurement",
    "jj_result_pool_stats": "three size_t out-parameters, no array",
    "jj_host_alloc": "returns an address through void**, writes no array",
    "jj_result_acquire": "returns an address through void**, writes no array",
    "jj_msm_basis_info": "a fixed int64[4] describing a handle",
    "jj_msm_allgather": "a collective over an RCCL communicator: its parts (jj_msm_partial, jj_msm_combine_dev) have rows",
    "jj_msm_allgather_begin": "a collective; finished by jj_msm_finish, which has a row",
    "jj_host_free": "takes an address, writes nothing through it",
    "jj_host_register": "page-locks a range, writes nothing through it",
    "jj_host_unregister": "takes an address, writes nothing through it",
    "jj_result_release": "takes an address, writes nothing through it",
    "jj_ctx_set_stream": "takes a stream handle, no array",
    "jj_ctx_set_comm": "takes a communicator and a function address, no array",
}

MAX_ROW_BYTES = max(w for c in CASES for name, w in c.outs if c.nrows(name, 2) == 2)        # the widest per-unit output row of the table
# twice the most bytes one workgroup or one wave can reach past an output's end: a whole workgroup's rows of the widest output, or every unit a
# wave of k_varbase_mont_x1 touches (MONT_X1_UNITS per lane) as 64-byte rows
GUARD = -(-2 * max(K["block"] * MAX_ROW_BYTES, K["wave"] * K["mont_x1_units"] * 64) // ALIGN) * ALIGN


# ---------------------------------------------------------------------------------------------------- one call
ANY = object()


class Run:
    """One call of one row at one size: regions carved into the arenas `place` names, the call, the checks.
    place(name, role) -> arena key; skew(name, role) -> skew; allocs {key: alloc | None}."""

    def __init__(self, case, n, place, skew, allocs, data=None):
        """data: (inputs, expected outputs) instead of the row's own at this size; an expected output of ANY is not compared"""
        self.case, self.n = case, n
        self.inputs, self.expected = case.data(n) if data is None else data
        self.arenas, self.where = {}, {}
        sizes = case.out_bytes(n)
        for name, w in case.ins:
            assert self.inputs[name].shape == (case.nrows(name, n), w), (case.id, name, self.inputs[name].shape)
        for role, names in (("in", [k for k, _ in case.ins]), ("out", [k for k, _ in case.outs])):
            for name in names:
                key = place(name, role)
                a = self.arenas.setdefault(key, Arena())
                a.carve(self.inputs[name].nbytes if role == "in" else sizes[name], skew(name, role), role, name)
                self.where[name] = a
        for key, a in self.arenas.items():
            a.commit(allocs.get(key), {r.name: self.inputs[r.name] for r in a.regions if r.role == "in"})

    def ptr(self, name):
        return self.where[name].ptr(name)

    def call(self, lib, ctx=None, env=None, n=None, swap=None):
        """the return code; n: the size handed to the entry point when it is not the size the regions were carved for; swap: {position in the
        row's argument list: address or None} handed over in place of that pointer argument"""
        c, n = self.case, self.n if n is None else n
        if c.call is not None:
            return c.call(self, lib, ctx, env)
        fn = getattr(lib, c.fn)
        vals = []
        for a in c.args:
            if a == "ctx":
                vals.append(ctx)
            elif a == "n":
                vals.append(C.c_size_t(n))
            elif isinstance(a, str):
                vals.append(C.c_void_p(self.ptr(a)))
            elif a[0] == "handle":
                vals.append(env.handle(a[1]))
            elif a[0] == "handles":
                self._keep = (C.c_void_p * len(a[1]))(*[env.handle(k) for k in a[1]])
                vals.append(C.cast(self._keep, C.c_void_p))
            else:
                vals.append(a[0](a[1](n) if callable(a[1]) else a[1]))
        for i, address in (swap or {}).items():
            vals[i] = C.c_void_p(address)
        types = fn.argtypes
        if types:                                   # region addresses for parameters the binding declares as typed pointers
            assert len(types) == len(vals), (c.fn, len(types), len(vals))
            vals = [C.cast(v, t) if isinstance(v, C.c_void_p) and t is not C.c_void_p and issubclass(t, C._Pointer) else v for v, t in zip(vals, types)]
        return fn(*vals)

    def problems(self, lib=None):
        """every way this call broke the contract: output bytes that differ from the oracle's, guard or input bytes that changed"""
        c, out = self.case, []
        for name, w in c.outs:
            want, a = self.expected[name], self.where[name]
            if want is ANY:
                continue
            if want is None:
                if not a.untouched(name):
                    out.append("%s: written, though the call was to leave it alone" % name)
                continue
            got = a.read(name)
            if name in c.verify:
                p = c.verify[name](got, self.inputs, self.n, lib)
                if p:
                    out.append("%s: %s" % (name, p))
                continue
            want = np.ascontiguousarray(want, dtype=np.uint8).reshape(-1)
            assert want.size <= got.size, (c.id, name, want.size, got.size)
            if want.size < got.size:                 # a capped writer with room to spare: the rest of the room stays as it was
                if (got[want.size:] != a.fill(name)[want.size:]).any():
                    out.append("%s: written past the %d bytes of the result" % (name, want.size))
                got = got[:want.size]
            bad = np.flatnonzero(got != want)
            if bad.size:
                out.append("%s: %d bytes differ from the oracle, the first in row %d (byte %d of it)" % (name, bad.size, bad[0] // w, bad[0] % w))
        for key, a in self.arenas.items():
            out += ["%s arena: %r" % (key, v) for v in a.violations()]
        return out

    def counts(self):
        """(output bytes compared with the oracle, guard bytes verified)"""
        return sum(self.case.out_bytes(self.n).values()), sum(a.guard_bytes() for a in self.arenas.values())
