"""
Call sequences on ONE context, as plain data and constructors (numpy, the oracle, Python integers): no GPU import.

Every other GPU file holds one feature at a time to the oracle, on a context made for it.  A context is full of state that its entry points
share -- lane 0's MSM buffers mean different things to jj_msm, jj_msm_batch / jj_msm_basis_mul, jj_msm_ragged and jj_msm_dev; counters and
histogram halves are "left clean" by whichever kernel ran last; the WorkSet's SoA stride is the last call's n; the staging buffers and the ring
of eight host slots behind every device-bound result serve everybody -- so what a call computes may depend on the call BEFORE it.  This file
builds the call kinds of two groups and, per group, a walk:

  group M  the entry points that use lane 0's MSM workspaces (13 kinds)
  group W  the entry points that use the WorkSet and the staging buffers (19 kinds)
  walk     one fixed, seeded order of k^2 + 1 calls of a group's k kinds in which every ordered pair (A, B), (A, A) included, occurs at
           consecutive positions exactly once: an Eulerian circuit of the complete digraph with loops on k vertices

A Kind carries seeded inputs (numpy), the oracle's answer (computed once, on first use) and a function that makes the call on an Engine with
the inputs in whatever form the caller converted them to (numpy arrays or torch device tensors).  tests/test_sequence_cases_cpu.py pins the
walks, the sizes against the thresholds parsed from the sources, the planted rows and the expected values (two oracle routes);
tests/test_gpu_sequences.py runs the walks.
"""
import os
import random
import re

import numpy as np

from msm_bucket_cases import buckets_per_window
from oracle import c_oracle as O
from oracle import jubjub_ref as J
from util import Q, arr32, pt64, rand_points, rand_scalars

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
IDENTITY = np.concatenate([np.zeros(32, np.uint8), np.frombuffer((1).to_bytes(32, "little"), np.uint8)])
WALK_SEED = 0x57414C4B
MSM_REC_BYTES = 8256
SM_W = 64                                             # windows of the small-batch layout (the header of an empty record names them)


def source_constants():
    """the thresholds the sizes below are steered by, read from jj_msm.hip and jj_engine.h"""
    msm = open(os.path.join(ROOT, "jubjub_amd", "csrc", "jj_msm.hip")).read()
    eng = open(os.path.join(ROOT, "jubjub_amd", "csrc", "jj_engine.h")).read()

    def one(text, pattern):
        m = re.search(pattern, text)
        assert m, pattern
        return m

    out = {}
    m = one(msm, r"constexpr\s+size_t\s+MSM_LARGE_MIN\s*=\s*\(size_t\)\s*(\d+)\s*<<\s*(\d+)\s*;")
    out["MSM_LARGE_MIN"] = int(m.group(1)) << int(m.group(2))
    m = one(msm, r"constexpr\s+size_t\s+MSM_BATCH_MAX\s*=\s*(\d+)\s*<<\s*(\d+)\s*;")
    out["MSM_BATCH_MAX"] = int(m.group(1)) << int(m.group(2))
    m = one(msm, r"constexpr\s+size_t\s+MSM_BATCH_WAVES\s*=\s*(\d+)\s*;")
    out["MSM_BATCH_WAVES"] = int(m.group(1))
    m = one(msm, r"constexpr\s+size_t\s+MSM_BATCH_SLICE_MIN\s*=\s*(\d+)\s*;")
    out["MSM_BATCH_SLICE_MIN"] = int(m.group(1))
    m = one(msm, r"return\s+n\s*>=\s*\(\(size_t\)1\s*<<\s*(\d+)\)\s*\?\s*(\d+)\s*:\s*n\s*>=\s*MSM_LARGE_MIN\s*\?\s*(\d+)\s*:\s*(\d+)\s*;")
    out["WIDE_LOG2"], out["W_WIDE"], out["W_LARGE"], out["W_MID"] = (int(m.group(i)) for i in (1, 2, 3, 4))
    m = one(msm, r"const\s+bool\s+two_pass\s*=\s*B\s*>\s*(\d+)\s*\|\|")
    out["ONE_PASS_BUCKETS"] = int(m.group(1))
    m = one(eng, r"int\s+msm_small_max\s*=\s*(\d+)\s*<<\s*(\d+)\s*;")
    out["msm_small_max"] = int(m.group(1)) << int(m.group(2))
    m = one(eng, r"int\s+vb_quad_max\s*=\s*(\d+)\s*;")
    out["vb_quad_max"] = int(m.group(1))
    m = one(eng, r"int\s+msm_segments\s*=\s*(-?\d+)\s*;")
    out["msm_segments"] = int(m.group(1))
    m = one(eng, r"int\s+msm_lanes\s*=\s*(\d+)\s*;")
    out["msm_lanes"] = int(m.group(1))
    m = one(eng, r"uint8_t\s+host_out\[(\d+)\]\[64\]\s*;")
    out["HOST_OUT_SLOTS"] = int(m.group(1))
    return out


def msm_path(n, K):
    """what a default context's jj_msm does with n terms: "small" (two launches, 64 windows), or (windows, sort, accumulation)"""
    if n <= K["msm_small_max"]:
        return "small"
    W = K["W_WIDE"] if n >= 1 << K["WIDE_LOG2"] else K["W_LARGE"] if n >= K["MSM_LARGE_MIN"] else K["W_MID"]
    return (W, "two-pass" if buckets_per_window(W) > K["ONE_PASS_BUCKETS"] else "one-pass", "segments" if n >= K["MSM_LARGE_MIN"] else "chunks")


def batch_slices(rows, n, K):
    """msm_batch_slices (jj_msm.hip): slices a row's terms are cut into"""
    want, most = -(-K["MSM_BATCH_WAVES"] // rows), max(1, n // K["MSM_BATCH_SLICE_MIN"])
    return max(1, min(want, most))


# ------------------------------------------------------------------------------------------------------------------ inputs
_POOL = None


def pool():
    """2^14 curve points from the oracle: prime-order and full-group points interleaved.  Longer inputs repeat them (distinct scalars): the
    oracle's side of a 2^18-term sum stays cheap"""
    global _POOL
    if _POOL is None:
        a, b = rand_points(0x5EC1, 1 << 13, subgroup=True), rand_points(0x5EC2, 1 << 13)
        _POOL = np.stack([a, b], axis=1).reshape(-1, 64)
        _POOL.setflags(write=False)
    return _POOL


def points_for(count, offset=0):
    idx = (np.arange(count, dtype=np.int64) * 7 + offset) % pool().shape[0]
    return np.ascontiguousarray(pool()[idx])


def torsion():
    """the eight points of small order: j G8, G8 = r G"""
    g8 = J.scalar_mul_fast(J.GENERATOR, J.R_MOD)
    return np.stack([pt64(J.scalar_mul_fast(g8, j) if j else J.AFFINE_IDENTITY) for j in range(8)])


def nonsquare_vs(count, seed):
    """v for which (v^2 - 1) / (1 + d v^2) is no square: no point has this v"""
    rng, out = random.Random(seed), []
    while len(out) < count:
        v = rng.randrange(Q)
        u2 = (v * v - 1) * pow(1 + J.EDWARDS_D * v * v, -1, Q) % Q
        if u2 and pow(u2, (Q - 1) // 2, Q) == Q - 1:
            out.append(v)
    return out


DEC_PLANTS = ("v>=q", "nonsquare", "u=0,sign,v=1", "u=0,sign,v=q-1", "junk", "small-order", "coset")


def decoder_rows(n, seed):
    """(encodings, {plant name: row indices}): n compressed points with, every 9th row, a planted one of the kinds DEC_PLANTS in turn -- v not
    below q, a v of no point, u = 0 with the sign bit set (ZIP-216 refuses, flags 0 accepts), raw bytes, a point of small order, a point outside
    the prime-order subgroup (a subgroup point plus a point of small order)"""
    pts = points_for(n, offset=seed)
    enc = O.compress(pts)
    rng = np.random.default_rng(seed)
    tors = torsion()
    nsq = nonsquare_vs(4, seed)
    where = {k: [] for k in DEC_PLANTS}
    for a, i in enumerate(range(0, n, 9)):
        kind = DEC_PLANTS[a % len(DEC_PLANTS)]
        sign = int(rng.integers(0, 2)) << 255
        if kind == "v>=q":
            e = arr32([(Q + int(rng.integers(0, 1 << 30))) | sign])[0]
        elif kind == "nonsquare":
            e = arr32([nsq[a % len(nsq)] | sign])[0]
        elif kind == "u=0,sign,v=1":
            e = arr32([1 | (1 << 255)])[0]
        elif kind == "u=0,sign,v=q-1":
            e = arr32([(Q - 1) | (1 << 255)])[0]
        elif kind == "junk":
            e = rng.integers(0, 256, size=32, dtype=np.uint8)
        elif kind == "small-order":
            e = O.compress(tors[1 + a % 7][None])[0]
        else:
            sub = pool()[2 * (a % 4096)]                                     # even rows of the pool: prime order
            e = O.compress(O.point_op("add", sub[None], tors[1 + a % 7][None]))[0]
        enc[i] = e
        where[kind].append(i)
    return enc, where


def _mask_bits(scalars, bits):
    return scalars & np.frombuffer(((1 << bits) - 1).to_bytes(32, "little"), dtype=np.uint8)


# ------------------------------------------------------------------------------------------------------------------ kinds
class Kind:
    """name; args: {name: numpy array}; call(eng, a, res) with a = args converted by the caller (-> one result or a tuple, or a Deferred);
    want(): the oracle's answer as a tuple of numpy arrays, computed once; setup(eng, a) -> what `call` finds as res[name] (made before the
    walk); path: what the size was chosen to reach (pinned by the CPU test); host_args: names of args that stay numpy whatever the walk"""

    def __init__(self, name, args, call, want, path=None, setup=None, host_args=()):
        self.name, self.args, self.call, self._want_fn, self.path, self.setup, self.host_args = name, args, call, want, path, setup, host_args
        self._want = None
        for v in args.values():
            v.setflags(write=False)

    def want(self):
        if self._want is None:
            w = self._want_fn(self.args)
            self._want = tuple(w) if isinstance(w, tuple) else (w,)
            for v in self._want:
                v.setflags(write=False)
        return self._want

    def __repr__(self):
        return self.name


class Deferred:
    """a call whose result arrives later: finish() after the NEXT call of the walk has been made"""

    def __init__(self, finish):
        self.finish = finish


def _msm_kind(idx, n, seed, path):
    args = {"s": rand_scalars(seed, n, full_width=True), "p": points_for(n, offset=seed)}
    return Kind("M%d:msm[%d]" % (idx, n), args, lambda eng, a, res: eng.msm(a["s"], a["p"]),
                lambda a: O.msm(a["s"], a["p"]) if n <= 1000 else O.msm_pippenger(a["s"], a["p"]), path=path)


def _batch_want(a):
    s, p = a["s"], a["p"]
    return np.stack([O.msm(s[b], p if p.ndim == 2 else p[b]) for b in range(s.shape[0])])


def _ragged_want(a):
    s, p, o = a["s"], a["p"], a["offsets"]
    return np.stack([O.msm(s[int(o[k]):int(o[k + 1])], p[int(o[k]):int(o[k + 1])]) for k in range(len(o) - 1)])


def kinds_m(K=None):
    """group M: the entry points that use lane 0's MSM workspaces"""
    K = K or source_constants()
    bmax = K["MSM_BATCH_MAX"]
    out = [
        _msm_kind(1, 700, 101, "small"),
        _msm_kind(2, 20000, 102, (23, "one-pass", "chunks")),
        _msm_kind(3, K["MSM_LARGE_MIN"] + 5, 103, (17, "two-pass", "segments")),
        _msm_kind(4, (1 << K["WIDE_LOG2"]) + 3, 104, (16, "two-pass", "segments")),
    ]
    # 5: few long rows over shared points -> slices and arrival counters; 6: many short rows, one slice each; 7: the jobs route
    n5 = 4000
    out.append(Kind("M5:msm_batch[2x%d,shared]" % n5, {"s": rand_scalars(105, 2 * n5, full_width=True).reshape(2, n5, 32), "p": points_for(n5, offset=105)},
                    lambda eng, a, res: eng.msm_batch(a["s"], a["p"]), _batch_want, path=("batched", "slices")))
    out.append(Kind("M6:msm_batch[50x20,distinct]", {"s": rand_scalars(106, 50 * 20, full_width=True).reshape(50, 20, 32), "p": points_for(50 * 20, offset=106).reshape(50, 20, 64)},
                    lambda eng, a, res: eng.msm_batch(a["s"], a["p"]), _batch_want, path=("batched", "one slice")))
    n7 = bmax + 1
    out.append(Kind("M7:msm_batch[3x%d,jobs]" % n7, {"s": rand_scalars(107, 3 * n7, full_width=True).reshape(3, n7, 32), "p": points_for(3 * n7, offset=107).reshape(3, n7, 64)},
                    lambda eng, a, res: eng.msm_batch(a["s"], a["p"]), _batch_want, path=("jobs",)))
    lengths = [0, 1, 17, 5000, bmax + 7, 0, 300]
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    N = int(offsets[-1])
    out.append(Kind("M8:msm_ragged%s" % lengths, {"s": rand_scalars(108, N, full_width=True), "p": points_for(N, offset=108), "offsets": offsets},
                    lambda eng, a, res: eng.msm_ragged(a["s"], a["p"], a["offsets"]), _ragged_want, path=tuple(lengths), host_args=("offsets",)))
    # 9: rows of m < n terms over the resident tables of a "points" basis; 10: one row over the window table of a "windows" basis (a job on lane 0)
    nb9, m9 = 3000, 2000
    out.append(Kind("M9:msm_basis_mul[points,3x%d of %d]" % (m9, nb9), {"s": rand_scalars(109, 3 * m9, full_width=True).reshape(3, m9, 32), "basis": points_for(nb9, offset=109)},
                    lambda eng, a, res: eng.msm_basis_mul(res["M9"], a["s"]),
                    lambda a: np.stack([O.msm(a["s"][b], a["basis"][:m9]) for b in range(3)]), path=("points", m9, nb9),
                    setup=lambda eng, a: ("M9", eng.msm_basis(a["basis"], mode="points"))))
    nb10, m10 = bmax + 808, bmax + 300
    out.append(Kind("M10:msm_basis_mul[windows,%d of %d]" % (m10, nb10), {"s": rand_scalars(110, m10, full_width=True), "basis": points_for(nb10, offset=110)},
                    lambda eng, a, res: eng.msm_basis_mul(res["M10"], a["s"]),
                    lambda a: O.msm_pippenger(a["s"], a["basis"][:m10]), path=("windows", m10, nb10),
                    setup=lambda eng, a: ("M10", eng.msm_basis(a["basis"], mode="windows"))))
    a11 = {"s": rand_scalars(111, 20000, full_width=True), "p": points_for(20000, offset=111)}
    out.append(Kind("M11:msm_dev[20000]", a11, lambda eng, a, res: eng.msm_dev(a["s"], a["p"]), lambda a: O.msm_pippenger(a["s"], a["p"]),
                    path=(23, "one-pass", "chunks")))

    def partial_combine(eng, a, res):
        recs = [eng.msm_partial(a["s"], a["p"], g, 3) for g in range(3)]
        if isinstance(recs[0], np.ndarray):
            return eng.msm_combine(np.stack(recs))
        import torch

        return eng.msm_combine(torch.stack(recs))

    a12 = {"s": rand_scalars(112, 20000, full_width=True), "p": points_for(20000, offset=112)}
    out.append(Kind("M12:msm_partial[20000,g of 3]+combine", a12, partial_combine, lambda a: O.msm_pippenger(a["s"], a["p"]), path=(23, "one-pass", "chunks")))

    def begin_host(eng, a, res):
        job = eng.msm_begin(a["s"], a["p"])
        return Deferred(lambda: eng.msm_finish(job))

    a13 = {"s": rand_scalars(113, 20000, full_width=True), "p": points_for(20000, offset=113)}
    out.append(Kind("M13:msm_begin[20000,host arrays] finished after the next call", a13, begin_host, lambda a: O.msm_pippenger(a["s"], a["p"]),
                    path=(23, "one-pass", "chunks"), host_args=("s", "p")))
    return out


def kinds_w(K=None):
    """group W: the entry points that use the WorkSet (ext SoA, scratch, var-base tables, cursor) and the staging buffers; big and small sizes
    alternate so that the SoA stride changes from call to call"""
    K = K or source_constants()
    base = pt64(J.GENERATOR)
    base2 = np.array(pool()[5])
    tors = torsion()

    def vb_want(a):
        return O.varbase_mul(a["s"], a["p"])

    def sp(n, seed, full=True):
        return {"s": rand_scalars(seed, n, full_width=full), "p": points_for(n, offset=seed)}

    out = []
    n1 = K["vb_quad_max"] + 7233
    out.append(Kind("W1:varbase_mul[%d]" % n1, sp(n1, 201), lambda eng, a, res: eng.varbase_mul(a["s"], a["p"]), vb_want, path="ladder"))
    out.append(Kind("W2:varbase_mul[5]", sp(5, 202), lambda eng, a, res: eng.varbase_mul(a["s"], a["p"]), vb_want, path="quad"))
    out.append(Kind("W3:varbase_mul_vartime[3000]", sp(3000, 203), lambda eng, a, res: eng.varbase_mul_vartime(a["s"], a["p"]), vb_want))
    a4 = {"a": rand_scalars(204, 1000, full_width=True), "p": points_for(1000, offset=204), "b": rand_scalars(1204, 1000, full_width=True), "q": points_for(1000, offset=1204)}
    out.append(Kind("W4:varbase_mul2_vartime[1000]", a4, lambda eng, a, res: eng.varbase_mul2_vartime(a["a"], a["p"], a["b"], a["q"]),
                    lambda a: O.point_op("add", O.varbase_mul(a["a"], a["p"]), O.varbase_mul(a["b"], a["q"]))))
    a5 = {"k": rand_scalars(205, 1, full_width=True).reshape(32), "p": points_for(700, offset=205)}
    out.append(Kind("W5:varbase_mul_scalar[700]", a5, lambda eng, a, res: eng.varbase_mul_scalar(a["k"], a["p"]),
                    lambda a: O.varbase_mul(np.repeat(a["k"][None], 700, axis=0), a["p"])))

    def table(name, b, wbits):
        return lambda eng, a: (name, eng.fixedbase_table(b, wbits))

    out.append(Kind("W6:fixedbase_mul[comb,4097]", {"s": rand_scalars(206, 4097, full_width=True)}, lambda eng, a, res: eng.fixedbase_mul(res["comb"], a["s"]),
                    lambda a: O.fixedbase_mul(a["s"], base), setup=table("comb", base, 0)))
    out.append(Kind("W7:fixedbase_mul[13-bit table,300]", {"s": rand_scalars(207, 300, full_width=True)}, lambda eng, a, res: eng.fixedbase_mul(res["w13"], a["s"]),
                    lambda a: O.fixedbase_mul(a["s"], base2), setup=table("w13", base2, 13)))
    out.append(Kind("W8:fixedbase_multi_mul[comb+6-bit,513]", {"s": rand_scalars(208, 2 * 513, full_width=True).reshape(2, 513, 32)},
                    lambda eng, a, res: eng.fixedbase_multi_mul([res["comb"], res["w6"]], a["s"]),
                    lambda a: O.point_op("add", O.fixedbase_mul(a["s"][0], base), O.fixedbase_mul(a["s"][1], base2)), setup=table("w6", base2, 6)))
    bits = [64, 64, 64]
    cb = np.array(pool()[10:13])

    def composite_want(a):
        acc = None
        for b in range(3):
            t = O.fixedbase_mul(_mask_bits(a["s"][b], bits[b]), cb[b])
            acc = t if acc is None else O.point_op("add", acc, t)
        return acc

    out.append(Kind("W9:fixedbase_composite_mul[64,64,64;100]", {"s": rand_scalars(209, 3 * 100, full_width=True).reshape(3, 100, 32)},
                    lambda eng, a, res: eng.fixedbase_composite_mul(res["composite"], a["s"]), composite_want,
                    setup=lambda eng, a: ("composite", eng.fixedbase_composite_table(cb, bits))))
    out.append(Kind("W10:point_add[1000]", {"p": points_for(1000, offset=210), "q": points_for(1000, offset=1210)},
                    lambda eng, a, res: eng.point_add(a["p"], a["q"]), lambda a: O.point_op("add", a["p"], a["q"])))
    out.append(Kind("W11:mul_by_cofactor[3]", {"p": points_for(3, offset=211)}, lambda eng, a, res: eng.mul_by_cofactor(a["p"]),
                    lambda a: O.point_op("mul_by_cofactor", a["p"])))
    enc12, _ = decoder_rows(2049, 212)
    out.append(Kind("W12:decompress[flags 15,2049]", {"enc": enc12}, lambda eng, a, res: eng.decompress(a["enc"], 1 | 2 | 4 | 8), lambda a: O.decompress(a["enc"], 15)))
    enc13, _ = decoder_rows(7, 213)
    out.append(Kind("W13:decompress[flags 0,7]", {"enc": enc13}, lambda eng, a, res: eng.decompress(a["enc"], 0), lambda a: O.decompress(a["enc"], 0)))
    out.append(Kind("W14:compress[777]", {"p": points_for(777, offset=214)}, lambda eng, a, res: eng.compress(a["p"]), lambda a: O.compress(a["p"])))
    ext = O.varbase_mul_ext(rand_scalars(215, 4097), points_for(4097, offset=215))         # (U, V, Z, T1, T2): Z neither 0 nor 1
    ext[2048, 64:96] = 0                                                                     # one row with Z = 0: skipped by the shared inversion, (0, 0) out
    out.append(Kind("W15:batch_normalize[4097,one Z=0]", {"ext": ext}, lambda eng, a, res: eng.batch_normalize(a["ext"]), lambda a: O.batch_normalize(a["ext"])))
    out.append(Kind("W16:point_sum[5000]", {"p": points_for(5000, offset=216)}, lambda eng, a, res: eng.point_sum(a["p"]), lambda a: O.point_sum(a["p"])))
    p17 = np.array(pool()[0:1200:2])                                                         # 600 prime-order points ...
    p17 = O.point_op("add", p17, tors[np.arange(600) * 5 % 8])                               # ... moved into all eight cosets (5 i mod 8 = 0: left alone)
    out.append(Kind("W17:is_torsion_free[600,cosets]", {"p": p17}, lambda eng, a, res: eng.predicate("is_torsion_free", a["p"]),
                    lambda a: O.predicate("is_torsion_free", a["p"])))
    a18 = rand_scalars(218, 300, full_width=True)
    a18[:100] = O.field_op(O.FQ, "square", rand_scalars(1218, 100, full_width=True))[0]      # squares for sure; the rest: about half
    a18[100] = 0
    out.append(Kind("W18:fq_sqrt[300]", {"a": a18}, lambda eng, a, res: eng.field_unary_ok("fq", "sqrt", a["a"]), lambda a: O.field_op(O.FQ, "sqrt", a["a"])))
    out.append(Kind("W19:to_niels[65]", {"p": points_for(65, offset=219)}, lambda eng, a, res: eng.to_niels(a["p"]), lambda a: O.to_niels(a["p"])))
    return out


# ------------------------------------------------------------------------------------------------------------------ walks
def euler_walk(k, seed=WALK_SEED):
    """k^2 + 1 vertices of {0 .. k-1}: a closed walk over every ordered pair (a, b), (a, a) included, exactly once (Hierholzer on the complete
    digraph with loops; the order each vertex leaves by its edges is shuffled by `seed`)"""
    rng = random.Random(seed * 1000003 + k)
    nxt = []
    for _ in range(k):
        targets = list(range(k))
        rng.shuffle(targets)
        nxt.append(targets)
    stack, walk = [rng.randrange(k)], []
    while stack:
        v = stack[-1]
        if nxt[v]:
            stack.append(nxt[v].pop())
        else:
            walk.append(stack.pop())
    walk.reverse()
    return walk


def one_cycle(k, seed=WALK_SEED):
    """every vertex once, in a seeded order"""
    order = list(range(k))
    random.Random(seed * 7919 + k).shuffle(order)
    return order


def empty_record(n=0, windows=SM_W):
    """the record jj_msm_partial leaves for a part that owns no window: magic, version 2, the layout's windows, one record, no window present, n"""
    rec = np.zeros(MSM_REC_BYTES, np.uint8)
    rec[:32] = np.frombuffer(np.array([0x504D4A4A, 2, windows, 1, 0, 0, n & 0xFFFFFFFF, n >> 32], dtype="<u4").tobytes(), np.uint8)
    return rec
