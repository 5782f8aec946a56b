"""Batches of Schnorr signatures GROUPED BY KEY for jj_sigbatch_keyed_begin, and what the job's finish must write for each.  Plain data (numpy + the
oracle, no GPU import); tests/test_sig_keyed_cases_cpu.py pins every expected value to the oracle, tests/test_gpu_sig_keyed.py runs the same cases
through the C ABI.  Test infrastructure only.

Two families.  regrouped(): every planted variant of tests/sig_batch_cases.py, its signatures brought into a stable order by key -- the sum does not
depend on the order of its terms and z travels with its signature, so the expected bytes are the batch's own.  layout(): signatures made for a
given list of group sizes, for what a regrouping cannot produce (keys without signatures, a key listed twice) and for group boundaries placed where
the kernels can go wrong: k_sig_keyed_terms adds z_i c_i over the lanes of a 64-lane wave that share a key and leaves one sum at every run head --
where a group starts and where a wave starts inside a group; k_sig_keyed_close adds a key's heads, a whole wave striding over them when there
are several.
The check:   out = [8] (sum_i [z_i] R_i + sum_k [sum_{i in k} z_i c_i mod r] A_k - [sum z_i s_i mod r] B)   ->   (0, 1) accept, (0, -1) malformed."""
import functools

import numpy as np

from oracle import c_oracle as O
from tests import sig_batch_cases as SC

R = SC.R
SIZES = (1, 2, 63, 64, 65, 257)                   # regrouped(): the sizes of every planted variant
TRIANGLE = tuple(range(1, 24))                    # groups of 1, 2, 3, ... signatures: 276 in all, 23 residues mod 64, past one workgroup ([3] * 90: every residue)
LARGE = 4200                                      # one group of 66 heads: the close kernel's lane loop wraps (more heads than lanes)


class Keyed:
    """one call's arguments (host arrays) + what jj_msm_finish must write"""

    def __init__(self, name, base, keys, offsets, r, s, c, z, flags, expected):
        self.name, self.base, self.keys, self.r, self.s, self.c, self.z, self.flags, self.expected = name, base, keys, r, s, c, z, flags, expected
        self.offsets = np.asarray(offsets, dtype=np.uint64)
        assert self.offsets.shape == (len(keys) + 1,) and int(self.offsets[-1]) == len(s)

    @property
    def n(self):
        return len(self.s)

    @property
    def K(self):
        return len(self.keys)

    def sizes(self):
        return np.diff(self.offsets.astype(np.int64))

    def has_empty_group(self):
        return bool((self.sizes() == 0).any())

    def arrays(self):
        """R, s, c, z: the four per-signature arrays, in the order of the C arguments"""
        return self.r, self.s, self.c, self.z

    def expanded(self):
        """the batch jj_sigbatch_begin takes: a32[k] repeated over its group (a key without signatures drops out)"""
        a = np.repeat(self.keys, self.sizes(), axis=0) if self.K else np.zeros((0, 32), np.uint8)
        return SC.Batch(self.name + " expanded", self.base, self.r, a, self.s, self.c, self.z, self.flags, self.expected)


def heads(offsets):
    """per key: the run heads of k_sig_keyed_terms -- the group's first signature and every multiple of 64 strictly inside the group"""
    o = [int(x) for x in offsets]
    return [([lo] + [m for m in range((lo // 64 + 1) * 64, hi, 64)]) if hi > lo else [] for lo, hi in zip(o[:-1], o[1:])]


def group(a):
    """(keys, offsets, order): the distinct rows of a (n, 32), the CSR offsets and a stable order by key (plain numpy, independent of Engine)"""
    a = np.asarray(a, np.uint8)
    if len(a) == 0:
        return np.zeros((0, 32), np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.int64)
    keys, inverse = np.unique(a, axis=0, return_inverse=True)
    inverse = inverse.reshape(-1)
    order = np.argsort(inverse, kind="stable")
    counts = np.bincount(inverse, minlength=len(keys))
    return keys, np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64), order


def regrouped(n, variant="valid", k=None):
    """SC.batch(n, variant, k) with its signatures grouped by key: keys = the distinct rows of its a32"""
    b = SC.batch(n, variant, k)
    keys, offsets, order = group(b.a)
    return Keyed(b.name + " regrouped", b.base, keys, offsets, b.r[order], b.s[order], b.c[order], b.z[order], b.flags, b.expected)


@functools.lru_cache(maxsize=None)
def _signatures(key_index, seed):
    """valid signatures under the given keys of SC's pool (a tuple of indices), built as SC._valid builds them: (r32, s32, c32, z16), read-only"""
    ki = np.array(key_index, dtype=np.int64)
    n = len(ki)
    _, _, _, Renc = SC._pools("prime")
    rng = np.random.default_rng(0x6B00 + seed)
    mi = rng.integers(0, SC.NNONCES, n)
    c = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    c[:, 31] &= 0x0F
    z = rng.integers(0, 256, size=(n, 16), dtype=np.uint8)
    z[~z.any(axis=1), 0] = 1
    s = np.zeros((n, 32), np.uint8)
    for i in range(n):
        ci = SC.to_int(c[i]) % R
        c[i] = SC.b32(ci)
        s[i] = SC.b32((SC.NONCE[mi[i]] + ci * SC.SK[ki[i]]) % R)
    out = (Renc[mi] if n else np.zeros((0, 32), np.uint8), s, c, z)
    for x in out:
        x.setflags(write=False)
    return out


def layout(name, sizes, variant="valid", pos=None, key_index=None, bad_key=None, seed=0):
    """groups of the given sizes; group g is checked under key key_index[g] of SC's pool (default g mod 8: a list longer than the pool repeats
    keys, each listing a group of its own).  variant: "valid", or "bad_s" planted at signature `pos` (expected -[8 z delta] B, as in SC.batch).
    bad_key: the index of a group whose key is replaced by an off-curve encoding -> malformed."""
    sizes = list(sizes)
    K = len(sizes)
    key_index = list(key_index) if key_index is not None else [g % SC.NKEYS for g in range(K)]
    assert len(key_index) == K
    B = SC.bases()["prime"]
    Aenc = SC._pools("prime")[2]
    keys = Aenc[key_index].copy() if K else np.zeros((0, 32), np.uint8)
    per_sig = tuple(int(key_index[g]) for g in range(K) for _ in range(sizes[g]))
    r, s, c, z = _signatures(per_sig, seed)
    expected = SC.IDENTITY
    if variant == "bad_s":
        s0, s = SC.to_int(s[pos]), s.copy()
        s[pos] = SC.b32((s0 + 5) % R)
        delta = (SC.to_int(s[pos]) - s0) % R
        expected = O.point_op("neg", SC._mul(SC.to_int(z[pos]) * delta % R, O.point_op("mul_by_cofactor", B[None])[0])[None])[0]
    elif variant != "valid":
        raise KeyError(variant)
    if bad_key is not None:
        keys[bad_key] = SC.off_curve_encoding()
        if len(per_sig):                                             # n = 0: nothing is read, the identity
            expected = SC.MALFORMED
    return Keyed(name, B, keys, np.concatenate([[0], np.cumsum(sizes)]) if K else [0], r, s, c, z, 0, expected)


def regrouped_cases():
    return [regrouped(n, v, k) for n in SIZES for v, k in SC.variants(n)]


def planted_cases():
    """layouts a regrouping cannot produce"""
    return [
        layout("empty group first", [0, 20, 30]),
        layout("empty group last", [20, 30, 0]),
        layout("empty group between", [20, 0, 30]),
        layout("empty group between, bad s after it", [20, 0, 30], "bad_s", 20),
        layout("off-curve key without signatures", [20, 0, 30], bad_key=1),
        layout("off-curve key without signatures, last", [70, 0], bad_key=1),
        layout("off-curve key with signatures", [20, 3, 30], bad_key=1),
        layout("one key listed twice, its signatures split", [30, 40, 25], key_index=[3, 5, 3]),
        layout("one key listed twice, adjacent, split inside a wave", [10, 10], key_index=[2, 2]),
        layout("all signatures under one key", [100]),
        layout("every group of one", [1] * 130),
        layout("every group of one, bad s at a wave's first lane", [1] * 130, "bad_s", 64),
        layout("300 groups of one: two workgroups of keys", [1] * 300),
        layout("300 groups of one, the last key off-curve", [1] * 300, bad_key=299),
        layout("no keys, no signatures", []),
        layout("three keys, no signatures", [0, 0, 0]),
        layout("three keys (one off-curve), no signatures: nothing is read", [0, 0, 0], bad_key=2),
    ]


def boundary_cases():
    """group sizes whose boundaries fall on the wave (64) and workgroup (256) edges of the kernels"""
    tri_end = int(np.sum(TRIANGLE))
    return [
        layout("sizes [1]", [1]),
        layout("sizes [63, 1]", [63, 1]),
        layout("sizes [63, 1], bad s in the group of one", [63, 1], "bad_s", 63),
        layout("sizes [64, 64]", [64, 64]),
        layout("sizes [64, 64], bad s at the second group's head", [64, 64], "bad_s", 64),
        layout("sizes [65]", [65]),
        layout("sizes [65], bad s in the second wave", [65], "bad_s", 64),
        layout("sizes 1, 2, 3, ..., 23", TRIANGLE),
        layout("sizes 1, 2, 3, ..., 23, bad s in the last group", TRIANGLE, "bad_s", tri_end - 1),
        layout("90 groups of three", [3] * 90),
        layout("90 groups of three, bad s in a group across a wave edge", [3] * 90, "bad_s", 128),
        layout("sizes [0, 5, 0, 0, 300, 0]", [0, 5, 0, 0, 300, 0]),
        layout("sizes [0, 5, 0, 0, 300, 0], bad s", [0, 5, 0, 0, 300, 0], "bad_s", 256),
        layout("one group of %d" % LARGE, [LARGE], seed=1),
        layout("one group of %d, bad s in its last wave" % LARGE, [LARGE], "bad_s", LARGE - 10, seed=1),
    ]


@functools.lru_cache(maxsize=None)
def all_cases():
    return tuple(regrouped_cases() + planted_cases() + boundary_cases())


def keyed_evaluation(case):
    """what the issue defines, evaluated term by term by the oracle: decode the n + K encodings, the n + K + 1 scalars with Python integers, O.msm,
    three doublings.  n = 0: the identity, nothing is read."""
    n, K = case.n, case.K
    if n == 0:
        return SC.IDENTITY
    rp, rok = O.decompress(case.r, case.flags)
    ap, aok = O.decompress(case.keys, case.flags)
    sv = [SC.to_int(x) for x in case.s]
    bad = not rok.all() or not aok.all() or any(x >= R for x in sv)
    rp[rok == 0] = SC.IDENTITY
    ap[aok == 0] = SC.IDENTITY
    zv = [SC.to_int(x) for x in case.z]
    cv = [SC.to_int(x) % R for x in case.c]
    o = [int(x) for x in case.offsets]
    folded = [sum(zv[i] * cv[i] for i in range(o[k], o[k + 1])) % R for k in range(K)]
    sigma = sum(zi * si for zi, si in zip(zv, sv)) % R
    scalars = np.stack([SC.b32(zi) for zi in zv] + [SC.b32(t) for t in folded] + [SC.b32((R - sigma) % R)])
    total = O.msm(scalars, np.concatenate([rp, ap, case.base[None]]))[None]
    for _ in range(3):
        total = O.point_op("double", total)
    return SC.MALFORMED if bad else total[0]
