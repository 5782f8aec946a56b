"""Batches of Schnorr signatures for jj_sigverify_each, built with the oracle, and the verdict byte every unit must get in both modes.
Plain data (numpy + the oracle, no GPU import); tests/test_sig_each_cases_cpu.py pins every expected byte to the oracle's term-by-term evaluation,
tests/test_emu_sig_each.py and tests/test_gpu_sigverify_each.py run the same units through the host emulation and the C ABI.  Test
infrastructure only.

The valid units are those of tests/sig_batch_cases.py (R = [k]B, A = [sk]B, s = k + c sk mod r; its pools of keys and nonces), repeated beyond
POOL units so that a large batch costs no oracle work per unit; the planted units sit at sig_batch_cases.positions(n), a few per batch, so a
size has several batches.  Every expected byte is a closed form:
    cofactored    OK iff [8]([s]B - [c mod r]A - R) = O            cofactorless    OK iff [s]B - [c mod r]A - R = O
    MALFORMED (both modes) iff R or A does not decode under the batch's flags, or s >= r."""
import functools

import numpy as np

from oracle import c_oracle as O
from tests import sig_batch_cases as SC
from tests.sig_batch_cases import NONCE, SK, Q, R, b32, pt64, to_int

REJECT, OK, MALFORMED = 0, 1, 2
ZIP216, COFACTORLESS = 1, 16
POOL = 1024

# planted kinds -> (cofactored, cofactorless) verdicts.  The two non-canonical kinds must not share a batch (ZIP-216 is a flag of the call): they
# sit six apart, and a batch plants at most five kinds.
KINDS = [
    ("noncanonical_a_zip216", MALFORMED, MALFORMED),      # sig_batch_cases' variants, per unit
    ("torsion_r", OK, REJECT),
    ("bad_s", REJECT, REJECT),
    ("bad_r", REJECT, REJECT),
    ("s_plus_r", MALFORMED, MALFORMED),
    ("off_curve_r", MALFORMED, MALFORMED),
    ("noncanonical_a", OK, OK),
    ("c_plus_r", OK, OK),
    ("torsion_a_odd_c", OK, REJECT),                      # A + T8 with an odd challenge: [c]T8 has order 8
    ("r_order2", OK, REJECT),                             # R = (0, -1) and [s]B = [c]A: the difference is the point of order 2
    ("r_identity_zero", OK, OK),                          # R = O, s = c = 0
    ("a_is_b", OK, OK),
    ("a_is_neg_b", OK, OK),
    ("s_r_minus_1", OK, OK),
    ("c_r_minus_1", OK, OK),
    ("c_all_ones", OK, OK),                               # c = 2^256 - 1, reduced by the call
    ("both_undecodable", MALFORMED, MALFORMED),
]
TORSION_KINDS = {k for k, v, w in KINDS if v != w}


class Batch:
    """one call's arrays (host), its flags, the expected bytes per mode (expect[True]: cofactored) and where the two modes must differ"""

    def __init__(self, name, base_name, r, a, s, c, flags, cof, less, planted):
        self.name, self.base_name, self.r, self.a, self.s, self.c, self.flags, self.planted = name, base_name, r, a, s, c, flags, planted
        self.expect = {True: cof, False: less}
        self.base = SC.bases()[base_name]

    @property
    def n(self):
        return len(self.s)

    def arrays(self):
        return self.r, self.a, self.s, self.c

    @property
    def torsion(self):
        return self.expect[True] != self.expect[False]

    def failing(self):
        """sig_locate's list: the units that fail the cofactored check on their own"""
        e = self.expect[True]
        return [(int(i), "malformed" if e[i] == MALFORMED else "reject") for i in np.nonzero(e != OK)[0]]


@functools.lru_cache(maxsize=None)
def _pool(m, base_name):
    """sig_batch_cases' m valid units and the cofactorless verdict of each.  Over the prime-order base both modes accept.  Over G (order 8r)
    s = k + c sk - w r, so [s]G - [c]A - R = [-w r]G: the identity iff 8 | w, always of small order."""
    r, a, s, c, _, ki, mi = SC._valid(m, base_name)
    less = np.full(m, OK, np.uint8)
    if base_name == "order8r":
        for i in range(m):
            w = (NONCE[mi[i]] + to_int(c[i]) * SK[ki[i]]) // R
            less[i] = OK if w % 8 == 0 else REJECT
    return r, a, s, c, ki, mi, less


def valid(n, base_name="prime"):
    """(r, a, s, c, key index, nonce index, cofactorless verdicts) of n valid units: writable copies, the pool repeated beyond POOL units"""
    m = max(1, min(n, POOL))
    idx = np.arange(n) % m
    return tuple(np.ascontiguousarray(x[idx]) for x in _pool(m, base_name))


@functools.lru_cache(maxsize=None)
def _fixed_points():
    B = SC.bases()["prime"]
    enc = lambda p: O.compress(np.asarray(p, np.uint8).reshape(1, 64))[0]      # noqa: E731
    return {"order2": enc(pt64((0, Q - 1))), "identity": enc(SC.IDENTITY), "b": enc(B), "neg_b": enc(O.point_op("neg", B[None])[0]),
            "d": SC._mul(0xD15, B)}


def plant(kind, k, r, a, s, c, ki, mi):
    """writes the planted unit `kind` over unit k of a batch over the prime-order base (arrays modified in place)"""
    A, Rp, _, _ = SC._pools("prime")
    B = SC.bases()["prime"]
    sk, nonce, ck = SK[ki[k]], NONCE[mi[k]], to_int(c[k])
    fp = _fixed_points()
    if kind == "torsion_r":
        r[k] = O.compress(O.point_op("add", Rp[mi[k]][None], SC.T8[None]))[0]
    elif kind == "bad_s":
        s[k] = b32((to_int(s[k]) + 5) % R)
    elif kind == "bad_r":
        r[k] = O.compress(O.point_op("add", Rp[mi[k]][None], fp["d"][None]))[0]
    elif kind == "s_plus_r":
        s[k] = b32(to_int(s[k]) + R)
    elif kind == "off_curve_r":
        r[k] = SC.off_curve_encoding()
    elif kind in ("noncanonical_a_zip216", "noncanonical_a"):
        a[k] = SC.NONCANONICAL_IDENTITY                      # A = O: valid with s = the nonce when the encoding is accepted
        s[k] = b32(nonce)
    elif kind == "c_plus_r":
        c[k] = b32(ck + R)
    elif kind == "torsion_a_odd_c":
        ck |= 1
        c[k] = b32(ck)
        s[k] = b32((nonce + (ck % R) * sk) % R)
        a[k] = O.compress(O.point_op("add", A[ki[k]][None], SC.T8[None]))[0]
    elif kind == "r_order2":
        r[k] = fp["order2"]
        s[k] = b32(ck * sk % R)
    elif kind == "r_identity_zero":
        r[k] = fp["identity"]
        s[k] = b32(0)
        c[k] = b32(0)
    elif kind == "a_is_b":
        a[k] = fp["b"]
        s[k] = b32((nonce + ck) % R)
    elif kind == "a_is_neg_b":
        a[k] = fp["neg_b"]
        s[k] = b32((nonce - ck) % R)
    elif kind == "s_r_minus_1":
        kk = (R - 1 - ck * sk) % R
        r[k] = O.compress(O.fixedbase_mul(b32(kk)[None], B))[0]
        s[k] = b32(R - 1)
    elif kind == "c_r_minus_1":
        c[k] = b32(R - 1)
        s[k] = b32((nonce + (R - 1) * sk) % R)
    elif kind == "c_all_ones":
        c[k] = b32((1 << 256) - 1)
        s[k] = b32((nonce + (((1 << 256) - 1) % R) * sk) % R)
    elif kind == "both_undecodable":
        r[k] = SC.off_curve_encoding()
        a[k] = SC.off_curve_encoding()
    else:
        raise KeyError(kind)


def planted_batch(n, kinds, name=None):
    """n units over the prime-order base with kinds[j] planted at positions(n)[j]"""
    pos = SC.positions(n)
    assert len(kinds) <= len(pos) and not {"noncanonical_a", "noncanonical_a_zip216"} <= set(kinds)
    r, a, s, c, ki, mi, less = valid(n)
    cof = np.full(n, OK, np.uint8)
    table = {k: (v, w) for k, v, w in KINDS}
    for kind, k in zip(kinds, pos):
        plant(kind, k, r, a, s, c, ki, mi)
        cof[k], less[k] = table[kind]
    flags = ZIP216 if "noncanonical_a_zip216" in kinds else 0
    return Batch(name or "n=%d %s" % (n, "+".join(kinds)), "prime", r, a, s, c, flags, cof, less, list(zip(pos, kinds)))


def kind_groups(n):
    g = len(SC.positions(n))
    names = [k for k, _, _ in KINDS]
    return [names[i:i + g] for i in range(0, len(names), g)]


@functools.lru_cache(maxsize=None)
def batches(n):
    """every batch of n units: no plant, the base of order 8r, every planted kind at the planted positions, every unit failing, every unit
    malformed.  Shared by the tests: read-only."""
    out = []
    r, a, s, c, _, _, less = valid(n)
    out.append(Batch("n=%d valid" % n, "prime", r, a, s, c, 0, np.full(n, OK, np.uint8), less, []))
    r, a, s, c, _, _, less = valid(n, "order8r")
    out.append(Batch("n=%d order8r" % n, "order8r", r, a, s, c, 0, np.full(n, OK, np.uint8), less, []))
    out += [planted_batch(n, kinds) for kinds in kind_groups(n)]
    r, a, s, c, _, _, _ = valid(n)
    for i in range(n):
        s[i] = b32((to_int(s[i]) + 5) % R)
    out.append(Batch("n=%d all_fail" % n, "prime", r, a, s, c, 0, np.full(n, REJECT, np.uint8), np.full(n, REJECT, np.uint8), []))
    r, a, s, c, _, _, _ = valid(n)
    r[:] = SC.off_curve_encoding()
    out.append(Batch("n=%d all_malformed" % n, "prime", r, a, s, c, 0, np.full(n, MALFORMED, np.uint8), np.full(n, MALFORMED, np.uint8), []))
    for b in out:
        for x in b.arrays() + (b.expect[True], b.expect[False]):
            x.setflags(write=False)
    return out


def large_batch(n):
    """one batch for the sizes where only the closed forms are affordable: every planted kind that fits, at positions spread over the whole batch
    (the ends, the wave boundaries, the middle, and evenly between), a few dozen failing units at most"""
    names = [k for k, _, _ in KINDS if k != "noncanonical_a"]                    # the batch runs under ZIP-216
    pos = sorted({0, 63, 64, n // 2, n - 65, n - 64, n - 1} | {int(x) for x in np.linspace(1, n - 2, 2 * len(names))})
    pos = [p for p in pos if 0 <= p < n]
    r, a, s, c, ki, mi, less = valid(n)
    cof = np.full(n, OK, np.uint8)
    table = {k: (v, w) for k, v, w in KINDS}
    planted = []
    for j, k in enumerate(pos):
        kind = names[j % len(names)]
        plant(kind, k, r, a, s, c, ki, mi)
        cof[k], less[k] = table[kind]
        planted.append((k, kind))
    return Batch("n=%d large" % n, "prime", r, a, s, c, ZIP216, cof, less, planted)


def full_evaluation(b, cofactored):
    """what the issue defines, evaluated unit by unit by the oracle: decode, [s]B by its fixed-base ladder, [c mod r]A by its variable-base
    ladder, two subtractions, three doublings unless cofactorless, the identity test"""
    n = b.n
    if n == 0:
        return np.zeros(0, np.uint8)
    rp, rok = O.decompress(b.r, b.flags)
    ap, aok = O.decompress(b.a, b.flags)
    sv = [to_int(x) for x in b.s]
    bad = (rok == 0) | (aok == 0) | np.array([x >= R for x in sv])
    rp[rok == 0] = SC.IDENTITY
    ap[aok == 0] = SC.IDENTITY
    sB = O.fixedbase_mul(np.stack([b32(x % R) for x in sv]), b.base)
    cA = O.varbase_mul(np.stack([b32(to_int(x) % R) for x in b.c]), ap)
    d = O.point_op("sub", O.point_op("sub", sB, cA), rp)
    if cofactored:
        d = O.point_op("mul_by_cofactor", d)
    ident = O.predicate("is_identity", d)
    return np.where(bad, MALFORMED, np.where(ident != 0, OK, REJECT)).astype(np.uint8)
