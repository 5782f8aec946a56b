"""
Every fixed-base kernel, window width and base kind held to the oracle (tests/fixedbase_cover.py builds the scalars): k_fixedbase_comb
(window_bits 0 / 7), k_fixedbase (6, and composite tables), k_fixedbase_gather (8..16), their chains (jj_fixedbase_multi_mul), at ragged
sizes and around each kernel's grid round, through device tensors, pipelined host batches, a second context and MultiEngine.

The oracle's answer for each (base, scalar set) is computed once (O.fixedbase_mul) and every kernel and width is compared with it
bit for bit.  Batches above one grid round compare a sample of indices (a stride plus every index near a round boundary) with the
oracle and the whole batch with other kernel kinds.
"""
import numpy as np
import pytest

import fixedbase_cover as C
from oracle import c_oracle as O
from oracle import jubjub_ref as J
from util import EDGE_SCALARS, arr32, pt64, rand_points, rand_scalars, torsion_points

pytestmark = pytest.mark.gpu

KIND_BITS = {"comb": 7, "lds6": 6, "g8": 8, "g13": 13}
STATS = {"window_bits": set(), "oracle_rows": 0}


def _eq(got, want, what):
    got = np.asarray(got)
    assert got.shape == want.shape, what
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, "%s: %d rows differ, first at %s" % (what, bad.size, bad[:8])
    STATS["oracle_rows"] += want.shape[0]


@pytest.fixture(scope="module")
def eng():
    from jubjub_amd import Engine

    e = Engine(0)
    yield e
    e.close()
    print("\nfixed-base matrix: window_bits run %s; %d rows compared with the oracle"
          % (sorted(STATS["window_bits"]), STATS["oracle_rows"]))


@pytest.fixture(scope="module")
def bases(golden):
    tors = torsion_points(golden)
    ident = pt64(J.AFFINE_IDENTITY)

    def order(p):
        for m in (1, 2, 4, 8):
            if (O.fixedbase_mul(arr32([m]), p)[0] == ident).all():
                return m
        return 0

    by_order = {}
    for t in tors:
        by_order.setdefault(order(t), t)
    g = pt64(J.GENERATOR)
    p = rand_points(901, 1)[0]
    return {"G": g, "8G": O.fixedbase_mul(arr32([8]), g)[0], "P": p, "T2": by_order[2], "T4": by_order[4], "T8": by_order[8],
            "I": ident, "P+T8": O.point_op("add", p[None], by_order[8][None])[0]}


FULL_COVER = ("G", "P")          # the small-order bases run a slice of the wide cover sets
_ORACLE = {}


def oracle(base_name, key, S, base):
    """the oracle's answer for one base and one named scalar array, computed once"""
    k = (base_name, key)
    if k not in _ORACLE:
        _ORACLE[k] = O.fixedbase_mul(S, base)
    return _ORACLE[k]


def cover_array(kind, w, seed, full):
    """the cover set of a kernel kind as 32-byte rows; half the rows get random top 4 bits (ignored by every kernel and the oracle)"""
    ks = C.cover_scalars(kind, w)
    if not full and len(ks) > 1024:
        ks = ks[:64] + ks[64:-64:max(1, len(ks) // 1024)] + ks[-64:]
    rnd = np.random.default_rng(seed)
    top = rnd.integers(0, 16, size=len(ks))
    return arr32([k | (int(t) << 252 if i % 2 else 0) for i, (k, t) in enumerate(zip(ks, top))])


def width_scalars(wb, base_name):
    kind, w = C.kind_of_window_bits(wb)
    return np.concatenate([arr32(EDGE_SCALARS), cover_array(kind, w, 40 + (w or 0), base_name in FULL_COVER),
                           rand_scalars(700 + (w or 0), 500, full_width=True)]), (kind, w)


# ------------------------------------------------------------------------------------------------ widths x bases
def test_refused_window_bits(eng, bases):
    for wb in C.REFUSED_WINDOW_BITS:
        with pytest.raises(Exception):
            eng.fixedbase_table(bases["G"], wb)


@pytest.mark.parametrize("wb", C.ACCEPTED_WINDOW_BITS)
def test_every_width_every_base(eng, bases, wb):
    """fixedbase_mul and fixedbase_mul_compressed of every accepted window_bits on every base kind: edge scalars, the width's cover
    set (whole on G and P, a slice on the others) and full-width random scalars"""
    STATS["window_bits"].add(wb)
    for name, b in bases.items():
        S, (kind, w) = width_scalars(wb, name)
        want = oracle(name, (kind, w, name in FULL_COVER), S, b)
        tab = eng.fixedbase_table(b, wb)
        _eq(eng.fixedbase_mul(tab, S), want, (wb, name))
        if name in ("G", "T8", "I"):
            _eq(eng.fixedbase_mul_compressed(tab, S), O.compress(want), (wb, name, "compressed"))
        for m in (1, 63, 64, 65):
            _eq(eng.fixedbase_mul(tab, S[-m:]), want[-m:], (wb, name, m))
        assert eng.fixedbase_mul(tab, S[:0]).shape == (0, 64)
        tab.close()


# ------------------------------------------------------------------------------------------------ sizes around the grid rounds
@pytest.fixture(scope="module")
def big(eng, bases):
    """scalars for sizes past two rounds of the widest kernel, the sample of indices checked with the oracle, and the lane counts"""
    cus = eng.device_info()["cus"]
    T = {k: C.grid_lanes(k, cus) for k in ("comb", "lds6", "gather")}
    n = 2 * max(T.values()) + 37
    S = rand_scalars(911, n, full_width=True)
    S[:len(EDGE_SCALARS)] = arr32(EDGE_SCALARS)
    idx = set(range(0, n, 97)) | set(range(200)) | set(range(n - 200, n))
    for t in T.values():
        for r in (1, 2):
            idx |= set(range(max(0, r * t - 80), min(n, r * t + 80)))
    idx = np.array(sorted(idx))
    return {"T": T, "n": n, "S": S, "idx": idx}


def sampled_oracle(big, base_name, base, shift=0):
    """the oracle at the sampled indices of np.roll(S, shift)"""
    k = (base_name, "big", shift)
    if k not in _ORACLE:
        _ORACLE[k] = O.fixedbase_mul(np.roll(big["S"], shift, axis=0)[big["idx"]], base)
    return _ORACLE[k]


def check_sampled(got, big, want, m, what):
    sel = big["idx"] < m
    _eq(np.asarray(got)[big["idx"][sel]], want[sel], what)


def test_sizes_around_grid_rounds(eng, bases, big):
    """each kernel at 1, 63, 64, 65 and T - 1, T, T + 1, 2T + 37 of its own lane count T; the largest batch of every kind equal to
    the comb's in full"""
    want = sampled_oracle(big, "G", bases["G"])
    S, full = big["S"], {}
    for kind, wb in (("comb", 7), ("lds6", 6), ("gather", 8), ("gather", 9), ("gather", 11)):
        STATS["window_bits"].add(wb)
        T = big["T"][kind]
        tab = eng.fixedbase_table(bases["G"], wb)
        for m in (1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 37, big["n"]):
            got = eng.fixedbase_mul(tab, S[:m])
            check_sampled(got, big, want, m, (wb, m))
            if m == big["n"]:
                full[wb] = got
        tab.close()
    for wb, got in full.items():
        assert (got == full[7]).all(), wb


def test_device_tensors_and_device_base(eng, bases, big):
    """a base given as a device tensor, scalars and results as device tensors, on every kernel kind, at the largest size"""
    import torch

    S = big["S"]
    want = sampled_oracle(big, "P", bases["P"])
    sd = torch.from_numpy(S).cuda()
    bd = torch.from_numpy(bases["P"].copy()).cuda()
    for wb in (7, 6, 10, 15):
        STATS["window_bits"].add(wb)
        tab = eng.fixedbase_table(bd, wb)
        got = eng.fixedbase_mul(tab, sd)
        assert got.is_cuda and tuple(got.shape) == (big["n"], 64)
        check_sampled(got.cpu().numpy(), big, want, big["n"], (wb, "device"))
        enc = eng.fixedbase_mul_compressed(tab, sd[:4097])
        _eq(enc.cpu().numpy()[big["idx"][big["idx"] < 4097]], O.compress(want[big["idx"] < 4097]), (wb, "device compressed"))
        tab.close()


# ------------------------------------------------------------------------------------------------ chains
def _chain_want(big, parts):
    """sum of the oracle's per-base answers at the sampled indices; parts: [(base name, base, shift)]"""
    acc = None
    for name, b, shift in parts:
        t = sampled_oracle(big, name, b, shift)
        acc = t if acc is None else O.point_op("add", acc, t)
    return acc


def _chain_scalars(big, shifts, m):
    return np.stack([np.roll(big["S"], s, axis=0)[:m] for s in shifts])


def test_chains_every_ordered_pair(eng, bases, big):
    """jj_fixedbase_multi_mul over every ordered pair of {comb, 6-bit, gather 8, gather 13} (slot 0: base G, slot 1: base P), and the
    same table twice, at n = 1, 65 and past two grid rounds of the widest kernel: every order gives the same batch"""
    tabs = {(k, nm): eng.fixedbase_table(bases[nm], wb) for k, wb in KIND_BITS.items() for nm in ("G", "P")}
    shifts = (0, 12345)
    want = _chain_want(big, [("G", bases["G"], 0), ("P", bases["P"], 12345)])
    want2 = _chain_want(big, [("G", bases["G"], 0), ("G", bases["G"], 12345)])
    for m in (1, 65, big["n"]):
        S2 = _chain_scalars(big, shifts, m)
        first = None
        for a in KIND_BITS:
            for b in KIND_BITS:
                if a == b:
                    continue
                got = eng.fixedbase_multi_mul([tabs[(a, "G")], tabs[(b, "P")]], S2)
                check_sampled(got, big, want, m, (a, b, m))
                if first is None:
                    first = got
                else:
                    assert (got == first).all(), (a, b, m)
        for k in ("comb", "g13"):                                     # one table twice
            check_sampled(eng.fixedbase_multi_mul([tabs[(k, "G")], tabs[(k, "G")]], S2), big, want2, m, (k, "twice", m))
    for t in tabs.values():
        t.close()


def test_chain_of_five_with_small_order_bases(eng, bases, big):
    """a 5-table chain mixing every kernel kind, with the identity and torsion bases inside it"""
    chain = [("comb", "G"), ("lds6", "T8"), ("g8", "I"), ("g13", "P+T8"), ("lds6", "T4")]
    shifts = (0, 7, 1001, 54321, 3)
    tabs = [eng.fixedbase_table(bases[nm], KIND_BITS[k]) for k, nm in chain]
    want = _chain_want(big, [(nm, bases[nm], s) for (_, nm), s in zip(chain, shifts)])
    for m in (1, 65, big["n"]):
        check_sampled(eng.fixedbase_multi_mul(tabs, _chain_scalars(big, shifts, m)), big, want, m, ("five", m))
    for t in tabs:
        t.close()


# ------------------------------------------------------------------------------------------------ composite tables
@pytest.mark.parametrize("bits,ok,why", C.composite_cases(), ids=[c[2] for c in C.composite_cases()])
def test_composite_partitions(eng, bases, bits, ok, why):
    """composite tables at the slot and base limits on every base kind (duplicates included), against the oracle on the masked
    scalars and against fixedbase_multi_mul; refused partitions raise"""
    names = list(bases)
    nb = len(bits)
    B = np.stack([bases[names[(j * 3) % len(names)]] for j in range(nb)])
    if not ok:
        with pytest.raises(Exception):
            eng.fixedbase_composite_table(B, bits)
        return
    vals = [C.composite_field_values(b) for b in bits]
    n = max(len(v) for v in vals) + 64
    rnd = np.random.default_rng(nb * 1000 + bits[0])
    S = np.stack([rand_scalars(int(rnd.integers(1 << 30)), n, full_width=True) for _ in range(nb)])
    masked = np.zeros_like(S)
    for j, b in enumerate(bits):
        for r in range(n):
            raw = int.from_bytes(bytes(S[j, r]), "little")
            f = vals[j][r % len(vals[j])] if r < n - 64 else raw & ((1 << b) - 1)
            S[j, r] = np.frombuffer(((raw >> b << b) | f).to_bytes(32, "little"), np.uint8)
            masked[j, r] = np.frombuffer(f.to_bytes(32, "little"), np.uint8)
    want = None
    for j in range(nb):
        t = O.fixedbase_mul(masked[j], B[j])
        want = t if want is None else O.point_op("add", want, t)
    tab = eng.fixedbase_composite_table(B, bits)
    _eq(eng.fixedbase_composite_mul(tab, S), want, why)
    _eq(eng.fixedbase_composite_mul(tab, S[:, :1].copy()), want[:1], (why, 1))
    tab.close()
    uniq = {}                                                         # one default table per distinct base, shared by its duplicates
    for j in range(nb):
        if B[j].tobytes() not in uniq:
            uniq[B[j].tobytes()] = eng.fixedbase_table(B[j])
    tabs = [uniq[B[j].tobytes()] for j in range(nb)]
    _eq(eng.fixedbase_multi_mul(tabs, masked), want, (why, "multi_mul"))
    for t in uniq.values():
        t.close()


# ------------------------------------------------------------------------------------------------ options and plumbing
def test_fixedbase_default_option(bases):
    from jubjub_amd import Engine

    e6 = Engine(0, options={"fixedbase_default": 6})
    assert e6.get_option("fixedbase_default") == 6
    S, _ = width_scalars(6, "P")
    want = oracle("P", ("lds6", None, True), S, bases["P"])
    tab = e6.fixedbase_table(bases["P"], 0)
    _eq(e6.fixedbase_mul(tab, S), want, "fixedbase_default 6")
    tab.close()
    e6.close()
    e7 = Engine(0)
    assert e7.get_option("fixedbase_default") == 7
    e7.close()


def test_table_from_another_context(eng, bases):
    """a table built on one context serves another context of the same device"""
    from jubjub_amd import Engine

    e2 = Engine(0)
    for wb in (7, 6, 12):
        S, (kind, w) = width_scalars(wb, "T8")
        want = oracle("T8", (kind, w, False), S, bases["T8"])
        tab = eng.fixedbase_table(bases["T8"], wb)
        _eq(e2.fixedbase_mul(tab, S), want, (wb, "second context"))
        _eq(eng.fixedbase_mul(tab, S), want, (wb, "own context"))
        tab.close()
    e2.close()


def test_pipelined_host_batches(eng, bases, big):
    """pipe_chunk_log2 = 10: host batches cut into chunks of 1024 (pinned and pageable, ragged tails) for a 6-bit, a comb and a
    w = 9 table; and the default chunking of a host batch of 2.4 M units, where each kernel kind rounds its chunks to its own lanes"""
    from jubjub_amd import Engine

    ep = Engine(0, options={"pipe_chunk_log2": 10})
    S = big["S"]
    want = sampled_oracle(big, "G", bases["G"])
    for wb in (6, 7, 9):
        tab = ep.fixedbase_table(bases["G"], wb)
        for m in (2048, 2048 + 1, 5 * 1024 + 37, 65 * 1024 - 1):
            check_sampled(ep.fixedbase_mul(tab, S[:m]), big, want, m, (wb, m, "pageable"))
            pin = ep.host_alloc((m, 32))
            pin[:] = S[:m]
            out = ep.host_alloc((m, 64))
            ep.fixedbase_mul(tab, pin, out=out)
            check_sampled(out, big, want, m, (wb, m, "pinned"))
            del pin, out
        tab.close()
    ep.close()
    n = (1 << 21) + 12345          # default chunking: chunks of 2^19 rounded to the kernel's lanes, short first and last chunks
    reps = -(-n // big["n"])
    L = np.concatenate([S] * reps)[:n]
    first = None
    for wb in (7, 6, 9):
        tab = eng.fixedbase_table(bases["G"], wb)
        got = eng.fixedbase_mul(tab, L)
        for r in range(reps):
            lo = r * big["n"]
            check_sampled(got[lo:lo + big["n"]], big, want, min(big["n"], n - lo), (wb, "long host batch", r))
        if first is None:
            first = got
        else:
            assert (got == first).all(), wb
        tab.close()


def test_multi_engine_tables(bases):
    from jubjub_amd import MultiEngine

    me = MultiEngine([0, 0])
    for wb in (6, 11):
        STATS["window_bits"].add(wb)
        S, (kind, w) = width_scalars(wb, "T8")
        want = oracle("T8", (kind, w, False), S, bases["T8"])
        S, want = np.resize(S, (1001, 32)), np.resize(want, (1001, 64))     # the set repeated up to 1001 rows
        t = me.fixedbase_table(bases["T8"], wb)
        for m in (0, 1, 1001):
            got = me.fixedbase_mul(t, S[:m])
            assert got.shape == (m, 64)
            _eq(got, want[:m], (wb, m, "multi"))
    me.close()
