"""
Every planner override and decoder variant held to the oracle (include/jubjub_hip.h: "every value gives the same results").

MSM: one corpus -- ragged sizes around the workgroup, tile and chunk boundaries, adversarial digit distributions, a window partition
and one case large enough that the one-pass sort's part count is limited by the CUs -- with each oracle answer computed once, run
through every row of tests/planner_matrix.py on a context of its own: jj_msm (lane 0, host arrays) and jj_msm_begin / jj_msm_finish
(device arrays: lanes 1 and up, whose automatic chunk length differs), bit-exact.  Each row also runs a var-base corpus.

Decoder: k_decompress<1/4/8/16/32> at sizes taken from the device's lane count (decompress_dev), not multiples of CHUNK, with invalid
encodings planted at the first, middle and last position of a lane's group, whole groups and the ragged last lane: the encodings
of one lane share one inversion, so a wrong walk-back shows up in the valid neighbours of an invalid one.
"""
import numpy as np
import pytest

import planner_matrix as M
from oracle import c_oracle as O
from oracle import jubjub_ref as J
from util import EDGE_SCALARS, Q, arr32, arr64, b32, pt64, rand_points, rand_scalars, to_pt

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SIZES = (1, 2, 255, 257, 4095, 4097, 8191, 8193, 16385, 40000)
JJ_ERR_INVALID = -1


def _edge_corpus():
    g8 = J.scalar_mul_fast(J.GENERATOR, J.R_MOD)                   # a point of order 8
    special = [J.AFFINE_IDENTITY] + [J.scalar_mul_fast(g8, k) for k in range(1, 8)] + [J.GENERATOR, J.affine_neg(J.GENERATOR)]
    S = arr32([k for _ in special for k in EDGE_SCALARS])
    P = arr64([p for p in special for _ in EDGE_SCALARS])
    return S, P


@pytest.fixture(scope="module")
def corpus():
    """[(case name, scalars, points, oracle sum)] + the window-partition case, all built once"""
    pool_p = rand_points(9001, M.LARGE_N)
    pool_s = rand_scalars(9002, M.LARGE_N, full_width=True)
    cases = [("random-%d" % n, pool_s[:n], pool_p[:n]) for n in SIZES]
    cases.append(("random-%d" % M.LARGE_N, pool_s, pool_p))
    n = 20000
    P = pool_p[:n]
    cases.append(("all-equal-20000", np.repeat(pool_s[:1], n, axis=0), P))        # one bucket per window holds every term
    S2 = rand_scalars(9003, n)
    S2[: n // 2] = S2[0]
    S2[n // 2: n // 2 + 500] = 0
    S2[-1] = 0xFF
    S2[-1, 31] = 0x0F                                                                # 2^252 - 1: the largest top-window digit
    cases.append(("half-equal-zeros-top-20000", S2, P))
    m = 1 << 15
    S3 = np.zeros((m, 32), np.uint8)
    v = np.arange(1, m + 1, dtype=np.uint32)
    S3[:, 0] = v & 0xFF
    S3[:, 1] = (v >> 8) & 0xFF
    cases.append(("1..2^15", S3, np.repeat(pool_p[:8], m // 8, axis=0)))          # every low bucket, digits of both signs
    # a point and its negation under the same scalar: the buckets cancel to the identity (one shared scalar, then one per pair)
    A = pool_p[:1]
    h = 4096
    Sc = np.concatenate([np.repeat(pool_s[1:2], 2 * h, axis=0), np.repeat(pool_s[2:2 + h], 2, axis=0)])
    Pc = np.concatenate([np.tile(np.concatenate([A, O.point_op("neg", A)]), (h, 1)),
                         np.stack([pool_p[3:3 + h], O.point_op("neg", pool_p[3:3 + h])], axis=1).reshape(-1, 64)])
    cases.append(("cancelling-pairs-%d" % len(Sc), Sc, Pc))
    Se, Pe = _edge_corpus()
    cases.append(("edge-scalars-x-special-points", Se, Pe))
    out = [(name, np.ascontiguousarray(S), np.ascontiguousarray(P), O.msm(S, P)) for name, S, P in cases]
    assert to_pt(out[-2][3]) == J.AFFINE_IDENTITY
    Sv = np.concatenate([Se, rand_scalars(9004, 1000, full_width=True)])
    Pv = np.concatenate([Pe, pool_p[:1000]])
    return {"msm": out, "partition": (pool_s[:n], pool_p[:n], O.msm(pool_s[:n], pool_p[:n])),
            "varbase": (Sv, Pv, O.varbase_mul(Sv, Pv))}


def f2_parts(cus, W, bpc, n):
    """the part count of k_msm_front2 / k_msm_scatter2 (msm_enqueue_pippenger)"""
    return max(1, min(min(bpc * cus // W, 64), (n + 4095) // 4096))


@pytest.mark.parametrize("k", range(len(M.ROWS)), ids=[M.row_id(k) for k in range(len(M.ROWS))])
def test_planner_row(corpus, k):
    from jubjub_amd import Engine

    opts, reason = M.ROWS[k]
    eng = Engine(0, options=opts)
    try:
        cus = eng.device_info()["cus"]
        rid = "%s (%s) on %d CUs" % (M.row_id(k), reason, cus)
        if opts.get("msm_sort_blocks_per_cu") == 4 and opts.get("msm_windows") == 20 and cus == 256:
            parts = f2_parts(cus, 20, 4, M.LARGE_N)
            assert parts == 4 * cus // 20 < (M.LARGE_N + 4095) // 4096, (rid, parts)            # the large case is CU-limited
        for name, S, P, want in corpus["msm"]:
            got = eng.msm(S, P)
            assert (got == want).all(), "%s: msm, n=%d, case %s" % (rid, len(S), name)
        dev = torch.device("cuda", 0)
        jobs = [(name, len(S), eng.msm_begin(torch.from_numpy(S).to(dev), torch.from_numpy(P).to(dev)), want)
                for name, S, P, want in corpus["msm"]]
        for name, n, job, want in jobs:
            assert (eng.msm_finish(job) == want).all(), "%s: msm_begin/msm_finish, n=%d, case %s" % (rid, n, name)
        S, P, want = corpus["partition"]
        recs = np.stack([eng.msm_partial(S, P, g, 3) for g in range(3)])
        assert (eng.msm_combine(recs) == want).all(), "%s: msm_partial(g, 3) + msm_combine, n=%d" % (rid, len(S))
        S, P, want = corpus["varbase"]
        assert (eng.varbase_mul(S, P) == want).all(), "%s: varbase_mul, n=%d" % (rid, len(S))
        assert (eng.varbase_mul_vartime(S, P) == want).all(), "%s: varbase_mul_vartime, n=%d" % (rid, len(S))
    finally:
        eng.close()


def test_set_option_refuses_values_inside_the_table_range():
    """values inside a key's [lo, hi] that ctx_option_apply refuses: JJ_ERR_INVALID, the option keeps its value (a host-only check)"""
    from jubjub_amd import Engine

    eng = Engine(0)
    try:
        for key, v in M.REJECTED:
            before = eng.get_option(key)
            rc = eng._lib.jj_ctx_set_option(eng._ctx, key.encode(), int(v))
            assert rc == JJ_ERR_INVALID, (key, v, rc)
            assert eng.get_option(key) == before, (key, v)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------- decoder
def dec_chunk(n, lanes, c_mid):
    """CHUNK of the k_decompress launch decompress_dev picks (jj_abi.hip)"""
    if n >= 32 * lanes:
        return 32
    if 8 * lanes <= n < 16 * lanes and c_mid == 8:
        return 8
    if n >= 8 * lanes:
        return 16
    return 1 if n <= 16384 else 4


def _nonsquare_vs(count, seed):
    """canonical v for which u^2 = (v^2 - 1) / (1 + d v^2) has no square root"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        v = int.from_bytes(rng.bytes(32), "little") % Q
        u2 = (v * v - 1) * pow(1 + J.EDWARDS_D * v * v, -1, Q) % Q
        if u2 and pow(u2, (Q - 1) // 2, Q) == Q - 1:
            out.append(v)
    return out


def _plant(n, T, chunk, seed):
    """(indices, 32-byte encodings) of invalid or special encodings on lane positions j = 0, a middle j and CHUNK - 1, whole groups of
    two lanes and every position of the ragged last lane; kinds in turn: v >= q, a non-square, u = 0 with the sign bit set (v = 1 and
    v = q - 1), raw bytes"""
    rng = np.random.default_rng(seed)
    idx = set()
    for t in {0, 1, 2, T // 2, T - 2}:
        for j in {0, chunk // 2, chunk - 1}:
            if 0 <= t and t + j * T < n:
                idx.add(t + j * T)
    for t in {3, T // 3, T - 1}:                                      # whole groups; T - 1 is the ragged last lane
        idx.update(t + j * T for j in range(chunk) if t + j * T < n)
    idx = np.array(sorted(idx), dtype=np.int64)
    nsq = _nonsquare_vs(8, seed)
    enc = []
    for a, i in enumerate(idx):
        kind = a % 5
        sign = int(rng.integers(0, 2)) << 255
        if kind == 0:
            e = (Q + int(rng.integers(0, 1 << 30))) | sign
        elif kind == 1:
            e = nsq[a % len(nsq)] | sign
        elif kind == 2:
            e = 1 | (1 << 255)
        elif kind == 3:
            e = (Q - 1) | (1 << 255)
        else:
            e = int.from_bytes(rng.bytes(32), "little")
        enc.append(e)
    return idx, arr32(enc)


@pytest.fixture(scope="module")
def dec_env():
    from jubjub_amd import Engine

    eng = Engine(0)
    dev = torch.device("cuda", 0)
    table = eng.fixedbase_table(torch.from_numpy(pt64(J.GENERATOR).copy()).to(dev))
    lanes = eng.device_info()["cus"] * 512
    yield eng, dev, table, lanes
    table.close()
    eng.close()


DEC_CASES = [("1", 1, 8), ("4", 2, 8), ("8", 8, 8), ("16", 8, 16), ("16", 16, 8), ("32", 32, 8)]      # (variant, size in lanes, dec_c_mid)


@pytest.mark.parametrize("variant,mult,c_mid", DEC_CASES, ids=["k_decompress<%s>-%dxlanes-cmid%d" % c for c in DEC_CASES])
def test_decoder_variant(dec_env, variant, mult, c_mid):
    from jubjub_amd import Engine

    eng0, dev, table, lanes = dec_env
    chunk = int(variant)
    n = 12345 if chunk == 1 else max(16385, mult * lanes) + chunk // 2 + 1                  # not a multiple of CHUNK: short last groups
    assert dec_chunk(n, lanes, c_mid) == chunk and (chunk == 1 or n % chunk), (n, lanes, c_mid)
    T = (n + chunk - 1) // chunk
    where = "k_decompress<%d>, n=%d, T=%d, lanes=%d, dec_c_mid=%d" % (chunk, n, T, lanes, c_mid)
    g = torch.Generator(device=dev)
    g.manual_seed(0x4445434F44 + n)
    s = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev, generator=g)
    s[:, 31] &= 0x0F
    P = eng0.fixedbase_mul(table, s)
    enc = eng0.compress(P)
    idx, bad = _plant(n, T, chunk, n)
    enc[torch.from_numpy(idx).to(dev)] = torch.from_numpy(bad).to(dev)
    valid = torch.ones(n, dtype=torch.bool, device=dev)
    valid[torch.from_numpy(idx).to(dev)] = False
    eng = Engine(0, options={"dec_c_mid": c_mid})
    try:
        for flags in (1, 0):
            out, ok = eng.decompress(enc, flags)
            good = ok.bool() & valid
            if not bool(good[valid].all()) or not bool((out[valid] == P[valid]).all()):
                wrong = torch.nonzero(valid & ((out != P).any(dim=1) | ~ok.bool())).flatten()[:8].cpu().tolist()
                pytest.fail("%s, flags %d: valid encodings decoded wrong at %s (lane i %% T, position i // T: %s)"
                            % (where, flags, wrong, [(i % T, i // T) for i in wrong]))
            eo, ek = O.decompress(bad, flags)
            go, gk = out[torch.from_numpy(idx).to(dev)].cpu().numpy(), ok[torch.from_numpy(idx).to(dev)].cpu().numpy()
            for a in np.nonzero((gk != ek) | (go != eo).any(axis=1))[0][:1]:
                pytest.fail("%s, flags %d: planted encoding at i=%d (lane %d, position %d) ok %d, oracle %d"
                            % (where, flags, idx[a], idx[a] % T, idx[a] // T, gk[a], ek[a]))
            if flags == 0:
                assert gk[np.isin(np.arange(len(idx)) % 5, (2, 3))].all(), where           # u = 0 with the sign bit: accepted without ZIP-216
        sample = np.unique(np.concatenate([idx, np.arange(0, n, max(1, n // 2048))]))
        st = torch.from_numpy(sample).to(dev)
        for flags in (1 | 2, 1 | 4 | 8):
            out, ok = eng.decompress(enc, flags)
            eo, ek = O.decompress(enc[st].cpu().numpy(), flags)
            assert (ok[st].cpu().numpy() == ek).all() and (out[st].cpu().numpy() == eo).all(), "%s, flags %d" % (where, flags)
    finally:
        eng.close()
