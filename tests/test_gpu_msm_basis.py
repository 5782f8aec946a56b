"""
GPU tests of the fixed-basis MSM (Engine.msm_basis / msm_basis_mul over jj_msm_basis_*): every result bit-exact against the oracle's MSM
or jj_msm on the same inputs, for the resident-points mode (1) and the window-table mode (2), on both routes, every window layout, prefixes,
rows, skewed scalars, at size, and under planner overrides.  `info` is asserted so that no case passes on the other mode by accident.
"""
import numpy as np
import pytest

from oracle import c_oracle as O
from oracle import jubjub_ref as J
from planner_matrix import ROWS
from util import EDGE_SCALARS, R, arr32, pt64, rand_scalars, torsion_points

pytestmark = pytest.mark.gpu

IDENTITY = np.concatenate([np.zeros(32, np.uint8), np.frombuffer((1).to_bytes(32, "little"), np.uint8)])
MODES = ["points", "windows"]
SMALL_MAX = 8192


@pytest.fixture(scope="module")
def eng():
    from jubjub_amd import Engine

    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def pool(eng):
    """2^17 points: subgroup and full-group points interleaved"""
    a = eng.random_points(1 << 16, seed=71, subgroup=True)
    b = eng.random_points(1 << 16, seed=72, subgroup=False)
    return np.stack([a, b], axis=1).reshape(-1, 64)


def points_for(pool, count, offset=0):
    idx = (np.arange(count, dtype=np.int64) * 7 + offset) % pool.shape[0]
    return np.ascontiguousarray(pool[idx])


def basis_of(eng, p, mode, windows=0):
    b = eng.msm_basis(p, mode=mode, windows=windows)
    info = b.info
    assert info["n"] == len(p) and info["mode"] == mode, info
    small = min(len(p), SMALL_MAX) * 1296
    if len(p) > SMALL_MAX:
        assert info["bytes"] == small + len(p) * 128 * (info["windows"] if mode == "windows" else 1), info
        assert windows == 0 or info["windows"] == windows
    else:
        assert info["bytes"] == small and info["windows"] == 64
    return b


@pytest.mark.parametrize("mode", MODES)
def test_oracle_parity(eng, pool, mode):
    for n in (0, 1, 2, 3, 63, 64, 65, 1000, 8192, 8193, 1 << 14, (1 << 14) + 1, 40000, 150000):
        s = rand_scalars(900 + n, n, full_width=True)
        p = points_for(pool, n, offset=n)
        with basis_of(eng, p, mode) as b:
            got = eng.msm_basis_mul(b, s)
        assert got.shape == (64,)
        assert (got == (O.msm(s, p) if n <= 1000 else O.msm_pippenger(s, p))).all(), (mode, n)


@pytest.mark.parametrize("mode", MODES)
def test_edge_rows(eng, pool, golden, mode):
    """EDGE_SCALARS x {identity, an order-8 point, 4 x it, generator, -generator} as basis points: the tables then hold identities and
    small-order entries; alone, mixed with ordinary points, and on the Pippenger route"""
    def times4(q):
        return O.point_op("double", O.point_op("double", q[None]))[0]

    p8 = [q for q in torsion_points(golden) if not (times4(q) == IDENTITY).all()][0]
    g = pt64(J.GENERATOR)
    specials = [IDENTITY, p8, times4(p8), g, O.point_op("neg", g[None])[0]]
    k = len(EDGE_SCALARS)
    for sp in specials:
        p = np.stack([sp] * k)
        with basis_of(eng, p, mode) as b:
            assert (eng.msm_basis_mul(b, arr32(EDGE_SCALARS)) == O.msm(arr32(EDGE_SCALARS), p)).all()
    for n in (5 * k, 9000):
        reps = -(-n // k)
        s = np.concatenate([arr32(EDGE_SCALARS)] * reps)[:n]
        p = points_for(pool, n, offset=3)
        p[::3] = np.stack([specials[i % 5] for i in range(len(p[::3]))])
        with basis_of(eng, p, mode) as b:
            assert (eng.msm_basis_mul(b, s) == O.msm_pippenger(s, p)).all(), n


@pytest.mark.parametrize("mode", MODES)
def test_equal_to_jj_msm(eng, pool, mode):
    for n in (1, 100, 777, 8192, 20000):
        s = rand_scalars(77 + n, n, full_width=True)
        p = points_for(pool, n, offset=n)
        with basis_of(eng, p, mode) as b:
            assert (eng.msm_basis_mul(b, s) == eng.msm(s, p)).all(), n


@pytest.mark.parametrize("mode", MODES)
def test_every_layout(eng, pool, mode):
    for n, W in ((20000, 16), (20000, 17), (20000, 23), (20000, 36), (1 << 18, 16)):
        s = rand_scalars(W + n, n, full_width=True)
        p = points_for(pool, n, offset=W)
        with basis_of(eng, p, mode, windows=W) as b:
            assert (eng.msm_basis_mul(b, s) == O.msm_pippenger(s, p)).all(), (n, W)


@pytest.mark.parametrize("mode", MODES)
def test_prefixes(eng, pool, mode):
    """a prefix may fall on the other route than n does"""
    for n in (20000, 1000):
        s = rand_scalars(5 + n, n, full_width=True)
        p = points_for(pool, n, offset=1)
        with basis_of(eng, p, mode) as b:
            for m in (0, 1, 100, n // 2, n - 1, n):
                assert (eng.msm_basis_mul(b, s[:m]) == eng.msm(s[:m], p[:m])).all(), (n, m)


@pytest.mark.parametrize("mode", MODES)
def test_rows(eng, pool, mode):
    for B, n in ((1, 256), (3, 256), (130, 256), (3, 20000)):
        s = rand_scalars(B * 1000 + n, B * n, full_width=True).reshape(B, n, 32)
        p = points_for(pool, n, offset=B)
        with basis_of(eng, p, mode) as b:
            out = eng.msm_basis_mul(b, s)
        assert out.shape == (B, 64)
        for r in range(B):
            assert (out[r] == (O.msm(s[r], p) if n <= 1000 else O.msm_pippenger(s[r], p))).all(), (B, n, r)
    with basis_of(eng, points_for(pool, 10), mode) as b:
        assert eng.msm_basis_mul(b, np.zeros((0, 10, 32), np.uint8)).shape == (0, 64)
        assert (eng.msm_basis_mul(b, np.zeros((4, 0, 32), np.uint8)) == IDENTITY).all()


@pytest.mark.parametrize("mode", MODES)
def test_skewed_scalars(eng, pool, mode):
    """the folded bucket set makes the big-bucket / merge-list paths W times as likely as in jj_msm"""
    n = 1 << 16
    p = points_for(pool, n, offset=11)
    one = rand_scalars(1, 1, full_width=True)
    half = rand_scalars(2, n, full_width=True)
    half[::2] = 0
    with basis_of(eng, p, mode) as b:
        for name, s in (("equal", np.repeat(one, n, axis=0)), ("half zero", half), ("r - 1", np.repeat(arr32([R - 1]), n, axis=0))):
            assert (eng.msm_basis_mul(b, np.ascontiguousarray(s)) == O.msm_pippenger(np.ascontiguousarray(s), p)).all(), name


@pytest.mark.parametrize("mode", ["windows", "auto"])
def test_at_size(eng, mode):
    for lg in (17, 20):
        n = 1 << lg
        s = eng.synth_bytes32(n, seed=30 + lg)
        p = eng.random_points(n, seed=40 + lg, subgroup=False)
        b = eng.msm_basis(p, mode=mode)
        assert mode == "auto" or b.info["mode"] == "windows"
        assert b.info["n"] == n
        assert (eng.msm_basis_mul(b, s) == O.msm_pippenger(s, p)).all(), lg
        b.close()


@pytest.mark.parametrize("mode", MODES)
def test_ownership_and_interleaving(eng, pool, mode):
    n = 20000
    s = rand_scalars(8, n, full_width=True)
    p = points_for(pool, n, offset=2)
    p2 = points_for(pool, 9000, offset=5)
    want, want2 = O.msm_pippenger(s, p), O.msm_pippenger(s[:9000], p2)
    mine = p.copy()
    b = basis_of(eng, mine, mode)
    mine[...] = 0xA5                                             # the basis owns its copy
    b2 = basis_of(eng, p2, "windows" if mode == "points" else "points")
    for _ in range(2):
        assert (eng.msm_basis_mul(b, s) == want).all()
        assert (eng.msm_basis_mul(b2, s[:9000]) == want2).all()
    assert (eng.msm_basis_mul(b, s) == want).all()
    job = eng.msm_begin(s, p)                                    # an outstanding job and a plain MSM between two basis calls
    assert (eng.msm(s[:9000], p2) == want2).all()
    assert (eng.msm_basis_mul(b, s) == want).all()
    assert (eng.msm_finish(job) == want).all()
    assert (eng.msm_basis_mul(b2, s[:9000]) == want2).all()
    b.close()
    b2.close()


@pytest.mark.parametrize("mode", MODES)
def test_input_kinds(eng, pool, mode):
    import torch

    for B, n in ((3, 300), (2, 9000)):
        s = rand_scalars(19 + n, B * n, full_width=True).reshape(B, n, 32)
        p = points_for(pool, n, offset=19)
        want = np.stack([O.msm_pippenger(s[r], p) for r in range(B)])
        hp = eng.host_alloc(p.shape)
        hp[...] = p
        b = basis_of(eng, hp, mode)
        hs, ho = eng.host_alloc(s.shape), eng.host_alloc((B, 64))
        hs[...] = s
        assert eng.msm_basis_mul(b, hs, out=ho) is ho
        assert (ho == want).all()
        ho1 = eng.host_alloc((64,))
        assert eng.msm_basis_mul(b, hs[0], out=ho1) is ho1 and (ho1 == want[0]).all()
        b.close()
        ts, tp = torch.from_numpy(s).cuda(), torch.from_numpy(p).cuda()
        torch.cuda.synchronize()
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            bt = basis_of(eng, tp, mode)
            dev_out = torch.zeros((B, 64), dtype=torch.uint8, device="cuda")
            assert eng.msm_basis_mul(bt, ts, out=dev_out) is dev_out
            one = eng.msm_basis_mul(bt, ts[1])
            # m = 0 on device memory: the identity in every row; B = 0 touches nothing
            z = torch.full((B, 64), 7, dtype=torch.uint8, device="cuda")
            assert eng.msm_basis_mul(bt, torch.zeros((B, 0, 32), dtype=torch.uint8, device="cuda"), out=z) is z
            z1 = eng.msm_basis_mul(bt, torch.zeros((0, 32), dtype=torch.uint8, device="cuda"))
            assert eng.msm_basis_mul(bt, torch.zeros((0, n, 32), dtype=torch.uint8, device="cuda")).shape == (0, 64)
        torch.cuda.synchronize()
        assert (dev_out.cpu().numpy() == want).all() and one.is_cuda and (one.cpu().numpy() == want[1]).all()
        assert (z.cpu().numpy() == IDENTITY).all() and z1.shape == (64,) and (z1.cpu().numpy() == IDENTITY).all()
        bt.close()


# six rows of tests/planner_matrix.py, picked by their reason strings: front end + segment accumulation, chunked accumulation + fix-up, the
# one-level reduce in both instantiations and at both bucket counts, the two-level reduce at both ends of its row count
PLANNER_REASONS = ["legacy one-pass sort in front of the segment accumulation",
                   "a chunk that divides no power of two, offsets in LDS",
                   "one-level reduce, L = 2 at 32768 buckets",
                   "one-level reduce, L = 256 at 1024 buckets",
                   "two-level reduce with the most rows (64)",
                   "two-level reduce, two rows, the longest level-2 chunk (64)"]


def planner_row(reason):
    hits = [k for k, (_, why) in enumerate(ROWS) if why.startswith(reason)]
    assert len(hits) == 1, (reason, hits)
    return hits[0]


@pytest.mark.parametrize("reason", PLANNER_REASONS)
def test_planner_rows(pool, reason):
    """the context option msm_windows does not reach a mode-2 table (its layout is fixed at create), so the basis is created with the row's
    window count: the folded one-window reduce then runs under the row's reduce overrides"""
    from jubjub_amd import Engine

    opts = ROWS[planner_row(reason)][0]
    W = opts.get("msm_windows", 0)
    if "reduce" in reason:
        assert "msm_reduce_chunk" in opts or "msm_reduce_l1" in opts
    e = Engine(0, options=opts)
    try:
        for n in (20000, 70000):
            s = rand_scalars(len(reason) + n, n, full_width=True)
            p = points_for(pool, n, offset=len(reason))
            want = O.msm_pippenger(s, p)
            for mode in MODES:
                b = e.msm_basis(p, mode=mode, windows=W)
                assert b.info["mode"] == mode and (W == 0 or b.info["windows"] == W), b.info
                assert (e.msm_basis_mul(b, s) == want).all(), (reason, n, mode)
                assert (e.msm_basis_mul(b, s[:n // 3]) == e.msm(s[:n // 3], p[:n // 3])).all(), (reason, n, mode)
                b.close()
    finally:
        e.close()


def test_refused_arguments(eng, pool):
    """the checks of jj_msm_basis_mul that need a basis to be reached: NULL out, NULL scalars, m > n, B * m * 32 beyond size_t -- all refused;
    B = 0 succeeds whatever else is passed"""
    import ctypes as C

    from jubjub_amd import _lib

    L, ctx = eng._lib, eng._ctx
    s = rand_scalars(1, 10, full_width=True)
    out = np.full(64, 7, np.uint8)
    with basis_of(eng, points_for(pool, 10), "points") as b:
        sp, op = s.ctypes.data, out.ctypes.data
        assert L.jj_msm_basis_mul(ctx, b._h, C.c_size_t(1), C.c_size_t(10), sp, None) == _lib.JJ_ERR_INVALID
        assert L.jj_msm_basis_mul(ctx, b._h, C.c_size_t(1), C.c_size_t(10), None, op) == _lib.JJ_ERR_INVALID
        assert L.jj_msm_basis_mul(ctx, b._h, C.c_size_t(1), C.c_size_t(11), sp, op) == _lib.JJ_ERR_INVALID
        assert L.jj_msm_basis_mul(ctx, b._h, C.c_size_t(1 << 40), C.c_size_t(1 << 30), sp, op) == _lib.JJ_ERR_INVALID
        assert L.jj_msm_basis_mul(ctx, b._h, C.c_size_t(1 << 59), C.c_size_t(0), None, op) == _lib.JJ_ERR_INVALID        # B * 64 beyond size_t
        assert (out == 7).all()
        assert L.jj_msm_basis_mul(ctx, b._h, C.c_size_t(0), C.c_size_t(10), None, None) == 0
        assert L.jj_msm_basis_mul(ctx, None, C.c_size_t(1), C.c_size_t(10), sp, op) == _lib.JJ_ERR_INVALID
        assert L.jj_msm_basis_mul(ctx, b._h, C.c_size_t(1), C.c_size_t(10), sp, op) == 0 and (out == O.msm(s, points_for(pool, 10))).all()
        h = C.c_void_p()
        p = points_for(pool, 10)
        assert L.jj_msm_basis_create(ctx, C.c_size_t(10), None, 0, 0, C.byref(h)) == _lib.JJ_ERR_INVALID and not h.value
        assert L.jj_msm_basis_create(ctx, C.c_size_t(10), p.ctypes.data, 3, 0, C.byref(h)) == _lib.JJ_ERR_INVALID and not h.value
        assert L.jj_msm_basis_create(ctx, C.c_size_t(10), p.ctypes.data, 2, 15, C.byref(h)) == _lib.JJ_ERR_INVALID and not h.value
