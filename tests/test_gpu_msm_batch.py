"""
GPU tests of jj_msm_batch (Engine.msm_batch, MultiEngine.msm_batch): B independent MSMs per call, every row bit-exact against the
oracle's MSM and against jj_msm on the same row, on both sides of every internal threshold of the batched path.
"""
import os
import re

import numpy as np
import pytest

from oracle import c_oracle as O
from oracle import jubjub_ref as J
from util import EDGE_SCALARS, R, arr32, pt64, rand_scalars, to_int, torsion_points

pytestmark = pytest.mark.gpu

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
IDENTITY = np.concatenate([np.zeros(32, np.uint8), np.frombuffer((1).to_bytes(32, "little"), np.uint8)])


def msm_constants():
    """the integer constexpr values of jj_msm.hip (MSM_BATCH_MAX, MSM_BATCH_TABLE_TERMS, ...)"""
    text = open(os.path.join(ROOT, "jubjub_amd", "csrc", "jj_msm.hip")).read()
    out = {}
    for m in re.finditer(r"constexpr\s+size_t\s+(MSM_BATCH_\w+)\s*=\s*([\d\s<()]+);", text):
        out[m.group(1)] = int(eval(m.group(2)))
    for key in ("MSM_BATCH_MAX", "MSM_BATCH_TABLE_TERMS", "MSM_BATCH_ROWS", "MSM_BATCH_WAVES", "MSM_BATCH_SLICE_MIN"):
        assert key in out, key
    return out


C = msm_constants()


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


def batch_inputs(pool, B, n, shared, seed):
    s = rand_scalars(seed, B * n, full_width=True).reshape(B, n, 32)
    p = points_for(pool, n if shared else B * n, offset=seed)
    return s, (p if shared else p.reshape(B, n, 64))


def row_points(p, b):
    return p if p.ndim == 2 else p[b]


@pytest.mark.parametrize("shared", [1, 0])
@pytest.mark.parametrize("B", [1, 2, 3, 17, 130])
def test_rows_match_the_oracle(eng, pool, B, shared):
    for n in (0, 1, 2, 3, 63, 64, 65, 255, 256, 1000):
        s, p = batch_inputs(pool, B, n, shared, seed=1000 * B + n)
        out = eng.msm_batch(s, p)
        assert out.shape == (B, 64)
        for b in range(B):
            assert (out[b] == O.msm(s[b], row_points(p, b))).all(), (B, n, shared, b)


def test_edge_rows(eng, pool, golden):
    """EDGE_SCALARS x {identity, an order-8 point, 4 x that point, the generator, -generator}, one row per point, next to ordinary rows"""
    def times4(q):
        return O.point_op("double", O.point_op("double", q[None]))[0]

    p8 = [q for q in torsion_points(golden) if not (times4(q) == IDENTITY).all()][0]       # a point of order 8
    p8x4 = times4(p8)
    g = pt64(J.GENERATOR)
    gneg = O.point_op("neg", g[None])[0]
    specials = [IDENTITY, p8, p8x4, g, gneg]
    n = len(EDGE_SCALARS)
    s_edge = np.stack([arr32(EDGE_SCALARS)] * len(specials))
    p_edge = np.stack([np.stack([sp] * n) for sp in specials])
    s_rand, p_rand = batch_inputs(pool, 4, n, 0, seed=5)
    s = np.concatenate([s_rand[:2], s_edge, s_rand[2:]])
    p = np.concatenate([p_rand[:2], p_edge, p_rand[2:]])
    out = eng.msm_batch(s, p)
    for b in range(s.shape[0]):
        assert (out[b] == O.msm(s[b], p[b])).all(), b
    # the same scalars over shared points that mix all five kinds
    ps = np.stack([specials[i % len(specials)] for i in range(n)])
    out = eng.msm_batch(s, ps)
    for b in range(s.shape[0]):
        assert (out[b] == O.msm(s[b], ps)).all(), b


@pytest.mark.parametrize("shared", [1, 0])
def test_rows_equal_jj_msm(eng, pool, shared):
    for B, n in ((5, 1), (9, 100), (40, 777), (3, C["MSM_BATCH_MAX"])):
        s, p = batch_inputs(pool, B, n, shared, seed=77 + n)
        out = eng.msm_batch(s, p)
        for b in range(B):
            assert (out[b] == eng.msm(s[b], row_points(p, b))).all(), (B, n, b)


@pytest.mark.parametrize("shared", [1, 0])
def test_both_sides_of_the_batched_limit(eng, pool, shared):
    """n = MSM_BATCH_MAX takes the batched kernels, MSM_BATCH_MAX + 1 the jobs route (one jj_msm_begin job per row)"""
    for n in (C["MSM_BATCH_MAX"], C["MSM_BATCH_MAX"] + 1):
        s, p = batch_inputs(pool, 5, n, shared, seed=n)
        out = eng.msm_batch(s, p)
        for b in range(5):
            assert (out[b] == O.msm_pippenger(s[b], row_points(p, b))).all(), (n, b)


def test_distinct_points_above_the_table_cap(eng, pool):
    """distinct points over more than MSM_BATCH_TABLE_TERMS terms: the rows run in several rounds (the last one short)"""
    n = 1000
    B = C["MSM_BATCH_TABLE_TERMS"] // n * 2 + 3
    s, p = batch_inputs(pool, B, n, 0, seed=9)
    out = eng.msm_batch(s, p)
    for b in list(range(0, B, 97)) + [B - 2, B - 1]:
        assert (out[b] == O.msm(s[b], p[b])).all(), b


@pytest.mark.parametrize("shared", [1, 0])
def test_with_and_without_slices(eng, pool, shared):
    """few rows: a row's terms are cut into slices whose partial sums the last wave adds; MSM_BATCH_WAVES rows or more: no slices"""
    n = C["MSM_BATCH_TABLE_TERMS"] // (C["MSM_BATCH_WAVES"] + 1)          # one round of tables holds all rows of the larger batch
    assert n > 4 * C["MSM_BATCH_SLICE_MIN"]
    for B in (2, C["MSM_BATCH_WAVES"] + 1):
        s, p = batch_inputs(pool, B, n, shared, seed=B)
        out = eng.msm_batch(s, p)
        for b in sorted(set(list(range(0, B, max(1, B // 24))) + [B - 1])):
            assert (out[b] == O.msm(s[b], row_points(p, b))).all(), (B, b)


def test_more_rows_than_one_finish_group(eng, pool):
    """shared points, more than MSM_BATCH_ROWS rows: several groups of window sums and finish launches"""
    B, n = C["MSM_BATCH_ROWS"] + 7, 3
    s, p = batch_inputs(pool, B, n, 1, seed=3)
    out = eng.msm_batch(s, p)
    for b in list(range(0, B, 211)) + [C["MSM_BATCH_ROWS"] - 1, C["MSM_BATCH_ROWS"], B - 1]:
        assert (out[b] == O.msm(s[b], p)).all(), b


def test_input_kinds(eng, pool):
    import torch

    B, n = 19, 300
    s, p = batch_inputs(pool, B, n, 0, seed=19)
    want = np.stack([O.msm(s[b], p[b]) for b in range(B)])
    # page-locked host arrays
    hs, hp, ho = eng.host_alloc(s.shape), eng.host_alloc(p.shape), eng.host_alloc((B, 64))
    hs[...] = s
    hp[...] = p
    assert eng.msm_batch(hs, hp, out=ho) is ho
    assert (ho == want).all()
    # torch tensors on a non-default stream: the call only queues work, the results are there after a synchronise
    ts, tp = torch.from_numpy(s).cuda(), torch.from_numpy(p).cuda()
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        out = eng.msm_batch(ts, tp)
        dev_out = torch.zeros((B, 64), dtype=torch.uint8, device="cuda")
        assert eng.msm_batch(ts, tp[0], out=dev_out) is dev_out
    torch.cuda.synchronize()
    assert out.is_cuda and (out.cpu().numpy() == want).all()
    assert (dev_out.cpu().numpy() == np.stack([O.msm(s[b], p[0]) for b in range(B)])).all()
    # n = 0 on device memory: the identity in every row
    z = torch.full((B, 64), 7, dtype=torch.uint8, device="cuda")
    eng.msm_batch(torch.zeros((B, 0, 32), dtype=torch.uint8, device="cuda"), torch.zeros((0, 64), dtype=torch.uint8, device="cuda"), out=z)
    torch.cuda.synchronize()
    assert (z.cpu().numpy() == IDENTITY).all()


def test_device_call_returns_before_the_work_is_done(eng, pool):
    """device pointers and rows the batched kernels take: the call queues work on the stream and returns (the stream is still busy)"""
    import torch

    B, n = 2048, 1024
    ts = torch.from_numpy(rand_scalars(4, B * n, full_width=True).reshape(B, n, 32)).cuda()
    tp = torch.from_numpy(points_for(pool, B * n).reshape(B, n, 64)).cuda()
    torch.cuda.synchronize()
    out = eng.msm_batch(ts, tp)
    busy = not torch.cuda.current_stream().query()
    torch.cuda.synchronize()
    assert busy
    h = out.cpu().numpy()
    for b in (0, 1, 1000, B - 1):
        assert (h[b] == O.msm(ts[b].cpu().numpy(), tp[b].cpu().numpy())).all(), b


def test_whole_batch_at_size(eng):
    B, n = 4096, 256
    # distinct points: the rows' sum is the MSM of all B n terms
    s = eng.synth_bytes32(B * n, seed=21)
    p = eng.random_points(B * n, seed=22, subgroup=False)
    out = eng.msm_batch(s.reshape(B, n, 32), p.reshape(B, n, 64))
    total = O.point_sum(out)
    whole = eng.msm(s, p)
    assert (whole == total).all()
    assert (O.msm_pippenger(s, p) == total).all()
    for b in range(0, B, B // 64):
        assert (out[b] == O.msm(s[b * n:(b + 1) * n], p[b * n:(b + 1) * n])).all(), b
    # shared subgroup points, canonical scalars: sum_b out_b = msm((sum_b s_b) mod r, points)
    ps = eng.random_points(n, seed=23, subgroup=True)
    sc = eng.synth_scalars(B * n, seed=24).reshape(B, n, 32)
    out = eng.msm_batch(sc, ps)
    ints = np.array([[to_int(sc[b, i]) for i in range(n)] for b in range(B)], dtype=object)
    col = [int(sum(ints[:, i])) % R for i in range(n)]
    assert (O.point_sum(out) == O.msm(arr32(col), ps)).all()
    for b in range(0, B, B // 64):
        assert (out[b] == O.msm(sc[b], ps)).all(), b


@pytest.mark.parametrize("shared", [1, 0])
def test_multi_engine_matches_engine(eng, pool, shared):
    from jubjub_amd import MultiEngine

    m = MultiEngine([0, 0])
    try:
        for B in (1, 5, 64):
            s, p = batch_inputs(pool, B, 130, shared, seed=300 + B)
            assert (m.msm_batch(s, p) == eng.msm_batch(s, p)).all(), B
        assert m.msm_batch(np.zeros((0, 4, 32), np.uint8), np.zeros((4, 64), np.uint8)).shape == (0, 64)
    finally:
        m.close()
