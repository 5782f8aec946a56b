"""
GPU tests of jj_msm_ragged (Engine.msm_ragged): S independent MSMs of different lengths per call, every row bit-exact against the oracle's
MSM and against jj_msm / jj_msm_batch on the same terms: single-slice, exactly-full, one-over and many-slice segments side by side, empty
segments, the jobs route beside the batched one, every planner override, every kind of pointer, and the reuse of the context's workspaces.
"""
import numpy as np
import pytest

from oracle import c_oracle as O
from oracle import jubjub_ref as J
from util import EDGE_SCALARS, arr32, pt64, rand_scalars, torsion_points

pytestmark = pytest.mark.gpu

IDENTITY = np.concatenate([np.zeros(32, np.uint8), np.frombuffer((1).to_bytes(32, "little"), np.uint8)])
# with the default slice length t = 16 (N_short < 16 * 2048): one slice, exactly full, one over, many slices, side by side
MIXED = [0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 255, 256, 1000]


@pytest.fixture(scope="module")
def eng():
    from jubjub_amd import Engine

    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def pool(eng):
    """2^15 points: subgroup and full-group points interleaved"""
    a = eng.random_points(1 << 14, seed=71, subgroup=True)
    b = eng.random_points(1 << 14, seed=72, subgroup=False)
    return np.stack([a, b], axis=1).reshape(-1, 64)


def offsets_of(lens):
    return np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64))])


def inputs(pool, lens, seed):
    n = int(sum(lens))
    idx = (np.arange(n, dtype=np.int64) * 7 + seed) % pool.shape[0]
    return rand_scalars(seed, n, full_width=True).reshape(n, 32), np.ascontiguousarray(pool[idx]).reshape(n, 64), offsets_of(lens)


def oracle_rows(s, p, off, msm=O.msm):
    return np.stack([msm(s[off[k]:off[k + 1]], p[off[k]:off[k + 1]]).reshape(64) if off[k + 1] > off[k] else IDENTITY for k in range(len(off) - 1)])


def check(out, want, what):
    assert out.shape == want.shape, what
    bad = [k for k in range(want.shape[0]) if not (out[k] == want[k]).all()]
    assert not bad, (what, bad)


@pytest.fixture(scope="module")
def mixed(pool):
    """the corpus of the override test: inputs and the oracle's rows, computed once"""
    lens = MIXED + [3000, 2, 0, 4999]
    s, p, off = inputs(pool, lens, seed=11)
    return lens, s, p, off, oracle_rows(s, p, off)


@pytest.mark.parametrize("lens", [MIXED, MIXED[::-1], [0], [1], [17], [0] * 5, [1] * 257], ids=["mixed", "reversed", "S1-0", "S1-1", "S1-17", "empty5", "ones257"])
def test_rows_match_the_oracle(eng, pool, lens):
    s, p, off = inputs(pool, lens, seed=100 + len(lens))
    check(eng.msm_ragged(s, p, off), oracle_rows(s, p, off), lens)


def test_rows_equal_jj_msm_and_jj_msm_batch(eng, pool):
    s, p, off = inputs(pool, MIXED, seed=5)
    out = eng.msm_ragged(s, p, off)
    for k in range(len(MIXED)):
        assert (out[k] == eng.msm(s[off[k]:off[k + 1]], p[off[k]:off[k + 1]])).all(), k
    for n in (1, 100, 777):
        s, p, off = inputs(pool, [n] * 9, seed=n)
        assert (eng.msm_ragged(s, p, off) == eng.msm_batch(s.reshape(9, n, 32), p.reshape(9, n, 64))).all(), n


def test_edge_rows(eng, pool, golden):
    """EDGE_SCALARS x {identity, an order-8 point, 4 x that point, the generator, -generator}, one segment per point, between ordinary segments"""
    def times4(q):
        return O.point_op("double", O.point_op("double", q[None]))[0]

    p8 = [q for q in torsion_points(golden) if not (times4(q) == IDENTITY).all()][0]       # a point of order 8
    specials = [IDENTITY, p8, times4(p8), pt64(J.GENERATOR), O.point_op("neg", pt64(J.GENERATOR)[None])[0]]
    n = len(EDGE_SCALARS)
    rs, rp, _ = inputs(pool, [40, 7, 19], seed=6)
    parts_s, parts_p, lens = [rs[:40]], [rp[:40]], [40]
    for k, sp in enumerate(specials):
        parts_s.append(arr32(EDGE_SCALARS)); parts_p.append(np.stack([sp] * n)); lens.append(n)
        if k == 1:
            parts_s.append(rs[40:47]); parts_p.append(rp[40:47]); lens.append(7)
    # all five kinds mixed in one segment, then an ordinary one
    parts_s.append(arr32(EDGE_SCALARS)); parts_p.append(np.stack([specials[i % 5] for i in range(n)])); lens.append(n)
    parts_s.append(rs[47:]); parts_p.append(rp[47:]); lens.append(19)
    s, p, off = np.concatenate(parts_s), np.concatenate(parts_p), offsets_of(lens)
    check(eng.msm_ragged(s, p, off), oracle_rows(s, p, off), lens)


def test_both_routes_in_one_call(eng, pool):
    """8192 terms: the batched kernels' longest segment; 8193: a jj_msm_begin job.  Empty rows are (0, 1) next to either"""
    lens = [5, 8192, 0, 8193, 40, 0]
    s, p, off = inputs(pool, lens, seed=8)
    out = eng.msm_ragged(s, p, off)
    check(out, oracle_rows(s, p, off, msm=O.msm_pippenger), lens)
    assert (out[2] == IDENTITY).all() and (out[5] == IDENTITY).all()


@pytest.mark.parametrize("options", [{"msm_ragged_slice_min": 1}, {"msm_ragged_slice_min": 64}, {"msm_ragged_waves": 1}, {"msm_ragged_waves": 65536},
                                     {"msm_ragged_round_terms": 64}, {"msm_ragged_round_terms": 4096}], ids=lambda o: "-".join("%s=%d" % kv for kv in o.items()))
def test_planner_overrides_give_the_same_bytes(eng, mixed, options):
    from jubjub_amd import Engine

    lens, s, p, off, want = mixed
    default = eng.msm_ragged(s, p, off)
    check(default, want, "default")
    (key, value), = options.items()
    plan = eng.plan_msm_ragged(off, **{key[len("msm_ragged_"):]: value})
    if options != {"msm_ragged_waves": 65536}:          # (65536 waves ask for slices below the 16 terms slice_min keeps: the default's plan)
        assert plan != eng.plan_msm_ragged(off), "the override does not change the plan of this corpus"
    e = Engine(0, options=options)
    try:
        out = e.msm_ragged(s, p, off)
    finally:
        e.close()
    assert (out == default).all(), [k for k in range(len(lens)) if not (out[k] == default[k]).all()]


def test_pointer_kinds(eng, pool):
    import torch

    lens = [0, 3, 70, 0, 1, 300, 16, 0]
    s, p, off = inputs(pool, lens, seed=19)
    want = oracle_rows(s, p, off)
    check(eng.msm_ragged(s, p, off), want, "host")
    ts, tp = torch.from_numpy(s).cuda(), torch.from_numpy(p).cuda()
    torch.cuda.synchronize()
    out = eng.msm_ragged(ts, tp, off)
    dev_out = torch.full((len(lens), 64), 7, dtype=torch.uint8, device="cuda")
    assert eng.msm_ragged(ts, tp, torch.from_numpy(off), out=dev_out) is dev_out
    torch.cuda.synchronize()
    assert out.is_cuda
    check(out.cpu().numpy(), want, "device")
    check(dev_out.cpu().numpy(), want, "device, caller's out")
    # mixed: host scalars (and so a host result), device points
    check(eng.msm_ragged(s, tp, off), want, "host scalars, device points")
    # page-locked host arrays and a page-locked result
    hs, hp, ho = eng.host_alloc(s.shape), eng.host_alloc(p.shape), eng.host_alloc((len(lens), 64))
    hs[...] = s
    hp[...] = p
    assert eng.msm_ragged(hs, hp, list(off), out=ho) is ho
    check(np.asarray(ho), want, "page-locked")
    # no terms at all on device memory: identities, nothing else touched
    z = torch.full((4, 64), 7, dtype=torch.uint8, device="cuda")
    eng.msm_ragged(torch.zeros((0, 32), dtype=torch.uint8, device="cuda"), torch.zeros((0, 64), dtype=torch.uint8, device="cuda"), [0, 0, 0, 0, 0], out=z)
    torch.cuda.synchronize()
    assert (z.cpu().numpy() == IDENTITY).all()
    assert eng.msm_ragged(s[:0], p[:0], [0]).shape == (0, 64)


def test_device_calls_in_a_row_keep_their_work_lists(eng, pool):
    """device pointers: a call returns before its kernels run, and the next call's work list must not overwrite the one still in flight"""
    import torch

    cases = []
    for k, lens in enumerate(([700, 0, 33, 2000], [5] * 40, [64, 1, 1500, 0, 17])):
        s, p, off = inputs(pool, lens, seed=50 + k)
        cases.append((torch.from_numpy(s).cuda(), torch.from_numpy(p).cuda(), off, oracle_rows(s, p, off)))
    torch.cuda.synchronize()
    outs = [eng.msm_ragged(ts, tp, off) for ts, tp, off, _ in cases]
    torch.cuda.synchronize()
    for out, (_, _, _, want) in zip(outs, cases):
        check(out.cpu().numpy(), want, "queued")


def test_workspace_reuse(eng, pool):
    """a small call, a larger one, the small one again: a stale counter, work list or row of window sums would show in the third"""
    small = inputs(pool, [40, 0, 100, 7, 33], seed=31)
    large = inputs(pool, [900, 33, 0, 1200, 64, 5, 2500, 17] * 3, seed=32)
    first = eng.msm_ragged(*small)
    check(first, oracle_rows(*small), "small")
    check(eng.msm_ragged(*large), oracle_rows(*large), "large")
    third = eng.msm_ragged(*small)
    assert (third == first).all()
