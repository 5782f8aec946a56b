"""
The layouts of tests/msm_bucket_cases.py are what they say (CPU only).  The constants they are derived from are the ones in
jj_msm_kernels.h / jj_msm.hip; the bucket sizes of every layout are recomputed from the generated scalars through msm_signed_digits (never
taken from what the generator was asked for), and from those sizes the model must show the head counts, the extra-segment counts, the
overflow of the big-bucket list, the wave positions and the empty runs the layout is named after.  These are conditions: a layout that
misses one fails here, before any GPU run.  Every test prints the model's numbers of its layout (pytest -s).
"""
import os
import re

import numpy as np
import pytest

import msm_bucket_cases as M
from util import msm_signed_digits, msm_window_layout, to_int

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = os.path.join(ROOT, "jubjub_amd", "csrc", "jj_msm_kernels.h")
HOST = os.path.join(ROOT, "jubjub_amd", "csrc", "jj_msm.hip")


def _const(src, name):
    m = re.search(r"^constexpr (?:u32|int|size_t) %s = ([^;]+);" % name, src, re.M)
    assert m, name
    expr = re.sub(r"\(size_t\)", "", m.group(1))
    assert re.fullmatch(r"[\d\s<()]+", expr), (name, expr)
    return int(eval(expr))


def test_constants_are_the_source():
    ker, host = open(KERNELS).read(), open(HOST).read()
    for name in ("FIXUP_SERIAL_MAX", "FIXUP_BIG_MAX", "FIXUP_BIG_QUADS", "SEG_PMAX", "MSM_LO_BITS", "MSM_P1_TILE"):
        assert _const(ker, name) == getattr(M, name), name
    assert _const(host, "MSM_LARGE_MIN") == M.MSM_LARGE_MIN
    assert _const(host, "MSM_BATCH_MAX") == M.BASIS_MIN
    # ... and they are used the way the model uses them
    assert "big = some && t_last - t_first + 1 > FIXUP_SERIAL_MAX;" in ker                       # chunks: the pair takes up to 32 heads
    assert "t_first = (size_t)s * nchunk + lo / chunk + 1; t_last = (size_t)s * nchunk + (hi - 1) / chunk;" in ker
    assert "const size_t g = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 1;" in ker       # two lanes per bucket: 32 buckets per wave
    assert "if (extra > FIXUP_SERIAL_MAX) {" in ker and "if (slot < FIXUP_BIG_MAX) {" in ker     # segments: listed, or merged when the list is full
    assert "if (cnt > FIXUP_BIG_MAX) cnt = FIXUP_BIG_MAX;" in ker
    assert "return n >= ((size_t)1 << 18) ? 16 : n >= MSM_LARGE_MIN ? 17 : 23;" in host
    assert "u32 P = (u32)std::min<size_t>(SEG_PMAX, std::max<size_t>(32, 2 * n / B));" in host
    assert "const size_t max_segs = nb + (n * (size_t)Ws) / P + 1;" in host
    assert "std::max<size_t>((size_t)Ws * nchunk, (n * (size_t)Ws) / 8 + 1)" in host
    assert [M.default_windows(n) for n in (M.SMALL_N, M.MSM_LARGE_MIN - 1, M.MSM_LARGE_MIN, M.LARGE_N, 1 << 18)] == [23, 23, 17, 17, 16]
    assert M.buckets_per_window(23) == 1024 and M.buckets_per_window(17) == 16384 and M.buckets_per_window(17) > 8192   # MSM_ACC_LDS_BUCKETS
    assert M.top_digit_max(23) == 1023 and M.usable_buckets(23) == 1023 and M.usable_buckets(17) == 8191


def test_chunk_heads_is_the_cut():
    """the closed form against the cut itself: chunk t (entries t unit ..) inherits the bucket that began before it and is not over"""
    rng = np.random.default_rng(5)
    for unit in (8, 13):
        sizes = rng.integers(0, 4, size=400) * rng.integers(0, 40, size=400)
        hi = np.cumsum(sizes)
        lo = hi - sizes
        want = [sum(1 for t in range(1, int(hi[-1]) // unit + 1) if a < t * unit < b) for a, b in zip(lo, hi)]
        assert M.chunk_heads(sizes, unit).tolist() == want
    assert M.extra_segments([0, 1, 8, 9, 264, 265], 8).tolist() == [0, 0, 0, 1, 32, 33]
    assert M.empty_runs([3, 0, 0, 5, 2, 0, 1, 0], 4) == [(2, 3), (1, 2)]


def test_the_generator_refuses_what_it_cannot_encode():
    D = np.zeros((23, 2), dtype=np.int64)
    D[22, 0] = M.top_digit_max(23) + 1                                       # 2^252 and above
    with pytest.raises(AssertionError):
        M.scalars_from_digits(D, 23)
    D[22, 0], D[3, 1] = 0, -5                                                # a negative scalar
    with pytest.raises(AssertionError):
        M.scalars_from_digits(D, 23)
    D[3, 1] = 1024                                                           # no such digit: it recodes as -1024 with a carry
    with pytest.raises(AssertionError):
        M.scalars_from_digits(D, 23)
    D[3, 1], D[22, 1] = -1024, 1
    S = M.scalars_from_digits(D, 23)
    assert msm_signed_digits(to_int(S[1]), 23) == D[:, 1].tolist() and to_int(S[0]) == 0


_SIZES = {}


def _sizes(key):
    if key not in _SIZES:
        lay = M.build(key)
        assert lay.S.shape == (lay.n, 32) and lay.S.dtype == np.uint8
        _SIZES[key] = M.bucket_sizes(lay.S, lay.W)
    return _SIZES[key]


def _units(key):
    """the (scheme, unit) of every configuration that runs the layout"""
    return sorted({M.pass_unit(cfg, M.build(key).n) for cfg, k in M.pairs() if k == key})


def _report(key, sizes):
    lay = M.build(key)
    for scheme, unit in _units(key):
        print("%s | %s unit %d | %s" % (M.layout_id(key), scheme, unit, M.describe(M.model(sizes, scheme, unit, lay.n))))


def _keys(*names):
    return [k for k in M.all_keys() if k[0] in names]


def _ids(keys):
    return [M.layout_id(k) for k in keys]


def test_every_configuration_runs_its_layouts():
    names = {cfg.id: {k[0] for k in M.config_layouts(cfg)} for cfg in M.CONFIGS}
    for cfg in M.CONFIGS:
        assert set(M.DEGENERATE) | {"extreme-buckets"} <= names[cfg.id], cfg.id
        if cfg.scheme == "chunks":
            assert {"heads-boundary", "sparse-runs"} <= names[cfg.id], cfg.id
        if cfg.scheme == "segments":
            assert "segment-sizes" in names[cfg.id], cfg.id
            assert ("big-list-overflow" in names[cfg.id]) == (cfg.unit == 8), cfg.id
        for k in M.config_layouts(cfg):
            assert cfg.scheme is None or k[1] == cfg.W == cfg.options["msm_windows"], (cfg.id, k)
            assert cfg.scheme is not None or k[1] == M.default_windows(k[3]), (cfg.id, k)
    assert sum(cfg.basis for cfg in M.CONFIGS) == 2 and {cfg.scheme for cfg in M.CONFIGS if cfg.basis} == {"chunks", "segments"}
    assert {(c.W, c.unit) for c in M.CONFIGS if c.scheme == "chunks"} == {(23, 8), (23, 13), (17, 8)}
    assert {(c.W, c.unit) for c in M.CONFIGS if c.scheme == "segments"} == {(23, 8), (17, 8), (23, 33)}
    for key in M.all_keys():
        n = M.build(key).n
        assert n <= 50000 or (key[3] == M.LARGE_N and key[0] in M.DEGENERATE + ("extreme-buckets",)), key
        assert n > M.BASIS_MIN, key                                          # a basis row of these terms takes the Pippenger pass


@pytest.mark.parametrize("key", M.all_keys(), ids=_ids(M.all_keys()))
def test_buffers_hold_the_layout(key):
    """heads <= n Ws / 8 + 1 and segments <= nb + n Ws / P + 1 (the sizes msm_enqueue_pippenger gives the head and segment arrays), for
    the whole pass and for each third of the windows (msm_partial(g, 3)); no bucket index beyond what its window has"""
    lay, sizes = M.build(key), _sizes(key)
    W, B = lay.W, M.buckets_per_window(lay.W)
    assert sizes.shape == (W, B) and (sizes.sum(axis=1) <= lay.n).all()
    for w, h in enumerate(M.half_widths(W)):
        assert not sizes[w, h:].any(), w
    assert not sizes[W - 1, M.top_digit_max(W):].any()
    for scheme, unit in _units(key):
        if scheme != "segments":
            continue
        extra = M.extra_segments(sizes, unit)
        for ws in [range(W)] + [range(g, W, 3) for g in range(3)]:
            ws = list(ws)
            heads, segs = int(extra[ws].sum()), int((sizes[ws] > 0).sum() + extra[ws].sum())
            assert heads <= lay.n * len(ws) // 8 + 1, (unit, ws, heads)
            assert segs <= len(ws) * B + lay.n * len(ws) // unit + 1, (unit, ws, segs)


@pytest.mark.parametrize("key", _keys("heads-boundary"), ids=_ids(_keys("heads-boundary")))
def test_heads_boundary(key):
    lay, sizes = M.build(key), _sizes(key)
    unit, wb = lay.unit, M.FIXUP_WAVE_BUCKETS
    assert M.buckets_per_window(lay.W) % wb == 0                               # g % 32 == j % 32
    _report(key, sizes)
    for w in range(lay.W):
        heads, lo = M.chunk_heads(sizes[w], unit), M.bucket_starts(sizes[w])
        hi, full = lo + sizes[w], sizes[w] > 0
        for h in M.HEADS:
            for a in (0, unit - 1):
                assert (full & (heads == h) & (lo % unit == a)).any(), (w, h, a)
        for h in (32, 33):
            assert (full & (heads == h) & (lo % unit == 0) & (hi % unit == 0)).any(), (w, h)      # boundary to boundary
            assert (full & (heads == h) & (hi % unit != 0)).any(), (w, h)
        assert (full & (heads == 33) & (lo % unit == unit - 1) & (hi % unit == 0)).any(), w
        assert heads.max() == 129
        big = heads > M.FIXUP_SERIAL_MAX
        waves = big.reshape(-1, wb)
        assert (waves[:, 0] & waves[:, wb - 1]).any(), w                         # the first and the last pair of one wave
        assert (waves.sum(axis=1) >= 3).any(), w                                 # several turns of the loop over the ballot
        assert (big[:-1] & big[1:]).any(), w                                     # neighbours
        serial = full & ~big
        assert (waves.any(axis=1) & serial.reshape(-1, wb).any(axis=1)).any(), w  # pairs and the wave in the same wave


@pytest.mark.parametrize("key", _keys("sparse-runs"), ids=_ids(_keys("sparse-runs")))
def test_sparse_runs(key):
    lay, sizes = M.build(key), _sizes(key)
    unit = lay.unit
    _report(key, sizes)
    wave_folded = 0
    for w in range(lay.W):
        runs = M.empty_runs(sizes[w], unit)
        assert len(runs) >= 3 and len(runs) == (sizes[w] > 0).sum() - 1, w       # no two non-empty buckets are neighbours
        assert min(r[0] for r in runs) >= M.GAP_MIN, (w, runs)
        assert {r[1] for r in runs} == ({0} if w % 2 == 0 else {unit // 2}), (w, runs)   # the gap begins on a chunk boundary / inside a chunk
        assert sizes[w, 0] > 0                                                   # the first chunk starts in bucket 0
        wave_folded += int((M.chunk_heads(sizes[w], unit) > M.FIXUP_SERIAL_MAX).sum())
    assert wave_folded >= lay.W


@pytest.mark.parametrize("key", _keys("segment-sizes", "big-list-overflow"), ids=_ids(_keys("segment-sizes", "big-list-overflow")))
def test_segment_layouts(key):
    lay, sizes = M.build(key), _sizes(key)
    P = lay.unit
    _report(key, sizes)
    extra = M.extra_segments(sizes, P)
    big = int((extra > M.FIXUP_SERIAL_MAX).sum())
    for w in range(lay.W):
        have = sorted(int(c) for c in sizes[w][sizes[w] > 0])
        for c in M.seg_sizes(P):
            assert c in have, (w, c)
        ex = extra[w][sizes[w] > 0]
        assert {0, 1, 31, 32, 33} <= set(ex.tolist()), w
        assert (ex == M.FIXUP_SERIAL_MAX).sum() == 2, w                          # merge items with k = 32: 32 P + 1 and 33 P entries
        multi = np.nonzero(extra[w])[0] % 64
        assert 0 in multi and 63 in multi, w                                     # the ends of the wave-wide prefix sum of k_seg_scatter
    if lay.name == "segment-sizes":
        assert [sorted(int(c) for c in s[s > 0]) for s in sizes] == [sorted(M.seg_sizes(P))] * lay.W
        assert big == 2 * lay.W < M.FIXUP_BIG_MAX                                # 33 P + 1 and 34 P: the list does not fill
    else:
        assert big > M.FIXUP_BIG_MAX + M.OVERFLOW_MARGIN, big                    # whichever 2048 are listed, more than 256 are not:
        assert int(extra.max()) == M.FIXUP_SERIAL_MAX + 1                        # ... merge items with k = 33
        assert (extra[0::3] > M.FIXUP_SERIAL_MAX).sum() < M.FIXUP_BIG_MAX        # (a third of the windows alone does not overflow)


@pytest.mark.parametrize("key", _keys("extreme-buckets"), ids=_ids(_keys("extreme-buckets")))
def test_extreme_buckets(key):
    lay, sizes = M.build(key), _sizes(key)
    _report(key, sizes)
    B, n = M.buckets_per_window(lay.W), lay.n
    halves = M.half_widths(lay.W)
    assert max(halves) == B and (lay.W != 17 or min(halves) == B // 2)         # 17 windows: two widths, the narrow ones use half the slots
    for w, h in enumerate(halves):
        assert sizes[w, h - 1] == n // 2 and sizes[w, h - 2] == n - n // 2 and sizes[w].sum() == n, w
    top = sizes[lay.W - 1]
    assert top.sum() == n and top[0] > 0 and top[M.top_digit_max(lay.W) - 1] > 0   # top digit >= 1, the largest one among them
    digs = [msm_signed_digits(to_int(lay.S[i]), lay.W) for i in range(0, n, 997)]
    for ds in digs:
        assert all(d in (-h, h - 1) for d, h in zip(ds, halves)) and ds[-1] >= 1
    assert any(ds[0] == -halves[0] for ds in digs) and any(ds[0] == halves[0] - 1 for ds in digs)


@pytest.mark.parametrize("key", _keys(*M.DEGENERATE), ids=_ids(_keys(*M.DEGENERATE)))
def test_degenerate(key):
    lay, sizes = M.build(key), _sizes(key)
    _report(key, sizes)
    W, n = lay.W, lay.n
    per_window = sizes.sum(axis=1)
    if lay.name == "all-zero":
        assert not lay.S.any() and not sizes.any()
    elif lay.name == "one-nonzero":
        assert not lay.S[: n - 1].any() and lay.S[n - 1].any()
        assert sizes.max() == 1 and (per_window > 0).sum() >= W - 2                # one entry in (nearly) every window
    else:
        w = W // 2 if lay.name == "mid-window-only" else W - 1
        assert per_window[w] == n and per_window.sum() == n                      # every term, one window
        assert (sizes[w] > 0).sum() >= 500                                       # ... spread over its buckets
