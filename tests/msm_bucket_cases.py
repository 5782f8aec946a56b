"""
Planted bucket layouts for the two accumulation schemes of the Pippenger MSM (jj_msm_kernels.h), as plain data and constructors
(numpy, the oracle for the points, Python integers): no GPU import.

A layout says, per window, how many entries each bucket holds.  The scalars are built backwards from it: target signed digits D[w][i]
(the digit model of tests/util.py: msm_window_layout / msm_signed_digits), k_i = sum_w D[w][i] 2^start_w, every k checked to lie in
[0, 2^252) and to recode to exactly D.  Bucket j of window w holds the terms with |D[w][i]| = j + 1; every window deals the terms out
by a permutation of its own, so the windows are uncorrelated.  `unit` is what the layout is measured in: the chunk length (option
msm_chunk) for the chunked accumulation (k_msm_accumulate + k_msm_fixup), the segment cap P (option msm_seg_len) for the segment
accumulation (k_seg_* + k_msm_accumulate_seg + k_msm_fixup_big).  Two model functions turn bucket sizes into what the kernels make
of them: chunk_heads (the inherited runs k_msm_fixup folds into a bucket) and extra_segments (the heads k_seg_scatter allocates; a
bucket is listed as big iff it has more than FIXUP_SERIAL_MAX of them).

tests/test_msm_bucket_cases_cpu.py pins the constants to the source and shows, from the generated scalars alone, that every layout is
what it says; tests/test_gpu_msm_buckets.py runs the layouts through the kernels.
"""
import collections
import functools

import numpy as np

from util import msm_signed_digits, msm_window_layout, to_int

# ---- the constants of jj_msm_kernels.h / jj_msm.hip the layouts are derived from (pinned by test_msm_bucket_cases_cpu.py)
FIXUP_SERIAL_MAX = 32          # heads a pair of lanes (chunks) / a quad (segments: merge item) walks itself
FIXUP_BIG_MAX = 2048           # capacity of the big-bucket work list of the segment path
FIXUP_BIG_QUADS = 64           # partial sums per listed bucket
SEG_PMAX = 1024                # largest segment cap
MSM_LO_BITS = 8                # the two-pass sort's second pass orders 2^8 buckets per workgroup
MSM_P1_TILE = 8192             # terms per tile of its first pass
MSM_LARGE_MIN = 9 << 14        # from this many terms: 17 windows + segments by default; below: 23 windows + chunks
FIXUP_WAVE_BUCKETS = 32        # k_msm_fixup: two lanes per bucket, 32 buckets per wave
BASIS_MIN = 8192               # jj_msm_basis_mul: rows of more terms than this take the Pippenger pass (MSM_BATCH_MAX)

HEADS = (0, 1, 2, 31, 32, 33, 34, 64, 65, 128, 129)    # pair / wave boundary; 0, 1, 2, 3 heads per lane before the butterfly
OVERFLOW_MARGIN = 256
GAP_MIN = 300


def default_windows(n):
    """msm_windows_default (jj_msm.hip)"""
    return 16 if n >= 1 << 18 else 17 if n >= MSM_LARGE_MIN else 23


def buckets_per_window(W):
    """B of msm_layout: the bucket slots of the widest window"""
    return 1 << (max(wd for _, wd in msm_window_layout(W)) - 1)


def half_widths(W):
    """2^(width - 1) per signed window: the digit -2^(width - 1) alone reaches bucket 2^(width - 1) - 1"""
    return [1 << (wd - 1) for _, wd in msm_window_layout(W)[:-1]]


def top_digit_max(W):
    """the largest digit of the (unsigned) top window of a scalar below 2^252"""
    return (1 << (252 - msm_window_layout(W)[-1][0])) - 1


def usable_buckets(W):
    """buckets 0 .. U - 1 exist in every window and are reached by digits of both signs (the top window: positive ones)"""
    return min([top_digit_max(W)] + [h - 1 for h in half_widths(W)])


# ------------------------------------------------------------------------------------------------------------------ the model
def chunk_heads(sizes, unit):
    """heads per bucket of one window: the entries of the window, in bucket order, are cut every `unit`; a bucket [lo, hi) leaves one head
    per chunk it continues into: (hi - 1) // unit - lo // unit (k_msm_fixup: t_first = lo / chunk + 1 .. t_last = (hi - 1) / chunk)"""
    sizes = np.asarray(sizes, dtype=np.int64)
    hi = np.cumsum(sizes)
    lo = hi - sizes
    return np.where(sizes > 0, (hi - 1) // unit - lo // unit, 0)


def bucket_starts(sizes):
    sizes = np.asarray(sizes, dtype=np.int64)
    return np.cumsum(sizes) - sizes


def extra_segments(sizes, unit):
    """heads per bucket on the segment path: ceil(c / unit) - 1 segments beyond the bucket's own (k_seg_scatter)"""
    sizes = np.asarray(sizes, dtype=np.int64)
    return np.where(sizes > 0, (sizes + unit - 1) // unit - 1, 0)


def empty_runs(sizes, unit):
    """[(length, offset of the run's first entry within its chunk)] of the runs of empty buckets that lie between two non-empty ones"""
    sizes = np.asarray(sizes, dtype=np.int64)
    nz = np.nonzero(sizes)[0]
    hi = np.cumsum(sizes)
    return [(int(b - a - 1), int(hi[a] % unit)) for a, b in zip(nz[:-1], nz[1:]) if b - a > 1]


def bucket_sizes(S, W):
    """per window, the entries of each of the B bucket slots -- recomputed from the scalars through msm_signed_digits"""
    B = buckets_per_window(W)
    out = np.zeros((W, B), dtype=np.int64)
    seen = {}
    for row in S:
        k = to_int(row)
        ds = seen.get(k)
        if ds is None:
            ds = seen[k] = [abs(d) - 1 for d in msm_signed_digits(k, W)]
        for w, j in enumerate(ds):
            if j >= 0:
                out[w, j] += 1
    return out


# -------------------------------------------------------------------------------------------------------------- the generator
def scalars_from_digits(D, W):
    """n x 32 bytes with msm_signed_digits(k_i, W) == D[:, i] and 0 <= k_i < 2^252, both asserted for every term"""
    lay = msm_window_layout(W)
    D = np.asarray(D, dtype=np.int64)
    assert D.shape[0] == W
    n = D.shape[1]
    K = [0] * n
    for w, (start, _) in enumerate(lay):
        K = [k + (d << start) if d else k for k, d in zip(K, D[w].tolist())]
    seen = {}
    for i, want in enumerate(D.T.tolist()):
        k = K[i]
        got = seen.get(k)
        if got is None:
            assert 0 <= k < 1 << 252, (i, k)
            got = seen[k] = msm_signed_digits(k, W)
        assert got == want, (i, got, want)
    return np.frombuffer(b"".join(k.to_bytes(32, "little") for k in K), dtype=np.uint8).reshape(n, 32).copy()


def _signed(A, W, rng):
    """signs for bucket indices A[w][i] = |digit|: the highest non-zero digit of a term positive (k >= 0), the digit 2^(width - 1) negative
    (there is no positive one), every other one at random"""
    n = A.shape[1]
    sign = rng.integers(0, 2, size=A.shape, dtype=np.int64) * 2 - 1
    nz = A != 0
    top = W - 1 - np.argmax(nz[::-1], axis=0)
    some = nz.any(axis=0)
    sign[top[some], np.arange(n)[some]] = 1
    for w, h in enumerate(half_widths(W)):
        ext = A[w] == h
        assert not (ext & (top == w)).any(), "a term whose highest digit is -2^(width-1) would be negative"
        sign[w, ext] = -1
        assert (A[w] <= h).all()
    assert (A[W - 1] <= top_digit_max(W)).all()
    return A * sign


def digits_from_sizes(spec, W, n, seed):
    """spec[w] = [(bucket j, entries)] in bucket order -> signed digits D[w][i]; window w deals the terms out by its own permutation"""
    rng = np.random.default_rng(seed)
    A = np.zeros((W, n), dtype=np.int64)
    for w in range(W):
        perm = rng.permutation(n)
        pos, last = 0, -1
        for j, c in spec[w]:
            assert j > last and c > 0, (w, j, c)
            A[w, perm[pos: pos + c]] = j + 1
            pos, last = pos + c, j
        assert pos <= n, (w, pos, n)
    return _signed(A, W, rng)


class _Run:
    """the buckets of one window laid down in order: every bucket knows where its entries start"""

    def __init__(self, unit, j=0):
        self.unit, self.pos, self.j, self.items = unit, 0, j, []

    def bucket(self, size, j=None):
        if j is not None:
            assert j >= self.j, (j, self.j)
            self.j = j
        self.items.append((self.j, int(size)))
        self.pos += int(size)
        self.j += 1

    def align(self, r):
        """a filler bucket, if one is needed, after which the next bucket starts r entries into a chunk"""
        d = (r - self.pos) % self.unit
        if d:
            self.bucket(d)

    def shortest(self, h):
        """the fewest entries with which a bucket that starts here has h heads"""
        return 1 if h == 0 else (self.pos // self.unit + h) * self.unit - self.pos + 1

    def longest(self, h):
        """the most: the bucket ends exactly on a chunk boundary"""
        return (self.pos // self.unit + h + 1) * self.unit - self.pos

    def ending(self, base, r):
        """at least `base` entries, as many as make the bucket end r entries into a chunk"""
        return base + (r - (self.pos + base)) % self.unit


def _heads_boundary(W, unit):
    spec = []
    for w in range(W):
        run = _Run(unit, j=FIXUP_WAVE_BUCKETS * (w % 3))
        for h in HEADS:
            for a in (0, unit - 1):                                  # starting on a chunk boundary, and one entry before it
                run.align(a)
                run.bucket(run.shortest(h))
        for h in (0, 1, 32, 33):                                     # from boundary to boundary
            run.align(0)
            run.bucket(run.longest(h))
        for h in (1, 33):                                            # ending on a boundary
            run.align(unit - 1)
            run.bucket(run.longest(h))
        run.align(0)
        j0 = -(-run.j // FIXUP_WAVE_BUCKETS) * FIXUP_WAVE_BUCKETS    # two big buckets in the first and the last pair of one wave
        run.bucket(run.shortest(33), j=j0)
        run.bucket(1)
        run.bucket(run.shortest(2), j=j0 + 16)
        run.bucket(run.shortest(34), j=j0 + FIXUP_WAVE_BUCKETS - 1)
        run.bucket(run.shortest(64), j=j0 + FIXUP_WAVE_BUCKETS + 5)  # three in the next wave, two of them neighbours
        run.bucket(run.shortest(33))
        run.bucket(run.shortest(32))
        run.bucket(run.shortest(129), j=j0 + 2 * FIXUP_WAVE_BUCKETS - 2)
        assert run.j <= usable_buckets(W)
        spec.append(run.items)
    n = max(BASIS_MIN + 808, max(sum(c for _, c in s) for s in spec) + 1000)
    return spec, n


def _sparse_runs(W, unit):
    """non-empty buckets at least GAP_MIN empty ones apart; in the even windows every bucket ends on a chunk boundary (the gap begins
    there), in the odd ones unit // 2 entries into a chunk"""
    U = usable_buckets(W)
    spec = []
    for w in range(W):
        run = _Run(unit)
        r = 0 if w % 2 == 0 else unit // 2
        bases = (3 * unit, 40 * unit, 1, 5 * unit - 1, unit, 2 * unit + 1)
        k = 0
        while run.j < U:
            run.bucket(run.ending(bases[k % len(bases)], r))
            run.j += GAP_MIN + 1 + (w + k) % 37
            k += 1
        spec.append(run.items)
    return spec, BASIS_MIN + 808


def seg_sizes(P):
    return (1, P - 1, P, P + 1, 2 * P, 32 * P, 32 * P + 1, 33 * P, 33 * P + 1, 34 * P)


SEG_SLOTS = (0, 1, 2, 62, 63, 64, 65, 127, 128, 200)               # first and last lane of a wave of k_seg_scatter among them


def _segment_sizes(W, P, fill=0):
    """seg_sizes(P); fill > 0: as many more buckets of 33 P + 1 entries (the fewest a listed bucket has) as `fill` terms hold"""
    U = usable_buckets(W)
    spec = []
    for w in range(W):
        shift = 64 * (w % 3) if U > 1024 else 0
        items = [(shift + j, c) for j, c in zip(SEG_SLOTS, seg_sizes(P))]
        if fill:
            c = (FIXUP_SERIAL_MAX + 1) * P + 1
            count = (fill - sum(seg_sizes(P))) // c
            j0 = shift + SEG_SLOTS[-1] + 1 + w % 4
            step = (U - j0) // count
            assert step >= 1
            items += [(j0 + step * t, c) for t in range(count)]
        spec.append(items)
    return spec, fill if fill else BASIS_MIN + 808


def _extreme(W, n, seed):
    """every signed window at -2^(width - 1) (the last bucket the window has) for half the terms and at 2^(width - 1) - 1 for the other
    half, the halves dealt out per window; top digits 1 .. the largest"""
    rng = np.random.default_rng(seed)
    D = np.zeros((W, n), dtype=np.int64)
    for w, h in enumerate(half_widths(W)):
        perm = rng.permutation(n)
        D[w, perm[: n // 2]] = -h
        D[w, perm[n // 2:]] = h - 1
    tm = top_digit_max(W)
    D[W - 1] = np.array([1, 2, tm, tm - 1, tm // 2])[np.arange(n) % 5]
    return D


DEGENERATE = ("all-zero", "one-nonzero", "mid-window-only", "top-window-only")


def _degenerate(kind, W, n, seed):
    rng = np.random.default_rng(seed)
    D = np.zeros((W, n), dtype=np.int64)
    if kind == "one-nonzero":
        k = int.from_bytes(rng.bytes(32), "little") >> 4
        D[:, n - 1] = msm_signed_digits(k, W)
    elif kind == "mid-window-only":
        D[W // 2] = rng.integers(1, half_widths(W)[W // 2], size=n)
    elif kind == "top-window-only":
        D[W - 1] = rng.integers(1, top_digit_max(W) + 1, size=n)
    else:
        assert kind == "all-zero"
    return D


# --------------------------------------------------------------------------------------------------------------------- layouts
Layout = collections.namedtuple("Layout", "key name W unit scheme n S")
# key = (layout, W, unit, n): unit 0 where the layout is not measured in one, n 0 where the layout decides it
OVERFLOW_N = 40000
SMALL_N, LARGE_N = 20000, 150001


@functools.lru_cache(maxsize=None)
def build(key):
    name, W, unit, n = key
    seed = [0x4D534D, W, unit, n, sum(name.encode())]
    scheme = None
    if name == "heads-boundary":
        (spec, n), scheme = _heads_boundary(W, unit), "chunks"
    elif name == "sparse-runs":
        (spec, n), scheme = _sparse_runs(W, unit), "chunks"
    elif name == "segment-sizes":
        (spec, n), scheme = _segment_sizes(W, unit), "segments"
    elif name == "big-list-overflow":
        (spec, n), scheme = _segment_sizes(W, unit, fill=OVERFLOW_N), "segments"
    else:
        spec = None
    if spec is not None:
        D = digits_from_sizes(spec, W, n, seed)
    elif name == "extreme-buckets":
        D = _extreme(W, n, seed)
    else:
        assert name in DEGENERATE, name
        D = _degenerate(name, W, n, seed)
    return Layout(key, name, W, unit, scheme, n, scalars_from_digits(D, W))


@functools.lru_cache(maxsize=None)
def point_pool():
    """4101 points: 2053 of the full group and 2048 of the prime-order subgroup"""
    from util import rand_points

    return np.concatenate([rand_points(0x4D534D50, 2053), rand_points(0x4D534D51, 2048, subgroup=True)])


def points(n):
    pool = point_pool()
    return np.ascontiguousarray(pool[(np.arange(n) * 7 + 3) % len(pool)])


def layout_id(key):
    name, W, unit, n = key
    return "%s-W%d" % (name, W) + ("-u%d" % unit if unit else "") + ("-n%d" % n if n else "")


# ---------------------------------------------------------------------------------------------------------------- what runs where
Config = collections.namedtuple("Config", "id scheme W unit options basis")


def _cfg(cid, scheme, W, unit, basis=False, **opts):
    return Config(cid, scheme, W, unit, dict(opts, msm_small_max=0, msm_windows=W), basis)


CONFIGS = (
    _cfg("chunks-W23-c8-mem", "chunks", 23, 8, msm_accum=0, msm_chunk=8, msm_acc_lds=0),
    _cfg("chunks-W23-c8-lds", "chunks", 23, 8, msm_accum=0, msm_chunk=8, msm_acc_lds=1),
    _cfg("chunks-W23-c13-mem", "chunks", 23, 13, msm_accum=0, msm_chunk=13, msm_acc_lds=0),
    _cfg("chunks-W23-c13-lds", "chunks", 23, 13, basis=True, msm_accum=0, msm_chunk=13, msm_acc_lds=1),
    _cfg("chunks-W17-c8", "chunks", 17, 8, msm_accum=0, msm_chunk=8),              # 16384 buckets: offsets from memory, two-pass sort
    _cfg("segments-W23-P8-front0", "segments", 23, 8, msm_accum=1, msm_seg_len=8, msm_front1=0),
    _cfg("segments-W23-P8-front1", "segments", 23, 8, basis=True, msm_accum=1, msm_seg_len=8, msm_front1=1),
    _cfg("segments-W17-P8-hist-separate", "segments", 17, 8, msm_accum=1, msm_seg_len=8, msm_sort_hist_fused=0),
    _cfg("segments-W17-P8-hist-fused", "segments", 17, 8, msm_accum=1, msm_seg_len=8, msm_sort_hist_fused=1),
    _cfg("segments-W23-P33", "segments", 23, 33, msm_accum=1, msm_seg_len=33),
    Config("defaults", None, 0, 0, {}, False),
)


def config_layouts(cfg):
    """the keys of the layouts a configuration runs"""
    if cfg.scheme is None:                                           # the defaults: 23 windows + chunks, then 17 windows + segments
        return tuple((name, default_windows(n), 0, n) for n in (SMALL_N, LARGE_N) for name in DEGENERATE + ("extreme-buckets",))
    keys = []
    if cfg.scheme == "chunks":
        keys += [("heads-boundary", cfg.W, cfg.unit, 0), ("sparse-runs", cfg.W, cfg.unit, 0)]
    else:
        keys += [("segment-sizes", cfg.W, cfg.unit, 0)]
        if (FIXUP_SERIAL_MAX + 1) * cfg.unit + 1 <= OVERFLOW_N * cfg.W // (FIXUP_BIG_MAX + OVERFLOW_MARGIN):     # the list can overflow within 40 000 terms
            keys += [("big-list-overflow", cfg.W, cfg.unit, 0)]
    keys += [("extreme-buckets", cfg.W, 0, SMALL_N)] + [(name, cfg.W, 0, SMALL_N) for name in DEGENERATE]
    return tuple(keys)


def all_keys():
    return tuple(dict.fromkeys(k for cfg in CONFIGS for k in config_layouts(cfg)))


def pairs():
    return tuple((cfg, key) for cfg in CONFIGS for key in config_layouts(cfg))


def pass_unit(cfg, n):
    """(scheme, unit) the pass of n terms takes under cfg; the defaults: the automatic chunk is not modelled (0), the segment cap is
    P = min(SEG_PMAX, max(32, 2 n / B))"""
    if cfg.scheme is not None:
        return cfg.scheme, cfg.unit
    if n >= MSM_LARGE_MIN:
        return "segments", min(SEG_PMAX, max(32, 2 * n // buckets_per_window(default_windows(n))))
    return "chunks", 0


def model(sizes, scheme, unit, n):
    """the quantities a failure message names: what the kernels make of the bucket sizes (W x B) under (scheme, unit)"""
    sizes = np.asarray(sizes)
    out = collections.OrderedDict(n=n, entries=int(sizes.sum()), nonempty=int((sizes > 0).sum()), largest=int(sizes.max()))
    if scheme == "chunks" and unit:
        heads = np.stack([chunk_heads(s, unit) for s in sizes])
        runs = [r for s in sizes for r in empty_runs(s, unit)]
        out.update(max_heads=int(heads.max()), wave_folded=int((heads > FIXUP_SERIAL_MAX).sum()),
                   pair_folded=int(((heads > 0) & (heads <= FIXUP_SERIAL_MAX)).sum()), at_32=int((heads == 32).sum()), at_33=int((heads == 33).sum()),
                   longest_empty_run=max([r[0] for r in runs], default=0))
    if scheme == "segments":
        extra = extra_segments(sizes, unit)
        big = int((extra > FIXUP_SERIAL_MAX).sum())
        out.update(big=big, listed=min(big, FIXUP_BIG_MAX), overflowed=max(0, big - FIXUP_BIG_MAX),
                   merge_k32=int((extra == FIXUP_SERIAL_MAX).sum()), merge_small=int(((extra > 0) & (extra < FIXUP_SERIAL_MAX)).sum()),
                   max_extra=int(extra.max()), heads=int(extra.sum()), segments=int((sizes > 0).sum() + extra.sum()))
    return out


def describe(m):
    return ", ".join("%s=%d" % kv for kv in m.items())
