"""
The parity matrix of the planner overrides (include/jubjub_hip.h: "every value gives the same results"), as plain data.

Each row is (options for jj_ctx_set_option, why the row exists).  tests/test_gpu_planner.py runs one shared corpus through every
row on a context of its own and compares bit for bit with the oracle; tests/test_planner_matrix_cpu.py fails when a key of the
planner section of ctx_options() (jubjub_amd/csrc/jj_pipeline.hip) has no row, or when an end of its range is neither in some row
nor explained in UNCOVERED_ENDS.  No GPU import here.

Bucket counts per window B = 2^(floor(253 / W) + [253 mod W != 0] - 1): W = 16 -> 32768, 17 -> 16384, 18 -> 8192, 20 -> 4096,
23 -> 1024, 28 -> 512, 33 and 36 -> 128.  Without msm_windows the planner takes 23 windows below 147 456 terms and 17 from there
(msm_windows_for), so the corpus's largest case (212 993 terms) runs 17 windows unless a row forces the layout.
"""

PIPPENGER = {"msm_small_max": 0}          # every corpus size through the Pippenger planner, not the small-batch path

# the largest corpus case: with 20 windows and msm_sort_blocks_per_cu = 4 the one-pass sort of 256 CUs is cut into 4 * 256 / 20 = 51
# parts, fewer than the (n + 4095) / 4096 = 52 parts the term count allows -- the part count is limited by the CUs, not by the terms
LARGE_N = 212993


def _row(reason, **opts):
    return (dict(opts), reason)


ROWS = [
    # ---- front end: the four-launch one-pass sort (k_msm_convert -> k_msm_hist -> k_msm_plan -> k_msm_scatter)
    _row("legacy one-pass sort at exactly 4096 buckets (20 windows; msm_sort_two_pass=0, or the two-pass sort takes them)",
         msm_front1=0, msm_windows=20, msm_sort_two_pass=0, **PIPPENGER),
    _row("legacy one-pass sort, 1024 buckets (23 windows)", msm_front1=0, msm_windows=23, **PIPPENGER),
    _row("legacy one-pass sort, 512 buckets, windows of two widths (28 windows)", msm_front1=0, msm_windows=28, **PIPPENGER),
    _row("legacy one-pass sort, the narrowest layout (36 windows: 128 and 64 buckets)", msm_front1=0, msm_windows=36, **PIPPENGER),
    _row("legacy one-pass sort in front of the segment accumulation", msm_front1=0, msm_windows=23, msm_accum=1, **PIPPENGER),
    _row("two-launch one-pass sort (k_msm_front2 / k_msm_scatter2) at exactly 4096 buckets",
         msm_front1=1, msm_windows=20, msm_sort_two_pass=0, **PIPPENGER),
    # ---- front-end parts of k_msm_front2 / k_msm_scatter2: f2_parts = min(blocks_per_cu * CUs / W, 64, (n + 4095) / 4096)
    _row("one part per CU at 4096 buckets", msm_sort_blocks_per_cu=1, msm_windows=20, msm_sort_two_pass=0, msm_accum=0, **PIPPENGER),
    _row("three parts per CU at 4096 buckets", msm_sort_blocks_per_cu=3, msm_windows=20, msm_sort_two_pass=0, msm_accum=0, **PIPPENGER),
    _row("four parts per CU at 4096 buckets: the large case is limited by the CU count (51 parts on 256 CUs)",
         msm_sort_blocks_per_cu=4, msm_windows=20, msm_sort_two_pass=0, msm_accum=0, **PIPPENGER),
    _row("one part per CU at 1024 buckets", msm_sort_blocks_per_cu=1, msm_windows=23, msm_accum=0, **PIPPENGER),
    _row("three parts per CU at 1024 buckets", msm_sort_blocks_per_cu=3, msm_windows=23, msm_accum=0, **PIPPENGER),
    _row("four parts per CU at 1024 buckets (44 parts on 256 CUs: the large case is CU-limited here too)",
         msm_sort_blocks_per_cu=4, msm_windows=23, msm_accum=0, **PIPPENGER),
    # ---- chunked accumulation (k_msm_accumulate<lds> + k_msm_fixup): entries per lane forced, offsets in LDS or in memory
    _row("shortest chunk, offsets in memory", msm_chunk=8, msm_acc_lds=0, msm_accum=0, **PIPPENGER),
    _row("shortest chunk, offsets in LDS", msm_chunk=8, msm_acc_lds=1, msm_accum=0, **PIPPENGER),
    _row("a chunk that divides no power of two, offsets in memory", msm_chunk=13, msm_acc_lds=0, msm_accum=0, **PIPPENGER),
    _row("a chunk that divides no power of two, offsets in LDS", msm_chunk=13, msm_acc_lds=1, msm_accum=0, **PIPPENGER),
    _row("1000 entries: longer than the small sizes (one chunk holds every term), ragged against the others; offsets in memory",
         msm_chunk=1000, msm_acc_lds=0, msm_accum=0, **PIPPENGER),
    _row("1000 entries, offsets in LDS", msm_chunk=1000, msm_acc_lds=1, msm_accum=0, **PIPPENGER),
    _row("longest chunk (1024 > n for the small sizes: one chunk per window), offsets in memory",
         msm_chunk=1024, msm_acc_lds=0, msm_accum=0, **PIPPENGER),
    _row("longest chunk, offsets in LDS", msm_chunk=1024, msm_acc_lds=1, msm_accum=0, **PIPPENGER),
    _row("automatic chunk sized for one round of workgroups per CU", msm_chunk_waves=1, msm_accum=0, **PIPPENGER),
    _row("automatic chunk sized for eight rounds of workgroups per CU", msm_chunk_waves=8, msm_accum=0, **PIPPENGER),
    # ---- one-level reduce (k_msm_reduce_fold): L buckets per quad; the <true> form needs K = B / L > 64 nblk, i.e. K > 4096
    _row("one-level reduce, L = 2 at 32768 buckets: K = 16384, k_msm_reduce_fold<true>", msm_windows=16, msm_reduce_l1=0, msm_reduce_chunk=2, **PIPPENGER),
    _row("one-level reduce, L = 4 at 32768 buckets: K = 8192, k_msm_reduce_fold<true>", msm_windows=16, msm_reduce_l1=0, msm_reduce_chunk=4, **PIPPENGER),
    _row("one-level reduce, L = 256 at 32768 buckets: k_msm_reduce_fold<false>", msm_windows=16, msm_reduce_l1=0, msm_reduce_chunk=256, **PIPPENGER),
    _row("one-level reduce, L = 2 at 1024 buckets: k_msm_reduce_fold<false>", msm_windows=23, msm_reduce_l1=0, msm_reduce_chunk=2, **PIPPENGER),
    _row("one-level reduce, L = 4 at 1024 buckets", msm_windows=23, msm_reduce_l1=0, msm_reduce_chunk=4, **PIPPENGER),
    _row("one-level reduce, L = 256 at 1024 buckets: four chunks per window", msm_windows=23, msm_reduce_l1=0, msm_reduce_chunk=256, **PIPPENGER),
    _row("msm_reduce_chunk larger than B (256 > 128 buckets): clamped to one chunk per window", msm_windows=36, msm_reduce_l1=0, msm_reduce_chunk=256, **PIPPENGER),
    # ---- two-level reduce (k_msm_reduce_l1 / _l2): both ends of the row count and of the level-2 chunk
    _row("two-level reduce with the most rows (64)", msm_windows=16, msm_reduce_l1=64, **PIPPENGER),
    _row("two-level reduce, two rows, the longest level-2 chunk (64)", msm_windows=16, msm_reduce_l1=2, msm_reduce_l2_chunk=64, **PIPPENGER),
    _row("two-level reduce, eight rows, the shortest level-2 chunk (2)", msm_windows=16, msm_reduce_l1=8, msm_reduce_l2_chunk=2, **PIPPENGER),
    # ---- small-batch path (k_msm_small_tables + k_msm_small_sum): 1..64 partial-sum trees per window
    _row("small path with one tree per window (every size up to 65536 terms)", msm_small_blk=1, msm_small_max=65536),
    _row("small path with two trees per window", msm_small_blk=2, msm_small_max=65536),
    _row("small path with all 64 trees (16385 and 40000 terms >= 64 * 256) and the largest msm_small_max: every corpus case small",
         msm_small_blk=64, msm_small_max=1 << 20),
    # ---- segment path (k_seg_* + k_msm_accumulate_seg + k_msm_fixup_big): segment cap P; the equal-scalar cases make buckets longer than P
    _row("segments of at most 8 entries", msm_accum=1, msm_seg_len=8, **PIPPENGER),
    _row("segments of at most 33 entries (not a power of two)", msm_accum=1, msm_seg_len=33, **PIPPENGER),
    _row("segments of at most 1024 entries (the largest cap)", msm_accum=1, msm_seg_len=1024, **PIPPENGER),
    # ---- narrow layouts
    _row("33 windows: 22 of 8 bits and 11 of 7 bits (128 and 64 buckets)", msm_windows=33, **PIPPENGER),
    _row("36 windows, the most there are: one of 8 bits and 35 of 7 bits", msm_windows=36, **PIPPENGER),
    # ---- two-pass sort
    _row("two-pass sort at exactly 4096 buckets", msm_windows=20, msm_sort_two_pass=1, **PIPPENGER),
    _row("two-pass sort with the separate histogram and plan kernels", msm_windows=18, msm_sort_hist_fused=0, **PIPPENGER),
    _row("two-pass sort with the histogram fused into the conversion", msm_windows=18, msm_sort_hist_fused=1, **PIPPENGER),
    # ---- the automatic values, spelled out
    _row("every planner value that means 'from n' set explicitly (the lower ends of msm_windows, msm_seg_len, msm_chunk, "
         "msm_reduce_chunk, msm_reduce_l2_chunk, and -1 of msm_accum / msm_reduce_l1 / msm_sort_two_pass)",
         msm_windows=0, msm_accum=-1, msm_seg_len=0, msm_chunk=0, msm_reduce_chunk=0, msm_reduce_l1=-1, msm_reduce_l2_chunk=0,
         msm_sort_two_pass=-1, **PIPPENGER),
    # ---- var-base ladders (the row's var-base corpus) and the decoder (test_gpu_planner.py's decoder section picks dec_c_mid per variant)
    _row("constant-time ladder with signed 2-bit windows, one scalar-mul per lane", vb_ct_window=2, vb_quad_max=0),
    _row("constant-time ladder with signed 3-bit windows, one scalar-mul per quad for every batch", vb_ct_window=3, vb_quad_max=1 << 20),
    _row("decoder: k_decompress<8> for [8, 16) x lanes", dec_c_mid=8),
    _row("decoder: k_decompress<16> for [8, 16) x lanes", dec_c_mid=16),
]

# (key, "lo" | "hi") -> why that end of the range has no row.  Empty: every end is in some row.
UNCOVERED_ENDS = {}

# option values jj_ctx_set_option must refuse (JJ_ERR_INVALID) although they lie inside the [lo, hi] of the table
REJECTED = [("msm_reduce_chunk", 3), ("msm_chunk", 7), ("msm_seg_len", 7), ("msm_windows", 15), ("dec_c_mid", 12)]


def row_id(k):
    opts = ROWS[k][0]
    return "r%02d-" % k + "-".join("%s=%d" % (key.replace("msm_", ""), v) for key, v in opts.items())
