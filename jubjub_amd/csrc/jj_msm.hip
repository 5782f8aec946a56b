// libjubjub_hip.so: multi-scalar multiplication (kernels: jj_msm_kernels.h; host tail: jj_host_tail.h).
#define JJ_KERNELS_MSM
#include "jj_engine.h"
#include "jj_sig_kernels.h"
#include "jj_sig_keyed_kernels.h"
#include "jj_sig_seg_kernels.h"

// MSM on the device up to the record of partial window sums (jj_msm_kernels.h); everything here is launches only (the
// workspaces are grown first), so a pass can be queued behind another one without any host synchronisation in between.
//   part_w0 / part_stride: the pass owns windows part_w0, part_w0 + part_stride, ... (0 / 1: all of them)
//   rec_dev: MSM_REC bytes of device memory for the record
static_assert(MSM_SMALL_BLK_MAX == MSM_TREE_QUADS, "JJ_MSM_SMALL_BLK bound");
struct MsmGeometry { bool small; MsmParams mp; u32 nblk; };
static void msm_layout(MsmParams& mp, int W, int w0, int wstride) {
  mp.W = W; mp.c = 253 / W; mp.r = 253 % W;
  mp.w0 = w0; mp.wstride = wstride < 1 ? 1 : wstride;
  mp.Ws = w0 < W ? (W - w0 + mp.wstride - 1) / mp.wstride : 0;
  mp.B = 1u << (mp.c + (mp.r ? 1 : 0) - 1);
  memset(mp.recode, 0, sizeof mp.recode);
  int bit = 0;
  for (int w = 0; w < W - 1; w++) { const int width = mp.c + (w < mp.r ? 1 : 0); const int b = bit + width - 1; mp.recode[b >> 5] |= 1u << (b & 31); bit += width; }
}
// number of windows for n terms (measured on MI355X; JJ_MSM_WINDOWS overrides): the windows tile the 253 scalar bits exactly, so
// any W is as good as its entry count n W and its bucket count ~ W 2^(253/W - 1) make it
// from this many terms the large-input configuration (17 / 16 windows, length-sorted segments) is faster than 23 windows + chunks + fix-up
// (experiments/misc/msm_crossover.py: 131 072 terms 0.438 against 0.448 ms, 150 000 terms 0.485 against 0.459 ms, 235 000 terms 0.727 against 0.533 ms)
constexpr size_t MSM_LARGE_MIN = (size_t)9 << 14;
static int msm_windows_default(size_t n);
static int msm_windows_for(jj_ctx* c, size_t n) {
  if (c->msm_windows >= MSM_WINDOWS_MIN && c->msm_windows <= MSM_WINDOWS_MAX) return c->msm_windows;
  return msm_windows_default(n);
}
static int msm_windows_default(size_t n) {
  // measured (experiments/misc/msm_sweep*.sh, profiles/r3_msm_window_sweep.txt, r3_msm_reduce_grid.txt): 16 windows (13 of 16 bits, 3 of
  // 15) from 2^18 terms (round 6; from 2^20 before: with the two-level reduce -- 8 level-1 rows -- the 2^15 buckets per window no longer cost
  // a 210 us chain, and 16 windows beat 17 by 0.5 % at 2^18 and 2 % at 2^19 terms, profiles/r5_msm_mid_sweep.txt); 17 windows (15 of 15 bits,
  // 2 of 14: half the buckets for 6 % more additions) from MSM_LARGE_MIN terms; below, 23 windows of 11 bits: wider windows cut the additions
  // but their buckets (4096+ per window) make the fix-up and reduce chains longer than the additions they save
  return n >= ((size_t)1 << 18) ? 16 : n >= MSM_LARGE_MIN ? 17 : 23;
}
// counters (MSM_COUNTER_WORDS words, cleared by the first kernel of a pass) | big-bucket work list | workgroup partial sums
constexpr size_t MSM_BIG_OFF = 512, MSM_PART_OFF = MSM_BIG_OFF + sizeof(BigBucket) * FIXUP_BIG_MAX;
static int msm_ensure_ctl(jj_ctx* c, MsmLane& L) { return ensure(c, L.ctl, MSM_PART_OFF + (size_t)64 * MSM_TREE_QUADS * MSM_PART_WORDS * 4); }
static int msm_enqueue_small(jj_ctx* c, MsmLane& L, size_t n, const void* ds, const void* dp, int part_w0, int part_stride, void* rec_dev) {
  MsmParams mp;
  msm_layout(mp, SM_W, part_w0, part_stride);
  int rc;
  if ((rc = ensure(c, L.buf[0], n * 32))) return rc;
  if ((rc = ensure(c, L.buf[1], n * (size_t)(SM_SLOTS * ENIELS_WORDS) * 4))) return rc;
  if ((rc = msm_ensure_ctl(c, L))) return rc;
  u32* counters = (u32*)L.ctl.p; u32* part = (u32*)((uint8_t*)L.ctl.p + MSM_PART_OFF);
  // workgroups of 64 quads per window: about 4 terms per quad, at most msm_small_blk (4 x 64 windows = one workgroup per CU)
  const u32 nblk = (u32)std::min<size_t>(c->msm_small_blk, std::max<size_t>(1, (n + 255) / 256));
  hipLaunchKernelGGL(k_msm_small_tables, dim3(blocks_for(4 * n)), dim3(256), 0, L.stream, n, ds, dp, mp, (u32*)L.buf[1].p, (u32*)L.buf[0].p, counters);
  hipLaunchKernelGGL(k_msm_small_sum, dim3(nblk, mp.Ws), dim3(4 * MSM_TREE_QUADS), 0, L.stream, n, mp, nblk, (const u32*)L.buf[1].p, (const u32*)L.buf[0].p, part, counters, (u32*)rec_dev);
  return JJ_OK;
}

// A pass over the resident records of a basis (jj_msm_basis_*) instead of the caller's points: `niels` replaces the lane's own array and no
// kernel converts points; W = the windows of the basis's layout (0: as jj_msm picks them); slot_stride > 0: the array is a WINDOW TABLE with
// row (w, i) at w * slot_stride + i -- the scatter writes that row into the sort's entries, every slot accumulates into its own bucket set as
// before, k_msm_fold_slots adds the sets into slot 0 and the reduce runs as a pass that owns window 0 alone (a record of one point).
struct MsmTab { const u32* niels; size_t slot_stride; int W; };
static int msm_enqueue_pippenger(jj_ctx* c, MsmLane& ln, size_t n, const void* ds, const void* dp, int part_w0, int part_stride, void* rec_dev, const MsmTab* tab = nullptr) {
  MsmParams mp;
  msm_layout(mp, tab && tab->W ? tab->W : msm_windows_for(c, n), part_w0, part_stride);
  const bool folded = tab && tab->slot_stride;
  MsmParams mpr = mp;                                                     // the layout of the reduce: the pass's own, or window 0 alone over the folded set
  if (folded) msm_layout(mpr, mp.W, 0, mp.W);
  const u32 B = mp.B, Ws = (u32)mp.Ws, Wr = (u32)mpr.Ws;
  const size_t nb = (size_t)Ws * B;
  // buckets per reduce chunk: a quad walks L buckets (2 L additions), then ~2 c operations multiply by the chunk's first index, and
  // every workgroup of 64 quads is one wave per SIMD of a CU.  The chains are bound by the instructions a wave issues, and a
  // second workgroup on a CU slows both by ~1.6x, so: the smallest L (at least 4) for which the workgroups that have chunks fit
  // one per CU.  JJ_MSM_REDUCE_CHUNK overrides; never more than one window.
  auto reduce_blocks = [&](u32 l) { const u32 nk = std::min<u32>(MSM_TREE_QUADS, (B / l + MSM_TREE_QUADS - 1) / MSM_TREE_QUADS); u32 t = 0; for (u32 s = 0; s < Wr; s++) t += msm_reduce_blocks(mpr, (int)s, l, nk); return t; };
  u32 L_auto = 4;
  while (L_auto < B && reduce_blocks(L_auto) > (u32)c->cus) L_auto <<= 1;
  const u32 L = std::min<u32>(c->msm_reduce_chunk ? (u32)c->msm_reduce_chunk : L_auto, B);
  if (B % L || (L & (L - 1))) { c->err = "inconsistent MSM tuning override (option msm_reduce_chunk must be a power of two dividing the bucket count)"; return JJ_ERR_INVALID; }
  const u32 K = B / L, nblk = std::min<u32>(MSM_TREE_QUADS, (K + MSM_TREE_QUADS - 1) / MSM_TREE_QUADS);      // workgroups of 64 quads per window, at most
  const u32 reduce_grid = reduce_blocks(L);
  int jbits = 0; while ((1u << jbits) < B) jbits++;
  // Two-level reduce (k_msm_reduce_l1 + k_msm_reduce_l2) for wide windows: level 1 sums R rows of the bucket matrix per lane (whole-lane
  // additions at full throughput), level 2 is the quad chain over M = B / R columns per window.  Narrow windows (2^17-term passes: 1024
  // buckets per window) keep the one-level kernel: level 1 would be an extra launch and ~20 us of chain for a level 2 that is as deep.
  u32 l1_rows = 0;
  if (c->msm_l1_rows > 0) l1_rows = (u32)c->msm_l1_rows;
  else if (c->msm_l1_rows < 0 && B >= 16384) l1_rows = B >= 32768 ? 8 : 4;
  const u32 Bmin = mp.r && !folded ? B / 2 : B;                           // buckets of the narrowest window of the layout (folded: window 0, the widest)
  while (l1_rows > 1 && (l1_rows > Bmin || B / l1_rows < 64)) l1_rows >>= 1;     // every window has at least one row; whole waves per window
  if (l1_rows < 2) l1_rows = 0;
  int mbits = 0; u32 L2 = 0, nblk2 = 0;
  if (l1_rows) {
    const u32 M = B / l1_rows;
    while ((1u << mbits) < M) mbits++;
    L2 = 4;
    while (L2 < M && ((u64)Wr * ((M / L2 + MSM_TREE_QUADS - 1) / MSM_TREE_QUADS) > (u64)c->cus || (M / L2 + MSM_TREE_QUADS - 1) / MSM_TREE_QUADS > (u32)MSM_TREE_QUADS)) L2 <<= 1;
    if (c->msm_l2_chunk && (u32)c->msm_l2_chunk <= M && (M / (u32)c->msm_l2_chunk + MSM_TREE_QUADS - 1) / MSM_TREE_QUADS <= (u32)MSM_TREE_QUADS) L2 = (u32)c->msm_l2_chunk;
    nblk2 = (M / L2 + MSM_TREE_QUADS - 1) / MSM_TREE_QUADS;
  }
  const size_t l1_bytes = l1_rows ? (size_t)Wr * (B / l1_rows) * ENIELS_WORDS * 4 : 0;      // one array of extended-Niels records (S, then T)
  int rc;
  DevBuf &kprime = ln.buf[0], &niels = ln.buf[1], &offb = ln.buf[2], &idx = ln.buf[3], &buckets = ln.buf[4], &ra = ln.buf[5], &tcnt = ln.buf[7];
  // Entries per lane of the chunked accumulation (below MSM_LARGE_MIN terms; above, the segments decide).  The launch is Ws x ceil(nchunk / 256)
  // workgroups of one wave per SIMD, and the dispatcher deals them round the CUs: what counts is how many ROUNDS of workgroups a CU gets, so the
  // chunk is the shortest one that fits the launch into msm_chunk_waves rounds (round 6: 2^17 terms ran 16 entries in 2.9 rounds -- three -- where
  // 24 entries in 1.9 rounds cost the same accumulation time and leave a third fewer heads to the fix-up: 353 -> 339 us per call; 2^16 terms ran
  // 1.4 rounds, i.e. two, of 16 entries for 23 entries' worth of work).  Rounds 2-5: 16 entries up to 2^19 terms, 8 below 2^15.
  u32 chunk = 8;
  // Jobs in flight (lanes of their own) share the CUs with the neighbouring job's kernels, the rounds argument does not hold for them and
  // shorter chunks interleave better: one round more (measured, four jobs in flight at 2^17 terms: 0.228-0.241 ms per MSM against 0.249-0.258).
  { const size_t cap = (size_t)(std::max(1, c->msm_chunk_waves) + (&ln != &c->lanes[0] ? 1 : 0)) * (size_t)c->cus;
    while (chunk < 1024 && (size_t)Ws * ((((n + chunk - 1) / chunk) + 255) / 256) > cap) chunk++; }
  if (c->msm_chunk) chunk = (u32)c->msm_chunk;
  const u32 nchunk = (u32)((n + chunk - 1) / chunk);
  const bool two_pass = B > 4096 || (B == 4096 && c->msm_two_pass != 0);      // the one-pass plan kernel covers 4096 buckets per window
  const u32 HB = B >> MSM_LO_BITS;
  if (two_pass && HB > MSM_HB_MAX) { c->err = "MSM window layout has more coarse bins per window than the two-pass sort holds (option msm_windows must be 16..36)"; return JJ_ERR_INVALID; }
  const u32 ptiles = (u32)((n + MSM_P1_TILE - 1) / MSM_P1_TILE);        // the first pass of the two-pass sort orders a whole tile in LDS
  const size_t pm = (size_t)HB * ptiles;                               // runs per slot
  // one-pass sort tiles: enough (tile, window) blocks to fill the GPU, each at least 4096 terms
  const u32 ntiles = (u32)std::max<size_t>(1, std::min<size_t>((size_t)(c->cus + Ws - 1) / Ws, (n + 4095) / 4096));
  const size_t tile = (n + ntiles - 1) / ntiles;
  // one-pass sort in two launches (round 6): counting blocks (part, slot), as many parts as give every CU one block, each part at least 4096 terms
  const u32 f2_parts = (u32)std::max<size_t>(1, std::min<size_t>(std::min<size_t>((size_t)c->msm_sort_blocks_per_cu * c->cus / Ws, MSM_F2_PARTS_MAX), (n + 4095) / 4096));
  const size_t f2_part_terms = (n + f2_parts - 1) / f2_parts;
  const bool front1 = !two_pass && c->msm_front1 && B <= 4096;
  const bool use_segments = c->msm_segments == 1 || (c->msm_segments < 0 && n >= MSM_LARGE_MIN);
  // segments of at most P entries, sorted by length; P bounds the serial depth of one lane: twice the mean bucket of the widest windows
  u32 P = (u32)std::min<size_t>(SEG_PMAX, std::max<size_t>(32, 2 * n / B));
  if (c->msm_seg_len >= 8 && c->msm_seg_len <= SEG_PMAX) P = (u32)c->msm_seg_len;
  const u32 stiles = (u32)std::max<size_t>(1, std::min<size_t>(4096, (nb + 255) / 256));          // tiles of the two segment passes: 256 buckets each, more above 2^20 buckets
  const u32 per_tile = (u32)((nb + stiles - 1) / stiles);
  // with the two-pass sort a tile of the segment passes is exactly the 256 buckets of one k_msm_part_sort workgroup, which then writes the tile's
  // histogram of segment lengths itself (no k_seg_hist launch)
  const bool seg_fused = use_segments && two_pass && per_tile == (1u << MSM_LO_BITS) && (size_t)stiles * per_tile == nb && stiles == Ws * HB;
  const size_t max_segs = nb + (n * (size_t)Ws) / P + 1;
  const size_t bh_words = (size_t)stiles * (P + 1), hdr_words = bh_words + 2 * (P + 2) + 16;
  if ((rc = ensure(c, kprime, n * 32))) return rc;
  if (!tab && (rc = ensure(c, niels, n * (size_t)GNIELS_WORDS * 4))) return rc;
  if ((rc = ensure(c, offb, (size_t)Ws * (B + 1) * 4))) return rc;
  if ((rc = ensure(c, idx, n * (size_t)Ws * 4))) return rc;
  if ((rc = ensure(c, tcnt, two_pass ? ((size_t)Ws * (2 * pm + 1)) * 4 : front1 ? (size_t)Ws * f2_parts * B * 4 : (size_t)Ws * ntiles * B * 4))) return rc;
  if ((rc = ensure(c, buckets, (size_t)EXT_AOS_WORDS * 4 * nb))) return rc;
  // ra: first the two-pass sort's records (4 + 1 bytes per entry), then the chunk heads / segment heads
  // (and, once the heads are folded in, the two arrays level 1 of the reduce hands to level 2)
  if ((rc = ensure(c, ra, std::max<size_t>(std::max<size_t>((size_t)EXT_AOS_WORDS * 4 * std::max<size_t>((size_t)Ws * nchunk, (n * (size_t)Ws) / 8 + 1), n * (size_t)Ws * 5 + 64), 2 * l1_bytes)))) return rc;
  if ((rc = msm_ensure_ctl(c, ln))) return rc;                                                           // counters, big-bucket work list, workgroup partial sums
  if ((rc = ensure(c, ln.bigpart, (size_t)5 * NL * 4 * FIXUP_BIG_MAX * FIXUP_BIG_QUADS))) return rc;      // the big buckets' partial sums
  if (use_segments && (rc = ensure(c, ln.seg, hdr_words * 4 + 16 + nb * sizeof(MergeItem) + max_segs * sizeof(Seg)))) return rc;   // bh [stiles][P+1] | count [P+1] | offset [P+2] | merge list | segments
  hipStream_t st = ln.stream;
  u32* off = (u32*)offb.p;
  u32* counters = (u32*)ln.ctl.p;                          // cleared by the sort's plan kernel
  BigBucket* big = (BigBucket*)((uint8_t*)ln.ctl.p + MSM_BIG_OFF);
  u32* part = (u32*)((uint8_t*)ln.ctl.p + MSM_PART_OFF);
  const u32* nl = tab ? tab->niels : (const u32*)niels.p;                    // the records the accumulation gathers
  const size_t ts = folded ? tab->slot_stride : 0;
  // One conversion launch for scalars and points.  (Rounds 2-3 ran the point half on a second stream beside the sort from 2^18
  // terms; with the entries staged through LDS the conversion is short enough that the fork, its two events and the contention
  // with the sort's first kernel cost more than the overlap returns: 2^18 terms 0.565 -> 0.556 ms, 2^20 1.262 -> 1.254 ms.)
  // Two-pass sort, round 5: the coarse histogram is taken by the conversion kernel itself (k_msm_convert_hist: totals per (slot, bin)), the tiles of
  // the first pass reserve their runs with one global atomic per bin: no k_msm_part_hist, no k_msm_part_plan.  JJ_MSM_SORT_HIST=separate keeps the
  // round-4 kernels (per-tile counts + a scan: the order of the entries inside a bucket is then the order of the terms).
  // (measured, experiments/misc/msm_sort_hist_ab.py, three boxes: 2^20 terms -3 ... -7 % (1.32 -> 1.24 ms), 2^19 -1 ... -4 %, 2^18 and 2^21 0 ... -2 %, 2^22 +0.7 ... -1.5 %:
  // at 2^22 terms the 8192 tiles' atomics on the same 2048 cursors cost about what the histogram pass they replace costs, so the fused form stops at 3 x 2^20 terms)
  const bool fused_hist = !tab && two_pass && c->msm_fused_hist && Ws <= 64 && Ws * HB <= 4096 && n <= ((size_t)3 << 20);
  if (fused_hist) {
    const bool fresh = ln.bins.cap == 0;
    if ((rc = ensure(c, ln.bins, (size_t)2 * 2 * MSM_BINS_WORDS * 4))) return rc;
    if (fresh) { HIPCHK(c, hipMemsetAsync(ln.bins.p, 0, ln.bins.cap, st)); ln.bins_parity = 0; }     // afterwards every pass clears the other parity's half
    // 160 KB: the staging of sixteen waves + up to 4096 counters.  Once per CONTEXT, with its device current: the attribute belongs to the
    // device's copy of the kernel (jj_multi_* drives several devices from one process)
    if (!c->msm_hist_lds_set) { HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(k_msm_convert_hist), hipFuncAttributeMaxDynamicSharedMemorySize, MSM_CH_STAGE_WORDS * 4 + 16384)); c->msm_hist_lds_set = true; }
    u32* totals = (u32*)ln.bins.p + (size_t)ln.bins_parity * 2 * MSM_BINS_WORDS;
    u32* cursor = totals + MSM_BINS_WORDS;
    u32* other = (u32*)ln.bins.p + (size_t)(ln.bins_parity ^ 1) * 2 * MSM_BINS_WORDS;
    ln.bins_parity ^= 1;
    u32* rec = (u32*)ra.p; uint8_t* lo8 = (uint8_t*)ra.p + n * (size_t)Ws * 4;     // the head buffer is free until the accumulation
    // terms per thread: four (4096 per workgroup: the fewest counter flushes) when that still gives every CU a workgroup, fewer for smaller inputs
    const int per = (int)std::max<size_t>(1, std::min<size_t>(MSM_CH_PER, n / ((size_t)c->cus * MSM_CH_THREADS)));
    hipLaunchKernelGGL(k_msm_convert_hist, dim3((unsigned)((n + (size_t)per * MSM_CH_THREADS - 1) / ((size_t)per * MSM_CH_THREADS))), dim3(MSM_CH_THREADS), MSM_CH_STAGE_WORDS * 4 + Ws * HB * 4, st, n, ds, dp, mp, (u32*)kprime.p, (u32*)niels.p, totals, other, counters, per);
    hipLaunchKernelGGL(k_msm_part_scatter, dim3(ptiles, Ws), dim3(MSM_SORT_THREADS), 0, st, n, (size_t)MSM_P1_TILE, mp, (const u32*)kprime.p, (const u32*)nullptr, rec, lo8, (const u32*)totals, cursor);
    if (seg_fused) hipLaunchKernelGGL(k_msm_part_sort<true>, dim3(HB, Ws), dim3(MSM_P2_THREADS), 0, st, mp, (u32)n, (const u32*)nullptr, (const u32*)rec, (const uint8_t*)lo8, (u32*)idx.p, off, P, ExtAoS{(u32*)buckets.p}, (u32*)ln.seg.p, (const u32*)totals);
    else hipLaunchKernelGGL(k_msm_part_sort<false>, dim3(HB, Ws), dim3(MSM_P2_THREADS), 0, st, mp, (u32)n, (const u32*)nullptr, (const u32*)rec, (const uint8_t*)lo8, (u32*)idx.p, off, P, ExtAoS{nullptr}, (u32*)nullptr, (const u32*)totals);
  } else if (two_pass) {
    // (a basis: the scalars alone, and the separate histogram kernels -- the fused one converts points on its way)
    hipLaunchKernelGGL(k_msm_convert, dim3(blocks_for(n)), dim3(256), 0, st, n, ds, dp, mp, (u32*)kprime.p, (u32*)niels.p, tab ? 1 : 3);
    u32* tc = (u32*)tcnt.p; u32* tcs = tc + (size_t)Ws * pm;
    u32* rec = (u32*)ra.p; uint8_t* lo8 = (uint8_t*)ra.p + n * (size_t)Ws * 4;     // the head buffer is free until the accumulation
    hipLaunchKernelGGL(k_msm_part_hist, dim3(ptiles, Ws), dim3(MSM_SORT_THREADS), 0, st, n, (size_t)MSM_P1_TILE, mp, (const u32*)kprime.p, tc);
    hipLaunchKernelGGL(k_msm_part_plan, dim3(Ws), dim3(1024), 0, st, n, (u32)pm, (const u32*)tc, tcs, counters);
    if (folded) hipLaunchKernelGGL(k_msm_part_scatter_tab, dim3(ptiles, Ws), dim3(MSM_SORT_THREADS), 0, st, n, (size_t)MSM_P1_TILE, mp, (const u32*)kprime.p, (const u32*)tcs, rec, lo8, (const u32*)nullptr, (u32*)nullptr, ts);
    else hipLaunchKernelGGL(k_msm_part_scatter, dim3(ptiles, Ws), dim3(MSM_SORT_THREADS), 0, st, n, (size_t)MSM_P1_TILE, mp, (const u32*)kprime.p, (const u32*)tcs, rec, lo8, (const u32*)nullptr, (u32*)nullptr);
    if (seg_fused) hipLaunchKernelGGL(k_msm_part_sort<true>, dim3(HB, Ws), dim3(MSM_P2_THREADS), 0, st, mp, ptiles, (const u32*)tcs, (const u32*)rec, (const uint8_t*)lo8, (u32*)idx.p, off, P, ExtAoS{(u32*)buckets.p}, (u32*)ln.seg.p, (const u32*)nullptr);
    else hipLaunchKernelGGL(k_msm_part_sort<false>, dim3(HB, Ws), dim3(MSM_P2_THREADS), 0, st, mp, ptiles, (const u32*)tcs, (const u32*)rec, (const uint8_t*)lo8, (u32*)idx.p, off, P, ExtAoS{nullptr}, (u32*)nullptr, (const u32*)nullptr);
  } else if (front1) {
    // round 6: counting (from the raw scalars) + point conversion in one launch, plan + scatter in the next (k_msm_front2 / k_msm_scatter2); no k'
    const size_t f2_lds = std::max<size_t>((size_t)B * 4, (size_t)MSM_F2_STAGE_WORDS * 4);
    if (!c->msm_front1_lds_set) { HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(k_msm_front2), hipFuncAttributeMaxDynamicSharedMemorySize, (int)std::max<size_t>((size_t)4096 * 4, (size_t)MSM_F2_STAGE_WORDS * 4))); c->msm_front1_lds_set = true; }
    // (a basis: the counting workgroups alone -- the grid ends before the workgroups that convert points)
    hipLaunchKernelGGL(k_msm_front2, dim3(f2_parts * Ws + (tab ? 0u : (unsigned)((n + MSM_F2_THREADS - 1) / MSM_F2_THREADS))), dim3(MSM_F2_THREADS), f2_lds, st, n, ds, dp, mp, (u32*)niels.p, (u32*)tcnt.p, counters, f2_parts, f2_part_terms);
    if (folded) hipLaunchKernelGGL(k_msm_scatter2_tab, dim3(f2_parts * 8 * ((Ws + 7) / 8)), dim3(MSM_SORT_THREADS), B * 4, st, n, f2_parts, f2_part_terms, mp, ds, (const u32*)tcnt.p, off, (u32*)idx.p, ts);
    else hipLaunchKernelGGL(k_msm_scatter2, dim3(f2_parts * 8 * ((Ws + 7) / 8)), dim3(MSM_SORT_THREADS), B * 4, st, n, f2_parts, f2_part_terms, mp, ds, (const u32*)tcnt.p, off, (u32*)idx.p);
  } else {
    hipLaunchKernelGGL(k_msm_convert, dim3(blocks_for(n)), dim3(256), 0, st, n, ds, dp, mp, (u32*)kprime.p, (u32*)niels.p, tab ? 1 : 3);
    hipLaunchKernelGGL(k_msm_hist, dim3(ntiles, Ws), dim3(MSM_SORT_THREADS), B * 4, st, n, tile, mp, (const u32*)kprime.p, (u32*)tcnt.p);
    hipLaunchKernelGGL(k_msm_plan, dim3(Ws), dim3(1024), 0, st, n, B, ntiles, (u32*)tcnt.p, off, counters);
    if (folded) hipLaunchKernelGGL(k_msm_scatter_tab, dim3(ntiles * 8 * ((Ws + 7) / 8)), dim3(MSM_SORT_THREADS), B * 4, st, n, tile, ntiles, mp, (const u32*)kprime.p, (const u32*)tcnt.p, (u32*)idx.p, ts);
    else hipLaunchKernelGGL(k_msm_scatter, dim3(ntiles * 8 * ((Ws + 7) / 8)), dim3(MSM_SORT_THREADS), B * 4, st, n, tile, ntiles, mp, (const u32*)kprime.p, (const u32*)tcnt.p, (u32*)idx.p);
  }
  const ExtAoS head{(u32*)ra.p}, bk{(u32*)buckets.p};
  SoA partial = soa_of(ln.bigpart, (size_t)FIXUP_BIG_MAX * FIXUP_BIG_QUADS);
  const MergeItem* merge_list = nullptr;
  if (use_segments) {
    u32* bh = (u32*)ln.seg.p; u32* soff = bh + bh_words + (P + 1);
    MergeItem* merge = (MergeItem*)(((uintptr_t)(bh + hdr_words) + 15) & ~(uintptr_t)15);
    Seg* seg = (Seg*)(merge + nb);
    if (!seg_fused) hipLaunchKernelGGL(k_seg_hist, dim3(stiles), dim3(256), 0, st, nb, B, per_tile, P, (const u32*)off, bk, bh);
    hipLaunchKernelGGL(k_seg_plan, dim3(P + 1), dim3(256), 0, st, stiles, bh, soff);
    hipLaunchKernelGGL(k_seg_scatter, dim3(stiles), dim3(256), 0, st, nb, B, per_tile, P, (const u32*)off, (const u32*)bh, (const u32*)soff, soff + (P + 1), seg, counters, merge, big);
    hipLaunchKernelGGL(k_msm_accumulate_seg, dim3(blocks_for(max_segs)), dim3(256), 0, st, (const u32*)(soff + (P + 1)), (const Seg*)seg, (const u32*)idx.p, nl, bk, head);
    merge_list = merge;
  } else {
    if (B <= MSM_ACC_LDS_BUCKETS && c->msm_acc_lds) hipLaunchKernelGGL(k_msm_accumulate<true>, dim3(blocks_for(nchunk), Ws), dim3(256), (B + 1) * 4, st, n, B, chunk, nchunk, (const u32*)off, (const u32*)idx.p, nl, bk, head);
    else hipLaunchKernelGGL(k_msm_accumulate<false>, dim3(blocks_for(nchunk), Ws), dim3(256), 0, st, n, B, chunk, nchunk, (const u32*)off, (const u32*)idx.p, nl, bk, head);
    hipLaunchKernelGGL(k_msm_fixup, dim3(blocks_for(2 * nb)), dim3(256), 0, st, n, B, Ws, chunk, nchunk, (const u32*)off, bk, head);      // (big buckets included: no second launch)
  }
  // (segment path: 512 workgroups, the merge list of repeated scalars is walked by the same launch as the big buckets)
  if (use_segments) hipLaunchKernelGGL(k_msm_fixup_big, dim3(2u * (unsigned)c->cus), dim3(256), 0, st, counters, (const BigBucket*)big, bk, head, partial, merge_list);
  if (folded && Ws > 1) {
    // lanes per bucket: as many (up to 8) as keep the launch within about two waves per SIMD
    u32 fp = 8;
    while (fp > 1 && (size_t)B * fp > (size_t)c->cus * 512) fp >>= 1;
    hipLaunchKernelGGL(k_msm_fold_slots, dim3(blocks_for((size_t)B * fp)), dim3(256), 0, st, B, Ws, fp, bk);
  }
  if (l1_rows) {
    u32* SN = (u32*)ra.p; u32* TN = (u32*)((uint8_t*)ra.p + l1_bytes);        // the heads are dead: k_msm_fixup_big was their last reader
    hipLaunchKernelGGL(k_msm_reduce_l1, dim3(blocks_for((size_t)Wr << mbits)), dim3(256), 0, st, mpr, mbits, bk, SN, TN);
    hipLaunchKernelGGL(k_msm_reduce_l2, dim3(Wr * nblk2), dim3(4 * MSM_TREE_QUADS), 0, st, n, mpr, mbits, L2, nblk2, (const u32*)SN, (const u32*)TN, part, counters, (u32*)rec_dev);
  } else if (K > MSM_TREE_QUADS * nblk) hipLaunchKernelGGL(k_msm_reduce_fold<true>, dim3(reduce_grid), dim3(4 * MSM_TREE_QUADS), 0, st, n, mpr, L, nblk, jbits, bk, part, counters, (u32*)rec_dev);
  else hipLaunchKernelGGL(k_msm_reduce_fold<false>, dim3(reduce_grid), dim3(4 * MSM_TREE_QUADS), 0, st, n, mpr, L, nblk, jbits, bk, part, counters, (u32*)rec_dev);
  return JJ_OK;
}
// one pass (at most 2^24 terms: 32-bit sort indices), record left at rec_dev
static int msm_enqueue(jj_ctx* c, MsmLane& L, size_t n, const void* ds, const void* dp, int part_w0, int part_stride, void* rec_dev, size_t* rec_bytes) {
  const bool small = n <= (size_t)c->msm_small_max;
  *rec_bytes = jjhost::rec_bytes(small ? SM_W : msm_windows_for(c, n));
  return small ? msm_enqueue_small(c, L, n, ds, dp, part_w0, part_stride, rec_dev) : msm_enqueue_pippenger(c, L, n, ds, dp, part_w0, part_stride, rec_dev);
}
// lane k of the context, ready for use: lane 0 IS the context's launch stream (synchronous calls, host-staged inputs); the others own
// their stream, created on first use, and start a job after everything already queued on the launch stream (the inputs may have been
// produced there).  Jobs in flight (device-pointer inputs) alternate over lanes 1 .. msm_lanes and never run on lane 0: a lane that is the
// launch stream makes every other lane's next job wait for ITS job, and the jobs then run in pairs that start together (round 5,
// profiles/r5_msm_allgather_timeline.txt: -6 % with two or three jobs in flight once the lanes are independent)
static int msm_lane(jj_ctx* c, int k, MsmLane** out) {
  MsmLane& L = c->lanes[k];
  if (k == 0) { L.stream = c->stream; *out = &L; return JJ_OK; }
  if (!L.owned) {
    // launch stream + two copy streams + this lane: from the second lane on the context has more streams than HIP's default of four hardware
    // queues.  Streams that share a queue serialise (1.7-2x slower pipelines); the library does not touch the environment, it says so once.
    if (k >= 2) {
      static std::atomic<bool> warned{false};
      const char* q = getenv("GPU_MAX_HW_QUEUES");
      if ((!q || atoi(q) < 8) && !warned.exchange(true)) fprintf(stderr, "libjubjub_hip: MSM jobs in flight use 5+ streams and fewer than 8 hardware queues are configured (HIP's GPU_MAX_HW_QUEUES): streams sharing a queue serialise (option msm_lanes=1 keeps the jobs on one stream)\n");
    }
    HIPCHK(c, hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking));
    HIPCHK(c, hipEventCreateWithFlags(&L.ready_ev, hipEventDisableTiming));
    L.owned = true;
  }
  HIPCHK(c, hipEventRecord(L.ready_ev, c->stream));
  HIPCHK(c, hipStreamWaitEvent(L.stream, L.ready_ev, 0));
  *out = &L;
  return JJ_OK;
}

// ---- asynchronous jobs: jj_msm_begin queues every pass of one MSM and the copy of its records into the job's own page-locked
// buffer, then returns; jj_msm_finish waits for that copy only and runs the host tail (window sums, Horner, one inversion),
// while the kernels of jobs begun meanwhile keep the device busy.  The context's workspaces are shared by all jobs: the stream
// orders them.
static int msm_job_get(jj_ctx* c, size_t nrec, jj_msm_job** out) {
  jj_msm_job* j = nullptr;
  if (!c->job_pool.empty()) { j = c->job_pool.back(); c->job_pool.pop_back(); }
  else {
    j = new jj_msm_job();
    j->c = c;
    if (hipEventCreateWithFlags(&j->ev, hipEventDisableTiming) != hipSuccess) { delete j; c->err = "hipEventCreate failed"; return JJ_ERR_HIP; }
  }
  const size_t want = std::max<size_t>(nrec, 1) * jjhost::REC_MAX_BYTES + MSM_JOB_TAIL_BYTES;
  if (j->cap < want) {
    if (j->host) (void)hipHostFree(j->host);
    j->host = nullptr; j->cap = 0;
    if (hipHostMalloc((void**)&j->host, want, hipHostMallocCoherent | hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); if (j->gdev) (void)hipFree(j->gdev); (void)hipEventDestroy(j->ev); delete j; c->err = "hipHostMalloc failed"; return JJ_ERR_NOMEM; }
    j->cap = want;
  }
  j->nrec = 0; j->gathered = 0; j->folded = false; j->sig = false;
  for (size_t r = 0; r < std::max<size_t>(nrec, 1); r++) memset(j->host + r * jjhost::REC_MAX_BYTES, 0, jjhost::REC_HDR_BYTES);   // a stale header of a pooled buffer must never validate
  *out = j;
  return JJ_OK;
}
void msm_job_put(jj_ctx* c, jj_msm_job* j) {
  if (c->job_pool.size() < 8) { c->job_pool.push_back(j); return; }
  if (j->host) (void)hipHostFree(j->host);
  if (j->gdev) (void)hipFree(j->gdev);
  (void)hipEventDestroy(j->ev);
  delete j;
}
// spread: device-pointer jobs alternate over the context's lanes 1 .. msm_lanes (jj_msm_begin); otherwise lane 0 (jj_msm; host arrays are
// staged through buffers the launch stream owns; JJ_MSM_LANES=1: every job).  have: a job the caller took from the pool for these n terms
// (sig_job_open) instead of a fresh one; it is the callee's from here on, put back on failure like its own.
int msm_begin_locked(jj_ctx* c, size_t n, const void* scalars, const void* points, int part_w0, int part_stride, bool spread, jj_msm_job** out, jj_msm_job* have) {
  size_t PASS = (size_t)1 << c->msm_pass_log2;
  // Host arrays of 2^19 terms and more are reduced in SEVERAL passes (one record each, one host tail): the copy of a pass's slice runs on the
  // copy stream beside the kernels of the pass before it -- 96 bytes per term over the link cost more than the whole reduction (2^20 terms:
  // 1.7 ms of copy, 1.3 ms of kernels).  Two to eight passes of at least 2^19 terms (smaller passes reduce less efficiently than the copy
  // they hide): page-locked arrays 2^20 terms 3.15 -> 2.67 ms, 2^22 terms 12.3 -> 9.7 ms with two passes.  JJ_MSM_HOST_SPLIT=0: one pass
  // after the whole copy (round 3).
  const bool host_in = n && !is_device_ptr(scalars) && !is_device_ptr(points);
  const bool split = host_in && c->msm_host_split && n >= ((size_t)1 << 19);
  PASS = msm_host_pass_terms(n, c->msm_pass_log2, split);
  const size_t npass = n ? (n + PASS - 1) / PASS : 0;
  jj_msm_job* j = have;
  int rc = have ? JJ_OK : msm_job_get(c, npass, &j); if (rc) return rc;
  int k = 0;
  if (spread && n && c->msm_lanes > 1 && is_device_ptr(scalars) && is_device_ptr(points)) k = 1 + (int)(c->next_lane++ % (unsigned)c->msm_lanes);
  MsmLane* L = nullptr;
  if ((rc = msm_lane(c, k, &L))) { msm_job_put(c, j); return rc; }
  auto fail = [&](int code) { if (split && c->pipe.h2d) (void)hipStreamSynchronize(c->pipe.h2d); (void)hipStreamSynchronize(L->stream); (void)hipGetLastError(); msm_job_put(c, j); return code; };   // kernels may still be writing into the job's buffer
  if (n) {
    const void *ds, *dp;
    if (split) {
      // the passes' slices are copied on the copy stream (ordered after what the launch stream has queued: the staging buffers may still
      // be read by an earlier call's kernels), each pass's kernels wait for their slice only
      if ((rc = ensure(c, c->in[0], 32 * n)) || (rc = ensure(c, c->in[1], 64 * n)) || (rc = pipe_prepare(c, 0, 0))) return fail(rc);
      ds = c->in[0].p; dp = c->in[1].p;
      hipError_t e0 = hipEventRecord(c->order_ev, c->stream);
      if (e0 == hipSuccess) e0 = hipStreamWaitEvent(c->pipe.h2d, c->order_ev, 0);
      if (e0 != hipSuccess) { c->err = std::string("MSM staging failed: ") + hipGetErrorString(e0); return fail(JJ_ERR_HIP); }
    } else if ((rc = stage_in(c, 0, scalars, 32 * n, &ds)) || (rc = stage_in(c, 1, points, 64 * n, &dp))) return fail(rc);
    size_t stage_seq = 0;             // staging slots of the bounce path, counted over all arrays of all passes
    for (size_t lo = 0; lo < n; lo += PASS) {
      const size_t cnt = std::min(PASS, n - lo);
      size_t used = 0;
      if (split) {
        const struct { const void* host; void* dev; size_t elem; } arr[2] = {{scalars, c->in[0].p, 32}, {points, c->in[1].p, 64}};
        for (const auto& a : arr) {
          const uint8_t* src = (const uint8_t*)a.host + lo * a.elem; uint8_t* dst = (uint8_t*)a.dev + lo * a.elem;
          if (cnt * a.elem >= BOUNCE_THRESHOLD && !is_pinned_host(src, cnt * a.elem)) { if ((rc = host_to_dev_bounced(c, dst, src, cnt * a.elem, c->pipe.h2d, &stage_seq))) return fail(rc); }
          else if (hipMemcpyAsync(dst, src, cnt * a.elem, hipMemcpyHostToDevice, c->pipe.h2d) != hipSuccess) { c->err = "MSM staging copy failed"; return fail(JJ_ERR_HIP); }
        }
        const int ei = (int)((lo / PASS) & 1);
        if (hipEventRecord(c->pipe.ev_in[ei], c->pipe.h2d) != hipSuccess || hipStreamWaitEvent(L->stream, c->pipe.ev_in[ei], 0) != hipSuccess) { c->err = "MSM staging event failed"; return fail(JJ_ERR_HIP); }
      }
      // the kernels that finish a window write its point straight into the job's page-locked buffer (device-visible host memory):
      // no copy operation between the last kernel and the host tail
      if ((rc = msm_enqueue(c, *L, cnt, (const uint8_t*)ds + lo * 32, (const uint8_t*)dp + lo * 64, part_w0, part_stride, j->host + j->nrec * jjhost::REC_MAX_BYTES, &used))) return fail(rc);
      j->nrec++;
    }
    if (stage_seq && (rc = stage_in_drain(c, stage_seq))) return fail(rc);     // the staging slots are free for the next call
  }
  hipError_t e = hipEventRecord(j->ev, L->stream);
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) { c->err = std::string("MSM launch failed: ") + hipGetErrorString(e); return fail(JJ_ERR_HIP); }
  *out = j;
  return JJ_OK;
}
JJ_API int jj_msm_begin(jj_ctx* c, size_t n, const void* scalars, const void* points, jj_msm_job** job) {
  if (!c || !job) return JJ_ERR_INVALID;
  *job = nullptr;
  JJ_ENTER(c);
  return msm_begin_locked(c, n, scalars, points, 0, 1, true, job);
}
// ---- the three batch signature entry points (jj_sigbatch_begin, _keyed_begin, _ragged) share what follows: the table of their five input arrays, the layout of
// a workspace in 256-byte regions, the staging copy, and -- the two that return a job -- the job that owns the workspace.
struct SigInputs {
  struct { const void* p; size_t rows, elem; } a[5];                             // r32, a32, s32, c32, z16
  bool dev[5];
  size_t o_in[5];                                                                // where a staged array lies in the workspace
  const void* in[5];                                                             // what the kernels read: the caller's device array or its staged copy
};
struct SigLayout {
  size_t off = 0;
  size_t take(size_t bytes) { const size_t o = off; off += sig_up(bytes); return o; }
};
// dev[] of the table; device arrays are read with 16-byte loads
static int sig_inputs_check(jj_ctx* c, SigInputs& t) {
  for (int k = 0; k < 5; k++) {
    t.dev[k] = is_device_ptr(t.a[k].p);
    if (t.dev[k] && ((uintptr_t)t.a[k].p & 15u)) { c->err = "device pointers must be 16-byte aligned"; return JJ_ERR_INVALID; }
  }
  return JJ_OK;
}
// regions for arrays first .. 4 where they are host arrays (the arrays before `first` have a region of the caller's: o_in[] is set)
static void sig_inputs_place(SigInputs& t, SigLayout& lay, int first) {
  for (int k = first; k < 5; k++) t.o_in[k] = t.dev[k] ? 0 : lay.take(t.a[k].rows * t.a[k].elem);
}
static int sig_to_dev(jj_ctx* c, void* dst, const void* src, size_t bytes, bool src_dev, const char* who) {
  if (!bytes) return JJ_OK;
  if (!src_dev && bytes >= BOUNCE_THRESHOLD && !is_pinned_host(src, bytes)) return host_to_dev_bounced(c, dst, src, bytes);
  if (hipMemcpyAsync(dst, src, bytes, src_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream) != hipSuccess) { c->err = std::string(who) + ": staging copy failed"; return JJ_ERR_HIP; }
  return JJ_OK;
}
// in[] of the table: arrays before `first` are copied to their region wherever they lie, the others only from host memory
static int sig_inputs_stage(jj_ctx* c, SigInputs& t, uint8_t* g, int first, const char* who) {
  for (int k = 0; k < 5; k++) {
    if (k >= first && t.dev[k]) { t.in[k] = t.a[k].p; continue; }
    const int rc = sig_to_dev(c, g + t.o_in[k], t.a[k].p, t.a[k].rows * t.a[k].elem, t.dev[k], who);
    if (rc) return rc;
    t.in[k] = g + t.o_in[k];
  }
  return JJ_OK;
}
// The job of a batch of T terms, taken from the pool before anything is queued: its workspace *g (gdev, at least `bytes`) and its flag word in
// the page-locked buffer are known to the kernels that write to them.  msm_begin_locked takes the job over (sig_job_submit); until then a
// failure gives it back through sig_job_fail.
static int sig_job_open(jj_ctx* c, size_t T, size_t bytes, jj_msm_job** job, uint8_t** g, u32** flag) {
  const size_t PASS = msm_host_pass_terms(T, c->msm_pass_log2, false);           // device pointers: the record count msm_begin_locked computes
  jj_msm_job* j = nullptr;
  int rc = msm_job_get(c, (T + PASS - 1) / PASS, &j); if (rc) return rc;
  if (j->gdev_cap < bytes) {
    if (j->gdev) (void)hipFree(j->gdev);
    j->gdev = nullptr; j->gdev_cap = 0;
    if (hipMalloc(&j->gdev, bytes) != hipSuccess) { (void)hipGetLastError(); msm_job_put(c, j); c->err = "hipMalloc failed"; return JJ_ERR_NOMEM; }
    j->gdev_cap = bytes;
  }
  *g = (uint8_t*)j->gdev;
  *flag = (u32*)(j->host + j->cap - MSM_JOB_TAIL_BYTES);
  **flag = 2u;                                                                   // neither verdict: k_sig_close has not run
  *job = j;
  return JJ_OK;
}
// synchronise first -- kernels may still be writing into the job's buffers -- then the job (if the caller still owns it) goes back to the pool
static int sig_job_fail(jj_ctx* c, jj_msm_job* j, int code) {
  (void)hipStreamSynchronize(c->stream); (void)hipGetLastError();
  if (j) msm_job_put(c, j);
  return code;
}
// the sum of the T prepared terms, queued on a lane like any device-pointer job, as job j's
static int sig_job_submit(jj_ctx* c, size_t T, const void* scalars, const void* points, jj_msm_job* j, jj_msm_job** job) {
  const int rc = msm_begin_locked(c, T, scalars, points, 0, 1, true, job, j);
  if (rc) return sig_job_fail(c, nullptr, rc);                                   // msm_begin_locked has put the job back
  j->sig = true;
  return JJ_OK;
}
// ---- batch Schnorr verification as one MSM job (kernels: jj_sig_kernels.h).  The 2n + 1 terms are prepared on the context's stream in a
// workspace the JOB owns (gdev: points | scalars | ok bytes | partials | B | staged host inputs), then msm_begin_locked queues the sum on a lane
// like any device-pointer job; jj_msm_finish clears the cofactor and turns k_sig_close's flag into the (0, -1) sentinel.
JJ_API int jj_sigbatch_begin(jj_ctx* c, const void* base64, size_t n, const void* r32, const void* a32, const void* s32, const void* c32, const void* z16, unsigned flags, jj_msm_job** job) {
  if (job) *job = nullptr;
  if (!c || !job || !base64 || (flags & ~(unsigned)JJ_DECOMPRESS_ZIP216)) return JJ_ERR_INVALID;
  if (n && (!r32 || !a32 || !s32 || !c32 || !z16)) return JJ_ERR_INVALID;
  if (n > (((size_t)1 << 24) - 1) / 2) return JJ_ERR_INVALID;                    // 2n + 1 terms: one pass of the MSM
  JJ_ENTER(c);
  if (n == 0) return msm_begin_locked(c, 0, nullptr, nullptr, 0, 1, true, job);   // the empty sum: [8] O = O
  const char* const who = "jj_sigbatch_begin";
  const size_t T = 2 * n + 1;
  const u32 nblk = blocks_for(n, SIG_THREADS);
  SigInputs t = {{{r32, n, 32}, {a32, n, 32}, {s32, n, 32}, {c32, n, 32}, {z16, n, 16}}, {}, {}, {}};
  int rc = sig_inputs_check(c, t); if (rc) return rc;
  SigLayout lay;
  const size_t o_pts = lay.take(T * 64), o_scal = lay.take(T * 32), o_ok = lay.take(2 * n), o_part = lay.take((size_t)nblk * SIG_PART_WORDS * 4), o_base = lay.take(64);
  sig_inputs_place(t, lay, 0);
  jj_msm_job* j = nullptr; uint8_t* g = nullptr; u32* flag = nullptr;
  if ((rc = sig_job_open(c, T, lay.off, &j, &g, &flag))) return rc;
  if ((rc = sig_inputs_stage(c, t, g, 0, who)) || (rc = sig_to_dev(c, g + o_base, base64, 64, is_device_ptr(base64), who))) return sig_job_fail(c, j, rc);
  if ((rc = decompress_dev(c, n, t.in[0], flags, g + o_pts, g + o_ok, false))) return sig_job_fail(c, j, rc);
  if ((rc = decompress_dev(c, n, t.in[1], flags, g + o_pts + 64 * n, g + o_ok + n, false))) return sig_job_fail(c, j, rc);
  hipLaunchKernelGGL(k_sig_terms, dim3(nblk), dim3(SIG_THREADS), 0, c->stream, n, t.in[2], t.in[3], t.in[4], (const uint8_t*)(g + o_ok), (void*)(g + o_pts), (void*)(g + o_scal), (u32*)(g + o_part));
  hipLaunchKernelGGL(k_sig_close, dim3(1), dim3(SIG_CLOSE_THREADS), 0, c->stream, n, nblk, (const u32*)(g + o_part), (const u32*)(g + o_base), (void*)(g + o_pts), (void*)(g + o_scal), flag);
  return sig_job_submit(c, T, g + o_scal, g + o_pts, j, job);
}
// ---- the same check for signatures grouped by key (kernels: jj_sig_keyed_kernels.h): n + K + 1 terms, n + K decodes in ONE decoder launch over
// r32 | a32 copied into one region of the job's workspace (gdev: points | scalars | ok bytes | partials | B | run heads | encodings | offsets |
// staged host inputs).  k_sig_close is launched with n = 0 on pointers moved to term n + K: it adds the partials of both kernels before it.
// The offsets of a call, checked without a context or a device: CSR (csr_offsets_ok), n + K + 1 terms in one pass of the MSM.
static bool sig_keyed_offsets_ok(size_t K, const uint64_t* off, size_t* n) {
  const uint64_t MAXT = (uint64_t)1 << 24;
  *n = 0;
  if (K >= MAXT) return false;
  if (!off) return K == 0;
  if (!csr_offsets_ok(K, off) || off[K] > MAXT - 1 - K) return false;
  *n = (size_t)off[K];
  return true;
}
JJ_API int jj_sigbatch_keyed_begin(jj_ctx* c, const void* base64, size_t K, const void* a32, const uint64_t* offsets, const void* r32, const void* s32, const void* c32, const void* z16,
                                   unsigned flags, jj_msm_job** job) {
  if (job) *job = nullptr;
  if (!c || !job || !base64 || (flags & ~(unsigned)JJ_DECOMPRESS_ZIP216)) return JJ_ERR_INVALID;
  size_t n = 0;
  if (K >= ((size_t)1 << 24) || (K && !offsets) || (offsets && is_device_ptr(offsets)) || !sig_keyed_offsets_ok(K, offsets, &n)) return JJ_ERR_INVALID;
  if (n && (!a32 || !r32 || !s32 || !c32 || !z16)) return JJ_ERR_INVALID;
  JJ_ENTER(c);
  if (n == 0) return msm_begin_locked(c, 0, nullptr, nullptr, 0, 1, true, job);   // the empty sum: [8] O = O
  const char* const who = "jj_sigbatch_keyed_begin";
  const size_t T = n + K + 1;
  const u32 nblk = blocks_for(n, SIG_THREADS), kblk = blocks_for(K, SIG_THREADS);
  SigInputs t = {{{r32, n, 32}, {a32, K, 32}, {s32, n, 32}, {c32, n, 32}, {z16, n, 16}}, {}, {}, {}};
  int rc = sig_inputs_check(c, t); if (rc) return rc;
  SigLayout lay;
  const size_t o_pts = lay.take(T * 64), o_scal = lay.take(T * 32), o_ok = lay.take(n + K), o_part = lay.take((size_t)(nblk + kblk) * SIG_PART_WORDS * 4), o_base = lay.take(64);
  const size_t o_heads = lay.take(n * 32), o_enc = lay.take((n + K) * 32), o_offs = lay.take((K + 1) * 8);
  t.o_in[0] = o_enc; t.o_in[1] = o_enc + 32 * n;                                  // R and A always land in the decoder's one input region
  sig_inputs_place(t, lay, 2);
  jj_msm_job* j = nullptr; uint8_t* g = nullptr; u32* flag = nullptr;
  if ((rc = sig_job_open(c, T, lay.off, &j, &g, &flag))) return rc;
  if ((rc = sig_inputs_stage(c, t, g, 2, who)) || (rc = sig_to_dev(c, g + o_offs, offsets, (K + 1) * 8, false, who)) || (rc = sig_to_dev(c, g + o_base, base64, 64, is_device_ptr(base64), who)))
    return sig_job_fail(c, j, rc);
  if ((rc = decompress_dev(c, n + K, g + o_enc, flags, g + o_pts, g + o_ok, false))) return sig_job_fail(c, j, rc);
  const unsigned long long* doffs = (const unsigned long long*)(g + o_offs);
  u32* part = (u32*)(g + o_part);
  hipLaunchKernelGGL(k_sig_keyed_terms, dim3(nblk), dim3(SIG_THREADS), 0, c->stream, n, (u32)K, doffs, t.in[2], t.in[3], t.in[4], (const uint8_t*)(g + o_ok), (void*)(g + o_pts), (void*)(g + o_scal),
                     (void*)(g + o_heads), part);
  hipLaunchKernelGGL(k_sig_keyed_close, dim3(kblk), dim3(SIG_THREADS), 0, c->stream, n, (u32)K, doffs, (const uint8_t*)(g + o_ok), (const void*)(g + o_heads), (void*)(g + o_pts), (void*)(g + o_scal),
                     part + (size_t)nblk * SIG_PART_WORDS);
  hipLaunchKernelGGL(k_sig_close, dim3(1), dim3(SIG_CLOSE_THREADS), 0, c->stream, (size_t)0, nblk + kblk, (const u32*)part, (const u32*)(g + o_base), (void*)(g + o_pts + (n + K) * 64),
                     (void*)(g + o_scal + (n + K) * 32), flag);
  return sig_job_submit(c, T, g + o_scal, g + o_pts, j, job);
}
// waits for the job's records, host tail, result to out64 (host pointer: written before the call returns; device pointer: a
// 64-byte copy queued on the context's stream).  The job is released in every case.
JJ_API int jj_msm_finish(jj_msm_job* j, void* out64) {
  if (!j || !j->c) return JJ_ERR_INVALID;
  jj_ctx* c = j->c;
  if (!out64) { (void)hipEventSynchronize(j->ev); std::lock_guard<std::recursive_mutex> lk(c->mu); msm_job_put(c, j); return JJ_ERR_INVALID; }   // the job's kernels may still be writing into its buffer
  hipError_t e = hipEventSynchronize(j->ev);                       // no context lock while waiting: other threads may queue work
  jjhost::Ext total = jjhost::identity();
  if (e == hipSuccess && j->gathered && j->folded) {
    // a job of jj_msm_allgather_begin: the fold kernel left ONE record -- or a zero header: records of different window layouts (ranks
    // with different term counts), which the host adds after one copy of all of them out of the job's own device buffer
    uint32_t magic; memcpy(&magic, j->host, 4);
    if (magic != MSM_REC_MAGIC) {
      // (the context's device current, the copy on the context's own stream and a wait for THAT stream only: a blocking hipMemcpy runs on the
      // null stream, which synchronises with every blocking stream of the process -- e.g. a caller's stream that carries the next job's gather)
      std::lock_guard<std::recursive_mutex> lk(c->mu);
      e = hipSetDevice(c->device);
      if (e == hipSuccess) e = hipMemcpyAsync(j->host, (const uint8_t*)j->gdev + JJ_MSM_PARTIAL_BYTES, (size_t)j->gathered * JJ_MSM_PARTIAL_BYTES, hipMemcpyDeviceToHost, c->own_stream);
      if (e == hipSuccess) e = hipStreamSynchronize(c->own_stream);
      j->nrec = (size_t)j->gathered;
    }
  }
  bool ok = e == hipSuccess && jjhost::combine_records(j->host, j->nrec, jjhost::REC_MAX_BYTES, &total);
  // a job of jj_sigbatch_begin: [8] of the sum, or the order-2 point (0, -1) when k_sig_close flagged a malformed unit
  bool malformed = false;
  if (ok && j->sig) {
    uint32_t flag; memcpy(&flag, j->host + j->cap - MSM_JOB_TAIL_BYTES, 4);
    if (flag > 1u) ok = false;                                       // never written
    malformed = flag == 1u;
    for (int k = 0; k < 3; k++) total = jjhost::point_dbl(total);
  }
  auto write64 = [&](uint8_t* dst) {
    if (!malformed) { jjhost::to_affine64(dst, total); return; }
    memset(dst, 0, 32);
    uint64_t v[4] = {jjhost::QL[0] - 1, jjhost::QL[1], jjhost::QL[2], jjhost::QL[3]};
    memcpy(dst + 32, v, 32);
  };
  JJ_ENTER(c);
  int rc = JJ_OK;
  if (e != hipSuccess) { c->err = std::string("hipEventSynchronize failed: ") + hipGetErrorString(e); rc = JJ_ERR_HIP; }
  else if (!ok) { c->err = "MSM record is damaged (bad header)"; rc = JJ_ERR_HIP; }
  else if (is_device_ptr(out64)) {
    write64(c->host_out[c->host_out_next]);
    e = hipMemcpyAsync(out64, c->host_out[c->host_out_next], 64, hipMemcpyHostToDevice, c->stream);
    c->host_out_next = (c->host_out_next + 1) % 8;
    if (e != hipSuccess) { c->err = std::string("hipMemcpyAsync failed: ") + hipGetErrorString(e); rc = JJ_ERR_HIP; }
  } else write64((uint8_t*)out64);
  msm_job_put(c, j);
  return rc;
}
JJ_API int jj_msm(jj_ctx* c, size_t n, const void* scalars, const void* points, void* out64) {
  if (!c || !out64) return JJ_ERR_INVALID;
  jj_msm_job* j = nullptr;
  {
    JJ_ENTER(c);
    prof_mark(c, 0);
    const int rc = msm_begin_locked(c, n, scalars, points, 0, 1, false, &j);
    if (rc) return rc;
  }
  const int rc = jj_msm_finish(j, out64);
  { JJ_ENTER(c); prof_mark(c, 1); prof_mark(c, 2); }
  return rc;
}
// Opt-in device-side finish: the record stays on the device, one quad runs the Horner chain and the inversion there, the affine sum
// is written to DEVICE memory; nothing is copied to the host and no host thread waits (fully asynchronous on the context's stream).
JJ_API int jj_msm_dev(jj_ctx* c, size_t n, const void* scalars, const void* points, void* out64_dev) {
  if (!c || !out64_dev) return JJ_ERR_INVALID;
  JJ_ENTER(c);
  if (!is_device_ptr(out64_dev) || ((uintptr_t)out64_dev & 15u)) { c->err = "jj_msm_dev writes its result to (16-byte aligned) device memory; use jj_msm for a host result"; return JJ_ERR_INVALID; }
  if (n > ((size_t)1 << c->msm_pass_log2)) { c->err = "jj_msm_dev takes at most one pass of terms (2^24); use jj_msm, or add the sums of the parts with jj_point_add"; return JJ_ERR_INVALID; }
  if (n == 0) { HIPCHK(c, hipMemcpyAsync(out64_dev, AFFINE_IDENTITY_BYTES, 64, hipMemcpyHostToDevice, c->stream)); return JJ_OK; }
  int rc;
  const void *ds, *dp;
  if ((rc = stage_in(c, 0, scalars, 32 * n, &ds))) return rc;
  if ((rc = stage_in(c, 1, points, 64 * n, &dp))) return rc;
  MsmLane* L = nullptr;
  if ((rc = msm_lane(c, 0, &L))) return rc;
  if ((rc = ensure(c, L->rec, JJ_MSM_PARTIAL_BYTES))) return rc;
  size_t used = 0;
  if ((rc = msm_enqueue(c, *L, n, ds, dp, 0, 1, L->rec.p, &used))) return rc;
  hipLaunchKernelGGL(k_msm_finish_dev, dim3(1), dim3(64), 0, c->stream, (const u32*)L->rec.p, out64_dev);
  return finish(c, false);
}
// ---- B independent MSMs of n terms each (jj_msm_batch).  Up to MSM_BATCH_MAX terms per row the batched kernels take the whole
// batch (k_msm_batch_tables / _sum / _finish, jj_msm_kernels.h) on the context's stream; above it every row is an MSM job of its own
// (msm_begin_locked: device-pointer rows alternate over the context's MSM lanes), finished by the host tail before the call returns.
// MSM_BATCH_MAX: crossover with the jobs route, profiles/r7_msm_batch.txt.
constexpr size_t MSM_BATCH_MAX = 1 << 13;
// workspaces per round: the tables of distinct points cover at most MSM_BATCH_TABLE_TERMS terms (1296 B each: 340 MB), the rows beyond
// go through in further rounds; the window sums of at most MSM_BATCH_ROWS rows (9 KB each) wait for one finish launch
constexpr size_t MSM_BATCH_TABLE_TERMS = 1 << 18;
constexpr size_t MSM_BATCH_ROWS = 1 << 13;
// a row's terms are cut into slices (one wave each) until rows x slices reaches MSM_BATCH_WAVES waves (two per SIMD of 256 CUs),
// with at least MSM_BATCH_SLICE_MIN terms per slice
constexpr size_t MSM_BATCH_WAVES = 2048;
constexpr size_t MSM_BATCH_SLICE_MIN = 16;
static size_t msm_batch_slices(size_t rows, size_t n) {
  const size_t want = (MSM_BATCH_WAVES + rows - 1) / rows, most = std::max<size_t>(1, n / MSM_BATCH_SLICE_MIN);
  return std::max<size_t>(1, std::min(want, most));
}
// rows [0, B) of device arrays -> out (device), all on the context's stream.  Workspaces of lane 0 (ordered with jj_msm by the stream):
// buf[1] tables, buf[2] window sums, buf[3] slice partials, buf[4] per-row counters
// resident: the tables {0 .. 8} P of a basis (jj_msm_basis_*), shared by all rows: no table launch, no table workspace
static int msm_batch_enqueue(jj_ctx* c, size_t B, size_t n, const uint8_t* ds, const uint8_t* dp, bool shared, uint8_t* dout, const u32* resident = nullptr) {
  MsmLane& L = c->lanes[0];
  MsmParams mp;
  msm_layout(mp, SM_W, 0, 1);
  const size_t TAB = (size_t)SM_SLOTS * ENIELS_WORDS * 4, SUMS = (size_t)SM_W * MSM_BATCH_PT_WORDS * 4;
  const size_t round_rows = shared ? MSM_BATCH_ROWS : std::max<size_t>(1, std::min(MSM_BATCH_ROWS, MSM_BATCH_TABLE_TERMS / n));
  const size_t group = std::min(B, MSM_BATCH_ROWS);
  const size_t rows0 = std::min(B, round_rows), slices0 = msm_batch_slices(rows0, n);
  int rc;
  if ((!resident && (rc = ensure(c, L.buf[1], (shared ? n : rows0 * n) * TAB))) || (rc = ensure(c, L.buf[2], group * SUMS))) return rc;
  if (slices0 > 1 && ((rc = ensure(c, L.buf[3], rows0 * slices0 * SUMS)) || (rc = ensure(c, L.buf[4], rows0 * 4)))) return rc;
  u32* tables = resident ? const_cast<u32*>(resident) : (u32*)L.buf[1].p; u32* sums = (u32*)L.buf[2].p;
  if (shared && !resident) hipLaunchKernelGGL(k_msm_batch_tables, dim3(blocks_for(4 * n)), dim3(256), 0, c->stream, n, (const void*)dp, tables);
  for (size_t g0 = 0; g0 < B; g0 += group) {
    const size_t gn = std::min(group, B - g0);
    for (size_t r0 = g0; r0 < g0 + gn; r0 += round_rows) {
      const size_t rows = std::min(round_rows, g0 + gn - r0), slices = msm_batch_slices(rows, n);
      if (slices > 1 && ((rc = ensure(c, L.buf[3], rows * slices * SUMS)) || (rc = ensure(c, L.buf[4], rows * 4)))) return rc;
      if (!shared) hipLaunchKernelGGL(k_msm_batch_tables, dim3(blocks_for(4 * rows * n)), dim3(256), 0, c->stream, rows * n, (const void*)(dp + r0 * n * 64), tables);
      if (slices > 1) HIPCHK(c, hipMemsetAsync(L.buf[4].p, 0, rows * 4, c->stream));
      hipLaunchKernelGGL(k_msm_batch_sum, dim3((unsigned)(rows * slices)), dim3(64), 0, c->stream, n, (u32)slices, (const void*)(ds + r0 * n * 32), (const u32*)tables,
                         shared ? (size_t)0 : n, mp, (u32*)L.buf[3].p, (u32*)L.buf[4].p, sums + (r0 - g0) * (SUMS / 4));
    }
    hipLaunchKernelGGL(k_msm_batch_finish, dim3(blocks_for(gn, MSM_BATCH_FINISH_ROWS)), dim3(64), 0, c->stream, (u32)gn, mp, (const u32*)sums, (void*)(dout + g0 * 64));
  }
  return JJ_OK;
}
// rows above MSM_BATCH_MAX terms: one MSM job per row, a few in flight (the host tail of one beside the kernels of the next), results
// through a host array
static int msm_batch_jobs(jj_ctx* c, size_t B, size_t n, const uint8_t* scalars, const uint8_t* points, bool shared, void* out64) {
  std::vector<uint8_t> res(B * 64);
  std::vector<std::pair<jj_msm_job*, size_t>> q;         // jobs in flight, oldest first
  const size_t depth = 2 * (size_t)std::max(1, c->msm_lanes);
  int rc = JJ_OK;
  size_t head = 0;
  auto finish_one = [&]() { const auto& f = q[head++]; const int r = jj_msm_finish(f.first, res.data() + 64 * f.second); if (!rc) rc = r; };
  for (size_t b = 0; b < B && !rc; b++) {
    jj_msm_job* j = nullptr;
    const int r = msm_begin_locked(c, n, scalars + b * n * 32, shared ? points : points + b * n * 64, 0, 1, true, &j);
    if (r) { rc = r; break; }
    q.emplace_back(j, b);
    if (q.size() - head > depth) finish_one();
  }
  while (head < q.size()) finish_one();                   // every job is finished (and released), also after a failure
  if (rc) return rc;
  if (is_device_ptr(out64)) {
    HIPCHK(c, hipMemcpyAsync(out64, res.data(), B * 64, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  } else memcpy(out64, res.data(), B * 64);
  return JJ_OK;
}
JJ_API int jj_msm_batch(jj_ctx* c, size_t B, size_t n, const void* scalars, const void* points, int points_shared, void* out64) {
  if (!c || (points_shared != 0 && points_shared != 1)) return JJ_ERR_INVALID;
  if (B == 0) return JJ_OK;
  if (n && (B > SIZE_MAX / n || B * n > SIZE_MAX / 64)) return JJ_ERR_INVALID;
  if (!out64 || (n && (!scalars || !points))) return JJ_ERR_INVALID;
  if (B > SIZE_MAX / 64) return JJ_ERR_INVALID;
  JJ_ENTER(c);
  const bool shared = points_shared == 1;
  if (n == 0) {
    if (is_device_ptr(out64)) {
      HIPCHK(c, hipMemsetAsync(out64, 0, B * 64, c->stream));
      HIPCHK(c, hipMemset2DAsync((uint8_t*)out64 + 32, 64, 1, 1, B, c->stream));
      return finish(c, false);
    }
    for (size_t b = 0; b < B; b++) memcpy((uint8_t*)out64 + 64 * b, AFFINE_IDENTITY_BYTES, 64);
    return JJ_OK;
  }
  if (n > MSM_BATCH_MAX) return msm_batch_jobs(c, B, n, (const uint8_t*)scalars, (const uint8_t*)points, shared, out64);
  int rc; OutRef o;
  const void *ds, *dp;
  if ((rc = stage_in(c, 0, scalars, 32 * B * n, &ds))) return rc;
  if ((rc = stage_in(c, 1, points, 64 * (shared ? n : B * n), &dp))) return rc;
  if ((rc = stage_out(c, c->out[0], out64, 64 * B, &o))) return rc;
  if ((rc = msm_batch_enqueue(c, B, n, (const uint8_t*)ds, (const uint8_t*)dp, shared, (uint8_t*)o.dev))) return rc;
  bool sync = false;
  if ((rc = finish_out(c, o, &sync))) return rc;
  return finish(c, sync);
}
// ---- S independent MSMs of different lengths over consecutive runs of one term array (jj_msm_ragged).  Segments of up to MSM_BATCH_MAX
// terms, the short ones, run through k_msm_ragged_sum / _finish (jj_msm_kernels.h) from a work list the planner below writes; longer ones are
// MSM jobs as in msm_batch_jobs.  The planner is a pure function of the offsets (jj_plan_msm_ragged, jj_plan_msm_ragged_items):
//   slice length  t = max(slice_min, ceil(N_short / waves)), N_short = the terms of the short segments: about `waves` waves in all, none below
//                 slice_min terms unless its segment is shorter (the reasoning of MSM_BATCH_WAVES / MSM_BATCH_SLICE_MIN)
//   slices        a short segment of len terms: ceil(len / t) slices of floor(len / slices) or one more terms; an empty segment: none
//   rounds        whole short segments, consecutive in input order, as long as their terms stay within round_terms (one table of 1296 B per term);
//                 a segment above round_terms has a round of its own.  A round's terms are contiguous: a long segment closes the round before it
//                 (it belongs to none), so that k_msm_batch_tables runs over one range and builds no table the sums never read.
struct RaggedRound { uint64_t t0, t1; size_t item0, item1, seg0, seg1, parts; };      // terms | items | non-empty short segments (counted over the call) | parked partial sums
struct RaggedPlan { uint64_t t = 0; size_t short_segs = 0, long_segs = 0, items = 0; std::vector<RaggedRound> rounds; };
// emit(round, segment, position of the segment among the round's non-empty segments, first term, end term, slices, slice, part0)
template <class Emit>
static void msm_ragged_plan(size_t S, const uint64_t* off, uint64_t slice_min, uint64_t waves, uint64_t round_terms, RaggedPlan& P, Emit emit) {
  uint64_t n_short = 0;
  for (size_t s = 0; s < S; s++) { const uint64_t len = off[s + 1] - off[s]; if (len <= MSM_BATCH_MAX) n_short += len; }
  const uint64_t t = std::max<uint64_t>(std::max<uint64_t>(slice_min, 1), (n_short + waves - 1) / waves);
  P.t = t;
  bool open = false;
  for (size_t s = 0; s < S; s++) {
    const uint64_t lo = off[s], len = off[s + 1] - lo;
    if (len == 0) continue;
    if (len > MSM_BATCH_MAX) { P.long_segs++; open = false; continue; }
    if (!open || P.rounds.back().t1 - P.rounds.back().t0 + len > round_terms) { P.rounds.push_back(RaggedRound{lo, lo, P.items, P.items, P.short_segs, P.short_segs, 0}); open = true; }
    RaggedRound& r = P.rounds.back();
    const uint64_t k = (len + t - 1) / t, base = len / k, rem = len % k;
    uint64_t first = lo;
    for (uint64_t j = 0; j < k; j++) {
      const uint64_t end = first + base + (j < rem ? 1 : 0);
      emit(P.rounds.size() - 1, s, r.seg1 - r.seg0, first, end, k, j, r.parts);
      first = end;
    }
    if (k > 1) r.parts += (size_t)k;
    P.items += (size_t)k; r.item1 = P.items;
    P.short_segs++; r.seg1 = P.short_segs;
    r.t1 = lo + len;
  }
}
// offsets[0] = 0, non-decreasing, and S, N whose byte counts fit size_t
static bool msm_ragged_offsets_ok(size_t S, const uint64_t* off) {
  return S < SIZE_MAX / 64 && csr_offsets_ok(S, off) && off[S] <= SIZE_MAX / 64;
}
static bool msm_ragged_plan_args(size_t S, const uint64_t* off, int& slice_min, int& waves, uint64_t& round_terms) {
  if (slice_min < 0 || waves < 0 || (S && !off) || (S && !msm_ragged_offsets_ok(S, off))) return false;
  if (!slice_min) slice_min = (int)MSM_BATCH_SLICE_MIN;
  if (!waves) waves = (int)MSM_BATCH_WAVES;
  if (!round_terms) round_terms = MSM_BATCH_TABLE_TERMS;
  return true;
}
JJ_API int jj_plan_msm_ragged(size_t S, const uint64_t* offsets, int slice_min, int waves, uint64_t round_terms, int64_t out[4]) {
  if (!out || !msm_ragged_plan_args(S, offsets, slice_min, waves, round_terms)) return JJ_ERR_INVALID;
  RaggedPlan P;
  msm_ragged_plan(S, offsets, (uint64_t)slice_min, (uint64_t)waves, round_terms, P, [](size_t, size_t, size_t, uint64_t, uint64_t, uint64_t, uint64_t, size_t) {});
  out[0] = (int64_t)P.short_segs; out[1] = (int64_t)P.long_segs; out[2] = (int64_t)P.items; out[3] = (int64_t)P.rounds.size();
  return JJ_OK;
}
JJ_API int jj_plan_msm_ragged_items(size_t S, const uint64_t* offsets, int slice_min, int waves, uint64_t round_terms, uint64_t* items, size_t cap, size_t* count) {
  if (!count || (cap && !items) || !msm_ragged_plan_args(S, offsets, slice_min, waves, round_terms)) return JJ_ERR_INVALID;
  RaggedPlan P;
  msm_ragged_plan(S, offsets, (uint64_t)slice_min, (uint64_t)waves, round_terms, P, [](size_t, size_t, size_t, uint64_t, uint64_t, uint64_t, uint64_t, size_t) {});
  *count = P.items;
  if (P.items > cap) return items ? JJ_ERR_INVALID : JJ_OK;          // cap = 0: the count only
  size_t k = 0;
  RaggedPlan Q;
  msm_ragged_plan(S, offsets, (uint64_t)slice_min, (uint64_t)waves, round_terms, Q, [&](size_t round, size_t s, size_t, uint64_t first, uint64_t end, uint64_t, uint64_t, size_t) {
    uint64_t* it = items + 4 * k++;
    it[0] = round; it[1] = s; it[2] = first; it[3] = end;
  });
  return JJ_OK;
}
// the short segments of a planned call: device arrays ds / dp (all N terms), results to their rows of dout; all on the context's stream.
// Workspaces of lane 0 as msm_batch_enqueue's (buf[1] tables, buf[2] window sums, buf[3] parked partial sums, buf[4] per-segment counters) and
// buf[6]: the work list (items, then the output row of every non-empty short segment).  The list is written into page-locked memory of the
// context and copied from there by the stream: the call may return before the copy runs, so the next call waits for ragged_ev before it
// writes the next list.
static int msm_ragged_enqueue(jj_ctx* c, size_t S, const uint64_t* off, const uint8_t* ds, const uint8_t* dp, uint8_t* dout) {
  MsmLane& L = c->lanes[0];
  MsmParams mp;
  msm_layout(mp, SM_W, 0, 1);
  const uint64_t slice_min = (uint64_t)c->msm_ragged_slice_min, waves = (uint64_t)c->msm_ragged_waves, round_terms = (uint64_t)c->msm_ragged_round_terms;
  RaggedPlan P;
  msm_ragged_plan(S, off, slice_min, waves, round_terms, P, [](size_t, size_t, size_t, uint64_t, uint64_t, uint64_t, uint64_t, size_t) {});
  if (!P.items) return JJ_OK;
  const size_t TAB = (size_t)SM_SLOTS * ENIELS_WORDS * 4, SUMS = (size_t)SM_W * MSM_BATCH_PT_WORDS * 4;
  const size_t map_off = P.items * sizeof(RaggedItem), list_bytes = map_off + P.short_segs * 8;
  size_t terms = 0, segs = 0, parts = 0;
  for (const RaggedRound& r : P.rounds) { terms = std::max<size_t>(terms, (size_t)(r.t1 - r.t0)); segs = std::max(segs, r.seg1 - r.seg0); parts = std::max(parts, r.parts); }
  int rc;
  if ((rc = ensure(c, L.buf[1], terms * TAB)) || (rc = ensure(c, L.buf[2], std::min(segs, MSM_BATCH_ROWS) * SUMS)) || (rc = ensure(c, L.buf[6], list_bytes))) return rc;
  if (parts && ((rc = ensure(c, L.buf[3], parts * SUMS)) || (rc = ensure(c, L.buf[4], segs * 4)))) return rc;
  if (!c->ragged_ev) HIPCHK(c, hipEventCreateWithFlags(&c->ragged_ev, hipEventDisableTiming));
  if (c->ragged_in_flight) { HIPCHK(c, hipEventSynchronize(c->ragged_ev)); c->ragged_in_flight = false; }     // the previous list has left the host buffer
  if (c->ragged_host_cap < list_bytes) {
    if (c->ragged_host) (void)hipHostFree(c->ragged_host);
    c->ragged_host = nullptr; c->ragged_host_cap = 0;
    const size_t want = std::max<size_t>(list_bytes + list_bytes / 2, 1 << 16);
    if (hipHostMalloc((void**)&c->ragged_host, want, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); c->ragged_host = nullptr; c->err = "hipHostMalloc(work list) failed"; return JJ_ERR_NOMEM; }
    c->ragged_host_cap = want;
  }
  RaggedItem* items = (RaggedItem*)c->ragged_host;
  uint64_t* rowmap = (uint64_t*)(c->ragged_host + map_off);
  std::vector<size_t> group_item;                       // first item of every finish group (MSM_BATCH_ROWS segments of a round), round after round
  {
    RaggedPlan Q;
    size_t k = 0;
    msm_ragged_plan(S, off, slice_min, waves, round_terms, Q, [&](size_t round, size_t s, size_t seg, uint64_t first, uint64_t end, uint64_t slices, uint64_t slice, size_t part0) {
      const uint64_t t0 = P.rounds[round].t0;
      if (slice == 0) { rowmap[P.rounds[round].seg0 + seg] = s; if (seg % MSM_BATCH_ROWS == 0) group_item.push_back(k); }
      items[k++] = RaggedItem{(u32)seg, (u32)(first - t0), (u32)(end - t0), (u32)slices, (u32)part0, (u32)slice, {0, 0}};
    });
  }
  HIPCHK(c, hipMemcpyAsync(L.buf[6].p, c->ragged_host, list_bytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipEventRecord(c->ragged_ev, c->stream));
  c->ragged_in_flight = true;
  const RaggedItem* ditems = (const RaggedItem*)L.buf[6].p;
  const unsigned long long* dmap = (const unsigned long long*)((const uint8_t*)L.buf[6].p + map_off);
  u32* tables = (u32*)L.buf[1].p; u32* sums = (u32*)L.buf[2].p;
  size_t g = 0;
  for (const RaggedRound& r : P.rounds) {
    const size_t rt = (size_t)(r.t1 - r.t0), rsegs = r.seg1 - r.seg0;
    hipLaunchKernelGGL(k_msm_batch_tables, dim3(blocks_for(4 * rt)), dim3(256), 0, c->stream, rt, (const void*)(dp + r.t0 * 64), tables);
    if (r.parts) HIPCHK(c, hipMemsetAsync(L.buf[4].p, 0, rsegs * 4, c->stream));
    for (size_t s0 = 0; s0 < rsegs; s0 += MSM_BATCH_ROWS, g++) {
      const size_t gn = std::min(MSM_BATCH_ROWS, rsegs - s0), i0 = group_item[g], i1 = s0 + gn < rsegs ? group_item[g + 1] : r.item1;
      hipLaunchKernelGGL(k_msm_ragged_sum, dim3((unsigned)(i1 - i0)), dim3(64), 0, c->stream, ditems + i0, (u32)s0, (const void*)(ds + r.t0 * 32), (const u32*)tables, mp,
                         (u32*)L.buf[3].p, (u32*)L.buf[4].p, sums);
      hipLaunchKernelGGL(k_msm_ragged_finish, dim3(blocks_for(gn, MSM_BATCH_FINISH_ROWS)), dim3(64), 0, c->stream, (u32)gn, mp, (const u32*)sums, dmap + r.seg0 + s0, (void*)dout);
    }
  }
  return JJ_OK;
}
// the sums of a call on device arrays ds / dp (all N terms), after staging: the identity to the rows of empty segments, the short segments through
// msm_ragged_enqueue, then the long ones as MSM jobs over the same arrays, a few in flight (the host tail of one beside the kernels of the next).
// The jobs' results come back in res (64 bytes per entry of longs): the caller puts them in place, behind everything queued here.
static int msm_ragged_locked(jj_ctx* c, size_t S, const uint64_t* offsets, const uint8_t* ds, const uint8_t* dp, uint8_t* dout, std::vector<size_t>& longs, std::vector<uint8_t>& res) {
  size_t empty = 0;
  longs.clear();                                        // the segments of the jobs route
  for (size_t s = 0; s < S; s++) { const uint64_t len = offsets[s + 1] - offsets[s]; if (!len) empty++; else if (len > MSM_BATCH_MAX) longs.push_back(s); }
  int rc;
  if (empty) {
    // the identity (0, 1) in every row; the finish launches and the jobs then write the rows of the non-empty segments
    HIPCHK(c, hipMemsetAsync(dout, 0, S * 64, c->stream));
    HIPCHK(c, hipMemset2DAsync(dout + 32, 64, 1, 1, S, c->stream));
  }
  if ((rc = msm_ragged_enqueue(c, S, offsets, ds, dp, dout))) return rc;
  res.assign(longs.size() * 64, 0);
  if (!longs.empty()) {
    const size_t depth = 2 * (size_t)std::max(1, c->msm_lanes);
    std::vector<std::pair<jj_msm_job*, size_t>> q;
    size_t head = 0;
    auto finish_one = [&]() { const auto& f = q[head++]; const int r = jj_msm_finish(f.first, res.data() + 64 * f.second); if (!rc) rc = r; };
    for (size_t k = 0; k < longs.size() && !rc; k++) {
      const uint64_t lo = offsets[longs[k]], len = offsets[longs[k] + 1] - lo;
      jj_msm_job* j = nullptr;
      const int r = msm_begin_locked(c, (size_t)len, ds + lo * 32, dp + lo * 64, 0, 1, true, &j);
      if (r) { rc = r; break; }
      q.emplace_back(j, k);
      if (q.size() - head > depth) finish_one();
    }
    while (head < q.size()) finish_one();                 // every job is finished (and released), also after a failure
  }
  return rc;
}
JJ_API int jj_msm_ragged(jj_ctx* c, size_t S, const uint64_t* offsets, const void* scalars, const void* points, void* out64) {
  if (!c) return JJ_ERR_INVALID;
  if (S == 0) return JJ_OK;
  if (!offsets || !out64 || is_device_ptr(offsets) || !msm_ragged_offsets_ok(S, offsets)) return JJ_ERR_INVALID;
  const size_t N = (size_t)offsets[S];
  if (N && (!scalars || !points)) return JJ_ERR_INVALID;
  JJ_ENTER(c);
  int rc; OutRef o;
  const void *ds = nullptr, *dp = nullptr;
  if ((rc = stage_in(c, 0, scalars, 32 * N, &ds))) return rc;
  if ((rc = stage_in(c, 1, points, 64 * N, &dp))) return rc;
  if ((rc = stage_out(c, c->out[0], out64, 64 * S, &o))) return rc;
  std::vector<size_t> longs;
  std::vector<uint8_t> res;
  if ((rc = msm_ragged_locked(c, S, offsets, (const uint8_t*)ds, (const uint8_t*)dp, (uint8_t*)o.dev, longs, res))) return rc;
  if (!o.host) for (size_t k = 0; k < longs.size(); k++) HIPCHK(c, hipMemcpyAsync((uint8_t*)o.dev + longs[k] * 64, res.data() + 64 * k, 64, hipMemcpyHostToDevice, c->stream));
  bool sync = !longs.empty();
  if ((rc = finish_out(c, o, &sync))) return rc;
  if ((rc = finish(c, sync))) return rc;
  if (o.host) for (size_t k = 0; k < longs.size(); k++) memcpy((uint8_t*)out64 + longs[k] * 64, res.data() + 64 * k, 64);
  return JJ_OK;
}
// ---- S batch Schnorr checks over consecutive runs of one signature array, one verdict point per run (jj_sigbatch_ragged; kernels:
// jj_sig_seg_kernels.h).  Segment g owns the terms 2 offsets[g] + g .. 2 offsets[g + 1] + g of ONE term array: its R terms, its A terms, its own
// term of B; msm_ragged_locked sums every segment (an empty one is the single term [0] B).  The decoder runs ONCE over r32 | a32 with the cofactor
// flag and [8] B comes from the cofactor operation (jj_point_mul_by_cofactor on one point), so every sum is the verdict point itself: neither
// k_msm_ragged_finish nor jj_msm_finish doubles anything.  The sums land in device memory (the caller's rows, or c->sigseg_out for a host result),
// the long segments' rows are copied there, k_sig_seg_verdict then writes (0, -1) over the rows of segments with a malformed unit, and a host
// result is copied out last.  Workspace c->sigseg: points | scalars | decoded points | ok bytes | head slots | encodings | offsets | bad | B, [8] B |
// staged host inputs; everything on the context's launch stream (the long segments' jobs are finished before the call returns).
static bool sig_seg_offsets_ok(size_t S, const uint64_t* off, size_t* n) {
  const uint64_t MAXT = (uint64_t)1 << 24;
  *n = 0;
  if (S > MAXT || !csr_offsets_ok(S, off) || off[S] > (MAXT - S) / 2) return false;      // 2n + S terms: one pass of the MSM for every segment, 32-bit term indices
  *n = (size_t)off[S];
  return true;
}
JJ_API int jj_sigbatch_ragged(jj_ctx* c, const void* base64, size_t S, const uint64_t* offsets, const void* r32, const void* a32, const void* s32, const void* c32, const void* z16,
                              unsigned flags, void* out64) {
  if (!c || !base64 || (flags & ~(unsigned)JJ_DECOMPRESS_ZIP216)) return JJ_ERR_INVALID;
  if (S == 0) return JJ_OK;
  size_t n = 0;
  if (!offsets || !out64 || is_device_ptr(offsets) || !sig_seg_offsets_ok(S, offsets, &n)) return JJ_ERR_INVALID;
  if (n && (!r32 || !a32 || !s32 || !c32 || !z16)) return JJ_ERR_INVALID;
  JJ_ENTER(c);
  const bool out_dev = is_device_ptr(out64);
  if ((out_dev && ((uintptr_t)out64 & 15u)) || (is_device_ptr(base64) && ((uintptr_t)base64 & 15u))) { c->err = "device pointers must be 16-byte aligned"; return JJ_ERR_INVALID; }
  if (n == 0) {                                                                // S identities; no array is read
    if (out_dev) {
      HIPCHK(c, hipMemsetAsync(out64, 0, S * 64, c->stream));
      HIPCHK(c, hipMemset2DAsync((uint8_t*)out64 + 32, 64, 1, 1, S, c->stream));
      return finish(c, false);
    }
    for (size_t g = 0; g < S; g++) memcpy((uint8_t*)out64 + 64 * g, AFFINE_IDENTITY_BYTES, 64);
    return JJ_OK;
  }
  const char* const who = "jj_sigbatch_ragged";
  const size_t T = 2 * n + S;
  SigInputs t = {{{r32, n, 32}, {a32, n, 32}, {s32, n, 32}, {c32, n, 32}, {z16, n, 16}}, {}, {}, {}};
  int rc = sig_inputs_check(c, t); if (rc) return rc;
  SigLayout lay;
  const size_t o_pts = lay.take(T * 64), o_scal = lay.take(T * 32), o_dec = lay.take(2 * n * 64), o_ok = lay.take(2 * n), o_heads = lay.take(n * 32), o_enc = lay.take(2 * n * 32);
  const size_t o_offs = lay.take((S + 1) * 8), o_bad = lay.take(S * 4), o_base = lay.take(64), o_b8 = lay.take(64);
  t.o_in[0] = o_enc; t.o_in[1] = o_enc + 32 * n;                                // R and A always land in the decoder's one input region
  sig_inputs_place(t, lay, 2);
  OutRef o;
  if ((rc = ensure(c, c->sigseg, lay.off)) || (rc = stage_out(c, c->sigseg_out, out64, 64 * S, &o))) return rc;
  uint8_t* g = (uint8_t*)c->sigseg.p;
  if ((rc = sig_inputs_stage(c, t, g, 2, who)) || (rc = sig_to_dev(c, g + o_offs, offsets, (S + 1) * 8, false, who)) || (rc = sig_to_dev(c, g + o_base, base64, 64, is_device_ptr(base64), who))) return rc;
  HIPCHK(c, hipMemsetAsync(g + o_bad, 0, S * 4, c->stream));
  if ((rc = jj_point_mul_by_cofactor(c, 1, g + o_base, g + o_b8))) return rc;
  if ((rc = decompress_dev(c, 2 * n, g + o_enc, flags | JJ_DECOMPRESS_CLEAR_COFACTOR, g + o_dec, g + o_ok, false))) return rc;
  const unsigned long long* doffs = (const unsigned long long*)(g + o_offs);
  hipLaunchKernelGGL(k_sig_seg_terms, dim3(blocks_for(n, SIG_THREADS)), dim3(SIG_THREADS), 0, c->stream, n, (u32)S, doffs, t.in[2], t.in[3], t.in[4], (const uint8_t*)(g + o_ok), (const void*)(g + o_dec),
                     (void*)(g + o_pts), (void*)(g + o_scal), (void*)(g + o_heads), (u32*)(g + o_bad));
  hipLaunchKernelGGL(k_sig_seg_close, dim3(blocks_for(S, SIG_THREADS)), dim3(SIG_THREADS), 0, c->stream, (u32)S, doffs, (const void*)(g + o_heads), (const void*)(g + o_b8), (void*)(g + o_pts),
                     (void*)(g + o_scal));
  std::vector<uint64_t> toff(S + 1);                                           // the term offsets of the S sums
  for (size_t k = 0; k <= S; k++) toff[k] = 2 * offsets[k] + k;
  std::vector<size_t> longs;
  std::vector<uint8_t> res;
  if ((rc = msm_ragged_locked(c, S, toff.data(), g + o_scal, g + o_pts, (uint8_t*)o.dev, longs, res))) return rc;
  for (size_t k = 0; k < longs.size(); k++) HIPCHK(c, hipMemcpyAsync((uint8_t*)o.dev + longs[k] * 64, res.data() + 64 * k, 64, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_sig_seg_verdict, dim3(blocks_for(S, SIG_THREADS)), dim3(SIG_THREADS), 0, c->stream, (u32)S, (const u32*)(g + o_bad), o.dev);
  bool sync = !longs.empty();                                                  // res leaves with this call
  if ((rc = finish_out(c, o, &sync))) return rc;
  return finish(c, sync);
}
// ---- fixed-basis MSM (jj_msm_basis_*): the points are handed over once, every call brings scalars only.  A basis keeps, in the memory of its
// device, the tables {0 .. 8} P of its first min(n, MSM_BATCH_MAX) points (rows of up to MSM_BATCH_MAX terms run through k_msm_batch_sum /
// _finish over them, whatever B is) and, when it has more points than that, the gathered-Niels records of all of them: one per point (mode 1:
// jj_msm's plan without the copy and the conversion of the points) or one per point and window of its layout (mode 2: the window table of
// jj_msm_kernels.h -- one bucket set, a record of one point, no Horner chain).  A prefix of m points takes the route m itself falls on.
constexpr size_t MSM_BASIS_MAX = (size_t)1 << 24;            // points per basis: one Pippenger pass (and rows w * n + i below 2^31 for every layout)
constexpr size_t MSM_BASIS_CHUNK = (size_t)1 << 16;          // points per launch of the table build (its workspace: 144 + 64 = 208 bytes per point and window)
// auto never takes the window table: with jj_msm's window counts mode 2 was measured SLOWER than mode 1 at every size (profiles/msm_basis_ab.txt,
// device-resident scalars: 2^14 terms 0.197 against 0.187 ms, 2^17 0.364 against 0.332 ms, 2^20 1.197 against 1.120 ms, spreads 0.001-0.005 ms: the
// W-times larger gather costs more than the W - 1 bucket reduces and the Horner chain it removes).  Mode 2 stays an explicit opt-in (its
// `windows` argument is there to look for a layout that wins); a table that would not fit half of the free memory is never auto's choice anyway.
constexpr bool MSM_BASIS_AUTO_WINDOWS = false;
struct jj_msm_basis {
  int device = -1;
  size_t n = 0, small_n = 0, bytes = 0;
  int mode = 1, windows = SM_W, windows_arg = 0;
  u32* small = nullptr;         // small_n tables of SM_SLOTS extended-Niels entries
  u32* niels = nullptr;         // n > MSM_BATCH_MAX: n (mode 1) or windows x n (mode 2) records of GNIELS_WORDS words
};
static int msm_basis_plan(size_t n, int mode, int windows, uint64_t budget, int64_t out[4]) {
  if (mode < 0 || mode > 2 || (windows != 0 && (windows < MSM_WINDOWS_MIN || windows > MSM_WINDOWS_MAX)) || n > MSM_BASIS_MAX) return JJ_ERR_INVALID;
  const bool pip = n > MSM_BATCH_MAX;
  const int W = pip ? (windows ? windows : msm_windows_default(n)) : SM_W;
  const uint64_t small_bytes = (uint64_t)std::min(n, MSM_BATCH_MAX) * SM_SLOTS * ENIELS_WORDS * 4, row = (uint64_t)GNIELS_WORDS * 4;
  const uint64_t b1 = small_bytes + (pip ? n * row : 0), b2 = small_bytes + (pip ? n * row * (uint64_t)W : 0);
  int m = mode;
  if (m == 0) m = MSM_BASIS_AUTO_WINDOWS && pip && b2 <= budget ? 2 : 1;
  out[0] = m; out[1] = W; out[2] = (int64_t)(m == 2 ? b2 : b1); out[3] = pip ? 1 : 0;
  return JJ_OK;
}
JJ_API int jj_plan_msm_basis(size_t n, int mode, int windows, uint64_t budget_bytes, int64_t out[4]) {
  if (!out) return JJ_ERR_INVALID;
  return msm_basis_plan(n, mode, windows, budget_bytes, out);
}
static void msm_basis_free(jj_msm_basis* b) {
  if (b->small) (void)hipFree(b->small);
  if (b->niels) (void)hipFree(b->niels);
  delete b;
}
JJ_API int jj_msm_basis_create(jj_ctx* c, size_t n, const void* points, int mode, int windows, jj_msm_basis** out) {
  if (!c || !out) return JJ_ERR_INVALID;
  *out = nullptr;
  int64_t plan[4];
  if ((n && !points) || msm_basis_plan(n, mode, windows, 0, plan)) return JJ_ERR_INVALID;
  JJ_ENTER(c);
  size_t free_b = 0, total_b = 0;
  HIPCHK(c, hipMemGetInfo(&free_b, &total_b));
  (void)msm_basis_plan(n, mode, windows, (uint64_t)free_b / 2, plan);
  jj_msm_basis* b = new jj_msm_basis();
  b->device = c->device; b->n = n; b->small_n = std::min(n, MSM_BATCH_MAX);
  b->mode = (int)plan[0]; b->windows = (int)plan[1]; b->windows_arg = windows; b->bytes = (size_t)plan[2];
  const bool pip = plan[3] != 0;
  const size_t small_bytes = b->small_n * (size_t)(SM_SLOTS * ENIELS_WORDS) * 4, niels_bytes = b->bytes - small_bytes;
  void *tmp = nullptr, *aff = nullptr;
  auto fail = [&](int code, const char* what) { (void)hipStreamSynchronize(c->stream); (void)hipGetLastError(); if (tmp) (void)hipFree(tmp); if (aff) (void)hipFree(aff); msm_basis_free(b); c->err = what; return code; };
  if (n == 0) { *out = b; return JJ_OK; }
  if (hipMalloc((void**)&b->small, small_bytes) != hipSuccess || (pip && hipMalloc((void**)&b->niels, niels_bytes) != hipSuccess)) return fail(JJ_ERR_NOMEM, "jj_msm_basis_create: out of device memory for the tables");
  int rc;
  const void* dp;
  if ((rc = stage_in(c, 1, points, 64 * n, &dp))) { const std::string keep = c->err; (void)fail(rc, ""); c->err = keep; return rc; }
  hipLaunchKernelGGL(k_msm_batch_tables, dim3(blocks_for(4 * b->small_n)), dim3(256), 0, c->stream, b->small_n, dp, b->small);
  if (pip) {
    MsmParams mp;
    msm_layout(mp, b->windows, 0, 1);
    if (b->mode == 1) hipLaunchKernelGGL(k_msm_convert, dim3(blocks_for(n)), dim3(256), 0, c->stream, n, (const void*)nullptr, dp, mp, (u32*)nullptr, b->niels, 2);
    else {
      const size_t W = (size_t)b->windows, ch = std::min(n, MSM_BASIS_CHUNK);
      if (hipMalloc(&tmp, ch * W * 4 * NL * 4) != hipSuccess || hipMalloc(&aff, ch * W * 64) != hipSuccess) return fail(JJ_ERR_NOMEM, "jj_msm_basis_create: out of device memory for the table build");
      for (size_t lo = 0; lo < n; lo += ch) {
        const size_t cn = std::min(ch, n - lo);
        SoA park; park.base = (u32*)tmp; park.n = cn;
        hipLaunchKernelGGL(k_msm_basis_chain, dim3(blocks_for(cn)), dim3(256), 0, c->stream, cn, (const void*)((const uint8_t*)dp + lo * 64), mp, park, aff);
        for (size_t w = 0; w < W; w++)
          hipLaunchKernelGGL(k_msm_convert, dim3(blocks_for(cn)), dim3(256), 0, c->stream, cn, (const void*)nullptr, (const void*)((const uint8_t*)aff + w * cn * 64), mp, (u32*)nullptr,
                             b->niels + (w * n + lo) * (size_t)GNIELS_WORDS, 2);
      }
    }
  }
  // the caller's array (and the build's workspace) are free when the call returns
  hipError_t e = hipStreamSynchronize(c->stream);
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) return fail(JJ_ERR_HIP, "jj_msm_basis_create: the table build failed");
  if (tmp) (void)hipFree(tmp);
  if (aff) (void)hipFree(aff);
  *out = b;
  return JJ_OK;
}
JJ_API int jj_msm_basis_destroy(jj_ctx* c, jj_msm_basis* b) {
  if (!c) return JJ_ERR_INVALID;
  if (!b) return JJ_OK;
  JJ_ENTER(c);
  if (b->device != c->device) { c->err = "this MSM basis lives on another device"; return JJ_ERR_INVALID; }
  msm_basis_free(b);
  return JJ_OK;
}
JJ_API int jj_msm_basis_info(const jj_msm_basis* b, int64_t out[4]) {
  if (!b || !out) return JJ_ERR_INVALID;
  out[0] = (int64_t)b->n; out[1] = b->mode; out[2] = b->windows; out[3] = (int64_t)b->bytes;
  return JJ_OK;
}
// one row over the basis's records (more than MSM_BATCH_MAX terms) or tables (a single short row): a job like jj_msm_begin's, finished by jj_msm_finish
static int msm_basis_begin(jj_ctx* c, const jj_msm_basis* b, size_t m, const void* ds, bool spread, jj_msm_job** out) {
  jj_msm_job* j;
  int rc = msm_job_get(c, 1, &j); if (rc) return rc;
  int k = 0;
  if (spread && c->msm_lanes > 1) k = 1 + (int)(c->next_lane++ % (unsigned)c->msm_lanes);
  MsmLane* L = nullptr;
  if ((rc = msm_lane(c, k, &L))) { msm_job_put(c, j); return rc; }
  const MsmTab tab{b->niels, b->mode == 2 ? b->n : (size_t)0, b->mode == 2 ? b->windows : b->windows_arg};
  hipError_t e = hipSuccess;
  if (m <= MSM_BATCH_MAX) {
    // jj_msm's small-batch pass (msm_enqueue_small) without its table half
    MsmParams mp;
    msm_layout(mp, SM_W, 0, 1);
    if (!(rc = ensure(c, L->buf[0], m * 32)) && !(rc = msm_ensure_ctl(c, *L))) {
      u32* counters = (u32*)L->ctl.p; u32* part = (u32*)((uint8_t*)L->ctl.p + MSM_PART_OFF);
      const u32 nblk = (u32)std::min<size_t>(c->msm_small_blk, std::max<size_t>(1, (m + 255) / 256));
      hipLaunchKernelGGL(k_msm_small_recode, dim3(blocks_for(m)), dim3(256), 0, L->stream, m, ds, mp, (u32*)L->buf[0].p, counters);
      hipLaunchKernelGGL(k_msm_small_sum, dim3(nblk, mp.Ws), dim3(4 * MSM_TREE_QUADS), 0, L->stream, m, mp, nblk, (const u32*)b->small, (const u32*)L->buf[0].p, part, counters, (u32*)j->host);
    }
  } else rc = msm_enqueue_pippenger(c, *L, m, ds, nullptr, 0, 1, j->host, &tab);
  if (!rc) {
    j->nrec = 1;
    e = hipEventRecord(j->ev, L->stream);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) { c->err = std::string("MSM launch failed: ") + hipGetErrorString(e); rc = JJ_ERR_HIP; }
  }
  if (rc) { (void)hipStreamSynchronize(L->stream); (void)hipGetLastError(); msm_job_put(c, j); return rc; }
  *out = j;
  return JJ_OK;
}
JJ_API int jj_msm_basis_mul(jj_ctx* c, const jj_msm_basis* b, size_t B, size_t m, const void* scalars, void* out64) {
  if (!c || !b) return JJ_ERR_INVALID;
  if (B == 0) return JJ_OK;
  if (B > SIZE_MAX / 64 || (m && (B > SIZE_MAX / m || B * m > SIZE_MAX / 32))) return JJ_ERR_INVALID;
  if (!out64 || (m && !scalars) || m > b->n) return JJ_ERR_INVALID;
  if (B == 1 && m) {
    // one row: a job, queued under the context's lock and finished without it (as jj_msm: other threads may queue work while this one waits)
    jj_msm_job* j = nullptr;
    {
      JJ_ENTER(c);
      if (b->device != c->device) { c->err = "this MSM basis lives on another device"; return JJ_ERR_INVALID; }
      const void* ds1;
      int rc1;
      if ((rc1 = stage_in(c, 0, scalars, 32 * m, &ds1)) || (rc1 = msm_basis_begin(c, b, m, ds1, false, &j))) return rc1;
    }
    return jj_msm_finish(j, out64);
  }
  JJ_ENTER(c);
  if (b->device != c->device) { c->err = "this MSM basis lives on another device"; return JJ_ERR_INVALID; }
  if (m == 0) {
    if (is_device_ptr(out64)) {
      HIPCHK(c, hipMemsetAsync(out64, 0, B * 64, c->stream));
      HIPCHK(c, hipMemset2DAsync((uint8_t*)out64 + 32, 64, 1, 1, B, c->stream));
      return finish(c, false);
    }
    for (size_t r = 0; r < B; r++) memcpy((uint8_t*)out64 + 64 * r, AFFINE_IDENTITY_BYTES, 64);
    return JJ_OK;
  }
  int rc;
  const void* ds;
  if ((rc = stage_in(c, 0, scalars, 32 * B * m, &ds))) return rc;
  if (m <= MSM_BATCH_MAX) {
    OutRef o;
    if ((rc = stage_out(c, c->out[0], out64, 64 * B, &o))) return rc;
    if ((rc = msm_batch_enqueue(c, B, m, (const uint8_t*)ds, nullptr, true, (uint8_t*)o.dev, b->small))) return rc;
    bool sync = false;
    if ((rc = finish_out(c, o, &sync))) return rc;
    return finish(c, sync);
  }
  // several long rows: one job per row, a few in flight over the context's lanes (as msm_batch_jobs)
  std::vector<uint8_t> res(B * 64);
  std::vector<jj_msm_job*> q;
  const size_t depth = 2 * (size_t)std::max(1, c->msm_lanes);
  size_t head = 0;
  rc = JJ_OK;
  auto finish_one = [&]() { const int r = jj_msm_finish(q[head], res.data() + 64 * head); head++; if (!rc) rc = r; };
  for (size_t r = 0; r < B && !rc; r++) {
    jj_msm_job* j = nullptr;
    const int r1 = msm_basis_begin(c, b, m, (const uint8_t*)ds + r * m * 32, true, &j);
    if (r1) { rc = r1; break; }
    q.push_back(j);
    if (q.size() - head > depth) finish_one();
  }
  while (head < q.size()) finish_one();
  if (rc) return rc;
  if (is_device_ptr(out64)) {
    HIPCHK(c, hipMemcpyAsync(out64, res.data(), B * 64, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  } else memcpy(out64, res.data(), B * 64);
  return JJ_OK;
}
// First half of an MSM that is cut across devices or ranks: the record of partial window sums, left where the
// caller wants it (device memory: ready for an all_gather over RCCL; host memory: the call waits for the copy).
//   part_index / part_count = 0 / 1   all windows of the n terms given (term partition: every rank passes its own terms)
//   part_index = g, part_count = G    windows g, g + G, ... of the n terms given (window partition: every rank passes ALL terms)
JJ_API int jj_msm_partial(jj_ctx* c, size_t n, const void* scalars, const void* points, int part_index, int part_count, void* record) {
  if (!c || !record || part_count < 1 || part_index < 0 || part_index >= part_count) return JJ_ERR_INVALID;
  JJ_ENTER(c);
  if (n > ((size_t)1 << c->msm_pass_log2)) { c->err = "jj_msm_partial takes at most one pass of terms (2^24); cut larger inputs"; return JJ_ERR_INVALID; }
  int rc; OutRef o;
  if ((rc = stage_out(c, c->out[0], record, JJ_MSM_PARTIAL_BYTES, &o))) return rc;
  static_assert(JJ_MSM_PARTIAL_BYTES == jjhost::REC_MAX_BYTES, "record size");
  HIPCHK(c, hipMemsetAsync(o.dev, 0, JJ_MSM_PARTIAL_BYTES, c->stream));
  // the window count this call's layout has (as msm_enqueue picks it); a window partition over more parts than windows leaves
  // the parts beyond the last window nothing to do (zero-sized grids would fail the launches and no header would be written)
  const int layout_W = n <= (size_t)c->msm_small_max ? SM_W : msm_windows_for(c, n);
  if (n == 0 || part_index >= layout_W) {
    // an empty shard: a valid record without windows
    uint32_t hdr[MSM_REC_HDR_WORDS] = {MSM_REC_MAGIC, 2u, (uint32_t)(n == 0 ? SM_W : layout_W), 1u};
    hdr[6] = (uint32_t)n; hdr[7] = (uint32_t)((uint64_t)n >> 32);
    memcpy(c->host_out[c->host_out_next], hdr, 64);
    HIPCHK(c, hipMemcpyAsync(o.dev, c->host_out[c->host_out_next], 64, hipMemcpyHostToDevice, c->stream));
    c->host_out_next = (c->host_out_next + 1) % 8;
  } else {
    const void *ds, *dp;
    if ((rc = stage_in(c, 0, scalars, 32 * n, &ds))) return rc;
    if ((rc = stage_in(c, 1, points, 64 * n, &dp))) return rc;
    size_t used = 0;
    MsmLane* L = nullptr;
    if ((rc = msm_lane(c, 0, &L))) return rc;
    if ((rc = msm_enqueue(c, *L, n, ds, dp, part_index, part_count, o.dev, &used))) return rc;
  }
  bool sync = false;
  if ((rc = finish_out(c, o, &sync))) return rc;
  return finish(c, sync);
}
// Second half: `count` records (HOST memory, JJ_MSM_PARTIAL_BYTES apart: what the ranks' all_gather delivered, copied back once)
// -> one affine point.  Host only, no context: window sums of all records, one Horner chain per window layout, one inversion.
JJ_API int jj_msm_combine(size_t count, const void* records_host, void* out64_host) {
  if (!out64_host || (count && !records_host) || is_device_ptr(out64_host) || (count && is_device_ptr(records_host))) return JJ_ERR_INVALID;
  jjhost::Ext total = jjhost::identity();
  if (!jjhost::combine_records((const uint8_t*)records_host, count, JJ_MSM_PARTIAL_BYTES, &total)) return JJ_ERR_INVALID;
  jjhost::to_affine64((uint8_t*)out64_host, total);
  return JJ_OK;
}

// ---- multi-rank MSM behind the C ABI ("context: streams, tables, RCCL comm"; 8(e)).  The communicator is the caller's
// (its rendezvous -- who carries the ncclUniqueId to whom -- belongs to the application: examples/msm_rccl.cpp does it with a file,
// bench.py over torch.distributed); the context borrows it.  libjubjub_hip.so does not link RCCL: ncclAllGather is taken from the
// caller, or looked up in the process, or in librccl.so.1 -- it must be the ncclAllGather of the library that made the communicator.
JJ_API int jj_ctx_set_comm(jj_ctx* c, void* nccl_comm, int rank, int nranks, void* all_gather_fn) {
  if (!c) return JJ_ERR_INVALID;
  JJ_ENTER(c);
  if (!nccl_comm) { c->comm = nullptr; c->comm_rank = 0; c->comm_nranks = 1; c->all_gather = nullptr; return JJ_OK; }   // detach
  if (nranks < 1 || nranks > 4096 || rank < 0 || rank >= nranks) { c->err = "jj_ctx_set_comm: bad rank / nranks"; return JJ_ERR_INVALID; }
  void* fn = all_gather_fn;
  if (!fn) fn = dlsym(RTLD_DEFAULT, "ncclAllGather");
  if (!fn) { void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL); if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL); if (h) fn = dlsym(h, "ncclAllGather"); }
  if (!fn) { c->err = "jj_ctx_set_comm: ncclAllGather not found (pass its address, or load librccl first)"; return JJ_ERR_INVALID; }
  c->comm = nccl_comm; c->comm_rank = rank; c->comm_nranks = nranks; c->all_gather = (jj_ctx::AllGatherFn)fn;
  // With more than one rank the jobs in flight stay on ONE lane: consecutive all-gathers of one communicator are then queued on one stream, in
  // the same order on every rank.  Gathers alternating over streams rely on RCCL ordering collectives of a communicator across streams in
  // submission order -- seen with one rank and with the loopback stand-in only, never between GPUs (no multi-GPU box in five rounds).  A caller
  // that has checked it on its node sets option msm_lanes back to 2..4 AFTER this call.
  if (nranks > 1) c->msm_lanes = 1;
  return JJ_OK;
}
// `count` records in DEVICE memory (JJ_MSM_PARTIAL_BYTES apart: what an all_gather delivered) -> the sum of the MSMs they stand for.
// From msm_fold_min records (option, default 8) they are folded window by window ON THE DEVICE into one (k_msm_fold_records), that one is
// copied to the host (8 KB, whatever count is) and takes the single-record host tail.  Fewer records, records of different window layouts, or
// option msm_fold_dev = 0: all records are copied and the host adds them (round 4's path).  The context's lock is held by the caller.
static int msm_combine_dev_locked(jj_ctx* c, size_t count, const uint8_t* recs_dev, jjhost::Ext* total) {
  *total = jjhost::identity();
  if (count == 0) return JJ_OK;
  const size_t host_need = std::max<size_t>(count, 1) * JJ_MSM_PARTIAL_BYTES;
  if (c->gather_host_cap < host_need) {
    if (c->gather_host) (void)hipHostFree(c->gather_host);
    c->gather_host = nullptr; c->gather_host_cap = 0;
    // (coherent: the fold kernel writes its record straight into this buffer, as the MSM kernels write theirs into a job's)
    if (hipHostMalloc((void**)&c->gather_host, host_need, hipHostMallocCoherent | hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); c->err = "hipHostMalloc failed"; return JJ_ERR_NOMEM; }
    c->gather_host_cap = host_need;
  }
  bool folded = false;
  if (c->msm_fold_dev && count >= (size_t)c->msm_fold_min) {
    memset(c->gather_host, 0, jjhost::REC_HDR_BYTES);               // a stale header must never validate
    hipLaunchKernelGGL(k_msm_fold_records, dim3(jjhost::REC_MAX_W), dim3(4 * MSM_TREE_QUADS), 0, c->stream, (const u32*)recs_dev, (u32)count, (u32)(JJ_MSM_PARTIAL_BYTES / 4), (u32*)c->gather_host);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    uint32_t magic; memcpy(&magic, c->gather_host, 4);
    folded = magic == MSM_REC_MAGIC;                    // 0: the records have different window layouts (or one is damaged: the host path reports it)
  }
  if (folded) { if (!jjhost::combine_records(c->gather_host, 1, JJ_MSM_PARTIAL_BYTES, total)) { c->err = "the folded MSM record is damaged (bad header)"; return JJ_ERR_HIP; } return JJ_OK; }
  HIPCHK(c, hipMemcpyAsync(c->gather_host, recs_dev, count * JJ_MSM_PARTIAL_BYTES, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (!jjhost::combine_records(c->gather_host, count, JJ_MSM_PARTIAL_BYTES, total)) { c->err = "a gathered MSM record is damaged (bad header)"; return JJ_ERR_HIP; }
  return JJ_OK;
}
static int msm_write_total(jj_ctx* c, const jjhost::Ext& total, void* out64) {
  if (is_device_ptr(out64)) {
    jjhost::to_affine64(c->host_out[c->host_out_next], total);
    HIPCHK(c, hipMemcpyAsync(out64, c->host_out[c->host_out_next], 64, hipMemcpyHostToDevice, c->stream));
    c->host_out_next = (c->host_out_next + 1) % 8;
  } else jjhost::to_affine64((uint8_t*)out64, total);
  return JJ_OK;
}
JJ_API int jj_msm_combine_dev(jj_ctx* c, size_t count, const void* records_dev, void* out64) {
  if (!c || !out64 || (count && !records_dev)) return JJ_ERR_INVALID;
  JJ_ENTER(c);
  if (count && (!is_device_ptr(records_dev) || ((uintptr_t)records_dev & 15u))) { c->err = "jj_msm_combine_dev takes records in (16-byte aligned) device memory; jj_msm_combine takes host records"; return JJ_ERR_INVALID; }
  jjhost::Ext total;
  const int rc = msm_combine_dev_locked(c, count, (const uint8_t*)records_dev, &total);
  if (rc) return rc;
  return msm_write_total(c, total, out64);
}
// A rank that fails BEFORE its all-gather (its term count is over the pass limit, a workspace cannot grow, a launch fails) must not leave the
// other ranks waiting in theirs: it still takes part, with an all-zero record -- no valid header, so every rank's fold / host tail rejects the
// set and every rank's call returns an error ("a gathered MSM record is damaged") instead of hanging or summing without this rank's terms.
// Best effort: if even this gather cannot be queued, the communicator is lost, as after any failed RCCL collective.
static void msm_post_poison(jj_ctx* c, hipStream_t st) {
  (void)hipGetLastError();
  if (!c->comm || !c->all_gather) return;
  const size_t G = (size_t)c->comm_nranks;
  if (ensure(c, c->poison_dev, (G + 1) * JJ_MSM_PARTIAL_BYTES) != JJ_OK) return;
  uint8_t* mine = (uint8_t*)c->poison_dev.p;
  if (hipMemsetAsync(mine, 0, JJ_MSM_PARTIAL_BYTES, st) != hipSuccess) { (void)hipGetLastError(); return; }
  (void)c->all_gather(mine, mine + JJ_MSM_PARTIAL_BYTES, JJ_MSM_PARTIAL_BYTES, /* ncclUint8 */ 1, c->comm, st);
  (void)hipStreamSynchronize(st);
  (void)hipGetLastError();
}
// jj_msm_allgather in two halves (as jj_msm_begin / jj_msm_finish for the one-GPU sum): everything up to the folded record is queued on
// one of the context's lanes -- the rank's window sums, the ncclAllGather (stream-ordered like any kernel), the fold of the G records
// into one written straight into the job's page-locked buffer -- and the call returns; jj_msm_finish waits for that job and runs the
// single-record host tail.  With several jobs in flight the gather, the fold, the wait and the host tail of one MSM run beside the
// kernels of the next: a rank's sustained rate is that of its kernels, not of the call's latency.
JJ_API int jj_msm_allgather_begin(jj_ctx* c, size_t n, const void* scalars, const void* points, int partition, jj_msm_job** job) {
  if (!c || !job || (partition != 0 && partition != 1)) return JJ_ERR_INVALID;
  *job = nullptr;
  JJ_ENTER(c);
  if (!c->comm || !c->all_gather) { c->err = "jj_msm_allgather_begin: no communicator (jj_ctx_set_comm)"; return JJ_ERR_INVALID; }
  // (every failure from here to the gather posts a poison record: the other ranks are already on their way into the collective)
  if (n > ((size_t)1 << c->msm_pass_log2)) { msm_post_poison(c, c->stream); c->err = "jj_msm_allgather_begin takes at most one pass of terms (2^24) per rank; cut larger inputs"; return JJ_ERR_INVALID; }
  const int G = c->comm_nranks;
  const int part_index = partition ? c->comm_rank : 0, part_count = partition ? G : 1;
  jj_msm_job* j;
  int rc = msm_job_get(c, (size_t)G, &j); if (rc) { const std::string keep = c->err; msm_post_poison(c, c->stream); c->err = keep; return rc; }
  const size_t need = (size_t)(G + 1) * JJ_MSM_PARTIAL_BYTES;
  if (j->gdev_cap < need) {
    if (j->gdev) (void)hipFree(j->gdev);
    j->gdev = nullptr; j->gdev_cap = 0;
    if (hipMalloc(&j->gdev, need) != hipSuccess) { (void)hipGetLastError(); msm_job_put(c, j); msm_post_poison(c, c->stream); c->err = "hipMalloc failed"; return JJ_ERR_NOMEM; }
    j->gdev_cap = need;
  }
  uint8_t* mine = (uint8_t*)j->gdev;                                // this rank's record, then the G gathered ones
  uint8_t* all = mine + JJ_MSM_PARTIAL_BYTES;
  int k = 0;
  if (n && c->msm_lanes > 1 && is_device_ptr(scalars) && is_device_ptr(points)) k = 1 + (int)(c->next_lane++ % (unsigned)c->msm_lanes);
  MsmLane* L = nullptr;
  if ((rc = msm_lane(c, k, &L))) { const std::string keep = c->err; msm_job_put(c, j); msm_post_poison(c, c->stream); c->err = keep; return rc; }
  bool gathered = false;          // a failure before the gather posts the poison record in its place
  auto fail = [&](int code) { const std::string keep = c->err; (void)hipStreamSynchronize(L->stream); (void)hipGetLastError(); if (!gathered) msm_post_poison(c, L->stream); msm_job_put(c, j); c->err = keep; return code; };
  hipError_t e = hipMemsetAsync(mine, 0, JJ_MSM_PARTIAL_BYTES, L->stream);
  if (e != hipSuccess) { c->err = std::string("hipMemsetAsync failed: ") + hipGetErrorString(e); return fail(JJ_ERR_HIP); }
  const int layout_W = n <= (size_t)c->msm_small_max ? SM_W : msm_windows_for(c, n);
  if (n == 0 || part_index >= layout_W) {
    // an empty shard: a valid record without windows (as jj_msm_partial writes it)
    uint32_t hdr[MSM_REC_HDR_WORDS] = {MSM_REC_MAGIC, 2u, (uint32_t)(n == 0 ? SM_W : layout_W), 1u};
    hdr[6] = (uint32_t)n; hdr[7] = (uint32_t)((uint64_t)n >> 32);
    memcpy(c->host_out[c->host_out_next], hdr, 64);
    e = hipMemcpyAsync(mine, c->host_out[c->host_out_next], 64, hipMemcpyHostToDevice, L->stream);
    c->host_out_next = (c->host_out_next + 1) % 8;
    if (e != hipSuccess) { c->err = std::string("hipMemcpyAsync failed: ") + hipGetErrorString(e); return fail(JJ_ERR_HIP); }
  } else {
    const void *ds, *dp;
    size_t used = 0;
    if ((rc = stage_in(c, 0, scalars, 32 * n, &ds)) || (rc = stage_in(c, 1, points, 64 * n, &dp))) return fail(rc);
    if ((rc = msm_enqueue(c, *L, n, ds, dp, part_index, part_count, mine, &used))) return fail(rc);
  }
  const int nrc = c->all_gather(mine, all, JJ_MSM_PARTIAL_BYTES, /* ncclUint8 */ 1, c->comm, L->stream);
  gathered = true;                // (a failure of the collective itself is fatal for the communicator, as with any RCCL collective)
  if (nrc != 0) { c->err = "ncclAllGather failed with ncclResult_t " + std::to_string(nrc); return fail(JJ_ERR_HIP); }
  j->gathered = G;
  if (c->msm_fold_dev && G >= c->msm_fold_min) {
    hipLaunchKernelGGL(k_msm_fold_records, dim3(jjhost::REC_MAX_W), dim3(4 * MSM_TREE_QUADS), 0, L->stream, (const u32*)all, (u32)G, (u32)(JJ_MSM_PARTIAL_BYTES / 4), (u32*)j->host);
    j->folded = true; j->nrec = 1;
  } else {
    e = hipMemcpyAsync(j->host, all, (size_t)G * JJ_MSM_PARTIAL_BYTES, hipMemcpyDeviceToHost, L->stream);
    if (e != hipSuccess) { c->err = std::string("hipMemcpyAsync failed: ") + hipGetErrorString(e); return fail(JJ_ERR_HIP); }
    j->nrec = (size_t)G;
  }
  e = hipEventRecord(j->ev, L->stream);
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) { c->err = std::string("MSM launch failed: ") + hipGetErrorString(e); return fail(JJ_ERR_HIP); }
  *job = j;
  return JJ_OK;
}
// One MSM over the terms (partition 0: each rank passes ITS terms) or the windows (partition 1: each rank passes ALL terms) of every
// rank of the communicator: record of window sums on this device -> ncclAllGather of JJ_MSM_PARTIAL_BYTES per rank over xGMI -> fold on
// the device (from msm_fold_min records) or ONE copy of the gathered records -> ONE host tail on every rank.  Every rank gets the same point.
JJ_API int jj_msm_allgather(jj_ctx* c, size_t n, const void* scalars, const void* points, int partition, void* out64) {
  if (!c || !out64 || (partition != 0 && partition != 1)) return JJ_ERR_INVALID;
  JJ_ENTER(c);                                                       // held through the gather and the host tail (jj_msm_partial re-enters it: the mutex is recursive)
  if (!c->comm || !c->all_gather) { c->err = "jj_msm_allgather: no communicator (jj_ctx_set_comm)"; return JJ_ERR_INVALID; }
  const int G = c->comm_nranks;
  int rc;
  if ((rc = ensure(c, c->gather_dev, (size_t)(G + 1) * JJ_MSM_PARTIAL_BYTES))) { const std::string keep = c->err; msm_post_poison(c, c->stream); c->err = keep; return rc; }
  uint8_t* mine = (uint8_t*)c->gather_dev.p;                       // this rank's record, then the G gathered ones
  uint8_t* all = mine + JJ_MSM_PARTIAL_BYTES;
  if ((rc = jj_msm_partial(c, n, scalars, points, partition ? c->comm_rank : 0, partition ? G : 1, mine))) { const std::string keep = c->err; msm_post_poison(c, c->stream); c->err = keep; return rc; }
  const int nrc = c->all_gather(mine, all, JJ_MSM_PARTIAL_BYTES, /* ncclUint8 */ 1, c->comm, c->stream);
  if (nrc != 0) { c->err = "ncclAllGather failed with ncclResult_t " + std::to_string(nrc); return JJ_ERR_HIP; }
  jjhost::Ext total;
  if ((rc = msm_combine_dev_locked(c, (size_t)G, all, &total))) return rc;
  return msm_write_total(c, total, out64);
}

