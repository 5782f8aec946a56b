/*
 * jubjub_hip.h — C ABI of libjubjub_hip.so, the MI355X-native batched Jubjub engine.
 *
 * This is the drop-in boundary for the scalar-multiplication hot path of the zkcrypto/jubjub crate
 * (reference: /root/reference, crate jubjub 0.10.0).  The reference has no FFI; its boundary is its public
 * Rust API.  Rust struct layouts are unspecified, so the only stable representations — and the wire formats
 * here — are the ones the reference itself exposes publicly:
 *
 *   scalar            32 bytes, little-endian integer      Fr::to_bytes / from_bytes      src/fr.rs:268-308
 *                     (ladder entry points take the raw 32-byte bit pattern, top 4 bits ignored:
 *                      ExtendedPoint::multiply / multiply_bits  src/lib.rs:272-301, 357-385, 831-833)
 *   base field elem   32 bytes, canonical little-endian     Fq::to_bytes / from_bytes      src/lib.rs:456-457, 500
 *   affine point      64 bytes = u || v, each canonical LE  AffinePoint::get_u/get_v       src/lib.rs:630-637,
 *                                                           from_raw_unchecked             src/lib.rs:662-664
 *   compressed point  32 bytes, v with sign(u) in bit 255   AffinePoint::to_bytes          src/lib.rs:455-464
 *   validity          one uint8_t per element (1 = Some, 0 = None); output zeroed when 0   (CtOption / Choice)
 *
 * Pointers may be host or device pointers (detected per pointer with hipPointerGetAttributes); host data is
 * staged through the context's buffers.  With device pointers the call is asynchronous on the context's
 * stream; with any host pointer it returns after the results are in host memory.  A context belongs to one
 * device; its entry points may be called from several host threads (they serialise on a per-context lock), and a
 * change of launch stream is ordered after the work queued on the previous stream (the context's workspaces are shared).
 * jj_multi_* below drives several devices of one node from one process.
 *
 * Every function returns 0 on success or a negative jj_status.
 *
 * BUFFERS -- the contract of every batch entry point below (enforced byte for byte by tests/test_gpu_buffers.py and, for the host-only
 * functions, tests/test_buffer_cases_cpu.py; the table of entry points is tests/buffer_cases.py):
 *   - an entry point writes exactly rows x width bytes of each output array (n x 32 / 64 / 96 / 160 / 256 bytes, n bytes of `ok` or of a
 *     predicate, 4 n bytes of `attempts`; one row where the result is one point or one record): not a byte in front of the array, not a byte
 *     behind it, whatever n is -- also when n is no multiple of a quad, a wave or a workgroup -- and every row of it, the rows whose `ok` is 0
 *     (zeroed) and the empty segments of jj_msm_ragged (the identity) included.  A writer with a `cap` writes at most cap entries;
 *   - it reads its input arrays and never writes them: no input serves as scratch;
 *   - a device pointer needs 16-byte alignment and nothing more (jj_status JJ_ERR_INVALID otherwise); a host pointer needs none.  Arrays of one
 *     call may be aligned differently and may lie directly next to each other;
 *   - n = 0 (B = 0, S = 0) succeeds and touches nothing, but for the one result row of jj_point_sum and the jj_msm family (the identity).
 * In-place calls -- an output array that overlaps an input array of the same call -- are NOT promised by any entry point: hand over disjoint arrays.
 */
#ifndef JUBJUB_HIP_H
#define JUBJUB_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct jj_ctx jj_ctx;
typedef struct jj_table jj_table;

typedef enum {
  JJ_OK = 0,
  JJ_ERR_INVALID = -1,   /* bad argument (null pointer, unknown op, length mismatch: cf. the assert at src/lib.rs:841) */
  JJ_ERR_HIP = -2,       /* a HIP runtime call failed; see jj_last_error() */
  JJ_ERR_NOMEM = -3,
  JJ_ERR_NODEVICE = -4   /* no gfx950 device visible — there is no CPU fallback */
} jj_status;

/* ---- context ------------------------------------------------------------------------------------------- */
int jj_ctx_create(int device, jj_ctx** out);
int jj_ctx_destroy(jj_ctx* ctx);
/* Run on a caller-owned hipStream_t (e.g. torch's current stream; NULL = HIP's default stream).  A new context
 * starts on its own non-blocking stream; jj_ctx_use_own_stream() returns to it. */
int jj_ctx_set_stream(jj_ctx* ctx, void* hip_stream);
int jj_ctx_use_own_stream(jj_ctx* ctx);
int jj_ctx_sync(jj_ctx* ctx);
/* Options.  The library reads NO environment variable: what a caller may tune is set per context, by key, right after jj_ctx_create (before the
 * first batch call).  No option changes WHAT an entry point computes or its timing discipline: the constant-time ladders and selects have no
 * switch (for public scalars there are the explicit *_vartime entry points).  Unknown key or value out of range: JJ_ERR_INVALID.
 *   msm_lanes 1..4 (3)            streams the jobs of jj_msm_begin / jj_msm_allgather_begin alternate over; 1 = every job on the context's stream
 *                                 (jj_ctx_set_comm with more than one rank sets 1: all gathers of one communicator then go through ONE stream)
 *   msm_fold_min 2..4096 (8)      jj_msm_allgather / _combine_dev fold the gathered records on the device from this many records
 *   msm_fold_dev 0|1 (1)          0: the gathered records are copied to the host and added there
 *   msm_host_split 0|1 (1)        host arrays of 2^19 terms and more in several passes, each copy beside the kernels of the pass before
 *   msm_pass_log2 10..24 (24)     terms per Pippenger pass
 *   result_pool_mb 0..2^20 (4096) bytes of released result buffers kept for reuse (jj_result_acquire)
 *   torsion_check_ladder 0|1 (0)  jj_is_torsion_free / _prime_order by [r]P (the reference's definition) instead of the order-8 pairing
 *   pipe_pageable_register 0|1 (0), pipe_copy_threads 0..64 (0 = auto), pipe_ramp 0|1 (1), pipe_prefault 0|1 (1), pipe_chunk_log2 0|8..24 (0 = per
 *                                 entry point): the host-buffer pipeline
 *   fixedbase_default 6|7 (7)     what window_bits = 0 means for jj_fixedbase_table_create
 *   vb_mul2_window 4|5 (4)        jj_varbase_mul2_*: signed window width of the two-term ladder; the same results, 5 = twice the table workspace
 *   msm_ragged_slice_min 1..8192 (16), msm_ragged_waves 1..65536 (2048), msm_ragged_round_terms 1..2^18 (2^18): jj_msm_ragged's planner -- terms
 *                                 per slice at least, waves the short segments are cut for, terms per round of tables; the same results for every value
 * Planner overrides, for tests and measurements (every value gives the same results): msm_windows, msm_small_max, msm_small_blk, msm_accum,
 * msm_seg_len, msm_chunk, msm_chunk_waves, msm_sort_blocks_per_cu, msm_reduce_chunk, msm_reduce_l1, msm_reduce_l2_chunk, msm_sort_hist_fused, msm_sort_two_pass,
 * msm_front1, msm_acc_lds, vb_ct_window, vb_quad_max, dec_c_mid (ranges: jj_pipeline.hip ctx_options; the parity rows of every one: tests/planner_matrix.py).
 * One process-wide option, set with ctx = NULL: host_tail_scalar 0|1 (0) -- the MSM host tail on the scalar 4 x 64-bit chain even where AVX-512 IFMA is there. */
int jj_ctx_set_option(jj_ctx* ctx, const char* key, long long value);
int jj_ctx_get_option(jj_ctx* ctx, const char* key, long long* value);
const char* jj_last_error(jj_ctx* ctx);
int jj_version(void);
/* WnafGroup::recommended_wnaf_for_num_scalars (src/lib.rs:1320-1335) */
int jj_recommended_wnaf_for_num_scalars(size_t num_scalars);
/* Device properties used for roofline accounting: out[0]=CU count, out[1]=clock kHz, out[2]=wavefront size. */
int jj_device_info(jj_ctx* ctx, int64_t out[4]);

/* Per-call kernel timing with HIP events on the launch stream (for roofline accounting).  While enabled, each
 * jj_varbase_mul / jj_fixedbase_mul call records (main kernel ms, normalise-tail ms); read drains the log. */
int jj_ctx_profile(jj_ctx* ctx, int enable);
int jj_ctx_profile_read(jj_ctx* ctx, int max, float* main_ms, float* tail_ms, int* count);
/* Integer-VALU roofline denominator, measured on this device: sustained v_mad_u64_u32 (32x32+64 -> 64 multiply-
 * accumulate) lane-operations per second. */
int jj_peak_imad32(jj_ctx* ctx, double* out_per_sec);                            /* median of five samples */
/* `count` (1..64) single timed launches after one warm-up launch, in launch order: the sustained clock moves by a few percent within a
 * session, so report median and spread (bench.py samples before and after its workload). */
int jj_peak_imad32_samples(jj_ctx* ctx, int count, double* out_per_sec);

/* ---- host buffers ---------------------------------------------------------------------------------------------------------
 * A drop-in caller (the Rust shim of INTEGRATION.md, examples/scalar_mul.c) hands HOST arrays to the entry points below.  Large
 * batches (>= 2^18 units: four chunks of 2^16 and up) of jj_varbase_mul(_compressed), jj_fixedbase_mul(_compressed) and jj_decompress are then cut into chunks
 * that flow over two copy streams while the kernels of the neighbouring chunk run.  That needs PAGE-LOCKED memory:
 *   - memory from jj_host_alloc, or memory registered once with jj_host_register, is used as it is: the copies run straight
 *     from and to it (2^24 fixed-base units: 0.90 of the device-resident rate, profiles/r4_pcie_inclusive.txt);
 *   - any other (pageable) array passes through page-locked staging buffers of the context, copied by a few host threads (default
 *     8, option pipe_copy_threads) beside the GPU's work: within 2-3 % of the page-locked rates, nothing of the caller's is registered,
 *     and a result array the caller has only just allocated costs no more than its page faults.  The GPU never touches the caller's
 *     pageable pages: arrays of 1 MB and more are not handed to the HIP runtime either (which would page-lock them itself).
 *     option pipe_pageable_register = 1 selects round 3's way instead for arrays that consist of whole pages (both ends page-aligned, 1 MB and
 *     more: page-locked in place for the call: no CPU copies, but a freshly allocated 1 GB result array then costs ~65 ms of serial page
 *     faults and pinning inside the call); all other arrays are staged in that mode too -- page-locking them in place would hand pages of
 *     neighbouring objects to the GPU as well (two GPU write faults in ~3000 randomised test rounds followed that).
 * Page-locked buffers that are reused across calls are the fastest arrangement and cost the host no copy threads.
 * These four functions need no context and no HIP headers on the caller's side.  jj_host_alloc: page-locked, visible to every
 * device of the node, *out = NULL for bytes = 0.  jj_host_register: p .. p + bytes must be mapped and stay mapped until
 * jj_host_unregister(p); registering overlapping ranges twice fails with JJ_ERR_INVALID.  The range must consist of WHOLE PAGES -- p
 * page-aligned AND bytes a multiple of the page size (JJ_ERR_INVALID otherwise): register mappings of your own (mmap; or a page-aligned
 * allocation whose length you rounded up to whole pages).  An array on the C heap shares its first and last page with other heap
 * objects -- so does aligned_alloc(4096, 5000) at its end -- and page-locking those pages for the GPU and releasing them again was
 * followed by GPU memory faults on later transfers.
 * HARDWARE QUEUES: HIP multiplexes a process's streams onto GPU_MAX_HW_QUEUES hardware queues (default 4).  A context's host pipeline uses
 * three streams (plus one per extra MSM lane); beside other streams of the process two of them may share a queue and then serialise (pipelines
 * 1.7-2x slower, profiles/r4_pcie_inclusive.txt).  Applications that drive host batches beside other HIP work should export
 * GPU_MAX_HW_QUEUES=8 before the first HIP call; the library does not touch the process environment. */
int jj_host_alloc(size_t bytes, void** out);
int jj_host_free(void* p);
int jj_host_register(void* p, size_t bytes);
int jj_host_unregister(void* p);
/* RESULT POOL: page-locked result buffers owned by the context, for callers whose API returns a NEW result per call -- the shape of
 * every batch function of the reference (`-> Vec<..>`: batch_from_bytes src/lib.rs:541-627, batch_normalize 1084-1107).  A fresh
 * pageable result array costs its page faults inside the call (2^24 fixed-base units: 195 M/s against 557 with reused page-locked
 * buffers, profiles/r4_bench_host_*_fresh.json); jj_result_acquire hands out a buffer of at least `bytes` bytes instead (allocated on
 * first use, recycled afterwards: the smallest free buffer that fits), the entry points recognise it as page-locked memory (copies run
 * straight into it), and jj_result_release gives it back when the caller has consumed the result -- several buffers may be out at a
 * time, so every call can return a DIFFERENT result object.  Released buffers are kept while the pool holds at most result_pool_mb (option)
 * (default 4096) megabytes, and freed with the context.  jj_result_release(NULL) is a no-op; a pointer the context did not hand out
 * is JJ_ERR_INVALID.  Thread-safe per context like every entry point. */
int jj_result_acquire(jj_ctx*, size_t bytes, void** out);
int jj_result_release(jj_ctx*, void* p);
int jj_result_pool_stats(jj_ctx*, size_t* buffers, size_t* bytes, size_t* in_use);
/* How a host batch is cut -- pure functions of their arguments (no context, no device: the CPU-side tests call them).
 * jj_plan_host_chunks: the chunk boundaries of a pipelined host batch of n >= 1 units with chunks of `chunk` units (what the library
 * picks per entry point or option pipe_chunk_log2 sets): chunk k = [bounds[k], bounds[k + 1]), *count = entries of bounds (chunks + 1).
 * ramp != 0: the first and the last chunk are chunk / 4 when the batch has at least four chunks of at least 2^18 units -- the first
 * copy in and the last copy out are the two transfers nothing overlaps; `quantum` (0 = none): the units one round of the kernel's
 * lanes takes, edges are whole multiples of it.  cap = 0 (bounds may be NULL) returns the count only.
 * jj_plan_msm_host_passes: terms per pass and number of passes of jj_msm over HOST arrays of n terms (2^pass_log2 terms per pass at
 * most, 24 by default; split != 0: arrays of 2^19 terms and more are cut into two to eight passes -- more when eight would exceed
 * 2^pass_log2 terms each -- whose copies overlap the kernels). */
int jj_plan_host_chunks(size_t n, size_t chunk, size_t quantum, int ramp, size_t* bounds, size_t cap, size_t* count);
int jj_plan_msm_host_passes(size_t n, int pass_log2, int split, size_t* pass_terms, size_t* passes);

/* ---- fields: Fq (base, = bls12_381::Scalar, src/lib.rs:62) and Fr (scalar, src/fr.rs) ------------------------ */
/* Elements are 32-byte little-endian integers; inputs are reduced mod p like from_raw (src/fr.rs:347-349),
 * outputs are canonical.  reference: add 638-647, sub 620-634, mul 592-616, neg 651-665, square 353-381,
 * double 261-263, invert 438-540 (ok=0 & out=0 for zero), sqrt 384-399 (Fr) / Tonelli-Shanks (Fq, bls12_381).
 * jj_fq_sqrt returns the root that ff 0.13's sqrt_tonelli_shanks is RECALLED to return (that crate is not part of the reference
 * tree and no reference test stores a raw Fq root), so WHICH of the two roots comes back is parity-UNVERIFIED; that it is a root
 * (or ok = 0 for a non-residue) is checked.  Point decompression does not depend on it: the encoding's sign bit picks the root
 * (src/lib.rs:518-520), and that path is pinned by the reference's vectors.
 * TIMING: jj_fq_sqrt / jj_fr_sqrt, jj_decompress and jj_random_points are VARIABLE-TIME in their input: the square root reads a
 * discrete-log table at an address derived from the element's bits (jj_kernels.h sqrt_pohlig).  The dependency's Fq::sqrt
 * (bls12_381, called at src/lib.rs:515) is constant-time; that does not matter for PUBLIC encodings (signature / note / proof
 * bytes), which is what these entry points are for -- do not feed them secret field elements. */
int jj_fq_add(jj_ctx*, size_t n, const void* a, const void* b, void* out);
int jj_fq_sub(jj_ctx*, size_t n, const void* a, const void* b, void* out);
int jj_fq_mul(jj_ctx*, size_t n, const void* a, const void* b, void* out);
int jj_fq_neg(jj_ctx*, size_t n, const void* a, void* out);
int jj_fq_square(jj_ctx*, size_t n, const void* a, void* out);
int jj_fq_double(jj_ctx*, size_t n, const void* a, void* out);
int jj_fq_invert(jj_ctx*, size_t n, const void* a, void* out, uint8_t* ok);
int jj_fq_sqrt(jj_ctx*, size_t n, const void* a, void* out, uint8_t* ok);
int jj_fr_add(jj_ctx*, size_t n, const void* a, const void* b, void* out);
int jj_fr_sub(jj_ctx*, size_t n, const void* a, const void* b, void* out);
int jj_fr_mul(jj_ctx*, size_t n, const void* a, const void* b, void* out);
int jj_fr_neg(jj_ctx*, size_t n, const void* a, void* out);
int jj_fr_square(jj_ctx*, size_t n, const void* a, void* out);
int jj_fr_double(jj_ctx*, size_t n, const void* a, void* out);
int jj_fr_invert(jj_ctx*, size_t n, const void* a, void* out, uint8_t* ok);
int jj_fr_sqrt(jj_ctx*, size_t n, const void* a, void* out, uint8_t* ok);
/* pow (src/fr.rs:403-414): out[i] = a[i] ^ exp[i], exponent = 32-byte little-endian integer, constant-time ladder */
int jj_fq_pow(jj_ctx*, size_t n, const void* a, const void* exp32, void* out);
int jj_fr_pow(jj_ctx*, size_t n, const void* a, const void* exp32, void* out);
/* from_bytes: ok=0 (and out=0) when the integer is >= p (src/fr.rs:268-292).  from_bytes_wide: 64-byte input
 * reduced mod p (src/fr.rs:312-343). */
int jj_fq_from_bytes(jj_ctx*, size_t n, const void* in32, void* out, uint8_t* ok);
int jj_fr_from_bytes(jj_ctx*, size_t n, const void* in32, void* out, uint8_t* ok);
int jj_fq_from_bytes_wide(jj_ctx*, size_t n, const void* in64, void* out);
int jj_fr_from_bytes_wide(jj_ctx*, size_t n, const void* in64, void* out);
/* PrimeFieldBits::to_le_bits (src/fr.rs:746-773): the canonical integer as 256 bytes of 0/1, bit 0 first;
 * char_le_bits (src/fr.rs:775-785): the modulus r in the same layout (host only, no context). */
int jj_fq_to_le_bits(jj_ctx*, size_t n, const void* a, void* out256);
int jj_fr_to_le_bits(jj_ctx*, size_t n, const void* a, void* out256);
int jj_fr_char_le_bits(uint8_t out256[256]);

/* ---- elementwise point operations (affine in, affine out; extended coordinates inside) ----------------- */
/* double src/lib.rs:739-828; add/sub = Ext +/- Affine src/lib.rs:1012-1028; neg 92-104; mul_by_cofactor 722-724 */
int jj_point_double(jj_ctx*, size_t n, const void* p, void* out);
int jj_point_add(jj_ctx*, size_t n, const void* p, const void* q, void* out);
int jj_point_sub(jj_ctx*, size_t n, const void* p, const void* q, void* out);
int jj_point_neg(jj_ctx*, size_t n, const void* p, void* out);
int jj_point_mul_by_cofactor(jj_ctx*, size_t n, const void* p, void* out);
/* AffinePoint::to_niels src/lib.rs:652-658: out = 96 bytes (v+u, v-u, 2d*u*v), each canonical LE */
int jj_point_to_niels(jj_ctx*, size_t n, const void* p, void* out96);
/* predicates -> uint8_t; src/lib.rs:691-719 and (is_on_curve) 670-675 */
int jj_is_identity(jj_ctx*, size_t n, const void* p, uint8_t* out);
int jj_is_small_order(jj_ctx*, size_t n, const void* p, uint8_t* out);
/* is_torsion_free: same predicate as [r]P == O (lib.rs:709-711) for points on the curve, computed with the order-8
 * Tate pairing (one exponentiation) instead of the 252-step ladder; option torsion_check_ladder = 1 selects the ladder. */
int jj_is_torsion_free(jj_ctx*, size_t n, const void* p, uint8_t* out);
int jj_is_prime_order(jj_ctx*, size_t n, const void* p, uint8_t* out);
int jj_is_on_curve(jj_ctx*, size_t n, const void* p, uint8_t* out);
/* Sum for ExtendedPoint (src/lib.rs:183-193): out = one affine point = sum of n affine points (identity if n=0) */
int jj_point_sum(jj_ctx*, size_t n, const void* p, void* out64);

/* ---- scalar multiplication ----------------------------------------------------------------------------- */
/* out[i] = to_affine(points[i] * scalars[i])   (`ExtendedPoint * Fr`, src/lib.rs:873-879 -> 831-833 -> 357-379).
 * scalars are raw 32-byte patterns; only the low 252 bits are used, as in the reference ladder.  Results are specified for on-curve points.
 * CONSTANT-TIME like the reference's ladder (conditional_select, src/lib.rs:334-343): neither the instruction stream nor any memory
 * address depends on the scalar.  The x-only Montgomery ladder on the birationally equivalent curve B y^2 = x^3 + A x^2 + x (A = 40962,
 * B = -40964): x1 = (1 + v)/(1 - v) of every base by one batch inversion per 16 units (k_varbase_mont_x1), then per bit of 251..0 one
 * masked swap and xDBLADD (4S + 5M and a multiplication by a24 = 10240; no table, three waves per SIMD: k_varbase_mont), the y-recovery
 * of Okeya-Sakurai and the map back to Edwards; the identity, the point of order 2 and results O, (0, -1) and -P are masked in.  Option
 * vb_ct_window = 3 / 2 takes the Edwards ladder with signed 3- / 2-bit windows instead (k_varbase_ct3: table {P .. 4P}, {3P, 4P} in a
 * per-lane LDS slot read whole for every window; 85 additions + 252 doublings), the same results.  Batches up to vb_quad_max (32 768)
 * units run one scalar multiplication per quad of lanes (signed 3-bit windows, every lane keeps its own coordinate of the four entries
 * in registers): same discipline, a third of the latency. */
int jj_varbase_mul(jj_ctx*, size_t n, const void* scalars32, const void* points64, void* out64);
/* same, result written as 32-byte compressed encodings (to_bytes of the product, src/lib.rs:455-464, 1419-1421) */
int jj_varbase_mul_compressed(jj_ctx*, size_t n, const void* scalars32, const void* points64, void* out32);
/* the name rounds 3-4 gave the constant-time ladder when it was the opt-in: the same as jj_varbase_mul */
int jj_varbase_mul_ct(jj_ctx*, size_t n, const void* scalars32, const void* points64, void* out64);
/* VARIABLE-TIME variants for PUBLIC scalars (what rounds 1-4 shipped as jj_varbase_mul): signed 5-bit windows, the lane's table
 * {0 .. 16} P in device memory, read at a digit-dependent address: a scalar-independent instruction stream but scalar-dependent
 * memory addresses (cache timing).  1.6-4.5 % faster than k_varbase_ct3 (vb_ct_window = 3) at 2^20 units depending on the box (ratios 0.984 and 0.955: profiles/r5_vb_ct_window.txt, r6_vb_ct_window.txt).
 * Nothing makes jj_varbase_mul / _compressed take this ladder: no option, no environment variable. */
int jj_varbase_mul_vartime(jj_ctx*, size_t n, const void* scalars32, const void* points64, void* out64);
int jj_varbase_mul_vartime_compressed(jj_ctx*, size_t n, const void* scalars32, const void* points64, void* out32);
/* One scalar, many bases: out[i] = points[i] * scalar (the `Wnaf::scalar(..).base(..)` reuse pattern of the group crate,
 * cf. WnafGroup src/lib.rs:1318-1336; the crate's Wnaf machinery is variable-time by design).  The kernel of jj_varbase_mul_vartime with the
 * one scalar read through a wave-uniform address. */
int jj_varbase_mul_scalar(jj_ctx*, size_t n, const void* scalar32, const void* points64, void* out64);
/* Two terms per unit, two variable bases: out[i] = to_affine(points_p[i] * a[i] + points_q[i] * b[i])   (the two-term linear combination of
 * every verifier equation: Schnorr / RedJubjub checks, folding two generator vectors, re-randomised Pedersen openings).
 * VARIABLE-TIME, for PUBLIC scalars, like jj_varbase_mul_vartime: ONE interleaved (Straus) ladder per unit -- both scalars in signed windows, the
 * lane's two tables {0 .. 2^(w-1)} P and {0 .. 2^(w-1)} Q in device memory, read at digit-dependent addresses; per window two additions, then w
 * doublings that serve both terms (w = 4, the default: 252 doublings + 128 additions against the 500 + 103 of two ladders and an addition).  Callers with
 * secret scalars compose jj_varbase_mul and jj_point_add.
 * Scalars are raw 32-byte patterns; only the low 252 bits are used (as jj_varbase_mul and jj_msm).  They are integers, never reduced mod r, so the
 * result is exact on the whole curve: cofactor components, the identity, (0, -1), scalars >= r.  Results are specified for on-curve points.
 * Every unit equals, byte for byte, jj_point_add(jj_varbase_mul(a, P), jj_varbase_mul(b, Q)) and row i of jj_msm_batch(n, 2, ...): canonical affine
 * (u, v), or to_bytes of it for _compressed.  The Edwards law used is complete: Q = P, Q = -P, a P = -b Q, identity bases and zero scalars take no
 * special path.
 * Pointers may be host or device, mixed freely.  n = 0 succeeds and touches nothing.  JJ_ERR_INVALID before any device work: a NULL context, a
 * NULL array with n > 0, NULL ab64.  Context lock, stream rules, jj_profile_*, the result pool and jj_host_alloc buffers: as jj_varbase_mul_vartime;
 * all-host arrays of pipeline size go through the host-buffer pipeline in chunks.
 * One unit per lane for every n: there is no quad-of-lanes form, so the latency of a small call is one lane's ladder.
 * Option vb_mul2_window 4|5 (4): the signed window width; the same results for both.  4 = 2 x 9 table entries (2592 B of workspace per resident
 * lane); 5 = 2 x 17 entries (4896 B) for 250 doublings + 102 additions: no faster beyond the spread at 2^20 units, 4.7 % slower at 2^16
 * (profiles/varbase_mul2_ab.txt). */
int jj_varbase_mul2_vartime(jj_ctx*, size_t n, const void* a32, const void* p64, const void* b32, const void* q64, void* out64);
int jj_varbase_mul2_vartime_compressed(jj_ctx*, size_t n, const void* a32, const void* p64, const void* b32, const void* q64, void* out32);
/* ONE pair of scalars for the whole batch (ab64 = a then b, 64 bytes, host or device): out[i] = a * P[i] + b * Q[i].  Both scalars are read through a
 * wave-uniform address: recoding and digits are scalar-unit work. */
int jj_varbase_mul2_scalars(jj_ctx*, size_t n, const void* ab64, const void* p64, const void* q64, void* out64);
/* Same group element, but computed with the reference's exact 252-step double-and-add-always ladder and
 * returned in projective form: out = 160 bytes (U,V,Z,T1,T2 canonical LE) matching the Rust ExtendedPoint
 * fields bit for bit.  For parity testing, not for throughput. */
int jj_varbase_mul_exact(jj_ctx*, size_t n, const void* scalars32, const void* points64, void* out160);

/* Fixed-base: `AffineNielsPoint * Fr` / multiply_bits (src/lib.rs:272-310) for one base point.
 * The table holds multiples of the base as affine-Niels triples.
 *   window_bits 0 or 7 : signed comb, 8 teeth x 8 column blocks, 140 KiB table staged in LDS: 32 mixed additions + 3 doublings
 *                        per scalar; the entry (one of 128) is selected with two ds_bpermute shuffles and a mask (constant-time:
 *                        no secret-dependent address);
 *   window_bits 6      : signed 6-bit windows, 152 KiB table staged in LDS, one ds_bpermute shuffle per entry (constant-time) —
 *                        43 mixed additions per scalar;
 *   window_bits 8..16  : wider windows (0.6 MB .. 64 MB table, one 128-byte line per entry) kept in L2 / Infinity Cache and gathered per lane
 *                        (variable-time addressing) — ceil(253/w) additions per scalar.
 * A table lives in the memory of the device of the context that built it and serves every context of that device; a context of
 * another device gets JJ_ERR_INVALID (jj_multi_fixedbase_table_create replicates a table per device). */
int jj_fixedbase_table_create(jj_ctx*, const void* base64, int window_bits /* 0 = default */, jj_table** out);
int jj_fixedbase_table_destroy(jj_ctx*, jj_table* t);
int jj_fixedbase_mul(jj_ctx*, const jj_table* t, size_t n, const void* scalars32, void* out64);
int jj_fixedbase_mul_compressed(jj_ctx*, const jj_table* t, size_t n, const void* scalars32, void* out32);
/* One fixed and one variable term per unit: out[i] = to_affine(a[i] * G + b[i] * Q[i]), G the base of `t` (jj_fixedbase_table_create; every
 * window_bits).  The shape of a Schnorr / RedJubjub check [s]G - [c]A (the caller negates A with jj_point_neg), of a re-randomised key
 * ak + [alpha]G and of a Pedersen opening against one fixed generator.  _compressed returns to_bytes of the point: what a verifier compares
 * with the signature's R.
 * VARIABLE-TIME, for PUBLIC scalars only: digit-dependent addresses in both terms, whatever the table kind.
 * Scalars are raw 32-byte patterns; only the low 252 bits are used.  They are integers, never reduced mod r, so the result is exact on the
 * whole curve: cofactor components, the identity, (0, -1), scalars >= r.  Results are specified for on-curve points.  The Edwards law used is
 * complete: Q = G, Q = -G, a G = -b Q, zero scalars and an identity Q take no special path.
 * Every unit equals, byte for byte, jj_point_add(jj_fixedbase_mul(t, a), jj_varbase_mul(b, Q)) and jj_varbase_mul2_vartime(a, G broadcast, b, Q).
 * Three routes, the same bytes from each, chosen by the table kind and n (no option picks one; vb_quad_max moves the boundary):
 *   window_bits 8..16, n > vb_quad_max : ONE kernel, one unit per lane: the signed 5-bit ladder of jj_varbase_mul_vartime on (b, Q) -- 250
 *       doublings, 51 additions, the lane's 17-entry table in device memory -- and then, in the same registers, ceil(253 / w) mixed additions of
 *       entries gathered from G's table (w = 10: 26): G costs no table build per lane and no doubling;
 *   window_bits 6, 7, n > vb_quad_max  : the ladder, then the table's own LDS kernel on the accumulator it left (two launches; the LDS kernels need
 *       a whole CU's LDS and one workgroup per CU);
 *   n <= vb_quad_max                   : the quad-of-lanes ladder, then the table's own kernel (the latency path).
 * Pointers may be host or device, mixed freely.  n = 0 succeeds and touches nothing.  JJ_ERR_INVALID before any device work: a NULL context or
 * table, a NULL array with n > 0, a table of another device (the message of jj_fixedbase_mul), a composite table from
 * jj_fixedbase_composite_create (the message says so).  Context lock, stream rules, jj_profile_*, the result pool and jj_host_alloc buffers: as
 * jj_varbase_mul2_vartime; all-host arrays of pipeline size go through the host-buffer pipeline in chunks (a, b and Q; the table stays resident).
 * Out of scope: a third addend and cofactor clearing -- compose jj_point_add / jj_point_mul_by_cofactor.
 * Measured on an MI355X (profiles/fixedvar_ab.txt, 2^20 units, device-resident, ms per call): table 13 is the fastest gathered width (13.99; 10: 14.19,
 * 8: 14.43; the default LDS table: 15.09) against 15.43 for the three composed calls and 17.45 for jj_varbase_mul2_vartime with G broadcast, spreads
 * <= 0.18; the fixed term costs 6.6 % (w = 13) to 9.9 % (w = 8) over jj_varbase_mul_vartime alone (13.13).  Recommended: window_bits 13 (a 10.5 MB
 * table), or 10 (3.4 MB) within 1.5 % of it. */
int jj_fixedvar_mul_vartime(jj_ctx*, const jj_table* t, size_t n, const void* a32, const void* b32, const void* q64, void* out64);
int jj_fixedvar_mul_vartime_compressed(jj_ctx*, const jj_table* t, size_t n, const void* a32, const void* b32, const void* q64, void* out32);
/* Sums over several fixed bases (the primitive is AffineNielsPoint::multiply_bits, src/lib.rs:297-301):
 *   out[i] = sum_{j < nbases} tables[j] * scalars32[j * n + i]      (base-major scalar array, nbases * n * 32 bytes)
 * e.g. value commitments v*G_v + r*G_r or windowed Pedersen sums.  One pass per base; the accumulator stays in
 * extended coordinates between the passes, so there is a single normalisation. */
int jj_fixedbase_multi_mul(jj_ctx*, const jj_table* const* tables, int nbases, size_t n, const void* scalars32, void* out64);

/* The same sums when the scalars are SHORT, in one pass over one shared LDS table set (Pedersen-style windowed sums, value
 * commitments v*G_v with 64-bit v, ...; the primitive is AffineNielsPoint::multiply_bits, src/lib.rs:297-301, which takes a bit
 * slice):   out[i] = sum_{b < nbases} bases[b] * (scalars32[b * n + i] mod 2^scalar_bits[b])
 * The 42 six-bit window slots of the LDS-staged table are divided among the bases (base b takes ceil((scalar_bits[b] + 2) / 6)
 * of them; the sum must not exceed 42, e.g. 3 bases x 64 bits, 2 x 124, 6 x 40), one accumulator per lane walks all of them:
 * 43 additions per unit whatever nbases is (jj_fixedbase_multi_mul: 32-43 per base), constant-time shuffle select.  The table
 * is destroyed with jj_fixedbase_table_destroy. */
int jj_fixedbase_composite_create(jj_ctx*, int nbases, const void* bases64, const int* scalar_bits, jj_table** out);
int jj_fixedbase_composite_mul(jj_ctx*, const jj_table* t, size_t n, const void* scalars32, void* out64);

/* Multi-scalar multiplication: out = to_affine(sum_i points[i] * scalars[i])  (semantics: iterator Sum of
 * `p * k`, src/lib.rs:183-193 + 873-879; the reference has no MSM algorithm).  n = 0 gives the identity.
 * The device reduces the terms to a record of partial window sums (two launches for small batches, Pippenger above); the last
 * step -- adding the partial sums of each window, Horner over the windows (a chain of 252 dependent doublings) and one
 * inversion -- runs on the calling host thread, so for every n this call waits for the stream even when all pointers are
 * device pointers (the 64-byte result is then copied to out64 asynchronously).  HOST arrays of 2^19 terms and more are summed in
 * two to eight passes, the copy of each pass's slice beside the kernels of the pass before (option msm_host_split = 0: one pass). */
int jj_msm(jj_ctx*, size_t n, const void* scalars32, const void* points64, void* out64);
/* The same in two halves, so that the host tail of one MSM overlaps the kernels of the next: jj_msm_begin queues all device
 * work of one MSM plus the copy of its records into a page-locked buffer owned by the job and returns at once (device
 * pointers; host arrays are staged first); jj_msm_finish waits for THAT job only, runs the host tail and writes the 64-byte
 * result (host pointer: complete on return; device pointer: copy queued on the context's stream).  A context owns several MSM
 * lanes (streams of their own + workspaces; option msm_lanes, default 3 (two until round 6; with three or more jobs in flight the third lane returns 10 % at 2^17 terms); 1 = every job on the context's stream): jobs with
 * device-pointer inputs alternate over them, so that the latency-bound end of one MSM (fix-up, bucket reduce: a few hundred
 * wavefronts) overlaps the sort and accumulation of the next; every job starts after the work already queued on the
 * context's stream when it was begun.  Jobs may be finished in any order, each
 * exactly once (finish releases the job, also on error).  Device input arrays must stay valid until the job is finished; every job must be finished
 * before its context is destroyed. */
typedef struct jj_msm_job jj_msm_job;
int jj_msm_begin(jj_ctx*, size_t n, const void* scalars32, const void* points64, jj_msm_job** job);
int jj_msm_finish(jj_msm_job* job, void* out64);
/* Opt-in device-side finish: the same sum with NO host hop.  The record of window sums stays on the device, one quad of lanes runs
 * the Horner chain (252 dependent doublings) and the inversion there and writes the affine point to out64_dev (DEVICE memory, 16-byte
 * aligned); the call only queues work on the context's stream and returns.  The finish is a ~0.5 ms chain on four lanes against ~0.05 ms
 * on a host core (profiles/r4_msm_dev_finish.txt): use it when the sum feeds the next kernel and the host thread must not wait on the
 * stream (jj_msm does: D2H of the record + host tail + H2D of the point); use jj_msm / jj_msm_begin for latency and throughput.
 * At most 2^24 terms per call; inputs may be host arrays (staged) or device arrays. */
int jj_msm_dev(jj_ctx*, size_t n, const void* scalars32, const void* points64, void* out64_dev);
/* B independent MSMs of n terms each: out64[b] = to_affine(sum_i points[b][i] * scalars[b][i]) for b < B; every row equals
 * jj_msm(ctx, n, row scalars, row points) byte for byte (raw 32-byte scalars, low 252 bits used; exact on the whole curve).
 * VARIABLE-TIME, like jj_msm: table addresses depend on the scalars' digits.
 *   scalars32  B x n x 32 bytes, row-major
 *   points64   n x 64 bytes when points_shared = 1 (every row uses the same points), B x n x 64 bytes when points_shared = 0
 *   out64      B x 64 bytes
 * B = 0 succeeds and touches nothing; n = 0 writes the identity (0, 1) to every row (scalars32 and points64 may then be NULL).
 * JJ_ERR_INVALID: a NULL context, a NULL pointer with a non-zero size, points_shared other than 0 or 1, B * n * 64 beyond size_t.
 * n <= 8192 (MSM_BATCH_MAX): the whole batch runs in a few launches on the context's stream (per-term tables {0..8}P as in jj_msm's
 * small-batch layout, one wave per row and slice of its terms, one lane per window, a device-side Horner chain and inversion per
 * row); with device pointers the call only queues that work and returns, with any host pointer it returns with the results in
 * host memory.  Tables of distinct points are built for at most 2^18 terms at a time (340 MB of device workspace): larger batches
 * run in rounds of whole rows.  n > 8192: every row is a jj_msm_begin job (device-pointer rows alternate over the context's
 * MSM lanes) finished by the host tail, and the call returns only after every row is finished, whatever the pointers. */
int jj_msm_batch(jj_ctx*, size_t B, size_t n, const void* scalars32, const void* points64, int points_shared, void* out64);
/* S independent MSMs of DIFFERENT lengths: sums over consecutive runs of ONE term array (CSR layout):
 *   out64[s] = to_affine(sum_{offsets[s] <= i < offsets[s+1]} points[i] * scalars[i])   for s < S
 * Every segment equals jj_msm(ctx, len, its scalars, its points) byte for byte (raw 32-byte scalars, low 252 bits used; exact on the whole
 * curve: cofactor components, the identity, (0, -1), scalars >= r).  VARIABLE-TIME, like jj_msm.
 *   offsets    S + 1 values in HOST memory, offsets[0] = 0, non-decreasing; N = offsets[S] terms in all.  Read before the call returns.
 *   scalars32  N x 32 bytes, points64 N x 64 bytes (host or device, mixed freely); out64 S x 64 bytes (host or device)
 * An empty segment writes the identity (0, 1).  S = 0 succeeds and touches nothing; N = 0 with S > 0 writes S identities (scalars32 and
 * points64 may then be NULL).
 * JJ_ERR_INVALID, before any device work: a NULL context; NULL offsets or out64 with S > 0; NULL scalars32 or points64 with N > 0;
 * offsets[0] != 0; a decreasing pair; offsets in device memory; S * 64 or N * 64 beyond size_t.
 * Segments of at most 8192 terms (MSM_BATCH_MAX), the short ones, run in a few launches on the context's stream: per-term tables {0..8}P as
 * in jj_msm_batch, a work list of slices built on the host (one wave per slice, one lane per window; the last slice of a segment to finish
 * adds the others), a device-side Horner chain and inversion per segment.  Tables are built for at most 2^18 terms at a time (340 MB of device
 * workspace): more terms run in rounds of whole segments.  Longer segments are one jj_msm_begin job each (over the context's MSM lanes),
 * finished by the host tail.  With only short segments and only device pointers the call queues work and returns; with any long segment or
 * any host pointer it returns with the results in place.  Arrays are staged whole: there is no host-buffer pipeline.
 * jj_plan_msm_ragged / jj_plan_msm_ragged_items: what the call does with these offsets -- pure functions (no context, no device), the same code
 * as the call's own planner.  slice_min / waves / round_terms: 0 = the defaults 16 / 2048 / 2^18 (a context: options msm_ragged_slice_min,
 * msm_ragged_waves, msm_ragged_round_terms).  Slice length t = max(slice_min, ceil(N_short / waves)) with N_short the terms of the short
 * segments; a short segment of len terms is cut into ceil(len / t) slices of near-equal length (each 1 .. t terms); a round holds whole short
 * segments, consecutive in input order, of at most round_terms terms together (a segment above round_terms: a round of its own); a long segment
 * belongs to no round and closes the round before it, so that a round's terms are one contiguous range.
 *   out[0] = short non-empty segments, out[1] = long segments (jobs route), out[2] = work items (slices), out[3] = rounds
 *   items: 4 values per work item -- round, segment, first term, end term -- in launch order; at most cap items are written, *count is always
 *   set (items = NULL with cap = 0: the count only); JJ_ERR_INVALID if cap is too small, and for offsets jj_msm_ragged refuses.
 * Measured (profiles/msm_ragged_ab.txt; one MI355X, 2^18 terms, device-resident, median ms per call [min .. max] of five alternating rounds):
 *   1024 segments of 256 terms             ragged 2.1396 [2.1286 .. 2.2154]   jj_msm_batch on the same rectangle 2.0663 [2.0570 .. 2.0811] and
 *                                          2.1553 [2.1526 .. 2.1710] (the same call in two slots of the loop)   a jj_msm_begin job per segment 45.9
 *   geometric lengths, mean 64             ragged 2.3974 [2.3657 .. 2.4781]   zero-padded jj_msm_batch 11.8380 (4.94 x)   jobs 186.95 (78 x)
 *   90 % of 4 terms, 10 % of 2000          ragged 2.2651 [2.2604 .. 2.2786]   zero-padded jj_msm_batch 15.1859 (6.70 x)   jobs 54.07 (24 x)
 * On a true rectangle the call sits within the spread of jj_msm_batch (its sum kernel is 2-4 % slower in a kernel trace,
 * profiles/msm_ragged_kernels.txt); on skewed lengths it beats both the padded batch and the job per segment. */
int jj_msm_ragged(jj_ctx*, size_t S, const uint64_t* offsets, const void* scalars32, const void* points64, void* out64);
int jj_plan_msm_ragged(size_t S, const uint64_t* offsets, int slice_min, int waves, uint64_t round_terms, int64_t out[4]);
int jj_plan_msm_ragged_items(size_t S, const uint64_t* offsets, int slice_min, int waves, uint64_t round_terms, uint64_t* items, size_t cap, size_t* count);
/* Fixed-basis MSM: many scalar vectors against ONE set of points that is handed over once (Pedersen vector commitments, value / note
 * commitments over many generators, an IPA prover, a batch verifier with a fixed key set) -- the MSM's counterpart of
 * jj_fixedbase_table_create / jj_fixedbase_mul.  jj_msm_basis_create copies the n points (host or device pointer; the caller's array may be
 * freed or overwritten when the call returns) into tables in device memory, jj_msm_basis_mul brings scalars only:
 *   rows b < B:  out64[b] = to_affine(sum_{i < m} points[i] * scalars32[b][i]),   m <= n: the FIRST m points of the basis
 * scalars32: B x m x 32 bytes, raw patterns, low 252 bits used; every row equals jj_msm(ctx, m, row, first m points) byte for byte (exact on
 * the whole curve: cofactor components, the identity, scalars >= r).  VARIABLE-TIME like jj_msm.
 *   mode 1 (points)   the converted points stay resident, 128 bytes per point: jj_msm's plan without the copy and the conversion of the points
 *   mode 2 (windows)  additionally 2^(start_w) P_i for every window w of the basis's layout, 128 bytes x windows per point: digit w of a scalar
 *                     selects row (w, i) and ALL windows add into one bucket set -- one bucket reduce instead of one per window, a record of
 *                     one point, no Horner chain on the host (one inversion)
 *   mode 0 (auto)     the faster of the two as measured (profiles/msm_basis_ab.txt) whose tables fit HALF of the device memory that is
 *                     free at create: today mode 1 for every n -- with jj_msm's window counts mode 2 measured 5-9 % slower, it is an opt-in
 *   windows           0 = what jj_msm takes for n terms (23 / 17 / 16), else 16 .. 36: the layout of the table (mode 2; fixed at create, also
 *                     for shorter prefixes) or of every call (mode 1; 0 there: chosen per call from m, option msm_windows included).
 *                     Out of range: JJ_ERR_INVALID.  Ignored for rows of up to 8192 terms.
 * Rows of up to 8192 terms (the limit of jj_msm_batch's batched kernels) run over per-point tables {0 .. 8} P (1296 bytes per point) that
 * every basis keeps for its first min(n, 8192) points, in both modes alike: for B > 1 a few launches on the context's stream whatever B is (with
 * device pointers the call only queues that work and returns); a single row takes jj_msm's small-batch pass over the tables and its host tail.  Longer rows are one Pippenger pass each over the resident records, several in
 * flight over the context's MSM lanes when B > 1, each finished by the host tail: the call then returns after every row is finished, whatever
 * the pointers (a device out64 is written by a copy the call waits for when B > 1, by a queued copy when B = 1, as jj_msm).  With any host
 * pointer the results are in memory on return.
 * B = 0 succeeds and touches nothing; m = 0 (also a basis of n = 0 points) writes the identity (0, 1) to every row.  JJ_ERR_INVALID, before any
 * device work: a NULL context or basis, NULL where a size is non-zero, m > n, an unknown mode, B * m * 32 beyond size_t, n above 2^24.
 * JJ_ERR_NOMEM: the tables do not fit (nothing is left behind).  A basis lives in the memory of the device of the context that built it and
 * serves every context of that device, from several threads at once; a context of another device gets JJ_ERR_INVALID.  Destroy it before the
 * last context of its device.
 * jj_msm_basis_info: out[0] = n, out[1] = mode in use (1 | 2; for at most 8192 points the mode asked for, 1 for auto), out[2] = windows of the
 * layout (64 for at most 8192 points), out[3] = bytes of device memory held.
 * jj_plan_msm_basis: what create chooses for n points when budget_bytes of device memory may be used -- a pure function (no context, no
 * device): out[0] = mode, out[1] = windows, out[2] = table bytes, out[3] = route of an n-term row (0 small tables, 1 Pippenger). */
typedef struct jj_msm_basis jj_msm_basis;
int jj_msm_basis_create(jj_ctx*, size_t n, const void* points64, int mode, int windows, jj_msm_basis** out);
int jj_msm_basis_destroy(jj_ctx*, jj_msm_basis* basis);
int jj_msm_basis_info(const jj_msm_basis* basis, int64_t out[4]);
int jj_msm_basis_mul(jj_ctx*, const jj_msm_basis* basis, size_t B, size_t m, const void* scalars32, void* out64);
int jj_plan_msm_basis(size_t n, int mode, int windows, uint64_t budget_bytes, int64_t out[4]);
/* MSM cut across devices or ranks.  jj_msm_partial leaves the RECORD of partial window sums instead of the
 * point: JJ_MSM_PARTIAL_BYTES bytes (64-byte header: magic, version, number of windows W, 1, bit mask of the windows
 * present, n; then one 128-byte point per window: U, V, Z and T = T1 T2, each the 256-bit little-endian integer of
 * value x 2^256 mod q, the Montgomery form of the host tail; unused space zeroed), written to device memory (asynchronous: ready for an all_gather over RCCL) or host memory.  At most 2^24 terms per call.
 *   part_index = 0, part_count = 1   all windows of the n terms given       (term partition: each rank passes ITS terms)
 *   part_index = g, part_count = G   windows g, g + G, ... of the n terms    (window partition: each rank passes ALL terms)
 * jj_msm_combine (host only, no context) adds any number of records -- window by window where their layouts agree, so the
 * Horner chain runs once per layout -- and returns the affine sum: one copy to the host, one host tail and one inversion
 * for the whole distributed MSM.  Records of a window partition must come from calls with the same n. */
#define JJ_MSM_PARTIAL_BYTES 8256u   /* 64 + 64 windows x 128 */
int jj_msm_partial(jj_ctx*, size_t n, const void* scalars32, const void* points64, int part_index, int part_count, void* record);
int jj_msm_combine(size_t count, const void* records_host, void* out64_host);
/* The same sum (Sum for ExtendedPoint, src/lib.rs:183-193, over the parts) for records that are in DEVICE memory -- what an all_gather
 * delivered, JJ_MSM_PARTIAL_BYTES apart, 16-byte aligned: the records are added window by window on the device into ONE record
 * (a quad of lanes per record and window, an LDS tree over the records), which takes one 8 KB copy and the single-record host tail
 * whatever `count` is.  Records of different window layouts fall back to one copy of all of them and the host's additions.
 * out64 may be a host or a device pointer. */
int jj_msm_combine_dev(jj_ctx*, size_t count, const void* records_dev, void* out64);

/* The same exchange behind ONE call, for callers that run one process per GPU (the context holds "streams, tables,
 * RCCL comm"; 8(e)).  jj_ctx_set_comm lends the context an RCCL communicator that the CALLER created (ncclCommInitRank; the
 * rendezvous that carries the ncclUniqueId between the processes belongs to the application -- examples/msm_rccl.cpp does it with a
 * file, bench.py over torch.distributed) together with this process's rank.  all_gather_fn: address of the ncclAllGather of the
 * RCCL library that made the communicator, or NULL (then looked up among the symbols of the process, then in librccl.so.1);
 * libjubjub_hip.so itself does not link RCCL.  nccl_comm = NULL detaches.  The communicator must outlive its use here; the caller
 * destroys it.
 * jj_msm_allgather: every rank calls it with ITS terms (partition 0) or with ALL terms (partition 1: rank g reduces windows g, g + G,
 * ... of the whole batch; same n on every rank): record of window sums (jj_msm_partial) -> ncclAllGather of JJ_MSM_PARTIAL_BYTES per
 * rank on the context's stream -> the G records folded into one on the device (jj_msm_combine_dev) -> one 8 KB copy -> one host tail.  Every rank returns the
 * same point; out64 may be a host or a device pointer.  A collective: all ranks must call it, in the same order -- a rank whose call
 * fails BEFORE the gather (bad arguments, out of memory) never enters it and the other ranks wait for it: treat an error of
 * jj_msm_allgather as fatal for the communicator (as with any RCCL collective). */
int jj_ctx_set_comm(jj_ctx*, void* nccl_comm, int rank, int nranks, void* all_gather_fn);
int jj_msm_allgather(jj_ctx*, size_t n, const void* scalars32, const void* points64, int partition, void* out64);
/* jj_msm_allgather in two halves, for a caller with many MSMs to sum (a prover's commitments): jj_msm_allgather_begin queues the
 * rank's window sums, the ncclAllGather and the fold of the gathered records on one of the context's MSM lanes (all stream-ordered;
 * the folded record lands in a page-locked buffer the job owns) and returns; jj_msm_finish (above) waits for THAT job and runs the
 * single-record host tail.  With two to four jobs in flight a rank's gather, fold, wait and host tail run beside the kernels of its
 * next MSM, so the sustained rate of the distributed sum is set by the kernels of one share (2^17 terms of a 2^20-term MSM cut
 * eight ways: 0.245-0.255 ms per MSM against 0.385 ms + the gather's latency for one synchronous call).  A collective like jj_msm_allgather:
 * every rank begins the same jobs in the same order (the gathers of one communicator run in the order they were queued); jobs
 * may be finished in any order, each exactly once; at most 2^24 terms per rank and job; device input arrays stay valid until the
 * job is finished. */
int jj_msm_allgather_begin(jj_ctx*, size_t n, const void* scalars32, const void* points64, int partition, jj_msm_job** job);
/* Batch verification of n Schnorr / RedJubjub-style signatures (R_i, s_i) under keys A_i and challenges c_i, as ONE MSM job:
 *   out64 = to_affine([8] * (sum_i [z_i] R_i + sum_i [z_i c_i mod r] A_i - [sum_i z_i s_i mod r] B))     written by jj_msm_finish(job, out64)
 *   base64   the affine base point B: any on-curve point, also one with a cofactor component (the library knows no particular generator)
 *   r32 a32  n compressed encodings each: the signature's R and the verification key A
 *   s32      n response scalars (canonical: s_i >= r is malformed)
 *   c32      n challenges as raw 32-byte integers, reduced mod r here (jj_sig_challenge hashes them on the device; a caller with another hash supplies its own)
 *   z16      n x 16 bytes of the caller's randomness, one 128-bit weight per signature (the library has no RNG; use non-zero weights)
 *   flags    0 or JJ_DECOMPRESS_ZIP216 (the decoder's rule for R and A)
 * Reducing the scalars mod r is exact because the cofactor is cleared at the end: [8][x]P = [x mod r][8]P for every P on the curve.
 * The verdict is the point:
 *   (0, 1)    every signature satisfies the COFACTORED check [8]([s]B - R - [c]A) = O (a torsion component of R, A or B is accepted, as
 *             by a per-signature cofactored verifier); with random z a batch holding a failing signature gives this with chance <= 2^-128;
 *   (0, -1)   malformed input: an encoding that does not decode under `flags`, or some s_i >= r.  [8] of anything lies in the prime-order
 *             subgroup, so the order-2 point cannot be a sum: the sentinel is unambiguous.  A failed decode contributes the identity;
 *   other     at least one signature fails: bisect, or check one by one with jj_fixedvar_mul_vartime_compressed.
 * VARIABLE-TIME: everything here is public.  Device work: the decoder over r32 and a32 into a workspace the job owns, one kernel that
 * writes the 2n scalars and a partial of sum z_i s_i per workgroup (k_sig_terms), one workgroup that closes the sum and writes the term of B
 * and the malformed flag (k_sig_close), then the 2n + 1 terms as a job of jj_msm_begin: context lock, lanes, stream rules and lifetime are
 * jj_msm_begin's; several jobs may be in flight and be finished in any order; the job owns its workspace until it is finished (96 bytes per
 * term; it stays with the pooled job afterwards).  Pointers may be host or device, mixed freely (device pointers 16-byte aligned; host
 * arrays are staged before the call returns).  n = 0 gives a job whose finish writes the identity (the arrays may then be NULL).
 * JJ_ERR_INVALID before any device work, *job = NULL: a NULL context, job or base64, a NULL array with n > 0, flags other than 0 or
 * JJ_DECOMPRESS_ZIP216, 2n + 1 > 2^24.  No synchronous twin, no per-signature ok array.
 * Measured on an MI355X (profiles/sig_batch_ab.txt, device-resident valid batches, signatures/s, median of five alternating rounds): 2^20 signatures 140.8 M/s with one job (7.45 ms) and 178.3 M/s with four in flight, against 26.7 M/s for the same check composed from jj_decompress x 2, jj_fr_mul, a host-side sum and jj_msm (5.3x / 6.7x) and 55.7 M/s for the per-signature route jj_decompress x 2 + jj_point_neg + jj_fixedvar_mul_vartime_compressed, table 13 (2.5x / 3.2x); 2^16: 23.9 M/s (one job) and 45.1 M/s (four) against 23.9 composed and 27.1 per signature -- one job alone is 12 % BEHIND the per-signature route there, the two decodes of 2^14 lanes each are its serial chain; 2^10: 1.68 / 2.12 M/s against 1.13 and 0.95.  Both routes decode 2n points: the decoder, not the MSM, is the larger part of this call. */
int jj_sigbatch_begin(jj_ctx*, const void* base64, size_t n, const void* r32, const void* a32, const void* s32, const void* c32, const void* z16,
                      unsigned flags, jj_msm_job** job);
/* The same batch check for signatures GROUPED BY KEY, with the terms of equal keys folded into one: n + K + 1 terms and n + K decodes for n
 * signatures under K keys (a validator set, a few signers of many messages), against 2n + 1 and 2n of jj_sigbatch_begin:
 *   out64 = to_affine([8] * (sum_i [z_i] R_i + sum_k [sum_{i in group k} z_i c_i mod r] A_k - [sum_i z_i s_i mod r] B))     written by jj_msm_finish(job, out64)
 *   a32      K compressed verification keys
 *   offsets  K + 1 values in HOST memory, CSR as in jj_msm_ragged: offsets[0] = 0, non-decreasing, n = offsets[K]; signatures
 *            offsets[k] .. offsets[k+1] are checked under key k.  Read before the call returns.
 *   r32 s32 c32 (n x 32), z16 (n x 16), base64, flags: as in jj_sigbatch_begin, in the grouped order.
 * The verdict is the point, as there: (0, 1) accept, (0, -1) malformed, any other point a failing signature.  For every input in which each
 * listed key has at least one signature, out64 equals BYTE FOR BYTE what jj_sigbatch_begin writes for the expanded arrays (a32[k] repeated over
 * its group) with the same z16: the two sums differ only by multiples of [r]A_k (the folded scalar is reduced mod r once, not once per
 * signature), and the three doublings of the finish clear those: [8][r]P = O for every P on the curve.
 *   Empty group: a key with no signatures contributes [0]A_k.  Undecodable key: EVERY key given is decoded, and one that does not decode under
 *   `flags` makes the batch malformed even if its group is empty.  Duplicate key: the same encoding listed twice is two groups, no special path.
 *   n = 0 (offsets[K] = 0, any K): a job whose finish writes the identity; the arrays are not read (no key is decoded) and may be NULL.
 * JJ_ERR_INVALID before any device work, *job = NULL: a NULL context, job or base64; NULL offsets with K > 0; a NULL array with n > 0;
 * offsets[0] != 0 or a decreasing pair; offsets in device memory; flags other than 0 or JJ_DECOMPRESS_ZIP216; n + K + 1 > 2^24.
 * Pointers may be host or device, mixed freely (offsets host only; device pointers 16-byte aligned, "device pointers must be 16-byte aligned"
 * otherwise).  VARIABLE-TIME: everything here is public.  Device work: r32 and a32 copied into one region of the job's workspace and ONE
 * decoder launch over the n + K encodings; k_sig_keyed_terms (jj_sig_keyed_kernels.h), one signature per lane, writes the n scalars z_i and adds
 * z_i c_i over the lanes of its wave that share a key; k_sig_keyed_close, one key per lane and a whole wave for a key whose group spans
 * several waves, writes the K folded scalars; k_sig_close writes the term of B and the malformed flag; then the n + K + 1 terms as a job of
 * jj_msm_begin.  Context lock, lanes, stream rules, job pool, workspace ownership and lifetime are jj_sigbatch_begin's (96 bytes per term
 * and 64 more per signature -- head slot and encoding copy -- in the job's workspace); several jobs may be in flight and be finished in any order.  No synchronous twin, no per-signature
 * ok array.
 * Measured on an MI355X (profiles/sig_keyed_ab.txt, against jj_sigbatch_begin on the expanded arrays, device-resident valid batches in equal groups, signatures/s, median of five alternating rounds, every ratio outside the rounds' spread): 2^20 signatures, K = 8 / 256 / n/4: 176.6 / 180.7 / 174.9 M/s with one job against 145.6-146.9 (1.21x / 1.23x / 1.19x) and 293.7 / 301.8 / 285.9 M/s with four in flight against 181.0-183.5 (1.62x / 1.65x / 1.58x); 2^16: 1.25-1.33x (one job) and 1.31-1.37x (four); 2^10: 1.41-1.54x and 1.57-1.77x.  K = n at 2^20 is BEHIND: 130.7 against 146.8 M/s with one job (12 % slower), 177.1 against 183.5 with four (3.5 % slower) -- the same decodes and terms plus a copy and one more kernel; the routes cross near K = 0.67 n (interpolated).  One job gains 19 %, not half, at K = 256: the decoder launch over n + K encodings measured ~3.1 ms where one over n takes 2.03 (unexplained). */
int jj_sigbatch_keyed_begin(jj_ctx*, const void* base64, size_t K, const void* a32, const uint64_t* offsets, const void* r32, const void* s32, const void* c32, const void* z16,
                            unsigned flags, jj_msm_job** job);
/* S batch checks over consecutive runs of ONE signature array, one verdict point per run, in one call: what a verifier needs to find the failing
 * signatures of a batch (bisection, Engine.sigbatch_locate) and to give many small batches a verdict each (the signatures of each transaction of
 * a block, of each peer's message).  Synchronous in the sense of jj_msm_ragged.
 *   offsets  S + 1 values in HOST memory, CSR as in jj_msm_ragged: offsets[0] = 0, non-decreasing, n = offsets[S]; segment g holds signatures
 *            offsets[g] .. offsets[g+1].  Read before the call returns.
 *   r32 a32 s32 c32 (n x 32), z16 (n x 16), base64, flags (0 or JJ_DECOMPRESS_ZIP216): as in jj_sigbatch_begin.
 *   out64    S x 64 bytes, host or device.
 * out64[g] equals BYTE FOR BYTE what jj_sigbatch_begin + jj_msm_finish write for the arrays of segment g alone with the same z16 rows: (0, 1)
 * accept, and also an empty segment; (0, -1) when a unit of that segment does not decode or has s >= r; otherwise the point
 * [8](sum z R + sum [z c mod r] A - [sum z s mod r] B) of that segment.  A malformed unit spoils its own segment only.  S = 0 succeeds and
 * touches nothing; n = 0 with S > 0 writes S identities and reads no array (they may be NULL).
 * Use non-zero weights.  A segment of ONE signature with a non-zero weight is an EXACT cofactored check of that signature, not a probabilistic
 * one: z < 2^128 < r is invertible mod r, so [z][8](R + [c]A - [s]B) = O exactly when [8](R + [c]A - [s]B) = O.  Single-signature segments take
 * the same path as every other segment.
 * JJ_ERR_INVALID before any device work: a NULL context or base64; NULL offsets or out64 with S > 0; a NULL array with n > 0; offsets[0] != 0, a
 * decreasing pair, or offsets in device memory; flags other than 0 or JJ_DECOMPRESS_ZIP216; 2n + S > 2^24; a misaligned device pointer ("device
 * pointers must be 16-byte aligned").  Pointers may be host or device, mixed freely (offsets host only).
 * VARIABLE-TIME: everything here is public.  Device work, all on the context's launch stream in a workspace the CONTEXT owns (96 bytes per term
 * of the 2n + S, 64 per decoded point, and per signature the two ok bytes, a head slot and the copy of its two encodings): r32 | a32 copied into
 * one region and ONE decoder launch over the 2n encodings with JJ_DECOMPRESS_CLEAR_COFACTOR, [8]B by the cofactor operation; k_sig_seg_terms
 * (jj_sig_seg_kernels.h), one signature per lane, lays the terms out segment by segment -- segment g owns terms 2 offsets[g] + g ..: its R terms,
 * its A terms, its own term of B -- and adds z_i s_i over the lanes of a wave that share a segment; k_sig_seg_close, one segment per lane, writes
 * the term of B; the S sums are those of jj_msm_ragged over the term offsets 2 offsets[g] + g (segments above 8192 terms as MSM jobs, finished
 * before the call returns); k_sig_seg_verdict writes (0, -1) over the rows of malformed segments.  Every term lies in the image of [8], so each
 * sum is the verdict point itself and nothing is doubled afterwards; the bytes equal those of the doubled sum because an affine point has one
 * encoding.  With a device out64 and no segment above 8192 terms the call only queues the work.
 * Measured on an MI355X (profiles/sig_ragged_ab.txt, device-resident valid batches, signatures/s, median of five alternating rounds, every ratio outside the rounds' spread; a = one jj_sigbatch_begin job per segment, four in flight; b = the per-signature route jj_decompress x 2 + jj_point_neg + jj_fixedvar_mul_vartime_compressed, table 13): 2^20 signatures in segments of 64: 47.9 M/s (21.9 ms) against 0.137 M/s for a (350x) and 54.9 M/s for b -- 13 % BEHIND b; geometric lengths of mean 16: 37.1 M/s, 1167x a, 33 % behind b; 16 equal segments (all on the jobs route): 49.3 M/s, 1.13x a, 11 % behind b, and a third of ONE jj_sigbatch_begin job over the whole batch (140.8 M/s); segments of ONE: 9.6 M/s, 5.7x SLOWER than b (three-term sums through per-term tables against one fused ladder).  2^16: segments of 64 29.1 M/s (1.05x b), geometric 28.0 (1.03x b), 16 equal 23.6 (2.9x a, 0.87x b), segments of one 9.3 (0.34x b).  So: far ahead of a job per segment wherever segments are short, level with or behind the per-signature route everywhere, and Engine.sigbatch_locate is BEHIND it too at 2^20: 36.7 ms with one failing signature and 128.8 ms with 16 (five calls each) against 19.0 ms -- its first call alone costs more than b.  One 2^20 call in segments of 64 (kernel trace, 22.8 ms of kernels): k_msm_ragged_sum 10.8 ms, k_msm_ragged_finish 5.1 ms (nine latency-bound launches, one per round of 2^18 terms), the decoder 4.5 ms, k_msm_batch_tables 1.8 ms; the decoder's extra cofactor pass 0.54 ms (2.4 %), the three new kernels 0.12 ms. */
int jj_sigbatch_ragged(jj_ctx*, const void* base64, size_t S, const uint64_t* offsets, const void* r32, const void* a32, const void* s32, const void* c32, const void* z16,
                       unsigned flags, void* out64);

/* ---- one Schnorr verdict PER SIGNATURE, in one synchronous call: what a verifier asks once a batch is rejected, or when it has no batch.
 *   t         a table of jj_fixedbase_table_create for the base B, any window_bits.  A composite table: JJ_ERR_INVALID.
 *   r32 a32   encodings of R_i and A_i;  s32: s_i canonical, s_i >= r is malformed;  c32: any 256-bit integer, reduced mod r here
 *             (n x 32 each, as in jj_sigbatch_begin)
 *   flags     a subset of JJ_DECOMPRESS_ZIP216 (the decoder's rule for R and A) | JJ_SIG_COFACTORLESS; anything else: JJ_ERR_INVALID
 *             before any device work
 *   verdict   n bytes:  JJ_SIG_MALFORMED  R_i or A_i does not decode, or s_i >= r
 *                       JJ_SIG_OK         otherwise, iff [8]([s_i]B - [c_i mod r]A_i - R_i) = O -- the COFACTORED equation of every jj_sigbatch_*
 *                                         call; with JJ_SIG_COFACTORLESS iff [s_i]B - [c_i mod r]A_i - R_i = O (the three doublings left out:
 *                                         what comparing encodings checks)
 *                       JJ_SIG_REJECT     otherwise
 *             Nothing else is written for a unit.
 * VARIABLE-TIME: digit-dependent table addresses in both terms.  Everything here is public (signatures, keys, challenges).
 * Pointers may be host or device, mixed freely (device pointers 16-byte aligned).  n = 0 succeeds, touches nothing, and the arrays may be
 * NULL.  JJ_ERR_INVALID: a NULL context or table, a NULL array with n > 0, a table of another device.  Synchronous under the context lock and
 * the stream rules of jj_fixedvar_mul_vartime (a device verdict array is written in launch-stream order).  n is processed in chunks of 2^20
 * units queued one after another; the context-owned workspace (162 bytes per unit and the ladder's own) is bounded by the chunk, not by n.
 * Kernels: k_decompress twice per chunk (R, then A: the caller's arrays are not contiguous; through jj_decompress one launch over 2^21 encodings
 * with the copy that makes them so takes 3.64 ms against 3.84 ms for two calls over 2^20, a difference below the 0.24 ms the second CALL costs
 * by itself, which two launches inside one entry point do not pay), k_sig_each_prep (c mod r, s < r, -A in place, the identity over a failed
 * decode, the MALFORMED bytes), the ladders of jj_fixedvar_mul_vartime by its own rule for the table and the size, and k_sig_each_tail on the
 * three coordinates they leave: R subtracted as an affine-Niels operand, three doublings, Curve::is_identity, ONE byte stored -- no k_normalize,
 * no compress, no jj_point_neg pass, no compare in the caller.  Bounds: the tail adds to the output of an addition and doubles the output of an
 * addition, both in the set tools/bounds_check.py check_curve iterates over (jj_sig_each.h).
 * Measured on an MI355X (profiles/sig_each_ab.txt: device-resident valid batches, five alternating rounds of one process per route, median; the
 * composed route -- jj_decompress x 2 + jj_point_neg + jj_fixedvar_mul_vartime_compressed + the caller's compare -- on a build of the parent
 * commit): 2^20 signatures, table 13: 18.25 ms per call cofactored (57.5 M signatures/s), 18.08 ms cofactorless, against 18.58 ms for the composed
 * route, which checks the cofactorless rule -- 1.018x and 1.028x, both outside the rounds' spread; table 10: 18.38 / 18.28 against 18.77 ms.  2^16:
 * 2.26 / 2.25 against 2.41 ms (1.07x); 2^10: 0.942 / 0.936 against 1.055 ms (1.12x: three calls fewer).  So the gain is what was supposed, a few
 * percent, and no more: one 2^20 call is k_varbase_fixed 14.9 ms, the decoder 2 x 2.23 ms, k_sig_each_tail 0.22 ms, k_sig_each_prep 0.04 ms
 * (kernel trace).  A fused kernel that kept the ladder's accumulator in registers for the tail (k_sig_each) was built and measured: level at 2^10
 * and 2^16, 2.3 % and 2.2 % SLOWER at 2^20 (tables 13, 10), beyond the spread; it is not in the library (experiments/sig_each_fused).
 * Engine.sig_locate (one jj_sigbatch_begin job, then this call only if the batch is rejected) at 2^20: 7.1 ms for a valid batch against 21.3 ms
 * for Engine.sigbatch_locate and 18.5 ms for the composed route; 26.0 ms with 1 or with 16 failing signatures against 36.8 / 150.3 ms for
 * sigbatch_locate -- and BEHIND the composed route or this call alone (18.6 / 18.3 ms) whenever the batch fails: the batch job is then paid on top. */
#define JJ_SIG_REJECT       0u
#define JJ_SIG_OK           1u
#define JJ_SIG_MALFORMED    2u
#define JJ_SIG_COFACTORLESS 16u  /* flag of jj_sigverify_each; clear of the JJ_DECOMPRESS_* bits */
int jj_sigverify_each(jj_ctx*, const jj_table* t, size_t n, const void* r32, const void* a32, const void* s32, const void* c32, unsigned flags, uint8_t* verdict);

/* ---- the challenges of the signature family, hashed on the device:
 *   c32[i] = Fr::from_bytes_wide(BLAKE2b-512(personal16; r32[i] || a32[i] || M_i))   as 32 canonical little-endian bytes
 * -- what every Schnorr scheme on Jubjub that the jj_sigbatch_* calls and jj_sigverify_each serve computes before the check (RedJubjub: the
 * personalisation "Zcash_RedJubjubH").  The library still knows no protocol: the personalisation is the caller's, as the base point is.
 * BLAKE2b as in RFC 7693: unkeyed, 64-byte digest, zero salt.
 *   personal16  16 bytes in HOST memory, read before the call returns; NULL = sixteen zero bytes (plain BLAKE2b-512)
 *   r32 a32     n x 32 bytes each, hashed as given (nothing is decoded).  Either may be NULL: that part is then left out of the hash; with
 *               both NULL the call is hash-to-scalar of the messages alone
 *   msgs        offsets == NULL: M_i is the msg_len bytes at msgs + i * msg_len (msg_len may be 0, msgs may then be NULL)
 *               offsets != NULL: n + 1 values in HOST memory, CSR as in jj_msm_ragged (offsets[0] = 0, non-decreasing); M_i is bytes
 *               offsets[i] .. offsets[i + 1] of msgs, msg_len must be 0.  The offsets are read before the call returns (copied to a workspace
 *               the context owns)
 *   c32         n x 32 bytes
 * Pointers may be host or device, mixed freely (offsets and personal16 host only; device pointers must be 16-byte aligned at their BASE --
 * a message inside msgs may start at any byte).  n = 0 succeeds and touches nothing.
 * JJ_ERR_INVALID, before any device work and with c32 untouched: a NULL context; NULL c32 with n > 0; NULL msgs with a non-zero total length;
 * offsets together with msg_len != 0; offsets[0] != 0 or a decreasing pair; offsets in device memory; n > 2^24; more than 2^32 message bytes
 * in all; a misaligned device pointer.
 * Synchronous in the sense of jj_sigverify_each: under the context lock, on the launch stream; a device c32 is written in launch-stream order.
 * NOTHING has to happen between this call with a device c32 and a jj_sigbatch_begin / _keyed_begin / jj_sigbatch_ragged / jj_sigverify_each
 * call that reads it: those calls read their challenges in kernels on the launch stream (k_sig_terms, k_sig_keyed_terms, k_sig_seg_terms,
 * k_sig_each_prep), and the MSM lanes start a job behind everything queued there.
 * Kernel: k_sig_challenge<parts> (jj_kernels.h, jj_blake2b.h), ONE launch over all n, one unit per lane, 256 lanes per workgroup, no workspace
 * beyond the offsets' copy (host arrays are staged like every entry point's).  The state, the 16 message words and the working vector stay in
 * registers: 96 VGPRs (five waves per SIMD), no scratch; one compression is 1962 vector instructions (576 64-bit adds as v_lshl_add_u64, 804
 * v_xor_b32, 576 v_alignbit_b32 for the rotations by 24, 16 and 63; the rotation by 32 is a rename).  A message is read as aligned dwords
 * through a funnel shift, only dwords that hold one of its bytes, so it may start anywhere; in a wave with messages of different lengths the
 * lanes whose message has ended neither compress nor load.  One lane per message is the shape for SHORT messages (a 32- or 64-byte sighash):
 * a kilobyte message serialises eight compressions and more in one lane and reads with a stride of its length across the wave -- the 1 KiB
 * row below.
 * Measured on an MI355X (profiles/sig_challenge_ab.txt: device-resident inputs and result, three alternating rounds of one process per route,
 * median; the old route -- a hashlib.blake2b loop and jj_fr_from_bytes_wide -- on a build of the parent commit):
 *     2^20 units, fixed stride   32-byte messages (one block with R and A)   0.084 ms per call (12.4 G challenges/s)   k_sig_challenge 0.098 ms traced
 *                                64-byte messages (128 bytes: ONE block)     0.083 ms                                  0.093 ms
 *                                96-byte messages (two blocks)               0.150 ms                                  0.171 ms
 *     2^16 units                 32 / 64 / 96 bytes                          0.012 / 0.012 / 0.016 ms                  0.011 / 0.011 / 0.017 ms
 *     2^10 units                 32 / 64 / 96 bytes                          0.012 / 0.012 / 0.016 ms (the launch)
 *     ragged (lengths L/2 .. 3L/2)  2^20: 0.84 ms per CALL for every L, of which the kernel is 0.10 (L = 32) to 0.17 ms (L = 96): the rest is the
 *                                8 MB of host offsets checked and copied; 2^16: 0.062 ms; 2^10: 0.019 ms
 *     2^16 units, 1 KiB messages 0.050 ms fixed stride (nine blocks per lane: 0.095 ns per block, the rate of the one-block rows), 0.103 ms ragged
 *     a caller's loop at 2^20 x 32 bytes: one thread 910 ms (10 800 x the call), 16 processes 101 ms (1 200 x), 113 ms with the copies of
 *     device-resident arrays to the host and of the digests back
 *     hash + check at 2^20, old (16 processes) against new: with jj_sigbatch_begin + jj_msm_finish 122.9 -> 7.24 ms (17.0 x), with
 *     jj_sigverify_each 134.0 -> 18.02 ms (7.4 x): the hash now costs 1 % of the check it feeds.
 * The estimate made before the kernel existed -- 2 500 lane-instructions per block, near 0.1 ms for 2^20 one-block challenges -- holds: 2 538 by
 * that count (1962 issued, a 64-bit add being one instruction here), and the wide reduction's 486 v_mad_i64_i32 on top. */
int jj_sig_challenge(jj_ctx*, size_t n, const void* personal16, const void* r32, const void* a32, const void* msgs, size_t msg_len, const uint64_t* offsets, void* c32);

/* ---- key agreement with ONE secret scalar and its KDF, then one ChaCha20 key per row: a wallet's trial decryption on the device.
 *   share_i  = [sk]P_i, or [8]([sk]P_i) with JJ_KA_COFACTOR, P_i = p32[i] decoded
 *   key32[i] = BLAKE2b(personal16; to_bytes(share_i)), or BLAKE2b(personal16; to_bytes(share_i) || p32[i]) with JJ_KA_HASH_INPUT
 * BLAKE2b as in RFC 7693 with a 32-BYTE digest (parameter word 0x01010020 -- not BLAKE2b-512 cut short), unkeyed, zero salt; the hashed string is
 * 32 or 64 bytes: one compression.  The library still knows no protocol: the personalisation, the decoding rule and the cofactor are the
 * caller's (the Sapling recipient: JJ_DECOMPRESS_ZIP216 | JJ_KA_COFACTOR | JJ_KA_HASH_INPUT with the personalisation "Zcash_SaplingKDF").
 *   sk32        ONE scalar, 32 bytes, host or device: a raw pattern of which the low 252 bits are used, as in jj_varbase_mul.  It is an integer,
 *               never reduced mod r, so the result is exact on the whole curve: points with a torsion component, sk >= r, sk = 0
 *   p32         n x 32 encodings, decoded by the decoder of jj_decompress (k_decompress) under the JJ_DECOMPRESS_ZIP216 | _TORSION_FREE |
 *               _NOT_SMALL_ORDER bits of flags
 *   flags       those three bits | JJ_KA_COFACTOR | JJ_KA_HASH_INPUT; JJ_DECOMPRESS_CLEAR_COFACTOR and any other bit: JJ_ERR_INVALID
 *   personal16  16 bytes in HOST memory, read before the call returns; NULL = sixteen zero bytes
 *   key32 ok    n x 32 bytes and n bytes: ok[i] = 1 and the key, or, where p32[i] fails the decoder's rules, ok[i] = 0 and 32 zero bytes
 * Pointers may be host or device, mixed freely (personal16 host only; device pointers must be 16-byte aligned).  n = 0 succeeds and touches
 * nothing.  JJ_ERR_INVALID, before any device work and with the outputs untouched: a NULL context; flags as above; NULL sk32, p32, key32 or ok
 * with n > 0; a misaligned device pointer.  Synchronous in the sense of jj_sigverify_each: under the context lock, on the launch stream, in
 * chunks of 2^20 units, so the workspace is bounded by the chunk and not by n.
 * CONSTANT-TIME in sk32 and in the share, like jj_varbase_mul: neither the instruction stream nor any memory address depends on them.  The
 * points and the ok bytes are public, and the decoder is the variable-time one of jj_decompress.  What the claim rests on: the source discipline
 * -- the ladder and the y-recovery are the functions of k_varbase_mont, called as they are (masked selects, no table); the one scalar is read
 * through a per-lane address whose uniformity the compiler cannot prove (the same eight dwords in every lane), so that a wave-uniform secret
 * does not become a scalar select or a branch on a bit of the key; the doublings, the normaliser's inversion by divsteps and the one BLAKE2b
 * compression are straight-line code -- and the pinned instruction counts of tests/test_codegen_ka.py: the loop of the new ladder kernel has
 * the conditional-branch count and the v_bfi_b32 count per bit of k_varbase_mont's and no memory access, no scratch, at most 168 VGPRs.  The
 * scalar's device copy is cleared before the call returns its stream to the caller; the shares' encodings stay in the context's workspace
 * until the next call overwrites them.
 * Kernels, per chunk: k_decompress and its flag kernels as they are; k_varbase_mont_x1 as it is; k_varbase_mont_ka<cofactor> beside
 * k_varbase_mont -- ONE unit per lane for every n: there is no quad-of-lanes form, as with jj_varbase_mul2_vartime, so a call of a few units
 * pays the latency of a full ladder --; the shared normaliser writing to_bytes of the share; k_ka_kdf<hash_input>, one unit per lane.
 * k_varbase_mont, its launch and its code are untouched.
 * OUT OF SCOPE: per-unit scalars (the sender's side: they are jj_ka_kdf_each's, behind jj_group_hash below), the note-commitment
 * check that follows a hit, and a _vartime variant.  (Poly1305 and the tag check that decides a hit: jj_aead_open, below.)
 *
 * jj_chacha20_xor: out[i][j] = in[i * in_stride + j] xor byte j of the ChaCha20 keystream (RFC 8439 section 2.3/2.4: 32-bit block counter,
 * 96-bit nonce) of key keys32[i]; out is n x len, dense.
 *   nonce12     12 bytes in HOST memory, read before the call returns; NULL = twelve zero bytes.  ONE nonce for all rows
 *   counter     the block counter of a row's first 64 bytes; byte j is in block counter + j / 64, wrapping modulo 2^32
 *   len         a multiple of 4 in 4..1024;  in_stride  a multiple of 4, >= len;  n * in_stride <= 2^32;  in and out must not overlap
 * Any violation (and a NULL context; NULL keys32, in or out with n > 0; a misaligned device pointer) returns JJ_ERR_INVALID before any work,
 * with out untouched.  n = 0 succeeds and touches nothing.  Pointer, lock and stream rules are those of jj_ka_kdf.  NOTHING has to happen
 * between jj_ka_kdf with a device key32 and this call reading it as keys32: both run their kernels on the launch stream.
 * Kernel k_chacha20_xor (jj_chacha20.h), ONE launch, one row per lane: the 16 state words and the 16 working words in registers, the 20 rounds
 * unrolled, each rotation one v_alignbit_b32, no scratch; rows are read and written as aligned dwords (what the multiple-of-4 rule buys at
 * every skew), and nothing is read past a row's len bytes.  The compact-note shape is len = in_stride = 52, counter = 1: one block; the 564
 * bytes of a full note ciphertext are nine.
 * Measured on an MI355X (profiles/ka_kdf_ab.txt: device-resident inputs and results, three alternating rounds of one process per route, median; the
 * old route on a build of the parent commit): 2^20 units of the Sapling recipient's shape 14.28 ms per jj_ka_kdf call (73.4 M keys/s), 14.43 ms with
 * the cipher at len 52 behind it, against 14.39 ms for the four-call composed route (jj_decompress, jj_varbase_mul with the scalar written n times,
 * jj_point_mul_by_cofactor, jj_compress), which has NO hash, 165 ms with the shares hashed by hashlib in 16 processes and 529 ms in one thread; 2^16:
 * 1.688 against 1.705 ms (6.9 ms with 16 hashing processes).  Traced kernels of one 2^20 call: k_decompress<8> 2.3 ms, k_varbase_mont_x1 0.17,
 * k_varbase_mont_ka<true> 12.3 - 14.2 over four traced calls, k_normalize<16> 0.11, k_ka_kdf<true> 0.06, k_chacha20_xor 0.13.  BEHIND at small n: 2^10 units take 1.244 ms against 0.744 ms for the
 * composed route, whose ladder runs one scalar multiplication per quad of lanes up to vb_quad_max units at a third of the latency; this call has no
 * such form.  With the hash a caller needs the old route is 1.21 ms there: level. */
#define JJ_KA_COFACTOR   32u   /* share = [8]([sk]P) instead of [sk]P */
#define JJ_KA_HASH_INPUT 64u   /* hash share32 || p32[i] instead of share32 alone */
int jj_ka_kdf(jj_ctx*, size_t n, const void* sk32, const void* p32, unsigned flags, const void* personal16, void* key32, uint8_t* ok);
int jj_chacha20_xor(jj_ctx*, size_t n, const void* keys32, const void* nonce12, unsigned counter, const void* in, size_t len, size_t in_stride, void* out);

/* ---- Poly1305 and the ChaCha20-Poly1305 AEAD of RFC 8439, one key per row, the tag checked on the device: the step of a trial decryption
 * that decides whether there was a hit.
 *   jj_poly1305   tag16[i] = Poly1305(keys32[i]; the len bytes at in + i * in_stride) (RFC 8439 section 2.5): keys32[i] is the ONE-TIME key,
 *                 r in bytes 0..15 (clamped by the library), s in bytes 16..31.  tag16 is n x 16, dense
 *   jj_aead_seal  out[i] = the ciphertext of the len bytes at in + i * in_stride under key keys32[i], followed by its 16-byte tag (section
 *                 2.8): out is n x (len + 16), dense
 *   jj_aead_open  the row at in + i * in_stride is len ciphertext bytes followed by the 16 tag bytes.  ok[i] = 1 and out[i] = the len
 *                 plaintext bytes where the tag verifies; ok[i] = 0 and out[i] = len ZERO bytes where it does not: a failed row never holds
 *                 plaintext when the call returns.  out is n x len, dense
 * The AEAD as the RFC has it: the one-time key is the first 32 bytes of ChaCha20 block 0 of (keys32[i], nonce12), the data stream starts at
 * block 1, the MAC runs over aad || pad16 || ciphertext || pad16 || le64(aad_len) || le64(len).
 *   nonce12     12 bytes in HOST memory, read before the call returns; NULL = twelve zero bytes.  ONE nonce for all rows
 *   aad         aad_len <= 64 bytes in HOST memory, read before the call returns, the same for all rows; NULL only with aad_len = 0
 *   len         a multiple of 4 in 4..1024;  in_stride  a multiple of 4, >= len (jj_poly1305, jj_aead_seal) or >= len + 16 (jj_aead_open);
 *               n * in_stride <= 2^32;  in and out (tag16) must not overlap: that is checked and refused.  keys32 and ok must not overlap in, out
 *               or each other either: that is the caller's to keep, as with the neighbouring calls, and is not checked
 * Any violation (and a NULL context; NULL keys32, in, out, tag16 or ok with n > 0; a misaligned device pointer) returns JJ_ERR_INVALID before
 * anything is staged or launched, with the outputs untouched.  n = 0 succeeds and touches nothing.  All other pointers may be host or device,
 * mixed freely (device pointers 16-byte aligned); a host `in` is staged as exactly the bytes that are read, (n - 1) * in_stride + len, plus 16
 * for jj_aead_open.  Lock and stream rules are those of jj_ka_kdf: NOTHING has to happen between jj_ka_kdf with a device key32 and one of
 * these calls reading it as keys32 -- both run their kernels on the launch stream, and the keys never have to leave the device.
 * The Sapling shapes: len 564 in a stride of 580 for a note ciphertext, len 64 in a stride of 80 for an out ciphertext, empty aad, zero nonce.
 * Both lengths are multiples of 4, which is why the multiple-of-4 rule costs nothing there.
 * TIMING: neither the instruction stream nor any memory address depends on keys, data, tags or verdicts.  Poly1305 is five 26-bit limbs in
 * registers, 25 v_mad_u64_u32 per block with 5 r precomputed (jj_poly1305.h shows why no column overflows), its final reduction complete
 * (h in [p, 2^130) comes out as h - p) and mask-selected; the tag is compared as an OR over the four xored words without an early exit, and the
 * plaintext words are ANDed with 0 - ok instead of being branched on, so the verdict costs no divergence where nearly every row fails.  Every
 * loop bound and predicate is a function of len and aad_len, the same in every lane.  tests/test_codegen_aead.py pins this on the gfx950
 * assembly: no scratch, at most 128 VGPRs, no sub-dword load, no lane-dependent branch or select behind the tag comparison.
 * Kernels (jj_poly1305.h), ONE launch each, one row per lane, aligned dwords only, the row offset formed in 64 bits, nothing read or written
 * outside a lane's own row: k_poly1305; k_aead<false> (open: the MAC over the ciphertext first, 16 words loaded per step, then the keystream
 * pass with the masked store -- the row is read twice); k_aead<true> (seal: the words are absorbed as they are produced).  The aad travels
 * zero-padded as a kernel argument.
 * Measured on an MI355X (profiles/aead_ab.txt: device-resident inputs and results, three alternating rounds of one process per route, median):
 * 2^20 full-note rows (len 564 in a stride of 580): jj_aead_open 1.212 ms, jj_aead_seal 0.860 ms, jj_poly1305 0.582 ms; 2^16 rows: 0.063, 0.057 and
 * 0.020 ms; 2^10 rows: 0.042, 0.038 and 0.011 ms.  jj_chacha20_xor at the same len and stride on the same build takes 4.488 ms per 2^20 rows
 * (0.093 at 2^16, 0.050 at 2^10): the call with the MAC and the second read is the faster one.  Supposed cause, not measured: this call issues a
 * step's 16 loads before the block function, while k_chacha20_xor's assembly alternates load, wait and store (that kernel is left as it is).
 * Engine.ka_open_aead, jj_ka_kdf then this call: 16.116 ms against 14.439 ms for jj_ka_kdf alone per 2^20 rows (11.6 % over the key agreement),
 * 1.776 against 1.673 ms at 2^16, 1.293 against 1.246 ms at 2^10.  The host route -- keys and rows copied out, EVP_chacha20_poly1305 of libcrypto
 * through ctypes -- takes 1675.9 ms with 16 processes and 2995.5 ms in one thread per 2^20 rows, 90.2 ms per 2^16 and 3.2 ms per 2^10: nothing is
 * BEHIND.  Bytes moved per row over the time: 1521 GB/s for jj_aead_open at 2^20, about a quarter of the 6 TB/s of HBM; the row-per-lane strided
 * reads look like the limit rather than the arithmetic, which is a supposition from that rate (no counters were read).
 * OUT OF SCOPE: per-unit scalars on the sender's side (jj_ka_kdf_each and jj_blake2b make the keys this call opens and seals with), the
 * note-commitment check that follows a hit, per-row nonces or aad, and a len that is not a multiple of 4. */
int jj_poly1305(jj_ctx*, size_t n, const void* keys32, const void* in, size_t len, size_t in_stride, void* tag16);
int jj_aead_open(jj_ctx*, size_t n, const void* keys32, const void* nonce12, const void* aad, size_t aad_len, const void* in, size_t len, size_t in_stride, void* out,
                 uint8_t* ok);
int jj_aead_seal(jj_ctx*, size_t n, const void* keys32, const void* nonce12, const void* aad, size_t aad_len, const void* in, size_t len, size_t in_stride, void* out);

/* ---- BLAKE2s-256 over prefix || M_i, and the hash to the curve built on it: a protocol's generators, the diversified base of a note.
 *   digest_i  = BLAKE2s-256(personal8; prefix || M_i), M_i the msg_len bytes at msgs + i * msg_stride
 *   jj_blake2s     out32[i] = digest_i
 *   jj_group_hash  out64[i], ok[i] = byte for byte what jj_decompress writes for digest_i under `flags`: the four JJ_DECOMPRESS_* bits with their
 *                  meaning there, no other bit; a refused row gets (0, 0) and ok = 0
 * BLAKE2s as in RFC 7693: unkeyed, 32-byte digest, zero salt, parameter word 0x01010020, the 8 bytes of personalisation in h[6] and h[7].
 * The library knows NONE of a protocol's personalisations or prefixes, and no message layout or decoding rule: all of them are the caller's
 * (the group hash of the Zcash protocol specification, GroupHash(D, M) = [8] * decode(BLAKE2s-256(D; URS || M)), is personal8 = D, prefix =
 * URS, flags = JJ_DECOMPRESS_ZIP216 | JJ_DECOMPRESS_NOT_SMALL_ORDER | JJ_DECOMPRESS_CLEAR_COFACTOR).
 *   personal8   8 bytes in HOST memory, read before the call returns; NULL = eight zero bytes
 *   prefix      prefix_len bytes (0..4096) in HOST memory, read before the call returns; NULL only when prefix_len = 0
 *   msgs        rows of msg_len bytes (0..65536, ONE length per call) at a stride of msg_stride >= msg_len, ANY byte value: rows may begin at
 *               any byte; NULL only when msg_len = 0;  n * msg_stride <= 2^32;  n <= 2^24
 *   out32       n x 32 bytes;   out64, ok   n x 64 bytes and n bytes
 * msgs, the outputs and ok may be host or device pointers, mixed freely (device pointers 16-byte aligned at their base).  n = 0 succeeds and
 * touches nothing.  JJ_ERR_INVALID, before any device work and with the outputs untouched: a NULL context; a NULL output with n > 0; flag bits
 * other than the four; a length, stride or count outside the bounds above; a NULL prefix or msgs that would be read; a misaligned device pointer.
 * Synchronous in the sense of jj_sigverify_each: under the context lock, on the launch stream, in chunks of 2^20 units like jj_ka_kdf; the
 * digests of jj_group_hash live in a context workspace of 32 bytes per unit of a chunk.  NOTHING has to happen between jj_blake2s with a device
 * out32 and a later call that reads it.
 * VARIABLE-TIME over public inputs, like jj_decompress: the decoder behind the hash is that variable-time one, and the block loop runs by the
 * (public) lengths.
 * Kernel k_blake2s (jj_blake2s.h), one message per lane, ONE launch per chunk: 32-bit words, the message schedule resolved at compile time so
 * that h, m and v stay in registers (no scratch), each rotation one v_alignbit_b32, 10 rounds.  The whole blocks of the prefix -- the same for
 * every lane -- are compressed ONCE on the host, never a block that could be the final one; the kernel gets the midstate, t and the prefix's
 * tail as arguments.  A lane's message follows the tail at any byte offset and is read as aligned dwords through a funnel shift, never outside
 * the dwords that hold a byte of its own row.  jj_group_hash then runs the decoder chain of jj_decompress (decompress_dev: k_decompress, the
 * flag kernels, the shared normaliser, k_mask_outputs) on the chunk's digests as it is.  There is NO fused hash-and-decode kernel: the decoder
 * is about 2 ms per 2^20 units, one block of this hash below 0.1 ms, and the 64 MB of digest traffic a fused form would save a few tens of
 * microseconds.
 * OUT OF SCOPE: ragged message lengths, other digest lengths, keyed or salted BLAKE2s, the rest of a note-commitment check, a jj_multi_* form.
 * Measured on an MI355X (profiles/group_hash_ab.txt: messages and results on the device, three alternating rounds of one process per route, median;
 * the old route on a build of the parent commit), a 64-byte prefix with 11-byte messages and the flags of the Zcash group hash: 2^20 rows 2.192 ms per
 * jj_group_hash call (478 M rows/s) against 2.146 ms for jj_decompress alone on ready digests -- the hash adds 0.047 ms (0.058 ms with 32-byte messages),
 * as expected before the run: near the traced k_blake2s (0.046 - 0.054 ms) and below the 0.084 ms of k_sig_challenge for one BLAKE2b block -- and
 * against 105.6 ms for hashlib in 16 processes + jj_decompress (490 ms in one thread); 2^16: 0.688 against 4.71 ms; 2^10: 0.301 against 0.750 ms.
 * jj_blake2s alone: 0.038 ms per call of 2^20 rows in a full queue (back-to-back calls with device outputs, one synchronisation at the end:
 * throughput, 27.7 G rows/s, not the latency of one call). */
int jj_blake2s(jj_ctx*, size_t n, const void* personal8, const void* prefix, size_t prefix_len, const void* msgs, size_t msg_len, size_t msg_stride, void* out32);
int jj_group_hash(jj_ctx*, size_t n, const void* personal8, const void* prefix, size_t prefix_len, const void* msgs, size_t msg_len, size_t msg_stride, unsigned flags,
                  void* out64, uint8_t* ok);

/* ---- the sender's side of a note: raw BLAKE2b digests over rows gathered from several arrays, and the key agreement with one secret scalar
 * PER ROW.  With them the ciphertexts of n outputs can be created, and sent notes recovered with an outgoing viewing key, without a key or
 * a share visiting the host.  The library still knows no protocol: personalisations, decoding flags and layouts remain the caller's.
 *
 * jj_blake2b: out[i] = BLAKE2b-digest_len(personal16; prefix || S_0[i] || .. || S_{nsrc-1}[i]), S_s[i] the lens[s] bytes at
 * srcs[s] + i * strides[s].  BLAKE2b as in RFC 7693: unkeyed, zero salt, parameter word 0x01010000 | digest_len -- BLAKE2b-256 is its own
 * hash, not BLAKE2b-512 cut short --, the 16 bytes of personalisation in h[6] and h[7].  out is n x digest_len, dense.
 *   digest_len  32 or 64; any other value is refused
 *   personal16  16 bytes in HOST memory, read before the call returns; NULL = sixteen zero bytes
 *   prefix      prefix_len bytes in HOST memory, read before the call returns; prefix_len 0..4096 and a multiple of 4; NULL only with length 0
 *   nsrc        0..4; with 0 every row gets the digest of the prefix alone
 *   srcs, lens, strides   HOST arrays of nsrc entries.  lens[s] a multiple of 4 in 4..65536; strides[s] a multiple of 4, >= lens[s], and
 *               n * strides[s] <= 2^32;  n <= 2^24.  One array may serve several sources
 * The sources and out may be host or device pointers, mixed freely; device pointers are 16-byte aligned.  A host source is staged as exactly
 * the (n - 1) * stride + len bytes that are read.  out must not overlap a source: that is checked and refused.
 * Every violation returns JJ_ERR_INVALID before anything is staged or launched, with out untouched: a NULL context, a NULL out or source with
 * n > 0, a misaligned device pointer, and srcs, lens, strides, prefix or personal16 in device memory among them.  n = 0 succeeds and touches
 * nothing.  The lock and stream rules are those of jj_ka_kdf: NOTHING has to happen between this call writing a device out and jj_aead_open or
 * jj_aead_seal reading it as keys32.
 * TIMING: nothing in the instruction stream or in any address depends on the data -- the prefix may be a viewing key --; the block loop runs by
 * the lengths, which are the same in every lane.
 * Kernel k_blake2b<32|64> (jj_blake2b.h: Blake2bRows on top of the compression and the rotations of k_sig_challenge's Blake2bT, reused as they
 * are), one row per lane, ONE launch.  The whole blocks of the prefix are compressed ONCE on the host, never a block that could be the final
 * one; the kernel gets the midstate, t, the prefix's tail and a per-call piece plan (which source, which byte offset, how many dwords) as
 * arguments.  Every length is the same in every lane, so the block loop, the piece boundaries and the final-block flag are uniform; every
 * index into m[] is a compile-time constant (no scratch); rows are read as aligned dwords, never outside a lane's own lens[s] bytes, and the
 * row offsets are formed in 64 bits.  tests/test_codegen_ovk.py pins on the gfx950 assembly: no scratch, at most 128 VGPRs, v_alignbit_b32
 * rotations, no sub-dword load.
 * The ock shape of Sapling: digest_len 32, prefix = the 32 bytes of ovk, three sources of 32 bytes (cv, cmu, epk): one compression per row.
 *
 * jj_ka_kdf_each: exactly jj_ka_kdf, with these differences:
 *   sk32   n x 32, host or device: each row is read as jj_varbase_mul reads a scalar, the low 252 bits, an integer never reduced mod r
 *   h32    with JJ_KA_HASH_INPUT the second hashed part is h32[i] (n x 32) when h32 is not NULL and p32[i] when it is NULL: the sender hashes
 *          share_i || epk_i, and epk_i is not the point that was multiplied (that is pk_d_i).  A non-NULL h32 without that flag: JJ_ERR_INVALID
 * The decoder bits, JJ_KA_COFACTOR, the ok and zero-key rule, the chunks of 2^20 units, the pointer rules and the refusals (JJ_ERR_INVALID before
 * any device work, the outputs untouched; n = 0 succeeds and touches nothing) are jj_ka_kdf's.
 * CONSTANT-TIME in the scalars and in the shares, on the same grounds as jj_ka_kdf: the ladder and the recovery are the functions of
 * k_varbase_mont called as they are, the scalars are loaded per lane as k_varbase_mont loads them, and tests/test_codegen_ovk.py holds the
 * loop of the new kernel to k_varbase_mont's counts of conditional branches, v_bfi_b32 and v_mad_i64_i32 per bit, with no v_cndmask, no scalar
 * select, no memory access and no call in it, no scratch, at most 168 VGPRs.  A host sk32 passes through a staging slot of the context on the
 * device; those n x 32 bytes are cleared on the launch stream behind the last chunk, as jj_ka_kdf clears its one scalar.  (An array of 1 MB and
 * more also passes through the context's page-locked HOST slots, which are host memory like the caller's own array and are not cleared.)
 * Kernels, per chunk: jj_ka_kdf's, with k_varbase_mont_ka_each<cofactor> in the place of k_varbase_mont_ka; k_ka_kdf<true> is launched with
 * h32 in the place of p32.  k_varbase_mont, k_varbase_mont_ka, k_varbase_mont_x1, k_ka_kdf and their launches are untouched.
 * OUT OF SCOPE: compaction of hit rows through the C ABI (Engine.ovk_open gathers them with index operations of numpy or torch), a
 * quad-of-lanes form for small n, ragged lengths, keyed or salted BLAKE2b, digest lengths other than 32 and 64, per-row nonces, and a
 * jj_multi_* form.
 * Measured on an MI355X (profiles/ovk_ab.txt, tools/ovk_ab.py: device-resident inputs and results, three alternating rounds of one process per
 * route, median; host-clock time per call over a window of back-to-back calls, so a figure below the launch latency is throughput, not the
 * latency of one call; the expectation stands in the file above the numbers, written before the run).  jj_blake2b at the ock shape: 0.099 ms
 * per 2^20 rows (10.6 G rows/s) -- the expectation was the 0.084 ms of the traced one-block k_sig_challenge: one compression, four times the
 * loads --, 0.015 ms at 2^16 and at 2^10; with jj_aead_open at len 64 in a stride of 80 behind it, the per-output cost of an ovk rescan,
 * 0.202 ms per 2^20 (5.2 G outputs/s), 0.028 ms at 2^16 and 2^10; hashlib over the same 128-byte rows: 318 ms per 2^20 in one thread, 213 ms
 * in 16 processes.  jj_ka_kdf_each: 14.293 ms per 2^20 rows [14.291 .. 14.308] against 14.507 ms for the composed five-call route on the same
 * build (jj_decompress, jj_varbase_mul, jj_point_mul_by_cofactor, jj_compress, jj_blake2b) and 14.411 ms for the parent commit's four-call
 * route without any hash: AHEAD of both by more than the larger range; 2^16: 1.640 against 1.716 and 1.700 ms, AHEAD.  BEHIND at 2^10: 1.208 ms
 * against 0.752 and 0.744 ms -- jj_varbase_mul has a quad-of-lanes ladder up to vb_quad_max units and this call has none, as expected. */
int jj_blake2b(jj_ctx*, size_t n, int digest_len, const void* personal16,
               const void* prefix, size_t prefix_len,
               int nsrc, const void* const* srcs, const size_t* lens, const size_t* strides,
               void* out);
int jj_ka_kdf_each(jj_ctx*, size_t n, const void* sk32, const void* p32, const void* h32,
                   unsigned flags, const void* personal16, void* key32, uint8_t* ok);

/* ---- windowed Pedersen hashes: one launch for n units, every segment in one accumulator.  VARIABLE-TIME (public inputs): the table address
 * depends on the message; a caller with secret inputs composes jj_pedersen_scalars with jj_fixedbase_multi_mul on the LDS tables.
 * A message M is `prefix_bits` bits of `prefix` (low bits first), then up to four fields of the unit's row; every bit is taken LSB-first within
 * its byte.  M is padded with zero bits to a multiple of 3 and cut into chunks (s0, s1, s2) in message order,
 *     enc = (1 - 2 s2)(1 + s0 + 2 s1)  in +-{1..4};   segment j takes chunks j c .. j c + c - 1, c = seg_chunks (the last takes what is left);
 *     <M_j> = sum_i enc(m_i) 16^i   (|<M_j>| <= 4 (16^63 - 1) / 15 < (r - 1) / 2);        H(M) = sum_j [<M_j>] P_j.
 * The empty message gives the identity; a chunk that is not there contributes nothing (it is not a zero chunk: 000 encodes +1).  The library
 * knows no protocol: generators, chunks per segment and prefix are the caller's (for the hash of the Zcash protocol specification section
 * 5.4.1.7: seg_chunks = 63, its generators; a Merkle layer over a buffer of node u-coordinates is ONE call with rows = the nodes, row_stride
 * = 64, fields = {0, 255, 32, 255}, prefix = the layer number, prefix_bits = 6, and its 32-byte output rows are the next layer's rows of 64).
 * jj_pedersen_table_create
 *   nseg 1..8, seg_chunks 1..63, window_chunks 1..4 or 0 = the default (4)
 *   gens64   nseg affine points, host or device; each must be on the curve and torsion-free, else JJ_ERR_INVALID -- the integer sum and the
 *            sum over scalars reduced mod r are then the same point
 *   The table holds, per segment and window of w = window_chunks chunks (windows never straddle a segment; the last is shorter), sub-tables for
 *   t = 1 .. w present chunks of 2^(3t - 1) entries, 128 bytes each (layout: jj_pedersen.h): 4 + 32 + 256 + 2048 entries per window at w = 4,
 *   106 176 entries = 13.6 MB for three segments of 63.  Built by jj_varbase_mul on host-made scalars and k_affine_to_table; freed by
 *   jj_fixedbase_table_destroy.  Every other entry point that takes a jj_table refuses a Pedersen table with JJ_ERR_INVALID.
 * jj_pedersen_hash_vartime
 *   fields   HOST array of 2 * nfields values (byte_offset, nbits), nfields 0..4: field f of unit i is nbits bits from byte
 *            rows + i * row_stride + byte_offset; nbits >= 1, byte_offset + ceil(nbits / 8) <= row_stride; fields may overlap.  The whole
 *            range is honoured: byte_offset up to 2^32 - 1 and a field that ends at byte 2^32 of the call's array (row_stride = 2^32, n = 1)
 *   rows     host or device (16-byte aligned); row_stride <= 2^32 and n * row_stride <= 2^32; may be NULL when nfields = 0
 *   the message (prefix_bits + sum nbits, ONE length per call) must fit 3 * seg_chunks * nseg bits
 *   flags    0: out is n x 32 bytes, the canonical u-coordinate;  JJ_PEDERSEN_POINT: n x 64 affine bytes
 *   JJ_ERR_INVALID before anything is staged or launched, out untouched: a table that is not a Pedersen table, prefix_bits outside 0..32, nfields
 *   outside 0..4, a field past row_stride, a message over capacity, unknown flags, a misaligned device pointer.  n = 0 succeeds and touches nothing.
 *   Kernel k_pedersen_gather (jj_kernels.h): one unit per lane, the walk of k_fixedbase_gather with the message's own bits as the digit; the
 *   per-window plan (which bytes, what shift, where a field ends -- the same for every unit) is made on the host and read with uniform
 *   addresses; rows are read as aligned dwords through a funnel shift, never beyond the last dword that holds a covered byte of the lane's own
 *   row.  Then the shared normaliser, and k_affine_u for the u-only form.  139 VGPRs, no scratch.
 *   Measured on an MI355X (profiles/pedersen_ab.txt: rows and results on the device, three alternating rounds of one process per route, median):
 *   2^20 hashes of the Merkle shape (516 bits, 44 additions) 2.097 ms per call at window_chunks 4 (500 M hashes/s; 2.68 ms at 3, 3.97 ms at 2),
 *   against 2.496 ms for jj_pedersen_scalars + jj_fixedbase_multi_mul over three 16-bit gathered tables (201 MB), 5.56 ms over the default LDS
 *   tables, and 2128 ms for a caller that encodes the scalars in numpy; 2^16: 0.219 ms; 2^10: 0.211 ms (44 dependent additions).  The 576-bit
 *   one-field shape (four segments): 2.364 against 3.294 ms.
 * jj_pedersen_scalars
 *   writes <M_j> mod r as canonical Fr bytes, (nseg, n, 32) -- the layout jj_fixedbase_multi_mul reads; a segment the message does not reach
 *   gets 0.  The composed device route and the cross-check of the fused kernel: jj_fixedbase_multi_mul over these scalars with tables of the
 *   same generators gives the bytes of jj_pedersen_hash_vartime(JJ_PEDERSEN_POINT).  Kernel k_pedersen_scalars, one (unit, segment) per lane. */
#define JJ_PEDERSEN_POINT 1u
int jj_pedersen_table_create(jj_ctx*, int nseg, const void* gens64, int seg_chunks, int window_chunks /* 0 = default */, jj_table** out);
int jj_pedersen_hash_vartime(jj_ctx*, const jj_table* t, size_t n, unsigned prefix, int prefix_bits,
                             const void* rows, size_t row_stride, int nfields, const uint32_t* fields, unsigned flags, void* out);
int jj_pedersen_scalars(jj_ctx*, int nseg, int seg_chunks, size_t n, unsigned prefix, int prefix_bits,
                        const void* rows, size_t row_stride, int nfields, const uint32_t* fields, void* scalars32);

/* ---- windowed Pedersen commitment over several row arrays:  out[i] = H(M_i) + [r_i] R  in one call.  VARIABLE-TIME in the message.
 * H is exactly the function of jj_pedersen_hash_vartime over `ped` (a table of jj_pedersen_table_create, any window_chunks).  M_i is prefix_bits
 * bits of `prefix` (low bits first), then up to four fields; field f is nbits bits from byte srcs[src] + i * strides[src] + byte_offset, LSB-first
 * within a byte.  Fields come in the order given, which need not be source order; a source may serve several fields; fields may overlap.
 *   ped      a Pedersen table;  rbase  the table of ONE base R, any table jj_fixedvar_mul_vartime accepts (every window_bits; a composite or a
 *            Pedersen table is refused);  r32  n x 32 raw bytes, read exactly as jj_fixedbase_mul reads its scalars (the low 252 bits)
 *   rbase == NULL together with r32 == NULL: the plain multi-source hash (with nsrc = 1 the bytes of jj_pedersen_hash_vartime); exactly one of
 *            the two being NULL is refused
 *   srcs, strides   HOST arrays of nsrc pointers / byte strides, nsrc 1..4 (0 only with nfields = 0); every source host or device (16-byte
 *            aligned), mixed freely; strides[s] <= 2^32 and n * strides[s] <= 2^32.  A host source is read up to the last byte its fields cover
 *            in its last row, a device source up to the end of the aligned dword of that byte
 *   fields   HOST array of 3 * nfields values (src, byte_offset, nbits), nfields 0..4: src < nsrc, nbits >= 1,
 *            byte_offset + ceil(nbits / 8) <= strides[src]; the message must fit 3 * seg_chunks * nseg bits; prefix_bits 0..32
 *   flags    0: out is n x 32 bytes, the canonical u-coordinate (Extract of the Zcash specification);  JJ_PEDERSEN_POINT: n x 64 affine bytes;
 *            any other bit is refused
 * The contract: for every kind of rbase every unit equals, byte for byte, the composed route on rows packed by the caller,
 *     jj_point_add(jj_pedersen_hash_vartime(.., JJ_PEDERSEN_POINT) on the packed rows, jj_fixedbase_mul(rbase, r)).
 * The Edwards law is complete: H(M) = -[r]R gives the identity (u = 0 in the u-only form), H(M) = [r]R takes no special path.
 * Every limit above is refused with JJ_ERR_INVALID before anything is staged or launched, out untouched; so are a table of another device and a
 * misaligned device pointer.  n = 0 succeeds and touches nothing.  The lock and stream rules are those of jj_pedersen_hash_vartime.
 * Kernel k_pedersen_commit (jj_kernels.h), beside k_pedersen_gather: one unit per lane, one accumulator; a piece of the host-made plan names
 * its source, the lane forms its row position and the clamp dword per source, and the funnel-shift rule of jj_pedersen_hash_vartime holds for
 * each source separately.  What depends on r:
 *   gathered rbase (window_bits 8..16)  the same kernel goes on in the same registers with the walk of k_fixedbase_gather (the recode addition,
 *       ceil(253 / w) signed entries, the first fetched before the message's last addition): VARIABLE-TIME in r as well
 *   LDS rbase (window_bits 6, 7, the default)  the kernel stops after the message and the table's own kernel finishes on the accumulator it left
 *       (the shape of jj_fixedvar_mul_vartime's LDS route): the blinding term is CONSTANT-TIME in r
 * Then the shared normaliser once, and k_affine_u for the u-only form.  No scratch.
 * NOT MEASURED YET: tools/commit_ab.py is written and its routes are held to the restatement, but profiles/commit_ab.txt does not exist --
 * the fused walk ships for gathered tables on the expectation alone 
 * (the shipped figures: 2.36 ms per 2^20 for the 576-bit four-segment hash, about 0.9 ms for a gathered fixed-base walk, so about 3 ms fused against about 4 ms composed), 
 * and the project's rule (fused only if ahead of the two-launch form by more than the larger range; BEHIND written where a size is behind) is still to be applied to a run.
 * Real hits are rare: the rate of this check matters for rescans and for callers who check every output they created.
 * The library knows no protocol.  The documented example is a note commitment: ped of four segments of 63 chunks, prefix 0b111111 (6 bits),
 * fields {0, value_offset, 64,  1, 0, 256,  2, 0, 256} over the plaintext rows, repr(g_d) and repr(pk_d): 582 bits, 194 chunks.
 * OUT OF SCOPE: a constant-time message term (compose jj_pedersen_scalars with jj_fixedbase_multi_mul), multi-source jj_pedersen_scalars,
 * compaction of hit rows, a jj_multi_* form. */
int jj_pedersen_commit_vartime(jj_ctx*, const jj_table* ped, const jj_table* rbase, size_t n,
                               unsigned prefix, int prefix_bits,
                               int nsrc, const void* const* srcs, const size_t* strides,
                               int nfields, const uint32_t* fields /* triples (src, byte_offset, nbits) */,
                               const void* r32, unsigned flags, void* out);

/* ---- encodings----------------------------------------------------------------------------------------- */
#define JJ_DECOMPRESS_ZIP216          1u  /* reject the two non-canonical encodings (src/lib.rs:469-471, 522-531) */
#define JJ_DECOMPRESS_TORSION_FREE    2u  /* additionally require [r]P = O  (SubgroupPoint::from_bytes, lib.rs:1427-1429) */
#define JJ_DECOMPRESS_NOT_SMALL_ORDER 4u  /* additionally reject small-order points (lib.rs:699-705) */
#define JJ_DECOMPRESS_CLEAR_COFACTOR  8u  /* return [8]P (lib.rs:722-724, 1343-1345) */
/* AffinePoint::from_bytes / from_bytes_pre_zip216_compatibility / batch_from_bytes (src/lib.rs:469-627) */
int jj_decompress(jj_ctx*, size_t n, const void* in32, unsigned flags, void* out64, uint8_t* ok);
/* AffinePoint::to_bytes src/lib.rs:455-464 */
int jj_compress(jj_ctx*, size_t n, const void* points64, void* out32);
/* batch_normalize src/lib.rs:1084-1107: n x 160 bytes (U,V,Z,T1,T2 canonical LE) -> n x 64 bytes affine.  A row with Z = 0 (mod q)
 * yields (0, 0) and leaves the other rows alone, as ff's BatchInverter does; coordinates of q or more are reduced mod q, as in the
 * field entry points; T1 and T2 are not read. */
int jj_batch_normalize(jj_ctx*, size_t n, const void* ext160, void* out64);


/* ---- synthetic inputs (Group::random semantics; counter-based, reproducible on any device or on the host) ---- */
/* scalars[i] = four splitmix64 words of the stream seed + (first_index + i) * 4 + j, top 4 bits cleared, minus r if >= r:
 * canonical Fr elements (the input side of Field::random, src/fr.rs:684-688, with a counter-based generator). */
int jj_synth_scalars(jj_ctx*, size_t n, uint64_t seed, uint64_t first_index, void* out32);
/* the same four words per unit as they come (arbitrary 256-bit patterns: values >= q, sign-bit noise for the decoder) */
int jj_synth_bytes32(jj_ctx*, size_t n, uint64_t seed, uint64_t first_index, void* out32);
/* ExtendedPoint::random (src/lib.rs:1244-1267): v = Fq::random (64 PRNG bytes through from_bytes_wide), flip = next_u32 % 2,
 * u = sqrt((v^2 - 1) / (1 + d v^2)) or draw again, (flip ? -u : u, v), draw again if it is the identity.  subgroup != 0:
 * SubgroupPoint::random (src/lib.rs:1290-1298), i.e. [8]P, drawn again if that is the identity.  Unit i reads the
 * splitmix64 stream seed + ((first_index + i) << 16) + 16 * attempt + {0..7: v, 8: flip}.  attempts (optional): draws used. */
int jj_random_points(jj_ctx*, size_t n, uint64_t seed, uint64_t first_index, int subgroup, void* out64, uint32_t* attempts);


/* ---- several devices of one node ---------------------------------------------------------- */
/* One context per listed device, one host thread + stream per device, contiguous shards [g*n/G, (g+1)*n/G); no data-path
 * collective for the independent-batch workloads (north_star: "shard embarrassingly across the 8 GPUs of one node").
 * jj_multi_msm: every device reduces its own terms to a record of partial window sums (jj_msm_partial); the records of all
 * devices meet in one host tail on the calling thread (jj_msm_combine).  Array arguments are HOST pointers (a device pointer is JJ_ERR_INVALID).  A device may be listed
 * more than once.  Processes that keep their batches resident in HBM run one process per GPU instead and exchange the MSM
 * records with an RCCL all_gather: jj_ctx_set_comm + jj_msm_allgather above (C / C++ / Rust: examples/msm_rccl.cpp), or
 * jubjub_amd/dist.py over torch.distributed.  A jj_ctx may be used from several host threads: its entry
 * points serialise on a per-context lock. */
typedef struct jj_multi jj_multi;
typedef struct jj_mtable jj_mtable;
int jj_multi_create(const int* devices, int ndev, jj_multi** out);
int jj_multi_destroy(jj_multi* m);
int jj_multi_device_count(jj_multi* m);
jj_ctx* jj_multi_ctx(jj_multi* m, int index);            /* the per-device context, for the single-device entry points */
const char* jj_multi_last_error(jj_multi* m);
int jj_multi_varbase_mul(jj_multi* m, size_t n, const void* scalars32, const void* points64, void* out64);
int jj_multi_fixedbase_table_create(jj_multi* m, const void* base64, int window_bits, jj_mtable** out);   /* replicated per device */
int jj_multi_fixedbase_table_destroy(jj_multi* m, jj_mtable* t);
int jj_multi_fixedbase_mul(jj_multi* m, const jj_mtable* t, size_t n, const void* scalars32, void* out64);
int jj_multi_decompress(jj_multi* m, size_t n, const void* in32, unsigned flags, void* out64, uint8_t* ok);
int jj_multi_msm(jj_multi* m, size_t n, const void* scalars32, const void* points64, void* out64);
/* jj_msm_batch over the devices: contiguous blocks of rows, one block per device, no exchange between devices (shared points go
 * to every device).  HOST pointers, like the other jj_multi_* calls; a device may receive no rows (B smaller than the device count). */
int jj_multi_msm_batch(jj_multi* m, size_t B, size_t n, const void* scalars32, const void* points64, int points_shared, void* out64);
/* Last step of an MSM cut across devices or processes (the reference's `Sum`, src/lib.rs:183-193, over the partial sums): adds
 * `count` partial points (canonical affine, 64 bytes each) -> one affine point.  HOST pointers, no context: a short chain of
 * dependent additions and one inversion, run on the calling thread with the arithmetic of the MSM's own host tail.
 * jj_multi_msm ends with it; processes that all_gather their partial points (one process per GPU) call it on the gathered bytes. */
int jj_msm_fold_partials(size_t count, const void* parts64_host, void* out64_host);

#ifdef __cplusplus
}
#endif
#endif /* JUBJUB_HIP_H */
