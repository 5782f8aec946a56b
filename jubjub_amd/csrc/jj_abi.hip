// libjubjub_hip.so: the batch entry points of the C ABI (include/jubjub_hip.h) and the launches of their kernels (jj_kernels.h).
#define JJ_KERNELS_BATCH
#include "jj_engine.h"

// Called once by jj_ctx_create (jj_pipeline.hip), with the context's device selected: what the batch kernels need before their first launch.
// On failure the caller releases the context (including sqrt_tabs).
int jj_batch_init(jj_ctx* c) {
  // the fixed-base kernels need the full 160 KiB LDS carve-out
  const struct { const void* fn; int bytes; } lds_needs[] = {
    {reinterpret_cast<const void*>(k_fixedbase<true>), FB_LDS_BYTES}, {reinterpret_cast<const void*>(k_fixedbase_comb<true>), FBC_LDS_BYTES},
#ifdef JJ_EXPERIMENTS   // the gather selects of JJ_FIXEDBASE_SELECT=gather: instantiated in probe builds only (fixedbase_launch)
    {reinterpret_cast<const void*>(k_fixedbase<false>), FB_LDS_BYTES}, {reinterpret_cast<const void*>(k_fixedbase_comb<false>), FBC_LDS_BYTES},
#endif
    {reinterpret_cast<const void*>(k_varbase_ct3), CT3_LDS_BYTES_PER_BLOCK}};
  for (const auto& a : lds_needs)
    if (hipFuncSetAttribute(a.fn, hipFuncAttributeMaxDynamicSharedMemorySize, a.bytes) != hipSuccess) return JJ_ERR_HIP;   // the kernels could not launch later
  // square-root tables (64 KiB dlog + 36 KiB powers), built on the device
  if (hipMalloc(&c->sqrt_tabs.p, 65536 + 4 * 256 * NL * 4) != hipSuccess) { c->sqrt_tabs.p = nullptr; return JJ_ERR_NOMEM; }
  c->sqrt_tabs.cap = 65536 + 4 * 256 * NL * 4;
  if (hipMemsetAsync(c->sqrt_tabs.p, 0, c->sqrt_tabs.cap, c->stream) != hipSuccess) return JJ_ERR_HIP;
  c->sqrt_tables.dlog = (const uint8_t*)c->sqrt_tabs.p;
  c->sqrt_tables.npow = (const u32*)((uint8_t*)c->sqrt_tabs.p + 65536);
  hipLaunchKernelGGL(k_sqrt_tables_init, dim3(5), dim3(256), 0, c->stream, (uint8_t*)c->sqrt_tabs.p, (u32*)((uint8_t*)c->sqrt_tabs.p + 65536));
  if (hipStreamSynchronize(c->stream) != hipSuccess) return JJ_ERR_HIP;
  return JJ_OK;
}

// ---------------------------------------------------------------------------------------------------- the front end
// What every batch entry point does around its launches: resolve the per-unit arrays of a call of n units, run
// `body(cn, din, dout, staged)`, deliver the results.  The body enqueues the kernels of cn units on c->stream; din[k] / dout[k] are device
// pointers in the order of `in` / `out`, null for an array of 0 bytes per unit.
//   ch != 0 (the entry point's own pipe_chunk_for; 0: never) and every array a host pointer: the host-buffer pipeline runs the body once
//   per chunk, with staged = false.
//   Otherwise, and when the pipeline could not page-lock the caller's arrays: every input is staged, then every output (a NULL array or a
//   misaligned device pointer is refused there, before any launch), the body runs once with cn = n and staged = true -- not at all when
//   n = 0 -- and the results are copied out, with the synchronisation that needs.
// The caller has checked its other arguments and holds the context (JJ_ENTER).  A new entry point supplies the descriptors and a body.
template <class Body>
static int run_batch(jj_ctx* c, size_t n, std::initializer_list<ArgIn> in, std::initializer_list<ArgOut> out, size_t ch, size_t quantum, Body body) {
  int rc;
  if (in.size() > (size_t)ARGS_IN_MAX || out.size() > (size_t)ARGS_OUT_MAX) { c->err = "run_batch: more arrays than ARGS_IN_MAX / ARGS_OUT_MAX"; return JJ_ERR_INVALID; }
  if (ch) {
    bool all_host = true;
    for (const ArgIn& a : in) all_host = all_host && a.p && !is_device_ptr(a.p);
    for (const ArgOut& a : out) all_host = all_host && a.p && !is_device_ptr(a.p);
    if (all_host) {
      rc = run_pipelined(c, n, ch, in.begin(), (int)in.size(), out.begin(), (int)out.size(),
                         [&](size_t cn, const void* const* din, void* const* dout) -> int { return body(cn, din, dout, false); }, quantum);
      if (rc <= 0) return rc;      // +1: buffers could not be page-locked -> plain staging below
    }
  }
  const void* din[ARGS_IN_MAX]; OutRef o[ARGS_OUT_MAX]; void* dout[ARGS_OUT_MAX];
  int nin = 0, nout = 0;
  for (const ArgIn& a : in) if ((rc = stage_in(c, a.slot, a.p, a.elem * n, &din[nin++]))) return rc;
  for (const ArgOut& a : out) { if ((rc = stage_out(c, *a.buf, a.p, a.elem * n, &o[nout]))) return rc; dout[nout] = o[nout].dev; nout++; }
  if (n && (rc = body(n, din, dout, true))) return rc;
  bool sync = false;
  for (int k = 0; k < nout; k++) if ((rc = finish_out(c, o[k], &sync))) return rc;
  return finish(c, sync);
}

// f(lo, cn) for every chunk of `chunk` units of n, in order: the bodies whose workspace is bounded by a chunk queue them one after another
template <class F>
static int for_chunks(size_t n, size_t chunk, F f) {
  for (size_t lo = 0; lo < n; lo += chunk) { const int rc = f(lo, std::min(chunk, n - lo)); if (rc) return rc; }
  return JJ_OK;
}

// ---------------------------------------------------------------------------------------------------- fields
template <class P, int OP>
static int field_op(jj_ctx* c, size_t n, const void* a, const void* b, void* out, uint8_t* ok, bool want_ok) {
  if (!c) return JJ_ERR_INVALID;
  JJ_ENTER(c);
  const bool binary = (OP == OP_ADD || OP == OP_SUB || OP == OP_MUL);
  return run_batch(c, n, {{a, OP == OP_FROM_WIDE ? 64 : 32, 0}, {b, (size_t)(binary ? 32 : 0), 1}}, {{out, 32, &c->out[0]}, {ok, (size_t)(want_ok ? 1 : 0), &c->okb}}, 0, 0,
                   [&](size_t n, const void* const* din, void* const* dout, bool) -> int {
    hipLaunchKernelGGL((k_field_op<P, OP>), dim3(blocks_for(n)), dim3(256), 0, c->stream, n, din[0], din[1], dout[0], (uint8_t*)dout[1], c->sqrt_tables);
    return JJ_OK;
  });
}
#define FIELD_BIN(name, P, OP) JJ_API int name(jj_ctx* c, size_t n, const void* a, const void* b, void* out) { return field_op<P, OP>(c, n, a, b, out, nullptr, false); }
#define FIELD_UN(name, P, OP) JJ_API int name(jj_ctx* c, size_t n, const void* a, void* out) { return field_op<P, OP>(c, n, a, nullptr, out, nullptr, false); }
#define FIELD_UN_OK(name, P, OP) JJ_API int name(jj_ctx* c, size_t n, const void* a, void* out, uint8_t* ok) { if (!ok && n) return JJ_ERR_INVALID; return field_op<P, OP>(c, n, a, nullptr, out, ok, true); }
FIELD_BIN(jj_fq_add, FqP, OP_ADD) FIELD_BIN(jj_fq_sub, FqP, OP_SUB) FIELD_BIN(jj_fq_mul, FqP, OP_MUL)
FIELD_UN(jj_fq_neg, FqP, OP_NEG) FIELD_UN(jj_fq_square, FqP, OP_SQUARE) FIELD_UN(jj_fq_double, FqP, OP_DOUBLE)
FIELD_UN_OK(jj_fq_invert, FqP, OP_INVERT) FIELD_UN_OK(jj_fq_sqrt, FqP, OP_SQRT) FIELD_UN_OK(jj_fq_from_bytes, FqP, OP_FROM_BYTES)
FIELD_UN(jj_fq_from_bytes_wide, FqP, OP_FROM_WIDE)
FIELD_BIN(jj_fr_add, FrP, OP_ADD) FIELD_BIN(jj_fr_sub, FrP, OP_SUB) FIELD_BIN(jj_fr_mul, FrP, OP_MUL)
FIELD_UN(jj_fr_neg, FrP, OP_NEG) FIELD_UN(jj_fr_square, FrP, OP_SQUARE) FIELD_UN(jj_fr_double, FrP, OP_DOUBLE)
FIELD_UN_OK(jj_fr_invert, FrP, OP_INVERT) FIELD_UN_OK(jj_fr_sqrt, FrP, OP_SQRT) FIELD_UN_OK(jj_fr_from_bytes, FrP, OP_FROM_BYTES)
FIELD_UN(jj_fr_from_bytes_wide, FrP, OP_FROM_WIDE)

template <class P>
static int field_pow(jj_ctx* c, size_t n, const void* a, const void* e, void* out) {
  if (!c) return JJ_ERR_INVALID;
  JJ_ENTER(c);
  return run_batch(c, n, {{a, 32, 0}, {e, 32, 1}}, {{out, 32, &c->out[0]}}, 0, 0, [&](size_t n, const void* const* din, void* const* dout, bool) -> int {
    hipLaunchKernelGGL((k_field_pow<P>), dim3(blocks_for(n)), dim3(256), 0, c->stream, n, din[0], din[1], dout[0]);
    return JJ_OK;
  });
}
JJ_API int jj_fq_pow(jj_ctx* c, size_t n, const void* a, const void* exp32, void* out) { return field_pow<FqP>(c, n, a, exp32, out); }
JJ_API int jj_fr_pow(jj_ctx* c, size_t n, const void* a, const void* exp32, void* out) { return field_pow<FrP>(c, n, a, exp32, out); }

template <class P>
static int field_to_bits(jj_ctx* c, size_t n, const void* a, void* out256) {
  if (!c) return JJ_ERR_INVALID;
  JJ_ENTER(c);
  return run_batch(c, n, {{a, 32, 0}}, {{out256, 256, &c->out[0]}}, 0, 0, [&](size_t n, const void* const* din, void* const* dout, bool) -> int {
    hipLaunchKernelGGL((k_field_to_bits<P>), dim3(blocks_for(n)), dim3(256), 0, c->stream, n, din[0], dout[0]);
    return JJ_OK;
  });
}
JJ_API int jj_fq_to_le_bits(jj_ctx* c, size_t n, const void* a, void* out256) { return field_to_bits<FqP>(c, n, a, out256); }
JJ_API int jj_fr_to_le_bits(jj_ctx* c, size_t n, const void* a, void* out256) { return field_to_bits<FrP>(c, n, a, out256); }
// PrimeFieldBits::char_le_bits (reference src/fr.rs:775-785): the modulus, same layout; host-only
JJ_API int jj_fr_char_le_bits(uint8_t out256[256]) {
  if (!out256) return JJ_ERR_INVALID;
  for (int b = 0; b < 256; b++) out256[b] = (FR_MODULUS_BYTES[b >> 3] >> (b & 7)) & 1;
  return JJ_OK;
}

// ---------------------------------------------------------------------------------------------------- normalisation
static int ensure_ext(jj_ctx* c, size_t n, int coords) { return ensure(c, c->ws->ext, (size_t)coords * NL * 4 * std::max(n, (size_t)1)); }

// ext SoA (coords 0..2) -> affine 64 B (mode 0) or compressed 32 B (mode 1) at device pointer dout
static int normalize_launch(jj_ctx* c, size_t n, SoA ext, void* dout, int mode) {
  if (!n) return JJ_OK;
  int rc = ensure(c, c->ws->scratch, (size_t)NL * 4 * n); if (rc) return rc;
  SoA scratch = soa_of(c->ws->scratch, n);
  // chunk length: amortise the ~330-multiplication inversion, but keep >= ~8 waves per CU in flight (and two rounds of them: a 64-point
  // chunk at 2^23 units loses more to the single-round tail than the shared inversion returns, measured on the decoder)
  const size_t lanes_wanted = (size_t)c->cus * 64 * 8;
  if (n >= lanes_wanted * 128) { size_t T = (n + 63) / 64; hipLaunchKernelGGL((k_normalize<64>), dim3(blocks_for(T)), dim3(256), 0, c->stream, n, T, ext, scratch, dout, mode); }   // 2^24 units: -17 % (1.59 -> 1.32 ms)
  else if (n >= lanes_wanted * 32) { size_t T = (n + 31) / 32; hipLaunchKernelGGL((k_normalize<32>), dim3(blocks_for(T)), dim3(256), 0, c->stream, n, T, ext, scratch, dout, mode); }
  else if (n >= lanes_wanted * 4) { size_t T = (n + 15) / 16; hipLaunchKernelGGL((k_normalize<16>), dim3(blocks_for(T)), dim3(256), 0, c->stream, n, T, ext, scratch, dout, mode); }
  else { size_t T = (n + 3) / 4; hipLaunchKernelGGL((k_normalize<4>), dim3(blocks_for(T)), dim3(256), 0, c->stream, n, T, ext, scratch, dout, mode); }
  return JJ_OK;
}

// The scalar-multiplication family on top of run_batch: `to_ext(cn, din, ext)` leaves cn extended points of `coords` coordinates in c->ws->ext,
// the normaliser turns them into the one output (mode 0: affine, 64 bytes; 1: compressed, 32).  A staged call records the profile's three marks
// around the two (bench.py's kernel_ms); in the pipeline the normaliser moves to the tail stream (stream mode 3) and nothing is recorded.
template <class ToExt>
static int run_to_points(jj_ctx* c, size_t n, std::initializer_list<ArgIn> in, void* out, int mode, int coords, size_t ch, size_t quantum, ToExt to_ext) {
  return run_batch(c, n, in, {{out, (size_t)(mode ? 32 : 64), &c->out[0]}}, ch, quantum, [&](size_t cn, const void* const* din, void* const* dout, bool staged) -> int {
    int rc;
    if ((rc = ensure_ext(c, cn, coords))) return rc;
    SoA ext = soa_of(c->ws->ext, cn);
    if (staged) prof_mark(c, 0);
    if ((rc = to_ext(cn, din, ext))) return rc;
    if (staged) prof_mark(c, 1);
    else if ((rc = pipe_to_tail(c))) return rc;
    if ((rc = normalize_launch(c, cn, ext, dout[0], mode))) return rc;
    if (staged) prof_mark(c, 2);
    return JJ_OK;
  });
}

// ---------------------------------------------------------------------------------------------------- point ops
template <int OP>
static int point_op(jj_ctx* c, size_t n, const void* p, const void* q, void* out, size_t out_elem) {
  if (!c) return JJ_ERR_INVALID;
  JJ_ENTER(c);
  return run_batch(c, n, {{p, 64, 0}, {q, (OP == PT_ADD || OP == PT_SUB) ? 64 : 0, 1}}, {{out, out_elem, &c->out[0]}}, 0, 0,
                   [&](size_t n, const void* const* din, void* const* dout, bool) -> int {
    int rc;
    if ((rc = ensure_ext(c, n, 3))) return rc;
    SoA ext = soa_of(c->ws->ext, n);
    hipLaunchKernelGGL((k_point_op<OP>), dim3(blocks_for(n)), dim3(256), 0, c->stream, n, din[0], din[1], ext, dout[0]);
    return OP <= PT_COFACTOR ? normalize_launch(c, n, ext, dout[0], 0) : JJ_OK;
  });
}
JJ_API int jj_point_double(jj_ctx* c, size_t n, const void* p, void* out) { return point_op<PT_DOUBLE>(c, n, p, nullptr, out, 64); }
JJ_API int jj_point_add(jj_ctx* c, size_t n, const void* p, const void* q, void* out) { return point_op<PT_ADD>(c, n, p, q, out, 64); }
JJ_API int jj_point_sub(jj_ctx* c, size_t n, const void* p, const void* q, void* out) { return point_op<PT_SUB>(c, n, p, q, out, 64); }
JJ_API int jj_point_neg(jj_ctx* c, size_t n, const void* p, void* out) { return point_op<PT_NEG>(c, n, p, nullptr, out, 64); }
JJ_API int jj_point_mul_by_cofactor(jj_ctx* c, size_t n, const void* p, void* out) { return point_op<PT_COFACTOR>(c, n, p, nullptr, out, 64); }
JJ_API int jj_point_to_niels(jj_ctx* c, size_t n, const void* p, void* out96) { return point_op<PT_TO_NIELS>(c, n, p, nullptr, out96, 96); }
JJ_API int jj_is_identity(jj_ctx* c, size_t n, const void* p, uint8_t* out) { return point_op<PT_IS_IDENTITY>(c, n, p, nullptr, out, 1); }
JJ_API int jj_is_small_order(jj_ctx* c, size_t n, const void* p, uint8_t* out) { return point_op<PT_IS_SMALL_ORDER>(c, n, p, nullptr, out, 1); }
JJ_API int jj_is_on_curve(jj_ctx* c, size_t n, const void* p, uint8_t* out) { return point_op<PT_IS_ON_CURVE>(c, n, p, nullptr, out, 1); }

// ---------------------------------------------------------------------------------------------------- var-base
// launch geometry of the windowed ladders: persistent grid (blocks of 256 lanes), one table slot of `lane_words` words per lane
// (k_varbase: 17 entries x 144 B = 2448 bytes) and the waves' work cursor, zeroed on c->stream ahead of the ladder
static int ladder_workspace(jj_ctx* c, size_t n, size_t lane_words, unsigned* blocks) {
  const size_t max_threads = (size_t)c->cus * 256 * c->vb_blocks_per_cu;   // k blocks of 256 per CU = k waves / SIMD
  size_t threads = std::min(max_threads, ((n + 255) / 256) * 256);
  if (threads == 0) threads = 256;
  *blocks = (unsigned)(threads / 256);
  int rc = ensure(c, c->ws->tables, threads * lane_words * 4); if (rc) return rc;
  if ((rc = ensure(c, c->ws->cursor, 64))) return rc;
  HIPCHK(c, hipMemsetAsync(c->ws->cursor.p, 0, 8, c->stream));
  return JJ_OK;
}
// x1 of n bases batch-inverted into ext, ahead of the Montgomery ladders: a wave takes 64 x MONT_X1_UNITS units
static void mont_x1_launch(jj_ctx* c, size_t n, const void* dp, SoA ext) {
  hipLaunchKernelGGL(k_varbase_mont_x1, dim3(blocks_for(64 * ((n + 64 * MONT_X1_UNITS - 1) / (64 * MONT_X1_UNITS)))), dim3(256), 0, c->stream, n, dp, ext);
}
// ct: the ladder with the reference's timing discipline (no scalar-dependent address or branch): k_varbase_mont / _ct3 / _ct / _ct_quad; otherwise the
// per-lane window table in memory (k_varbase / k_varbase_quad: digit-dependent addresses)
static int varbase_to_ext(jj_ctx* c, size_t n, const void* ds, const void* dp, SoA ext, bool five, bool shared_scalar = false, bool ct = false) {
  if (ct && !five && !shared_scalar) {
    if (n <= (size_t)c->vb_quad_max) hipLaunchKernelGGL(k_varbase_ct_quad, dim3(blocks_for(4 * n)), dim3(256), 0, c->stream, n, ds, dp, ext);   // small batch: one scalar multiplication per quad of lanes
    else if (c->vb_ct_window == 3) hipLaunchKernelGGL(k_varbase_ct3, dim3(blocks_for(n)), dim3(256), CT3_LDS_BYTES_PER_BLOCK, c->stream, n, ds, dp, ext);
    else if (c->vb_ct_window == 2) hipLaunchKernelGGL(k_varbase_ct, dim3(blocks_for(n)), dim3(256), 0, c->stream, n, ds, dp, ext);
    else {                                                   // default: the x-only Montgomery ladder, x1 of every base batch-inverted first
      mont_x1_launch(c, n, dp, ext);
      hipLaunchKernelGGL(k_varbase_mont, dim3(blocks_for(n)), dim3(256), 0, c->stream, n, ds, dp, ext);
    }
    return JJ_OK;
  }
  if (n <= (size_t)c->vb_quad_max && !shared_scalar) {      // small batch: one scalar multiplication per quad of lanes (3x lower latency)
    int rc = ensure(c, c->ws->tables, n * (size_t)(VB_SLOTS * ENIELS_WORDS) * 4); if (rc) return rc;
    if (five) hipLaunchKernelGGL(k_varbase_quad<true>, dim3(blocks_for(4 * n)), dim3(256), 0, c->stream, n, ds, dp, (u32*)c->ws->tables.p, ext);
    else hipLaunchKernelGGL(k_varbase_quad<false>, dim3(blocks_for(4 * n)), dim3(256), 0, c->stream, n, ds, dp, (u32*)c->ws->tables.p, ext);
    return JJ_OK;
  }
  unsigned blocks;
  int rc = ladder_workspace(c, n, VB_SLOTS * ENIELS_WORDS, &blocks); if (rc) return rc;
  if (shared_scalar) hipLaunchKernelGGL((k_varbase<false, true>), dim3(blocks), dim3(256), 0, c->stream, n, ds, dp, (u32*)c->ws->tables.p, ext, (unsigned long long*)c->ws->cursor.p);
  else if (five) hipLaunchKernelGGL((k_varbase<true, false>), dim3(blocks), dim3(256), 0, c->stream, n, ds, dp, (u32*)c->ws->tables.p, ext, (unsigned long long*)c->ws->cursor.p);
  else hipLaunchKernelGGL((k_varbase<false, false>), dim3(blocks), dim3(256), 0, c->stream, n, ds, dp, (u32*)c->ws->tables.p, ext, (unsigned long long*)c->ws->cursor.p);
  return JJ_OK;
}
static int varbase_api(jj_ctx* c, size_t n, const void* scalars, const void* points, void* out, int mode, bool ct) {
  if (!c) return JJ_ERR_INVALID;
  JJ_ENTER(c);
  return run_to_points(c, n, {{scalars, 32, 0}, {points, 64, 1}}, out, mode, 3, pipe_chunk_for(c, n, 18), 0, [&](size_t cn, const void* const* din, SoA ext) -> int {
    return varbase_to_ext(c, cn, din[0], din[1], ext, false, false, ct);
  });
}
// ExtendedPoint * Fr (reference src/lib.rs:873-879 -> 357-379): the reference's ladder is constant-time (conditional_select, 334-343), and so is
// the default here: the x-only Montgomery ladder (k_varbase_mont after k_varbase_mont_x1; vb_ct_window = 3 / 2: the signed-window Edwards
// ladders k_varbase_ct3 / k_varbase_ct; one scalar multiplication per quad of lanes up to JJ_VB_QUAD_MAX units: k_varbase_ct_quad).  The _vartime entry points keep the per-lane window table in memory and signed 5-bit windows
// (digit-dependent addresses): 1.6-4.5 % faster than k_varbase_ct3 at 2^20 units depending on the box (profiles/r5_vb_ct_window.txt: ratio 0.984, r6_vb_ct_window.txt: 0.955), for public scalars.
JJ_API int jj_varbase_mul(jj_ctx* c, size_t n, const void* scalars, const void* points, void* out) { return varbase_api(c, n, scalars, points, out, 0, c && c->vb_default_ct); }
JJ_API int jj_varbase_mul_compressed(jj_ctx* c, size_t n, const void* scalars, const void* points, void* out32) { return varbase_api(c, n, scalars, points, out32, 1, c && c->vb_default_ct); }
JJ_API int jj_varbase_mul_ct(jj_ctx* c, size_t n, const void* scalars, const void* points, void* out) { return varbase_api(c, n, scalars, points, out, 0, true); }      // (the name rounds 3-4 gave the opt-in; always constant-time)
JJ_API int jj_varbase_mul_vartime(jj_ctx* c, size_t n, const void* scalars, const void* points, void* out) { return varbase_api(c, n, scalars, points, out, 0, false); }
JJ_API int jj_varbase_mul_vartime_compressed(jj_ctx* c, size_t n, const void* scalars, const void* points, void* out32) { return varbase_api(c, n, scalars, points, out32, 1, false); }
// one scalar, many bases (group::Wnaf's `scalar(..).base(..)` reuse pattern): the ladder reads the one scalar through a
// wave-uniform address (k_varbase<.., SHARED>): recoding and window digits are scalar-unit work, nothing is broadcast.
// Small batches use the quad kernel on a broadcast copy (latency path).
JJ_API int jj_varbase_mul_scalar(jj_ctx* c, size_t n, const void* scalar32, const void* points, void* out) {
  if (!c || !scalar32) return JJ_ERR_INVALID;
  JJ_ENTER(c);
  return run_batch(c, n, {{points, 64, 1}}, {{out, 64, &c->out[0]}}, 0, 0, [&](size_t n, const void* const* din, void* const* dout, bool) -> int {
    int rc;
    if ((rc = ensure(c, c->ws_tmp[1], 32))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->ws_tmp[1].p, scalar32, 32, is_device_ptr(scalar32) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    if ((rc = ensure_ext(c, n, 3))) return rc;
    SoA ext = soa_of(c->ws->ext, n);
    if (n <= (size_t)c->vb_quad_max) {
      if ((rc = ensure(c, c->ws_tmp[0], 32 * n))) return rc;
      hipLaunchKernelGGL(k_fill_scalar, dim3(blocks_for(n)), dim3(256), 0, c->stream, n, c->ws_tmp[0].p, (const uint8_t*)c->ws_tmp[1].p);
      if ((rc = varbase_to_ext(c, n, c->ws_tmp[0].p, din[0], ext, false))) return rc;
    } else if ((rc = varbase_to_ext(c, n, c->ws_tmp[1].p, din[0], ext, false, true))) return rc;
    return normalize_launch(c, n, ext, dout[0], 0);
  });
}
// ---- two terms per unit: out[i] = a[i] P[i] + b[i] Q[i] in one interleaved ladder (k_varbase_mul2, jj_straus.h).  VARIABLE-TIME like the
// _vartime entry points above (per-lane tables in memory, digit-dependent addresses).  The lane kernel serves every n (no quad form).
// shared: `da` is ONE pair of scalars (a then b, 64 device bytes) for the whole batch, db is unused.
static int varbase_mul2_to_ext(jj_ctx* c, size_t n, const void* da, const void* dp, const void* db, const void* dq, SoA ext, bool shared) {
  unsigned blocks;
  const bool w5 = c->vb_mul2_window == 5;
  int rc = ladder_workspace(c, n, w5 ? Straus<5>::LANE_WORDS : Straus<4>::LANE_WORDS, &blocks); if (rc) return rc;
  u32* tables = (u32*)c->ws->tables.p; unsigned long long* cursor = (unsigned long long*)c->ws->cursor.p;
  if (w5 && shared) hipLaunchKernelGGL((k_varbase_mul2<5, true>), dim3(blocks), dim3(256), 0, c->stream, n, da, dp, db, dq, tables, ext, cursor);
  else if (w5) hipLaunchKernelGGL((k_varbase_mul2<5, false>), dim3(blocks), dim3(256), 0, c->stream, n, da, dp, db, dq, tables, ext, cursor);
  else if (shared) hipLaunchKernelGGL((k_varbase_mul2<4, true>), dim3(blocks), dim3(256), 0, c->stream, n, da, dp, db, dq, tables, ext, cursor);
  else hipLaunchKernelGGL((k_varbase_mul2<4, false>), dim3(blocks), dim3(256), 0, c->stream, n, da, dp, db, dq, tables, ext, cursor);
  return JJ_OK;
}
static int varbase_mul2_api(jj_ctx* c, size_t n, const void* a, const void* p, const void* b, const void* q, void* out, int mode) {
  if (!c) return JJ_ERR_INVALID;
  if (n && (!a || !p || !b || !q || !out)) return JJ_ERR_INVALID;
  JJ_ENTER(c);
  return run_to_points(c, n, {{a, 32, 0}, {p, 64, 1}, {b, 32, 2}, {q, 64, 3}}, out, mode, 3, pipe_chunk_for(c, n, 18), 0, [&](size_t cn, const void* const* din, SoA ext) -> int {
    return varbase_mul2_to_ext(c, cn, din[0], din[1], din[2], din[3], ext, false);
  });
}
JJ_API int jj_varbase_mul2_vartime(jj_ctx* c, size_t n, const void* a32, const void* p64, const void* b32, const void* q64, void* out64) { return varbase_mul2_api(c, n, a32, p64, b32, q64, out64, 0); }
JJ_API int jj_varbase_mul2_vartime_compressed(jj_ctx* c, size_t n, const void* a32, const void* p64, const void* b32, const void* q64, void* out32) { return varbase_mul2_api(c, n, a32, p64, b32, q64, out32, 1); }
// one pair of scalars, many pairs of bases: both scalars are read through a wave-uniform address (k_varbase_mul2<.., SHARED>)
JJ_API int jj_varbase_mul2_scalars(jj_ctx* c, size_t n, const void* ab64, const void* p, const void* q, void* out) {
  if (!c || !ab64) return JJ_ERR_INVALID;
  if (n && (!p || !q || !out)) return JJ_ERR_INVALID;
  JJ_ENTER(c);
  if (!n) return JJ_OK;
  int rc;
  if ((rc = ensure(c, c->ws_tmp[1], 64))) return rc;
  HIPCHK(c, hipMemcpyAsync(c->ws_tmp[1].p, ab64, 64, is_device_ptr(ab64) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));   // ahead of the pipeline's streams, which start behind c->stream
  return run_to_points(c, n, {{p, 64, 1}, {q, 64, 3}}, out, 0, 3, pipe_chunk_for(c, n, 18), 0, [&](size_t cn, const void* const* din, SoA ext) -> int {
    return varbase_mul2_to_ext(c, cn, c->ws_tmp[1].p, din[0], nullptr, din[1], ext, true);
  });
}
JJ_API int jj_varbase_mul_exact(jj_ctx* c, size_t n, const void* scalars, const void* points, void* out160) {
  if (!c) return JJ_ERR_INVALID;
  JJ_ENTER(c);
  return run_batch(c, n, {{scalars, 32, 0}, {points, 64, 1}}, {{out160, 160, &c->out[0]}}, 0, 0, [&](size_t n, const void* const* din, void* const* dout, bool) -> int {
    hipLaunchKernelGGL(k_varbase_exact, dim3(blocks_for(n)), dim3(256), 0, c->stream, n, din[0], din[1], dout[0]);
    return JJ_OK;
  });
}

// [r]P == O for affine device points -> ok bytes (combine: 0 set, 1 and).  Default: order-8 Tate pairing
// (k_torsion_free); JJ_TORSION_CHECK=ladder runs the reference's definition, a var-base multiplication by r.
static int torsion_free_dev(jj_ctx* c, size_t n, const void* dpts, uint8_t* dok, int combine) {
  int rc;
  if (!c->torsion_ladder) {
    hipLaunchKernelGGL(k_torsion_free, dim3(blocks_for(n)), dim3(256), 0, c->stream, n, dpts, dok, combine);
    return JJ_OK;
  }
  if ((rc = ensure(c, c->ws_tmp[0], 32 * std::max(n, (size_t)1)))) return rc;
  if ((rc = ensure(c, c->ws_tmp[1], 32))) return rc;
  HIPCHK(c, hipMemcpyAsync(c->ws_tmp[1].p, FR_MODULUS_BYTES, 32, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_fill_scalar, dim3(blocks_for(n)), dim3(256), 0, c->stream, n, c->ws_tmp[0].p, (const uint8_t*)c->ws_tmp[1].p);
  if ((rc = ensure_ext(c, n, 3))) return rc;
  SoA ext = soa_of(c->ws->ext, n);
  if ((rc = varbase_to_ext(c, n, c->ws_tmp[0].p, dpts, ext, false))) return rc;
  hipLaunchKernelGGL(k_is_identity_ext, dim3(blocks_for(n)), dim3(256), 0, c->stream, n, ext, dok, combine);
  return JJ_OK;
}
static int torsion_pred(jj_ctx* c, size_t n, const void* p, uint8_t* out, bool prime_order) {
  if (!c) return JJ_ERR_INVALID;
  JJ_ENTER(c);
  return run_batch(c, n, {{p, 64, 0}}, {{out, 1, &c->okb}}, 0, 0, [&](size_t n, const void* const* din, void* const* dout, bool) -> int {
    int rc;
    if ((rc = torsion_free_dev(c, n, din[0], (uint8_t*)dout[0], 0))) return rc;
    if (prime_order) {   // & !is_identity  (reference src/lib.rs:717-719)
      if ((rc = ensure(c, c->ws_tmp[2], n))) return rc;
      if ((rc = ensure_ext(c, n, 3))) return rc;
      hipLaunchKernelGGL((k_point_op<PT_IS_IDENTITY>), dim3(blocks_for(n)), dim3(256), 0, c->stream, n, din[0], (const void*)nullptr, soa_of(c->ws->ext, n), c->ws_tmp[2].p);
      hipLaunchKernelGGL(k_and_bytes, dim3(blocks_for(n)), dim3(256), 0, c->stream, n, (uint8_t*)dout[0], (const uint8_t*)c->ws_tmp[2].p, 1);
    }
    return JJ_OK;
  });
}
JJ_API int jj_is_torsion_free(jj_ctx* c, size_t n, const void* p, uint8_t* out) { return torsion_pred(c, n, p, out, false); }
JJ_API int jj_is_prime_order(jj_ctx* c, size_t n, const void* p, uint8_t* out) { return torsion_pred(c, n, p, out, true); }

// ---------------------------------------------------------------------------------------------------- fixed-base
// the tail of every table builder: ne affine points on the host -> a device table of `bytes` bytes, entries `stride` words apart (k_affine_to_table)
static int upload_table(jj_ctx* c, const uint8_t* aff, size_t ne, int stride, size_t bytes, u32** out_dev) {
  u32* dev = nullptr;
  if (hipMalloc((void**)&dev, bytes) != hipSuccess) { c->err = "hipMalloc(table) failed"; return JJ_ERR_NOMEM; }
  const void* dpts;
  int rc = stage_in(c, 0, aff, ne * 64, &dpts);
  if (!rc) {
    hipLaunchKernelGGL(k_affine_to_table, dim3(blocks_for(ne)), dim3(256), 0, c->stream, ne, dpts, dev, stride);
    rc = finish(c, true);
  }
  if (rc) { (void)hipFree(dev); return rc; }
  *out_dev = dev;
  return JJ_OK;
}
// entries (i, j) = j * 2^(w i) * B for i < W, j < E (j = 0: the identity), built on the GPU in two var-base passes
// (Q_i = 2^(w i) B, then (j+1) Q_i) so that no scalar ever reaches bit 252, which the ladder ignores.
static int build_window_table(jj_ctx* c, const uint8_t base[64], int w, int W, u32 E, size_t extra_top_entry, u32** out_dev, size_t* out_entries) {
  std::vector<uint8_t> s1((size_t)W * 32, 0), p1((size_t)W * 64), q((size_t)W * 64);
  for (int i = 0; i < W; i++) {
    const int bit = w * i;
    if (bit < 252) s1[(size_t)i * 32 + (bit >> 3)] = (uint8_t)(1u << (bit & 7));
    else { const int b2 = bit - 1; s1[(size_t)i * 32 + (b2 >> 3)] = (uint8_t)(1u << (b2 & 7)); }   // 2^(bit-1), doubled below
    memcpy(&p1[(size_t)i * 64], base, 64);
  }
  int rc = jj_varbase_mul(c, W, s1.data(), p1.data(), q.data()); if (rc) return rc;
  for (int i = 0; i < W; i++) if (w * i >= 252) { rc = jj_point_double(c, 1, &q[(size_t)i * 64], &q[(size_t)i * 64]); if (rc) return rc; }
  const size_t ne = (size_t)W * E + extra_top_entry;
  std::vector<uint8_t> s2(ne * 32, 0), p2(ne * 64), aff(ne * 64);
  for (size_t e = 0; e < (size_t)W * E; e++) {
    const size_t i = e / E; const u32 mult = (u32)(e % E);
    s2[e * 32] = (uint8_t)mult; s2[e * 32 + 1] = (uint8_t)(mult >> 8); s2[e * 32 + 2] = (uint8_t)(mult >> 16);
    memcpy(&p2[e * 64], &q[i * 64], 64);
  }
  rc = jj_varbase_mul(c, (size_t)W * E, s2.data(), p2.data(), aff.data()); if (rc) return rc;
  if (extra_top_entry) {                       // LDS layout: one extra entry 2^(w W) B = 2^w * Q_{W-1}
    uint8_t sc[32] = {0}; sc[w >> 3] = (uint8_t)(1u << (w & 7));
    rc = jj_varbase_mul(c, 1, sc, &q[(size_t)(W - 1) * 64], &aff[(size_t)W * E * 64]); if (rc) return rc;
  }
  const int stride = extra_top_entry ? ANIELS_WORDS : GNIELS_WORDS;      // LDS-staged table: packed; gathered table: one line per entry
  *out_entries = ne;
  return upload_table(c, aff.data(), ne, stride, ne * (size_t)stride * 4, out_dev);
}
// Signed-comb table (layout of k_fixedbase_comb): 8 tables T_{j1}[idx] = 2^(4 j1) (2^224 + sum_{i<7} (2 idx_i - 1) 2^(32 i)) B of 128
// entries, then T_0 - B and T_0 + B.  Built on the GPU through the library's own entry points: Q_i = 2^(32 i) B and
// R_{j1,i} = 2^(4 j1) Q_i by the var-base ladder (no scalar reaches bit 252), then seven rounds of batched point additions.
static int build_comb_table(jj_ctx* c, const uint8_t base[64], u32** out_dev) {
  int rc;
  std::vector<uint8_t> s1((size_t)FBC_TEETH * 32, 0), p1((size_t)FBC_TEETH * 64), q((size_t)FBC_TEETH * 64);
  for (int i = 0; i < FBC_TEETH; i++) { const int bit = FBC_SPACING * i; s1[(size_t)i * 32 + (bit >> 3)] = (uint8_t)(1u << (bit & 7)); memcpy(&p1[(size_t)i * 64], base, 64); }
  if ((rc = jj_varbase_mul(c, FBC_TEETH, s1.data(), p1.data(), q.data()))) return rc;
  const size_t nr = (size_t)FBC_BLOCKS * FBC_TEETH;
  std::vector<uint8_t> s2(nr * 32, 0), p2(nr * 64), r(nr * 64), nrg(nr * 64);
  for (int j1 = 0; j1 < FBC_BLOCKS; j1++)
    for (int i = 0; i < FBC_TEETH; i++) {
      const size_t e = (size_t)j1 * FBC_TEETH + i; const int bit = FBC_COLS * j1;
      s2[e * 32 + (bit >> 3)] = (uint8_t)(1u << (bit & 7));
      memcpy(&p2[e * 64], &q[(size_t)i * 64], 64);
    }
  if ((rc = jj_varbase_mul(c, nr, s2.data(), p2.data(), r.data()))) return rc;
  if ((rc = jj_point_neg(c, nr, r.data(), nrg.data()))) return rc;
  const size_t ne = (size_t)FBC_BLOCKS * FBC_TENT;
  std::vector<uint8_t> acc(ne * 64), opnd(ne * 64), all((size_t)FBC_ENTRIES * 64);
  for (size_t e = 0; e < ne; e++) memcpy(&acc[e * 64], &r[((e / FBC_TENT) * FBC_TEETH + (FBC_TEETH - 1)) * 64], 64);     // the top tooth, always +
  for (int i = 0; i < FBC_TEETH - 1; i++) {
    for (size_t e = 0; e < ne; e++) {
      const size_t src = ((e / FBC_TENT) * FBC_TEETH + i) * 64;
      memcpy(&opnd[e * 64], ((e >> i) & 1) ? &r[src] : &nrg[src], 64);
    }
    if ((rc = jj_point_add(c, ne, acc.data(), opnd.data(), acc.data()))) return rc;
  }
  memcpy(all.data(), acc.data(), ne * 64);
  std::vector<uint8_t> b64((size_t)FBC_TENT * 64);
  for (int e = 0; e < FBC_TENT; e++) memcpy(&b64[(size_t)e * 64], base, 64);
  if ((rc = jj_point_sub(c, FBC_TENT, acc.data(), b64.data(), &all[ne * 64]))) return rc;                    // T_0 - B
  if ((rc = jj_point_add(c, FBC_TENT, acc.data(), b64.data(), &all[(ne + FBC_TENT) * 64]))) return rc;       // T_0 + B
  return upload_table(c, all.data(), FBC_ENTRIES, ANIELS_WORDS, FBC_LDS_BYTES, out_dev);
}
JJ_API int jj_fixedbase_table_create(jj_ctx* c, const void* base64, int window_bits, jj_table** out) {
  if (!c || !out || !base64) return JJ_ERR_INVALID;
  if (window_bits == 0) window_bits = c->fb_default_kind;
  if (window_bits != FB_W && window_bits != 7 && (window_bits < 8 || window_bits > 16)) { c->err = "window_bits must be 0 (default), 7 (signed comb in LDS), 6 (window table in LDS) or 8..16 (table gathered from L2 / Infinity Cache)"; return JJ_ERR_INVALID; }
  JJ_ENTER(c);
  uint8_t base[64];
  if (is_device_ptr(base64)) { HIPCHK(c, hipMemcpy(base, base64, 64, hipMemcpyDeviceToHost)); } else memcpy(base, base64, 64);
  auto t = std::make_unique<jj_table>();
  t->window_bits = window_bits;
  t->device = c->device;
  size_t ne = 0; int rc;
  if (window_bits == 7) {
    rc = build_comb_table(c, base, &t->dev);
  } else if (window_bits == FB_W) {
    // 42 windows x 32 entries + the carry entry 2^252 B  (layout of k_fixedbase)
    rc = build_window_table(c, base, FB_W, FB_NWIN, FB_ENT, 1, &t->dev, &ne);
  } else {
    FbParams& fp = t->fp;
    fp.w = window_bits; fp.W = (253 + window_bits - 1) / window_bits; fp.E = 1u << (window_bits - 1);
    memset(fp.recode, 0, sizeof fp.recode);
    for (int i = 0; i < fp.W - 1; i++) { const int bit = fp.w * i + fp.w - 1; fp.recode[bit >> 5] |= 1u << (bit & 31); }
    rc = build_window_table(c, base, fp.w, fp.W, fp.E + 1, 0, &t->dev, &ne);
  }
  if (rc) return rc;
  *out = t.release();
  return JJ_OK;
}
JJ_API int jj_fixedbase_table_destroy(jj_ctx* c, jj_table* t) {
  if (!c || !t) return JJ_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lk(c->mu);
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  const std::unique_ptr<jj_table> owned(t);
  if (t->dev) (void)hipFree(t->dev);
  return JJ_OK;
}
static int fixedbase_launch(jj_ctx* c, const jj_table* t, size_t n, const void* ds, SoA ext, int chain = 0) {
  // one workgroup per CU (the table fills the LDS)
  if (t->window_bits == 7) {
    const unsigned cblocks = (unsigned)std::min((size_t)c->cus, (n + FBC_THREADS - 1) / FBC_THREADS);
#ifdef JJ_EXPERIMENTS   // the per-lane gather select exists in probe builds only (JJ_FIXEDBASE_SELECT=gather); the shipped code object carries the shuffle select alone
    if (!c->fb_const_time) hipLaunchKernelGGL(k_fixedbase_comb<false>, dim3(cblocks), dim3(FBC_THREADS), FBC_LDS_BYTES, c->stream, n, ds, (const u32*)t->dev, ext, chain);
    else
#endif
    hipLaunchKernelGGL(k_fixedbase_comb<true>, dim3(cblocks), dim3(FBC_THREADS), FBC_LDS_BYTES, c->stream, n, ds, (const u32*)t->dev, ext, chain);
  } else if (t->window_bits != FB_W) {
    const unsigned gblocks = (unsigned)std::min((size_t)c->cus * c->fb_gather_blocks_per_cu, (n + 255) / 256);
    hipLaunchKernelGGL(k_fixedbase_gather, dim3(gblocks), dim3(256), 0, c->stream, n, ds, (const u32*)t->dev, t->fp, ext, chain);
  } else {
    const unsigned wblocks = (unsigned)std::min((size_t)c->cus, (n + FB_THREADS - 1) / FB_THREADS);
#ifdef JJ_EXPERIMENTS
    if (!c->fb_const_time) hipLaunchKernelGGL(k_fixedbase<false>, dim3(wblocks), dim3(FB_THREADS), FB_LDS_BYTES, c->stream, n, ds, (const u32*)t->dev, ext, chain);
    else
#endif
    hipLaunchKernelGGL(k_fixedbase<true>, dim3(wblocks), dim3(FB_THREADS), FB_LDS_BYTES, c->stream, n, ds, (const u32*)t->dev, ext, chain);
  }
  return JJ_OK;
}
// The refusals of a table an entry point cannot use: one of another device, and one of a kind it does not take -- TBL_FIXED: the table of one
// base or a composite one; TBL_ONE_BASE: the first only (`who` names the entry point in the message); TBL_PEDERSEN: a Pedersen table.
enum TableKinds { TBL_FIXED, TBL_ONE_BASE, TBL_PEDERSEN };
static int table_check(jj_ctx* c, const jj_table* t, TableKinds takes, const char* who = "") {
  if (t->device != c->device) { c->err = "fixed-base table belongs to another device"; return JJ_ERR_INVALID; }
  if (takes != TBL_PEDERSEN && t->ped.nseg > 0) { c->err = "Pedersen table (jj_pedersen_table_create): only jj_pedersen_hash_vartime takes it"; return JJ_ERR_INVALID; }
  if (takes == TBL_ONE_BASE && t->fx.nb > 0) { c->err = std::string("composite table (jj_fixedbase_composite_create): ") + who + " needs the table of one base (jj_fixedbase_table_create)"; return JJ_ERR_INVALID; }
  return JJ_OK;
}
static int fixedbase_api(jj_ctx* c, const jj_table* t, size_t n, const void* scalars, void* out, int mode) {
  if (!c || !t) return JJ_ERR_INVALID;
  JJ_ENTER(c);
  int rc;
  if ((rc = table_check(c, t, TBL_FIXED))) return rc;
  // lanes of the table's kernel: one workgroup per CU for the LDS tables, fb_gather_blocks_per_cu blocks of 256 for the gathered ones
  const size_t fb_lanes = t->window_bits == 7 ? (size_t)c->cus * FBC_THREADS : t->window_bits == FB_W ? (size_t)c->cus * FB_THREADS : (size_t)c->cus * c->fb_gather_blocks_per_cu * 256;
  return run_to_points(c, n, {{scalars, 32, 0}}, out, mode, 3, pipe_chunk_for(c, n, 20, fb_lanes), fb_lanes, [&](size_t cn, const void* const* din, SoA ext) -> int {
    return fixedbase_launch(c, t, cn, din[0], ext);
  });
}

JJ_API int jj_fixedbase_mul(jj_ctx* c, const jj_table* t, size_t n, const void* scalars, void* out) { return fixedbase_api(c, t, n, scalars, out, 0); }
// out[i] = sum_j tables[j] * scalars[j * n + i]: the accumulator stays extended between the bases (one normalisation in all)
JJ_API int jj_fixedbase_multi_mul(jj_ctx* c, const jj_table* const* tables, int nbases, size_t n, const void* scalars, void* out64) {
  if (!c || !tables || nbases < 1) return JJ_ERR_INVALID;
  for (int j = 0; j < nbases; j++) if (!tables[j]) return JJ_ERR_INVALID;
  JJ_ENTER(c);
  for (int j = 0; j < nbases; j++) { const int rc = table_check(c, tables[j], TBL_FIXED); if (rc) return rc; }
  return run_to_points(c, n, {{scalars, 32 * (size_t)nbases, 0}}, out64, 0, 5, 0, 0, [&](size_t n, const void* const* din, SoA ext) -> int {
    for (int j = 0; j < nbases; j++) {
      const int chain = (j > 0 ? 1 : 0) | (j + 1 < nbases ? 2 : 0);
      int rc = fixedbase_launch(c, tables[j], n, (const uint8_t*)din[0] + (size_t)j * n * 32, ext, chain); if (rc) return rc;
    }
    return JJ_OK;
  });
}
// ---- several bases, short scalars, one pass (k_pack_composite + k_fixedbase on a composite table)
JJ_API int jj_fixedbase_composite_create(jj_ctx* c, int nbases, const void* bases64, const int* scalar_bits, jj_table** out) {
  if (!c || !out || !bases64 || !scalar_bits || nbases < 1 || nbases > FBX_MAX_BASES) return JJ_ERR_INVALID;
  JJ_ENTER(c);
  auto t = std::make_unique<jj_table>();
  t->window_bits = FB_W;
  t->device = c->device;
  int slots = 0;
  for (int b = 0; b < nbases; b++) {
    if (scalar_bits[b] < 1 || scalar_bits[b] > 250) { c->err = "composite table: scalar_bits must be 1..250"; return JJ_ERR_INVALID; }
    t->fx.off[b] = slots; t->fx.bits[b] = scalar_bits[b];
    slots += (scalar_bits[b] + 2 + FB_W - 1) / FB_W;                 // 6 W >= bits + 2: the field's recoding never carries out of it
  }
  if (slots > FB_NWIN) { c->err = "composite table: the bases need more than 42 six-bit windows (sum of ceil((bits + 2) / 6))"; return JJ_ERR_INVALID; }
  t->fx.nb = nbases;
  std::vector<uint8_t> bases((size_t)nbases * 64);
  if (is_device_ptr(bases64)) {
    const hipError_t e = hipMemcpy(bases.data(), bases64, bases.size(), hipMemcpyDeviceToHost);
    if (e != hipSuccess) { c->err = std::string("hipMemcpy(bases) failed: ") + hipGetErrorString(e); return JJ_ERR_HIP; }
  } else memcpy(bases.data(), bases64, bases.size());
  // Q_s = 64^(local window) B_b for every slot in use, then j Q_s for j = 0 .. 32; unused slots and the carry entry hold the identity
  int rc;
  std::vector<uint8_t> s1((size_t)slots * 32, 0), p1((size_t)slots * 64), q((size_t)slots * 64);
  for (int b = 0, sl = 0; b < nbases; b++) {
    const int W = (b + 1 < nbases ? t->fx.off[b + 1] : slots) - t->fx.off[b];
    for (int i = 0; i < W; i++, sl++) { const int bit = FB_W * i; s1[(size_t)sl * 32 + (bit >> 3)] = (uint8_t)(1u << (bit & 7)); memcpy(&p1[(size_t)sl * 64], &bases[(size_t)b * 64], 64); }
  }
  if ((rc = jj_varbase_mul(c, slots, s1.data(), p1.data(), q.data()))) return rc;
  const size_t ne = (size_t)slots * FB_ENT;
  std::vector<uint8_t> s2(ne * 32, 0), p2(ne * 64), aff((size_t)FB_ENTRIES * 64, 0);
  for (size_t e = 0; e < ne; e++) { s2[e * 32] = (uint8_t)(e % FB_ENT); memcpy(&p2[e * 64], &q[(e / FB_ENT) * 64], 64); }
  for (size_t e = 0; e < (size_t)FB_ENTRIES; e++) aff[e * 64 + 32] = 1;                    // affine identity (0, 1)
  if ((rc = jj_varbase_mul(c, ne, s2.data(), p2.data(), aff.data()))) return rc;
  for (size_t e = ne; e < (size_t)FB_ENTRIES; e++) { memset(&aff[e * 64], 0, 64); aff[e * 64 + 32] = 1; }
  if ((rc = upload_table(c, aff.data(), FB_ENTRIES, ANIELS_WORDS, FB_LDS_BYTES, &t->dev))) return rc;
  *out = t.release();
  return JJ_OK;
}
JJ_API int jj_fixedbase_composite_mul(jj_ctx* c, const jj_table* t, size_t n, const void* scalars, void* out64) {
  if (!c || !t || t->fx.nb < 1) return JJ_ERR_INVALID;
  JJ_ENTER(c);
  int rc;
  if ((rc = table_check(c, t, TBL_FIXED)) || (rc = ensure(c, c->ws_tmp[2], 32 * std::max<size_t>(n, 1)))) return rc;      // the packed scalars; grown ahead of the profile's first mark
  return run_to_points(c, n, {{scalars, 32 * (size_t)t->fx.nb, 0}}, out64, 0, 3, 0, 0, [&](size_t n, const void* const* din, SoA ext) -> int {
    hipLaunchKernelGGL(k_pack_composite, dim3(blocks_for(n)), dim3(256), 0, c->stream, n, din[0], t->fx, c->ws_tmp[2].p);
    return fixedbase_launch(c, t, n, c->ws_tmp[2].p, ext);
  });
}
JJ_API int jj_fixedbase_mul_compressed(jj_ctx* c, const jj_table* t, size_t n, const void* scalars, void* out32) { return fixedbase_api(c, t, n, scalars, out32, 1); }

// ---- one fixed and one variable term per unit: out[i] = a[i] G + b[i] Q[i], G the base of `t`.  VARIABLE-TIME like the _vartime entry points of the
// var-base ladder.  Three routes, the same bytes from each: a gathered table (window_bits 8..16) above vb_quad_max units runs both terms in one
// accumulator (k_varbase_fixed, jj_fixedvar.h); an LDS table (6, 7) runs k_varbase<true> and then its own kernel on the five coordinates left in
// `ext` (chain = 1: the LDS kernels need a whole CU's LDS and one workgroup per CU, the ladder a table slot per lane and two waves per SIMD); up to
// vb_quad_max units every table kind runs the quad ladder (k_varbase_quad<true>) and then its own kernel.  `ext` holds five coordinates.
// JJ_FIXEDVAR_PROBE_SPLIT (experiments only, the same results): gathered tables take the two launches of the LDS tables -- k_varbase<true>, then
// k_fixedbase_gather with chain = 1 -- which is what the fused kernel has to beat (tools/fixedvar_ab.py, profiles/fixedvar_ab.txt)
#if defined(JJ_FIXEDVAR_PROBE_SPLIT) && !defined(JJ_EXPERIMENTS)
#error "JJ_FIXEDVAR_PROBE_SPLIT needs -DJJ_EXPERIMENTS: the shipped library is built with the defaults"
#endif
#ifdef JJ_FIXEDVAR_PROBE_SPLIT
constexpr bool FIXEDVAR_FUSED = false;
#else
constexpr bool FIXEDVAR_FUSED = true;
#endif
static int fixedvar_to_ext(jj_ctx* c, const jj_table* t, size_t n, const void* da, const void* db, const void* dq, SoA ext) {
  if (n <= (size_t)c->vb_quad_max || t->window_bits < 8 || !FIXEDVAR_FUSED) {
    int rc = varbase_to_ext(c, n, db, dq, ext, true);
    if (rc) return rc;
    return fixedbase_launch(c, t, n, da, ext, /*chain=*/1);
  }
  unsigned blocks;
  int rc = ladder_workspace(c, n, FixedVar<VB_W>::LANE_WORDS, &blocks); if (rc) return rc;
  hipLaunchKernelGGL(k_varbase_fixed, dim3(blocks), dim3(256), 0, c->stream, n, da, db, dq, (const u32*)t->dev, t->fp, (u32*)c->ws->tables.p, ext, (unsigned long long*)c->ws->cursor.p);
  return JJ_OK;
}
static int fixedvar_api(jj_ctx* c, const jj_table* t, size_t n, const void* a, const void* b, const void* q, void* out, int mode) {
  if (!c || !t) return JJ_ERR_INVALID;
  if (n && (!a || !b || !q || !out)) return JJ_ERR_INVALID;
  JJ_ENTER(c);
  int rc;
  if ((rc = table_check(c, t, TBL_ONE_BASE, "jj_fixedvar_mul_vartime"))) return rc;
  return run_to_points(c, n, {{a, 32, 0}, {b, 32, 2}, {q, 64, 3}}, out, mode, 5, pipe_chunk_for(c, n, 18), 0, [&](size_t cn, const void* const* din, SoA ext) -> int {      // (the table stays resident)
    return fixedvar_to_ext(c, t, cn, din[0], din[1], din[2], ext);
  });
}
JJ_API int jj_fixedvar_mul_vartime(jj_ctx* c, const jj_table* t, size_t n, const void* a32, const void* b32, const void* q64, void* out64) { return fixedvar_api(c, t, n, a32, b32, q64, out64, 0); }
JJ_API int jj_fixedvar_mul_vartime_compressed(jj_ctx* c, const jj_table* t, size_t n, const void* a32, const void* b32, const void* q64, void* out32) { return fixedvar_api(c, t, n, a32, b32, q64, out32, 1); }

// ---------------------------------------------------------------------------------------------------- sums / MSM
// folds a 5-coordinate SoA of n extended points down to one, result left in (U,V,Z) coords of the returned SoA
static int sum_reduce(jj_ctx* c, size_t n, DevBuf* a, DevBuf* b, SoA* result) {
  constexpr int FOLD = 32;
  DevBuf* cur = a; DevBuf* nxt = b;
  size_t m = n;
  while (m > 1) {
    const size_t T = (m + FOLD - 1) / FOLD;
    int rc = ensure(c, *nxt, (size_t)5 * NL * 4 * T); if (rc) return rc;
    hipLaunchKernelGGL((k_sum_pass<FOLD>), dim3(blocks_for(T)), dim3(256), 0, c->stream, m, T, soa_of(*cur, m), soa_of(*nxt, T));
    std::swap(cur, nxt);
    m = T;
  }
  *result = soa_of(*cur, 1);
  return JJ_OK;
}
static int write_identity(jj_ctx* c, const OutRef& o) {
  HIPCHK(c, hipMemcpyAsync(o.dev, AFFINE_IDENTITY_BYTES, 64, hipMemcpyHostToDevice, c->stream));
  return JJ_OK;
}
JJ_API int jj_point_sum(jj_ctx* c, size_t n, const void* p, void* out64) {
  if (!c) return JJ_ERR_INVALID;
  JJ_ENTER(c);
  int rc; OutRef o;
  if ((rc = stage_out(c, c->out[0], out64, 64, &o))) return rc;
  if (n == 0) { if ((rc = write_identity(c, o))) return rc; }
  else {
    const void* dp;
    if ((rc = stage_in(c, 0, p, 64 * n, &dp))) return rc;
    if ((rc = ensure(c, c->ws_tmp[2], (size_t)5 * NL * 4 * n))) return rc;
    hipLaunchKernelGGL(k_affine_to_soa5, dim3(blocks_for(n)), dim3(256), 0, c->stream, n, dp, soa_of(c->ws_tmp[2], n));
    SoA res;
    if ((rc = sum_reduce(c, n, &c->ws_tmp[2], &c->ws_tmp[3], &res))) return rc;
    if ((rc = normalize_launch(c, 1, res, o.dev, 0))) return rc;
  }
  bool sync = false;
  if ((rc = finish_out(c, o, &sync))) return rc;
  return finish(c, sync);
}
// ---------------------------------------------------------------------------------------------------- synthetic inputs
static int synth32(jj_ctx* c, size_t n, uint64_t seed, uint64_t first_index, int raw, void* out32);
JJ_API int jj_synth_scalars(jj_ctx* c, size_t n, uint64_t seed, uint64_t first_index, void* out32) { return synth32(c, n, seed, first_index, 0, out32); }
JJ_API int jj_synth_bytes32(jj_ctx* c, size_t n, uint64_t seed, uint64_t first_index, void* out32) { return synth32(c, n, seed, first_index, 1, out32); }
static int synth32(jj_ctx* c, size_t n, uint64_t seed, uint64_t first_index, int raw, void* out32) {
  if (!c) return JJ_ERR_INVALID;
  JJ_ENTER(c);
  return run_batch(c, n, {}, {{out32, 32, &c->out[0]}}, 0, 0, [&](size_t n, const void* const*, void* const* dout, bool) -> int {
    hipLaunchKernelGGL(k_synth_scalars, dim3(blocks_for(n)), dim3(256), 0, c->stream, n, (u64)seed, (u64)first_index, raw, dout[0]);
    return JJ_OK;
  });
}
JJ_API int jj_random_points(jj_ctx* c, size_t n, uint64_t seed, uint64_t first_index, int subgroup, void* out64, uint32_t* attempts) {
  if (!c) return JJ_ERR_INVALID;
  JJ_ENTER(c);
  return run_batch(c, n, {}, {{out64, 64, &c->out[0]}, {attempts, (size_t)(attempts ? 4 : 0), &c->out[1]}}, 0, 0, [&](size_t n, const void* const*, void* const* dout, bool) -> int {
    hipLaunchKernelGGL(k_random_points, dim3(blocks_for(n)), dim3(256), 0, c->stream, n, (u64)seed, (u64)first_index, subgroup ? 1 : 0, c->sqrt_tables, dout[0], (u32*)dout[1]);
    return JJ_OK;
  });
}

// ---------------------------------------------------------------------------------------------------- encodings
JJ_API int jj_compress(jj_ctx* c, size_t n, const void* points, void* out32) {
  if (!c) return JJ_ERR_INVALID;
  JJ_ENTER(c);
  return run_batch(c, n, {{points, 64, 0}}, {{out32, 32, &c->out[0]}}, 0, 0, [&](size_t n, const void* const* din, void* const* dout, bool) -> int {
    hipLaunchKernelGGL(k_compress, dim3(blocks_for(n)), dim3(256), 0, c->stream, n, din[0], dout[0]);
    return JJ_OK;
  });
}
// the decoder and the flag kernels that follow it, on device pointers (n > 0), all on c->stream
int decompress_dev(jj_ctx* c, size_t n, const void* di, unsigned flags, void* dout, uint8_t* dok, bool prof) {
  int rc;
  if ((rc = ensure(c, c->ws->scratch, (size_t)NL * 4 * n))) return rc;
  SoA scratch = soa_of(c->ws->scratch, n);
  if (prof) prof_mark(c, 0);
  const size_t lanes_wanted = (size_t)c->cus * 64 * 8;
  if (n >= lanes_wanted * 32) { size_t T = (n + 31) / 32; hipLaunchKernelGGL((k_decompress<32>), dim3(blocks_for(T)), dim3(256), 0, c->stream, n, T, di, flags, scratch, c->sqrt_tables, dout, dok); }
  else if (n >= lanes_wanted * 8 && n < lanes_wanted * 16 && c->dec_c_mid == 8) { size_t T = (n + 7) / 8; hipLaunchKernelGGL((k_decompress<8>), dim3(blocks_for(T)), dim3(256), 0, c->stream, n, T, di, flags, scratch, c->sqrt_tables, dout, dok); }
  else if (n >= lanes_wanted * 8) { size_t T = (n + 15) / 16; hipLaunchKernelGGL((k_decompress<16>), dim3(blocks_for(T)), dim3(256), 0, c->stream, n, T, di, flags, scratch, c->sqrt_tables, dout, dok); }
  else if (n <= 16384) { hipLaunchKernelGGL((k_decompress<1>), dim3(blocks_for(n)), dim3(256), 0, c->stream, n, n, di, flags, scratch, c->sqrt_tables, dout, dok); }   // latency: no shared inversion
  else { size_t T = (n + 3) / 4; hipLaunchKernelGGL((k_decompress<4>), dim3(blocks_for(T)), dim3(256), 0, c->stream, n, T, di, flags, scratch, c->sqrt_tables, dout, dok); }
  if (prof) { prof_mark(c, 1); prof_mark(c, 2); }
  if ((rc = pipe_to_tail(c))) return rc;                      // (host-buffer pipeline, stream mode 3: the flag kernels run beside the next chunk's decoder)
  // Invalid encodings were written as (0,0); the subgroup kernels below may compute garbage for them, the ok byte masks it.
  if (flags & JJ_DECOMPRESS_TORSION_FREE) { if ((rc = torsion_free_dev(c, n, dout, dok, 1))) return rc; }
  if (flags & (JJ_DECOMPRESS_NOT_SMALL_ORDER | JJ_DECOMPRESS_CLEAR_COFACTOR)) {
    if ((rc = ensure_ext(c, n, 3))) return rc;
    SoA ext = soa_of(c->ws->ext, n);
    hipLaunchKernelGGL(k_small_order_cofactor, dim3(blocks_for(n)), dim3(256), 0, c->stream, n, (const void*)dout, flags, ext, dok);
    if (flags & JJ_DECOMPRESS_CLEAR_COFACTOR) { if ((rc = normalize_launch(c, n, ext, dout, 0))) return rc; }
  }
  if (flags & (JJ_DECOMPRESS_TORSION_FREE | JJ_DECOMPRESS_NOT_SMALL_ORDER | JJ_DECOMPRESS_CLEAR_COFACTOR))
    hipLaunchKernelGGL(k_mask_outputs, dim3(blocks_for(n)), dim3(256), 0, c->stream, n, dout, (const uint8_t*)dok);
  return JJ_OK;
}
JJ_API int jj_decompress(jj_ctx* c, size_t n, const void* in32, unsigned flags, void* out64, uint8_t* ok) {
  if (!c || (!ok && n)) return JJ_ERR_INVALID;
  JJ_ENTER(c);
  return run_batch(c, n, {{in32, 32, 0}}, {{out64, 64, &c->out[0]}, {ok, 1, &c->okb}}, pipe_chunk_for(c, n, 21), 0, [&](size_t cn, const void* const* din, void* const* dout, bool staged) -> int {
    return decompress_dev(c, cn, din[0], flags, dout[0], (uint8_t*)dout[1], staged);
  });
}
// ---- one Schnorr verdict per signature (kernels: beside k_varbase_fixed in jj_kernels.h, jj_sig_each.h): verdict[i] = OK iff
// [8]([s_i]B - [c_i mod r]A_i - R_i) = O, without the three doublings under JJ_SIG_COFACTORLESS; MALFORMED for an undecodable R_i or A_i and
// for s_i >= r.  VARIABLE-TIME.  Per chunk of SIG_EACH_CHUNK units, queued one after another on the launch stream: the decoder twice (R, then A:
// the caller's two arrays are not contiguous, and one launch over both needs a copy of 64 bytes per unit first; measured through jj_decompress,
// one launch over 2^21 with that copy takes 3.64 ms against 3.84 ms for two calls over 2^20 -- 0.20 ms, less than the 0.24 ms the second CALL
// costs by itself at 2^10, which two launches inside one entry point do not pay: two launches), k_sig_each_prep, fixedvar_to_ext unchanged --
// every table kind and size by its own rule: k_varbase_fixed, or a ladder and the table's kernel -- on (s, c mod r, -A), then k_sig_each_tail
// on the coordinates it leaves: R subtracted as an affine-Niels operand, three doublings, the identity test, one byte stored.  No
// k_normalize, no compress, no jj_point_neg pass, no compare in the caller.  The workspace (c->sigeach: 64 + 64 + 2 + 32 bytes per unit of a
// chunk, and the ladders' own) is bounded by the chunk; host arrays are staged whole by the front end like every entry point's.
// A fused k_sig_each (the ladder of k_varbase_fixed with the tail in registers: 196 VGPRs, no scratch, no coordinate stored) was built and
// measured against this route: level at 2^10 and 2^16 units, 2.3 % BEHIND at 2^20 with table 13 (18.67 against 18.25 ms) and 2.2 % with table
// 10 (18.78 against 18.38 ms), both beyond the spread of the rounds (1 % in an earlier session) -- the tail's 30 products run at two waves per
// SIMD there; here k_sig_each_tail takes 0.22 ms per 2^20 units at full occupancy.  It was removed (experiments/sig_each_fused holds it as a
// patch; profiles/sig_each_ab.txt the runs).
constexpr size_t SIG_EACH_CHUNK = (size_t)1 << 20;      // units per chunk
static_assert(SIG_EACH_REJECT == JJ_SIG_REJECT && SIG_EACH_OK == JJ_SIG_OK && SIG_EACH_MALFORMED == JJ_SIG_MALFORMED, "verdict bytes of jj_sig_each.h and jubjub_hip.h");
static_assert((JJ_SIG_COFACTORLESS & (JJ_DECOMPRESS_ZIP216 | JJ_DECOMPRESS_TORSION_FREE | JJ_DECOMPRESS_NOT_SMALL_ORDER | JJ_DECOMPRESS_CLEAR_COFACTOR)) == 0, "JJ_SIG_COFACTORLESS shares a bit with a decoder flag");
static int sig_each_chunk(jj_ctx* c, const jj_table* t, size_t n, const void* dr, const void* da, const void* ds, const void* dc, unsigned flags, uint8_t* dverdict) {
  int rc;
  uint8_t* g = (uint8_t*)c->sigeach.p;
  uint8_t* const pts = g; uint8_t* const ok = pts + sig_up(128 * n); uint8_t* const cp = ok + sig_up(2 * n);
  const unsigned dflags = flags & JJ_DECOMPRESS_ZIP216;
  const int cofactored = (flags & JJ_SIG_COFACTORLESS) ? 0 : 1;
  if ((rc = decompress_dev(c, n, dr, dflags, pts, ok, false))) return rc;
  if ((rc = decompress_dev(c, n, da, dflags, pts + 64 * n, ok + n, false))) return rc;
  hipLaunchKernelGGL(k_sig_each_prep, dim3(blocks_for(n)), dim3(256), 0, c->stream, n, ds, dc, ok, (void*)pts, (void*)cp, dverdict);
  if ((rc = ensure_ext(c, n, 5))) return rc;
  SoA ext = soa_of(c->ws->ext, n);
  if ((rc = fixedvar_to_ext(c, t, n, ds, cp, pts + 64 * n, ext))) return rc;
  hipLaunchKernelGGL(k_sig_each_tail, dim3(blocks_for(n)), dim3(256), 0, c->stream, n, ext, (const void*)pts, (const uint8_t*)ok, dverdict, cofactored);
  return JJ_OK;
}
JJ_API int jj_sigverify_each(jj_ctx* c, const jj_table* t, size_t n, const void* r32, const void* a32, const void* s32, const void* c32, unsigned flags, uint8_t* verdict) {
  if (!c || !t) return JJ_ERR_INVALID;
  if (n && (!r32 || !a32 || !s32 || !c32 || !verdict)) return JJ_ERR_INVALID;
  JJ_ENTER(c);
  if (flags & ~(unsigned)(JJ_DECOMPRESS_ZIP216 | JJ_SIG_COFACTORLESS)) { c->err = "jj_sigverify_each: flags other than the ZIP-216 bit (1) and the cofactorless bit (16)"; return JJ_ERR_INVALID; }
  int rc;
  if ((rc = table_check(c, t, TBL_ONE_BASE, "jj_sigverify_each"))) return rc;
  return run_batch(c, n, {{r32, 32, 0}, {a32, 32, 1}, {s32, 32, 2}, {c32, 32, 3}}, {{verdict, 1, &c->okb}}, 0, 0, [&](size_t n, const void* const* din, void* const* dout, bool) -> int {
    const size_t ch = std::min(n, SIG_EACH_CHUNK);
    int rc = ensure(c, c->sigeach, sig_up(128 * ch) + sig_up(2 * ch) + 32 * ch); if (rc) return rc;
    return for_chunks(n, SIG_EACH_CHUNK, [&](size_t lo, size_t cn) -> int {
      return sig_each_chunk(c, t, cn, (const uint8_t*)din[0] + 32 * lo, (const uint8_t*)din[1] + 32 * lo, (const uint8_t*)din[2] + 32 * lo, (const uint8_t*)din[3] + 32 * lo, flags, (uint8_t*)dout[0] + lo);
    });
  });
}
// ---- Schnorr challenges hashed on the device (kernel: k_sig_challenge beside the jj_sigverify_each kernels in jj_kernels.h; jj_blake2b.h):
// c32[i] = Fr::from_bytes_wide(BLAKE2b-512(personal16; r32[i] || a32[i] || M_i)).  Every argument is checked before anything is staged or
// launched; the arrays then go through the staging front end (stage_in / stage_out: a device pointer passes through, a host array is copied on
// the launch stream), the offsets through slot 3 of the same staging buffers -- the context's workspace for them --, and ONE launch over all n
// units follows, instantiated for the number of parts.  A device c32 is written in launch-stream order; k_sig_terms, k_sig_keyed_terms,
// k_sig_seg_terms and k_sig_each_prep read their challenges on that stream, so a jj_sigbatch_* job or jj_sigverify_each may follow at once.
constexpr uint64_t SIG_CHALLENGE_MAX_BYTES = (uint64_t)1 << 32;     // message bytes of one call: a lane addresses them with 32 bits
JJ_API int jj_sig_challenge(jj_ctx* c, size_t n, const void* personal16, const void* r32, const void* a32, const void* msgs, size_t msg_len, const uint64_t* offsets, void* c32) {
  if (!c) return JJ_ERR_INVALID;
  if (n == 0) return JJ_OK;
  if (n > ((size_t)1 << 24) || !c32 || (offsets && msg_len)) return JJ_ERR_INVALID;
  JJ_ENTER(c);
  uint64_t total;
  if (offsets) {
    if (is_device_ptr(offsets)) { c->err = "jj_sig_challenge: offsets must be in host memory"; return JJ_ERR_INVALID; }
    if (!csr_offsets_ok(n, offsets)) { c->err = offsets[0] != 0 ? "jj_sig_challenge: offsets[0] must be 0" : "jj_sig_challenge: offsets must be non-decreasing"; return JJ_ERR_INVALID; }
    total = offsets[n];
  } else {
    if ((uint64_t)msg_len > SIG_CHALLENGE_MAX_BYTES) { c->err = "jj_sig_challenge: more than 2^32 message bytes in one call"; return JJ_ERR_INVALID; }
    total = (uint64_t)n * msg_len;
  }
  if (total > SIG_CHALLENGE_MAX_BYTES) { c->err = "jj_sig_challenge: more than 2^32 message bytes in one call"; return JJ_ERR_INVALID; }
  if (total && !msgs) { c->err = "jj_sig_challenge: NULL msgs with message bytes to hash"; return JJ_ERR_INVALID; }
  for (const void* p : {r32, a32, total ? msgs : nullptr, (const void*)c32})
    if (p && ((uintptr_t)p & 15u) && is_device_ptr(p)) { c->err = "device pointers must be 16-byte aligned"; return JJ_ERR_INVALID; }
  uint64_t personal[2] = {0, 0};
  if (personal16) memcpy(personal, personal16, 16);
  int rc;
  const void *dr, *da, *dm, *doff;
  OutRef o;
  if ((rc = stage_in(c, 0, r32, r32 ? 32 * n : 0, &dr)) || (rc = stage_in(c, 1, a32, a32 ? 32 * n : 0, &da)) || (rc = stage_in(c, 2, msgs, (size_t)total, &dm)) ||
      (rc = stage_in(c, 3, offsets, offsets ? 8 * (n + 1) : 0, &doff)) || (rc = stage_out(c, c->out[0], c32, 32 * n, &o))) return rc;
  const void* p0 = dr ? dr : da;
  const dim3 grid(blocks_for(n)), block(256);
  if (dr && da) hipLaunchKernelGGL(k_sig_challenge<2>, grid, block, 0, c->stream, n, (u64)personal[0], (u64)personal[1], dr, da, (const uint8_t*)dm, (u64)msg_len, (const unsigned long long*)doff, o.dev);
  else if (p0) hipLaunchKernelGGL(k_sig_challenge<1>, grid, block, 0, c->stream, n, (u64)personal[0], (u64)personal[1], p0, (const void*)nullptr, (const uint8_t*)dm, (u64)msg_len, (const unsigned long long*)doff, o.dev);
  else hipLaunchKernelGGL(k_sig_challenge<0>, grid, block, 0, c->stream, n, (u64)personal[0], (u64)personal[1], (const void*)nullptr, (const void*)nullptr, (const uint8_t*)dm, (u64)msg_len, (const unsigned long long*)doff, o.dev);
  bool sync = false;
  if ((rc = finish_out(c, o, &sync))) return rc;
  return finish(c, sync);
}
// ---- key agreement and KDF with ONE secret scalar (a wallet's trial decryption): key32[i] = BLAKE2b-256(personal16; to_bytes(share_i) [|| p32[i]]),
// share_i = [sk]P_i or [8]([sk]P_i), P_i = the decoder's reading of p32[i].  CONSTANT-TIME in sk and in the shares; the points and ok bytes are
// public.  Every argument is checked before anything is staged or launched.  Per chunk of KA_CHUNK units, queued one after another on the launch
// stream: decompress_dev as it is (a refused encoding leaves (0, 0) and ok = 0: the ladder then runs on x1 = 1, an ordinary value, and the unit's
// key is zeroed at the end), k_varbase_mont_x1 as it is, k_varbase_mont_ka (the ladder of k_varbase_mont with the one scalar read for all lanes
// and the three doublings of the cofactor as a template flag; one unit per lane for every n), the shared normaliser in mode 1 (to_bytes of the
// share: 32 bytes per unit, not 64), k_ka_kdf.  The workspace (c->ka: the scalar's device copy, 64 + 32 bytes per unit of a chunk; the
// decoder's, the ladder's and the normaliser's own) is bounded by the chunk; host arrays are staged whole by the front end like every entry
// point's.  The scalar's device copy is cleared behind the last chunk.
constexpr size_t KA_CHUNK = (size_t)1 << 20;            // units per chunk
constexpr unsigned KA_DECODER_FLAGS = JJ_DECOMPRESS_ZIP216 | JJ_DECOMPRESS_TORSION_FREE | JJ_DECOMPRESS_NOT_SMALL_ORDER;
static_assert(((JJ_KA_COFACTOR | JJ_KA_HASH_INPUT) & (KA_DECODER_FLAGS | JJ_DECOMPRESS_CLEAR_COFACTOR | JJ_SIG_COFACTORLESS)) == 0 && (JJ_KA_COFACTOR & JJ_KA_HASH_INPUT) == 0,
              "the JJ_KA_* flags share a bit with another flag");
static int ka_chunk(jj_ctx* c, size_t n, const void* dp, unsigned flags, const uint64_t (&personal)[2], void* dkey, uint8_t* dok) {
  int rc;
  uint8_t* const sk = (uint8_t*)c->ka.p; uint8_t* const pts = sk + 256; uint8_t* const enc = pts + sig_up(64 * n);
  if ((rc = decompress_dev(c, n, dp, flags & KA_DECODER_FLAGS, pts, dok, false))) return rc;
  if ((rc = ensure_ext(c, n, 3))) return rc;
  SoA ext = soa_of(c->ws->ext, n);
  mont_x1_launch(c, n, pts, ext);
  if (flags & JJ_KA_COFACTOR) hipLaunchKernelGGL(k_varbase_mont_ka<true>, dim3(blocks_for(n)), dim3(256), 0, c->stream, n, (const u32*)sk, (const void*)pts, ext);
  else hipLaunchKernelGGL(k_varbase_mont_ka<false>, dim3(blocks_for(n)), dim3(256), 0, c->stream, n, (const u32*)sk, (const void*)pts, ext);
  if ((rc = normalize_launch(c, n, ext, enc, 1))) return rc;
  if (flags & JJ_KA_HASH_INPUT) hipLaunchKernelGGL(k_ka_kdf<true>, dim3(blocks_for(n)), dim3(256), 0, c->stream, n, (u64)personal[0], (u64)personal[1], (const void*)enc, dp, (const uint8_t*)dok, dkey);
  else hipLaunchKernelGGL(k_ka_kdf<false>, dim3(blocks_for(n)), dim3(256), 0, c->stream, n, (u64)personal[0], (u64)personal[1], (const void*)enc, dp, (const uint8_t*)dok, dkey);
  return JJ_OK;
}
JJ_API int jj_ka_kdf(jj_ctx* c, size_t n, const void* sk32, const void* p32, unsigned flags, const void* personal16, void* key32, uint8_t* ok) {
  if (!c) return JJ_ERR_INVALID;
  if (flags & ~(KA_DECODER_FLAGS | JJ_KA_COFACTOR | JJ_KA_HASH_INPUT)) return JJ_ERR_INVALID;
  if (n == 0) return JJ_OK;
  if (!sk32 || !p32 || !key32 || !ok) return JJ_ERR_INVALID;
  JJ_ENTER(c);
  for (const void* p : {sk32, p32, (const void*)key32, (const void*)ok})
    if (((uintptr_t)p & 15u) && is_device_ptr(p)) { c->err = "device pointers must be 16-byte aligned"; return JJ_ERR_INVALID; }
  uint64_t personal[2] = {0, 0};
  if (personal16) memcpy(personal, personal16, 16);
  return run_batch(c, n, {{p32, 32, 0}}, {{key32, 32, &c->out[0]}, {ok, 1, &c->okb}}, 0, 0, [&](size_t n, const void* const* din, void* const* dout, bool) -> int {
    const size_t ch = std::min(n, KA_CHUNK);
    int rc = ensure(c, c->ka, 256 + sig_up(64 * ch) + 32 * ch); if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->ka.p, sk32, 32, is_device_ptr(sk32) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    rc = for_chunks(n, KA_CHUNK, [&](size_t lo, size_t cn) -> int {
      return ka_chunk(c, cn, (const uint8_t*)din[0] + 32 * lo, flags, personal, (uint8_t*)dout[0] + 32 * lo, (uint8_t*)dout[1] + lo);
    });
    if (rc) return rc;
    HIPCHK(c, hipMemsetAsync(c->ka.p, 0, 32, c->stream));
    return JJ_OK;
  });
}
// ---- the same with one secret scalar PER ROW (the sender's side of a note: esk_i against pk_d_i, hashed with epk_i): jj_ka_kdf's checks, chunks
// and workspace (c->ka behind the 256 bytes of jj_ka_kdf's scalar, which this call leaves alone), with k_varbase_mont_ka_each in the place of
// k_varbase_mont_ka and, under JJ_KA_HASH_INPUT, h32 in the place of p32 as the second hashed part when it is given.  The scalars go through
// the staging front end like the points; where that staged a host sk32 (c->in[1]) its n x 32 bytes are cleared behind the last chunk.
static int ka_each_chunk(jj_ctx* c, size_t n, const void* dsk, const void* dp, const void* dh, unsigned flags, const uint64_t (&personal)[2], void* dkey, uint8_t* dok) {
  int rc;
  uint8_t* const pts = (uint8_t*)c->ka.p + 256; uint8_t* const enc = pts + sig_up(64 * n);
  if ((rc = decompress_dev(c, n, dp, flags & KA_DECODER_FLAGS, pts, dok, false))) return rc;
  if ((rc = ensure_ext(c, n, 3))) return rc;
  SoA ext = soa_of(c->ws->ext, n);
  mont_x1_launch(c, n, pts, ext);
  if (flags & JJ_KA_COFACTOR) hipLaunchKernelGGL(k_varbase_mont_ka_each<true>, dim3(blocks_for(n)), dim3(256), 0, c->stream, n, dsk, (const void*)pts, ext);
  else hipLaunchKernelGGL(k_varbase_mont_ka_each<false>, dim3(blocks_for(n)), dim3(256), 0, c->stream, n, dsk, (const void*)pts, ext);
  if ((rc = normalize_launch(c, n, ext, enc, 1))) return rc;
  if (flags & JJ_KA_HASH_INPUT) hipLaunchKernelGGL(k_ka_kdf<true>, dim3(blocks_for(n)), dim3(256), 0, c->stream, n, (u64)personal[0], (u64)personal[1], (const void*)enc, dh ? dh : dp, (const uint8_t*)dok, dkey);
  else hipLaunchKernelGGL(k_ka_kdf<false>, dim3(blocks_for(n)), dim3(256), 0, c->stream, n, (u64)personal[0], (u64)personal[1], (const void*)enc, dp, (const uint8_t*)dok, dkey);
  return JJ_OK;
}
JJ_API int jj_ka_kdf_each(jj_ctx* c, size_t n, const void* sk32, const void* p32, const void* h32, unsigned flags, const void* personal16, void* key32, uint8_t* ok) {
  if (!c) return JJ_ERR_INVALID;
  if (flags & ~(KA_DECODER_FLAGS | JJ_KA_COFACTOR | JJ_KA_HASH_INPUT)) return JJ_ERR_INVALID;
  if (h32 && !(flags & JJ_KA_HASH_INPUT)) return JJ_ERR_INVALID;
  if (n == 0) return JJ_OK;
  if (!sk32 || !p32 || !key32 || !ok) return JJ_ERR_INVALID;
  JJ_ENTER(c);
  for (const void* p : {sk32, p32, h32, (const void*)key32, (const void*)ok})
    if (p && ((uintptr_t)p & 15u) && is_device_ptr(p)) { c->err = "device pointers must be 16-byte aligned"; return JJ_ERR_INVALID; }
  uint64_t personal[2] = {0, 0};
  if (personal16) memcpy(personal, personal16, 16);
  const bool sk_staged = !is_device_ptr(sk32);
  return run_batch(c, n, {{p32, 32, 0}, {sk32, 32, 1}, {h32, h32 ? (size_t)32 : (size_t)0, 2}}, {{key32, 32, &c->out[0]}, {ok, 1, &c->okb}}, 0, 0,
                   [&](size_t n, const void* const* din, void* const* dout, bool) -> int {
    const size_t ch = std::min(n, KA_CHUNK);
    int rc = ensure(c, c->ka, 256 + sig_up(64 * ch) + 32 * ch); if (rc) return rc;
    rc = for_chunks(n, KA_CHUNK, [&](size_t lo, size_t cn) -> int {
      return ka_each_chunk(c, cn, (const uint8_t*)din[1] + 32 * lo, (const uint8_t*)din[0] + 32 * lo, din[2] ? (const uint8_t*)din[2] + 32 * lo : nullptr, flags, personal,
                           (uint8_t*)dout[0] + 32 * lo, (uint8_t*)dout[1] + lo);
    });
    if (sk_staged) HIPCHK(c, hipMemsetAsync(c->in[1].p, 0, 32 * n, c->stream));      // (also behind a chunk that failed to queue)
    return rc;
  });
}
// ---- raw BLAKE2b digests over rows gathered from up to four arrays (kernel: k_blake2b<32|64> in jj_kernels.h; Blake2bRows in jj_blake2b.h):
// out[i] = BLAKE2b-digest_len(personal16; prefix || S_0[i] || .. || S_{nsrc-1}[i]).  Every argument is checked before anything is staged or
// launched.  The host compresses the whole blocks of the prefix once (never a block that could be the final one); the kernel gets the
// midstate, t, the prefix's tail, the piece plan (one piece per source) and the sources' bases and strides as arguments.  The sources go
// through the staging front end (c->in[0..3]: a device pointer passes through, a host source is copied as the (n - 1) * stride + len bytes
// that are read) and ONE launch over all n rows follows on the launch stream, no workspace.  A device `out` is written in launch-stream
// order, where jj_aead_open and jj_aead_seal read their keys32: nothing has to happen between the calls.  The library holds no
// personalisation and no prefix of any protocol.
constexpr size_t B2B_PREFIX_MAX = 4096, B2B_LEN_MAX = 65536;
template <int DIGEST>
static void b2b_launch(jj_ctx* c, size_t n, const void* personal16, const void* prefix, size_t prefix_len, int nsrc, const size_t* lens, size_t rest, const B2bSrcs& S, void* dout) {
  B2bMid mid; B2bPlan plan;
  Blake2bRows<DIGEST>::midstate(mid, (const uint8_t*)personal16, (const uint8_t*)prefix, prefix_len, rest);
  Blake2bRows<DIGEST>::plan_sources(plan, nsrc, lens);
  hipLaunchKernelGGL(k_blake2b<DIGEST>, dim3(blocks_for(n)), dim3(256), 0, c->stream, n, mid, plan, S, dout);
}
JJ_API int jj_blake2b(jj_ctx* c, size_t n, int digest_len, const void* personal16, const void* prefix, size_t prefix_len, int nsrc, const void* const* srcs, const size_t* lens,
                      const size_t* strides, void* out) {
  if (!c) return JJ_ERR_INVALID;
  if (digest_len != 32 && digest_len != 64) return JJ_ERR_INVALID;
  if (prefix_len > B2B_PREFIX_MAX || (prefix_len & 3u) || (prefix_len && !prefix)) return JJ_ERR_INVALID;
  if (nsrc < 0 || nsrc > B2B_MAX_PIECES || (nsrc && (!srcs || !lens || !strides)) || n > ((size_t)1 << 24)) return JJ_ERR_INVALID;
  JJ_ENTER(c);
  if ((nsrc && (is_device_ptr(srcs) || is_device_ptr(lens) || is_device_ptr(strides))) || is_device_ptr(prefix) || is_device_ptr(personal16)) {
    c->err = "jj_blake2b: personal16, prefix, srcs, lens and strides must be in host memory"; return JJ_ERR_INVALID;
  }
  size_t rest = 0;
  for (int s = 0; s < nsrc; s++) {
    if (lens[s] < 4 || lens[s] > B2B_LEN_MAX || (lens[s] & 3u) || (strides[s] & 3u) || strides[s] < lens[s]) { c->err = "jj_blake2b: a length or stride that is not allowed"; return JJ_ERR_INVALID; }
    if (n > ((uint64_t)1 << 32) / strides[s]) { c->err = "jj_blake2b: more than 2^32 bytes of rows in one source"; return JJ_ERR_INVALID; }      // n * stride <= 2^32
    rest += lens[s];
  }
  if (n == 0) return JJ_OK;
  if (!out) return JJ_ERR_INVALID;
  const size_t out_bytes = n * (size_t)digest_len;
  if (((uintptr_t)out & 15u) && is_device_ptr(out)) { c->err = "device pointers must be 16-byte aligned"; return JJ_ERR_INVALID; }
  for (int s = 0; s < nsrc; s++) {
    if (!srcs[s]) { c->err = "jj_blake2b: NULL source"; return JJ_ERR_INVALID; }
    if (((uintptr_t)srcs[s] & 15u) && is_device_ptr(srcs[s])) { c->err = "device pointers must be 16-byte aligned"; return JJ_ERR_INVALID; }
    const size_t in_bytes = (n - 1) * strides[s] + lens[s];
    if ((uintptr_t)srcs[s] < (uintptr_t)out + out_bytes && (uintptr_t)out < (uintptr_t)srcs[s] + in_bytes) { c->err = "jj_blake2b: out overlaps a source"; return JJ_ERR_INVALID; }
  }
  int rc;
  B2bSrcs S; memset(&S, 0, sizeof S);
  for (int s = 0; s < nsrc; s++) {
    const void* d;
    if ((rc = stage_in(c, s, srcs[s], (n - 1) * strides[s] + lens[s], &d))) return rc;
    S.p[s] = (const uint8_t*)d; S.stride[s] = (u64)strides[s];
  }
  OutRef o;
  if ((rc = stage_out(c, c->out[0], out, out_bytes, &o))) return rc;
  if (digest_len == 32) b2b_launch<32>(c, n, personal16, prefix, prefix_len, nsrc, lens, rest, S, o.dev);
  else b2b_launch<64>(c, n, personal16, prefix, prefix_len, nsrc, lens, rest, S, o.dev);
  bool sync = false;
  if ((rc = finish_out(c, o, &sync))) return rc;
  return finish(c, sync);
}
// ---- one RFC 8439 ChaCha20 key per row (kernel: k_chacha20_xor in jj_kernels.h; jj_chacha20.h): out[i][j] = in[i * in_stride + j] xor byte j of
// the keystream of keys32[i] under nonce12, block counter from `counter`.  Every argument is checked before anything is staged or launched; ONE
// launch over all n rows, no workspace.  A host `in` is staged as the (n - 1) * in_stride + len bytes that are read.  keys32 is read on the
// launch stream, where jj_ka_kdf wrote it: nothing has to happen between the two calls.
JJ_API int jj_chacha20_xor(jj_ctx* c, size_t n, const void* keys32, const void* nonce12, unsigned counter, const void* in, size_t len, size_t in_stride, void* out) {
  if (!c) return JJ_ERR_INVALID;
  if (len < 4 || len > 1024 || (len & 3u) || (in_stride & 3u) || in_stride < len) return JJ_ERR_INVALID;
  if (n > ((uint64_t)1 << 32) / in_stride) return JJ_ERR_INVALID;                    // n * in_stride <= 2^32
  if (n == 0) return JJ_OK;
  if (!keys32 || !in || !out) return JJ_ERR_INVALID;
  JJ_ENTER(c);
  const size_t in_bytes = (n - 1) * in_stride + len, out_bytes = n * len;
  if ((uintptr_t)in < (uintptr_t)out + out_bytes && (uintptr_t)out < (uintptr_t)in + in_bytes) { c->err = "jj_chacha20_xor: in and out overlap"; return JJ_ERR_INVALID; }
  for (const void* p : {keys32, in, (const void*)out})
    if (((uintptr_t)p & 15u) && is_device_ptr(p)) { c->err = "device pointers must be 16-byte aligned"; return JJ_ERR_INVALID; }
  uint32_t nonce[3] = {0, 0, 0};
  if (nonce12) memcpy(nonce, nonce12, 12);
  int rc;
  const void *dk, *di;
  OutRef o;
  if ((rc = stage_in(c, 0, keys32, 32 * n, &dk)) || (rc = stage_in(c, 1, in, in_bytes, &di)) || (rc = stage_out(c, c->out[0], out, out_bytes, &o))) return rc;
  hipLaunchKernelGGL(k_chacha20_xor, dim3(blocks_for(n)), dim3(256), 0, c->stream, n, dk, (u32)nonce[0], (u32)nonce[1], (u32)nonce[2], (u32)counter, (const uint8_t*)di, (u32)(len / 4), in_stride,
                     (uint8_t*)o.dev);
  bool sync = false;
  if ((rc = finish_out(c, o, &sync))) return rc;
  return finish(c, sync);
}
// ---- Poly1305 and the RFC 8439 ChaCha20-Poly1305 AEAD, one key per row (kernels: k_poly1305, k_aead<seal> in jj_kernels.h; jj_poly1305.h).
// The bodies are jj_chacha20_xor's: every argument is checked before anything is staged or launched, a host `in` is staged as exactly the
// bytes that are read, ONE launch over all n rows on the launch stream, no workspace.  nonce12 and aad are host memory and travel as kernel
// arguments (the aad zero-padded to 64 bytes).  keys32 is read on the launch stream, where jj_ka_kdf wrote it.
static bool aead_shape_ok(size_t n, size_t len, size_t in_stride, size_t row) {          // row: the bytes of a source row (len, or len + 16)
  if (len < 4 || len > 1024 || (len & 3u) || (in_stride & 3u) || in_stride < row) return false;
  return n <= ((uint64_t)1 << 32) / in_stride;                                          // n * in_stride <= 2^32
}
JJ_API int jj_poly1305(jj_ctx* c, size_t n, const void* keys32, const void* in, size_t len, size_t in_stride, void* tag16) {
  if (!c) return JJ_ERR_INVALID;
  if (!aead_shape_ok(n, len, in_stride, len)) return JJ_ERR_INVALID;
  if (n == 0) return JJ_OK;
  if (!keys32 || !in || !tag16) return JJ_ERR_INVALID;
  JJ_ENTER(c);
  const size_t in_bytes = (n - 1) * in_stride + len, out_bytes = 16 * n;
  if ((uintptr_t)in < (uintptr_t)tag16 + out_bytes && (uintptr_t)tag16 < (uintptr_t)in + in_bytes) { c->err = "jj_poly1305: in and tag16 overlap"; return JJ_ERR_INVALID; }
  for (const void* p : {keys32, in, (const void*)tag16})
    if (((uintptr_t)p & 15u) && is_device_ptr(p)) { c->err = "device pointers must be 16-byte aligned"; return JJ_ERR_INVALID; }
  int rc;
  const void *dk, *di;
  OutRef o;
  if ((rc = stage_in(c, 0, keys32, 32 * n, &dk)) || (rc = stage_in(c, 1, in, in_bytes, &di)) || (rc = stage_out(c, c->out[0], tag16, out_bytes, &o))) return rc;
  hipLaunchKernelGGL(k_poly1305, dim3(blocks_for(n)), dim3(256), 0, c->stream, n, dk, (const uint8_t*)di, (u32)(len / 4), in_stride, o.dev);
  bool sync = false;
  if ((rc = finish_out(c, o, &sync))) return rc;
  return finish(c, sync);
}
template <bool SEAL>
static int aead_call(jj_ctx* c, const char* overlap, size_t n, const void* keys32, const void* nonce12, const void* aad, size_t aad_len, const void* in, size_t len, size_t in_stride,
                     void* out, uint8_t* ok) {
  if (!c) return JJ_ERR_INVALID;
  if (!aead_shape_ok(n, len, in_stride, SEAL ? len : len + 16) || aad_len > 64 || (aad_len && !aad)) return JJ_ERR_INVALID;
  if (n == 0) return JJ_OK;
  if (!keys32 || !in || !out || (!SEAL && !ok)) return JJ_ERR_INVALID;
  JJ_ENTER(c);
  const size_t in_bytes = (n - 1) * in_stride + len + (SEAL ? 0 : 16), out_bytes = n * (len + (SEAL ? 16 : 0));
  if ((uintptr_t)in < (uintptr_t)out + out_bytes && (uintptr_t)out < (uintptr_t)in + in_bytes) { c->err = overlap; return JJ_ERR_INVALID; }
  for (const void* p : {keys32, in, (const void*)out, (const void*)ok})
    if (p && ((uintptr_t)p & 15u) && is_device_ptr(p)) { c->err = "device pointers must be 16-byte aligned"; return JJ_ERR_INVALID; }
  uint32_t nonce[3] = {0, 0, 0};
  if (nonce12) memcpy(nonce, nonce12, 12);
  AeadAad a;
  memset(&a, 0, sizeof a);
  if (aad_len) memcpy(a.w, aad, aad_len);
  int rc;
  const void *dk, *di;
  OutRef o, k = {nullptr, nullptr, 0, false};
  if ((rc = stage_in(c, 0, keys32, 32 * n, &dk)) || (rc = stage_in(c, 1, in, in_bytes, &di)) || (rc = stage_out(c, c->out[0], out, out_bytes, &o))) return rc;
  if (!SEAL && (rc = stage_out(c, c->okb, ok, n, &k))) return rc;
  hipLaunchKernelGGL(k_aead<SEAL>, dim3(blocks_for(n)), dim3(256), 0, c->stream, n, dk, (u32)nonce[0], (u32)nonce[1], (u32)nonce[2], a, (u32)aad_len, (const uint8_t*)di, (u32)(len / 4),
                     in_stride, (uint8_t*)o.dev, (uint8_t*)k.dev);
  bool sync = false;
  if ((rc = finish_out(c, o, &sync))) return rc;
  if (!SEAL && (rc = finish_out(c, k, &sync))) return rc;
  return finish(c, sync);
}
JJ_API int jj_aead_open(jj_ctx* c, size_t n, const void* keys32, const void* nonce12, const void* aad, size_t aad_len, const void* in, size_t len, size_t in_stride, void* out,
                        uint8_t* ok) {
  return aead_call<false>(c, "jj_aead_open: in and out overlap", n, keys32, nonce12, aad, aad_len, in, len, in_stride, out, ok);
}
JJ_API int jj_aead_seal(jj_ctx* c, size_t n, const void* keys32, const void* nonce12, const void* aad, size_t aad_len, const void* in, size_t len, size_t in_stride, void* out) {
  return aead_call<true>(c, "jj_aead_seal: in and out overlap", n, keys32, nonce12, aad, aad_len, in, len, in_stride, out, nullptr);
}
// ---- BLAKE2s-256 of prefix || M_i and the hash to the curve built on it (kernel: k_blake2s in jj_kernels.h; jj_blake2s.h):
// digest_i = BLAKE2s-256(personal8; prefix || M_i), M_i the msg_len bytes at msgs + i * msg_stride; jj_group_hash hands the digests to
// decompress_dev as it is, so out64 and ok are what jj_decompress writes for them under the same flags.  VARIABLE-TIME over public inputs.
// Every argument is checked before anything is staged or launched (b2s_plan).  The host compresses the whole blocks of the prefix once
// (Blake2s::midstate: never a block that could be the final one) and the kernel gets h, t and the prefix's tail as arguments.  The message
// bytes go through the staging front end as the (n - 1) * msg_stride + msg_len bytes that are read; then per chunk of B2S_CHUNK units, queued
// one after another on the launch stream: ONE k_blake2s launch, and for jj_group_hash the decoder chain on the chunk's digests, which live in
// c->b2s (32 bytes per unit of a chunk).  A device out32 is written in launch-stream order, where every other entry point reads its inputs:
// nothing has to happen between jj_blake2s and a later call.  The library holds no personalisation and no prefix of any protocol.
constexpr size_t B2S_CHUNK = (size_t)1 << 20;           // units per chunk
constexpr size_t B2S_PREFIX_MAX = 4096, B2S_MSG_MAX = 65536;
constexpr unsigned B2S_DECODER_FLAGS = JJ_DECOMPRESS_ZIP216 | JJ_DECOMPRESS_TORSION_FREE | JJ_DECOMPRESS_NOT_SMALL_ORDER | JJ_DECOMPRESS_CLEAR_COFACTOR;
struct B2sPlan { B2sMid mid; u32 t0, tail_len; size_t msg_bytes; };
// the checks that need no context, and the plan of a call with n > 0
static bool b2s_plan(size_t n, const void* personal8, const void* prefix, size_t prefix_len, const void* msgs, size_t msg_len, size_t msg_stride, B2sPlan* p) {
  if (prefix_len > B2S_PREFIX_MAX || (prefix_len && !prefix) || msg_len > B2S_MSG_MAX || msg_stride < msg_len) return false;
  if (n > ((size_t)1 << 24) || (msg_stride && n > ((uint64_t)1 << 32) / msg_stride)) return false;        // n * msg_stride <= 2^32
  if (n == 0) return true;
  if (msg_len && !msgs) return false;
  const size_t B = Blake2s::midstate_blocks(prefix_len, msg_len);
  Blake2s::midstate(p->mid.h, p->mid.tail, (const uint8_t*)personal8, (const uint8_t*)prefix, prefix_len, B);
  p->t0 = (u32)(Blake2s::BLOCK * B); p->tail_len = (u32)(prefix_len - Blake2s::BLOCK * B);
  p->msg_bytes = msg_len ? (n - 1) * msg_stride + msg_len : 0;
  return true;
}
static void b2s_launch(jj_ctx* c, size_t n, size_t row0, const B2sPlan& p, const void* dm, size_t msg_len, size_t msg_stride, void* dout32) {
  hipLaunchKernelGGL(k_blake2s, dim3(blocks_for(n)), dim3(256), 0, c->stream, n, row0, p.mid, p.t0, p.tail_len, (const uint8_t*)dm, (u32)msg_len, msg_stride, dout32);
}
JJ_API int jj_blake2s(jj_ctx* c, size_t n, const void* personal8, const void* prefix, size_t prefix_len, const void* msgs, size_t msg_len, size_t msg_stride, void* out32) {
  if (!c) return JJ_ERR_INVALID;
  B2sPlan p;
  if (!b2s_plan(n, personal8, prefix, prefix_len, msgs, msg_len, msg_stride, &p)) return JJ_ERR_INVALID;
  if (n == 0) return JJ_OK;
  if (!out32) return JJ_ERR_INVALID;
  JJ_ENTER(c);
  for (const void* q : {p.msg_bytes ? msgs : nullptr, (const void*)out32})
    if (q && ((uintptr_t)q & 15u) && is_device_ptr(q)) { c->err = "device pointers must be 16-byte aligned"; return JJ_ERR_INVALID; }
  int rc;
  const void* dm;
  OutRef o;
  if ((rc = stage_in(c, 0, msgs, p.msg_bytes, &dm)) || (rc = stage_out(c, c->out[0], out32, 32 * n, &o))) return rc;
  (void)for_chunks(n, B2S_CHUNK, [&](size_t lo, size_t cn) -> int { b2s_launch(c, cn, lo, p, dm, msg_len, msg_stride, (uint8_t*)o.dev + 32 * lo); return JJ_OK; });
  bool sync = false;
  if ((rc = finish_out(c, o, &sync))) return rc;
  return finish(c, sync);
}
JJ_API int jj_group_hash(jj_ctx* c, size_t n, const void* personal8, const void* prefix, size_t prefix_len, const void* msgs, size_t msg_len, size_t msg_stride, unsigned flags,
                         void* out64, uint8_t* ok) {
  if (!c) return JJ_ERR_INVALID;
  if (flags & ~B2S_DECODER_FLAGS) return JJ_ERR_INVALID;
  B2sPlan p;
  if (!b2s_plan(n, personal8, prefix, prefix_len, msgs, msg_len, msg_stride, &p)) return JJ_ERR_INVALID;
  if (n == 0) return JJ_OK;
  if (!out64 || !ok) return JJ_ERR_INVALID;
  JJ_ENTER(c);
  for (const void* q : {p.msg_bytes ? msgs : nullptr, (const void*)out64, (const void*)ok})
    if (q && ((uintptr_t)q & 15u) && is_device_ptr(q)) { c->err = "device pointers must be 16-byte aligned"; return JJ_ERR_INVALID; }
  int rc;
  const void* dm;
  OutRef o, k;
  if ((rc = stage_in(c, 0, msgs, p.msg_bytes, &dm)) || (rc = stage_out(c, c->out[0], out64, 64 * n, &o)) || (rc = stage_out(c, c->okb, ok, n, &k))) return rc;
  if ((rc = ensure(c, c->b2s, 32 * std::min(n, B2S_CHUNK)))) return rc;
  rc = for_chunks(n, B2S_CHUNK, [&](size_t lo, size_t cn) -> int {
    b2s_launch(c, cn, lo, p, dm, msg_len, msg_stride, c->b2s.p);
    return decompress_dev(c, cn, c->b2s.p, flags, (uint8_t*)o.dev + 64 * lo, (uint8_t*)k.dev + lo, false);
  });
  if (rc) return rc;
  bool sync = false;
  if ((rc = finish_out(c, o, &sync)) || (rc = finish_out(c, k, &sync))) return rc;
  return finish(c, sync);
}
// ---- windowed Pedersen hashes (jj_pedersen.h: the function, the table layout, the plan; kernels k_pedersen_gather, k_pedersen_scalars, k_affine_u)
// sum_i e[i] 16^(chunk0 + i) mod r as canonical bytes, e[i] in +-{1..4}: the positive and the negative digits as two integers, one subtraction
static void ped_entry_scalar(const int* e, int t, int chunk0, uint8_t out[32]) {
  u32 P[8] = {0}, N[8] = {0};
  for (int i = 0; i < t; i++) {
    const int bit = 4 * (chunk0 + i);
    (e[i] > 0 ? P : N)[bit >> 5] |= (u32)(e[i] > 0 ? e[i] : -e[i]) << (bit & 31);
  }
  u32 d[8]; u64 br = 0, cy = 0;
  for (int x = 0; x < 8; x++) { const u64 v = (u64)P[x] - N[x] - br; d[x] = (u32)v; br = (v >> 32) & 1u; }
  const u32 addr = 0u - (u32)br;
  for (int x = 0; x < 8; x++) { const u64 v = (u64)d[x] + (FR_MODULUS_W[x] & addr) + cy; d[x] = (u32)v; cy = v >> 32; }
  memcpy(out, d, 32);
}
JJ_API int jj_pedersen_table_create(jj_ctx* c, int nseg, const void* gens64, int seg_chunks, int window_chunks, jj_table** out) {
  if (!c || !out || !gens64) return JJ_ERR_INVALID;
  JJ_ENTER(c);
  if (nseg < 1 || nseg > PED_MAX_SEG || seg_chunks < 1 || seg_chunks > PED_MAX_CHUNKS || window_chunks < 0 || window_chunks > PED_MAX_WINDOW) {
    c->err = "jj_pedersen_table_create: nseg must be 1..8, seg_chunks 1..63, window_chunks 0 (default) or 1..4"; return JJ_ERR_INVALID;
  }
  const int w = window_chunks ? window_chunks : PED_DEFAULT_WINDOW;
  std::vector<uint8_t> gens((size_t)nseg * 64), good((size_t)nseg);
  if (is_device_ptr(gens64)) { HIPCHK(c, hipMemcpy(gens.data(), gens64, gens.size(), hipMemcpyDeviceToHost)); } else memcpy(gens.data(), gens64, gens.size());
  // on the curve and torsion-free: the integer sum and the sum over scalars reduced mod r are then the same point
  int rc;
  if ((rc = jj_is_on_curve(c, nseg, gens.data(), good.data()))) return rc;
  for (int j = 0; j < nseg; j++) if (!good[j]) { c->err = "jj_pedersen_table_create: a generator is not on the curve"; return JJ_ERR_INVALID; }
  if ((rc = jj_is_torsion_free(c, nseg, gens.data(), good.data()))) return rc;
  for (int j = 0; j < nseg; j++) if (!good[j]) { c->err = "jj_pedersen_table_create: a generator has a torsion component"; return JJ_ERR_INVALID; }
  const size_t seg_e = ped_seg_entries(seg_chunks, w), ne = seg_e * nseg;
  std::vector<uint8_t> s(ne * 32), p(ne * 64), aff(ne * 64);
  size_t e = 0;
  for (int j = 0; j < nseg; j++)
    for (int k = 0; k < ped_windows(seg_chunks, w); k++)
      for (int t = 1; t <= std::min(w, seg_chunks - k * w); t++)
        for (u32 idx = 0; idx < ped_sub_entries(t); idx++, e++) {
          int enc[PED_MAX_WINDOW];
          for (int i = 0; i < t; i++) {
            const u32 ch = (idx >> (3 * i)) & 7u;                     // the last chunk's sign bit is not in the index: it reads as +
            enc[i] = (int)(1u + (ch & 1u) + (ch & 2u)) * ((ch & 4u) ? -1 : 1);
          }
          ped_entry_scalar(enc, t, k * w, &s[e * 32]);
          memcpy(&p[e * 64], &gens[(size_t)j * 64], 64);
        }
  if ((rc = jj_varbase_mul(c, ne, s.data(), p.data(), aff.data()))) return rc;
  auto t = std::make_unique<jj_table>();
  t->window_bits = 0; t->device = c->device;
  t->ped.nseg = nseg; t->ped.seg_chunks = seg_chunks; t->ped.window_chunks = w;
  if ((rc = upload_table(c, aff.data(), ne, GNIELS_WORDS, ne * (size_t)GNIELS_WORDS * 4, &t->dev))) return rc;
  *out = t.release();
  return JJ_OK;
}
// the checks jj_pedersen_hash_vartime and jj_pedersen_scalars share: everything about the message's layout, before anything is staged
static int ped_check_layout(jj_ctx* c, int nseg, int seg_chunks, size_t n, int prefix_bits, const void* rows, size_t row_stride, int nfields, const uint32_t* fields) {
  if (prefix_bits < 0 || prefix_bits > 32) { c->err = "Pedersen hash: prefix_bits must be 0..32"; return JJ_ERR_INVALID; }
  if (nfields < 0 || nfields > PED_MAX_FIELDS) { c->err = "Pedersen hash: nfields must be 0..4"; return JJ_ERR_INVALID; }
  if (nfields && (!fields || is_device_ptr(fields))) { c->err = "Pedersen hash: fields must be a host array"; return JJ_ERR_INVALID; }
  uint64_t bits = (uint64_t)prefix_bits;
  for (int f = 0; f < nfields; f++) {
    const uint64_t off = fields[2 * f], nb = fields[2 * f + 1];
    if (nb < 1 || off + (nb + 7) / 8 > (uint64_t)row_stride) { c->err = "Pedersen hash: a field is empty or reaches past row_stride"; return JJ_ERR_INVALID; }
    bits += nb;
  }
  if (bits > 3ull * (uint64_t)seg_chunks * (uint64_t)nseg) { c->err = "Pedersen hash: the message is longer than 3 * seg_chunks * nseg bits"; return JJ_ERR_INVALID; }
  if (nfields) {
    if (!rows) { c->err = "Pedersen hash: NULL rows"; return JJ_ERR_INVALID; }
    if ((uint64_t)row_stride > ((uint64_t)1 << 32) || (uint64_t)n * row_stride > ((uint64_t)1 << 32)) { c->err = "Pedersen hash: more than 2^32 bytes of rows in one call"; return JJ_ERR_INVALID; }
    if (((uintptr_t)rows & 15u) && is_device_ptr(rows)) { c->err = "device pointers must be 16-byte aligned"; return JJ_ERR_INVALID; }
  }
  return JJ_OK;
}
JJ_API int jj_pedersen_hash_vartime(jj_ctx* c, const jj_table* t, size_t n, unsigned prefix, int prefix_bits, const void* rows, size_t row_stride, int nfields,
                                    const uint32_t* fields, unsigned flags, void* out) {
  if (!c || !t) return JJ_ERR_INVALID;
  if (n == 0) return JJ_OK;
  if (!out) return JJ_ERR_INVALID;
  JJ_ENTER(c);
  if (t->ped.nseg < 1) { c->err = "jj_pedersen_hash_vartime needs a table of jj_pedersen_table_create"; return JJ_ERR_INVALID; }
  int rc;
  if ((rc = table_check(c, t, TBL_PEDERSEN))) return rc;
  if (flags & ~(unsigned)JJ_PEDERSEN_POINT) { c->err = "jj_pedersen_hash_vartime: flags other than the point bit (1)"; return JJ_ERR_INVALID; }
  if ((rc = ped_check_layout(c, t->ped.nseg, t->ped.seg_chunks, n, prefix_bits, rows, row_stride, nfields, fields))) return rc;
  if (((uintptr_t)out & 15u) && is_device_ptr(out)) { c->err = "device pointers must be 16-byte aligned"; return JJ_ERR_INVALID; }
  PedSegs segs; u32 cover;
  const std::vector<PedWin> plan = ped_build_plan(t->ped.nseg, t->ped.seg_chunks, t->ped.window_chunks, prefix, prefix_bits, nfields, fields, &segs, &cover);
  const bool point = (flags & JJ_PEDERSEN_POINT) != 0;
  const void *drows, *dplan;
  OutRef o;
  if ((rc = ensure_ext(c, n, 3)) || (!point && (rc = ensure(c, c->ws_tmp[2], 64 * n)))) return rc;
  if ((rc = stage_in(c, 0, rows, nfields ? n * row_stride : 0, &drows)) || (rc = stage_in(c, 3, plan.data(), plan.size() * sizeof(PedWin), &dplan)) ||
      (rc = stage_out(c, c->out[0], out, (point ? 64 : 32) * n, &o))) return rc;
  SoA ext = soa_of(c->ws->ext, n);
  prof_mark(c, 0);
  const unsigned gblocks = (unsigned)std::min((size_t)c->cus * c->fb_gather_blocks_per_cu, (n + 255) / 256);
  hipLaunchKernelGGL(k_pedersen_gather, dim3(gblocks), dim3(256), 0, c->stream, n, (const uint8_t*)drows, (u32)row_stride, cover, (const PedWin*)dplan, (int)plan.size(), (const u32*)t->dev, ext);
  prof_mark(c, 1);
  if ((rc = normalize_launch(c, n, ext, point ? o.dev : c->ws_tmp[2].p, 0))) return rc;
  if (!point) hipLaunchKernelGGL(k_affine_u, dim3(blocks_for(n)), dim3(256), 0, c->stream, n, (const void*)c->ws_tmp[2].p, o.dev);
  prof_mark(c, 2);
  bool sync = false;
  if ((rc = finish_out(c, o, &sync))) return rc;
  return finish(c, sync);
}
JJ_API int jj_pedersen_scalars(jj_ctx* c, int nseg, int seg_chunks, size_t n, unsigned prefix, int prefix_bits, const void* rows, size_t row_stride, int nfields,
                               const uint32_t* fields, void* scalars32) {
  if (!c) return JJ_ERR_INVALID;
  if (n == 0) return JJ_OK;
  if (!scalars32) return JJ_ERR_INVALID;
  JJ_ENTER(c);
  if (nseg < 1 || nseg > PED_MAX_SEG || seg_chunks < 1 || seg_chunks > PED_MAX_CHUNKS) { c->err = "jj_pedersen_scalars: nseg must be 1..8, seg_chunks 1..63"; return JJ_ERR_INVALID; }
  int rc;
  if ((rc = ped_check_layout(c, nseg, seg_chunks, n, prefix_bits, rows, row_stride, nfields, fields))) return rc;
  if (((uintptr_t)scalars32 & 15u) && is_device_ptr(scalars32)) { c->err = "device pointers must be 16-byte aligned"; return JJ_ERR_INVALID; }
  PedSegs segs; u32 cover;
  const std::vector<PedWin> plan = ped_build_plan(nseg, seg_chunks, PED_MAX_WINDOW, prefix, prefix_bits, nfields, fields, &segs, &cover);
  const void *drows, *dplan;
  OutRef o;
  if ((rc = stage_in(c, 0, rows, nfields ? n * row_stride : 0, &drows)) || (rc = stage_in(c, 3, plan.data(), plan.size() * sizeof(PedWin), &dplan)) ||
      (rc = stage_out(c, c->out[0], scalars32, 32 * n * (size_t)nseg, &o))) return rc;
  hipLaunchKernelGGL(k_pedersen_scalars, dim3(blocks_for(n), (unsigned)nseg), dim3(256), 0, c->stream, n, (const uint8_t*)drows, (u32)row_stride, cover, (const PedWin*)dplan, segs, o.dev);
  bool sync = false;
  if ((rc = finish_out(c, o, &sync))) return rc;
  return finish(c, sync);
}
// ---- windowed Pedersen commitment over several row arrays: out[i] = H(M_i) + [r_i] R (k_pedersen_commit; the contract: include/jubjub_hip.h).
// Staging slots: sources 0..2 in c->in[0..2], the plan in c->in[3] (as the hash), source 3 in c->in[4], r in c->in[5].
static const int PED_COMMIT_SRC_SLOT[PED_MAX_SRC] = {0, 1, 2, 4};
// JJ_COMMIT_PROBE_SPLIT (experiments only, the same results): a gathered rbase takes the two launches of the LDS tables -- k_pedersen_commit up to
// the message's end, then k_fixedbase_gather with chain = 1 -- which is what the fused walk has to beat (tools/commit_ab.py, profiles/commit_ab.txt)
#if defined(JJ_COMMIT_PROBE_SPLIT) && !defined(JJ_EXPERIMENTS)
#error "JJ_COMMIT_PROBE_SPLIT needs -DJJ_EXPERIMENTS: the shipped library is built with the defaults"
#endif
#ifdef JJ_COMMIT_PROBE_SPLIT
constexpr bool COMMIT_FUSED = false;
#else
constexpr bool COMMIT_FUSED = true;
#endif
JJ_API int jj_pedersen_commit_vartime(jj_ctx* c, const jj_table* ped, const jj_table* rbase, size_t n, unsigned prefix, int prefix_bits, int nsrc, const void* const* srcs,
                                      const size_t* strides, int nfields, const uint32_t* fields, const void* r32, unsigned flags, void* out) {
  if (!c || !ped) return JJ_ERR_INVALID;
  if (n == 0) return JJ_OK;
  if (!out) return JJ_ERR_INVALID;
  JJ_ENTER(c);
  const char* who = "jj_pedersen_commit_vartime";
  if (ped->ped.nseg < 1) { c->err = "jj_pedersen_commit_vartime needs a table of jj_pedersen_table_create"; return JJ_ERR_INVALID; }
  int rc;
  if ((rc = table_check(c, ped, TBL_PEDERSEN))) return rc;
  if ((rbase == nullptr) != (r32 == nullptr)) { c->err = "jj_pedersen_commit_vartime: rbase and r32 are both given or both NULL (the hash-only form)"; return JJ_ERR_INVALID; }
  if (rbase && (rc = table_check(c, rbase, TBL_ONE_BASE, who))) return rc;
  if (flags & ~(unsigned)JJ_PEDERSEN_POINT) { c->err = "jj_pedersen_commit_vartime: flags other than the point bit (1)"; return JJ_ERR_INVALID; }
  if (prefix_bits < 0 || prefix_bits > 32) { c->err = "Pedersen commit: prefix_bits must be 0..32"; return JJ_ERR_INVALID; }
  if (nfields < 0 || nfields > PED_MAX_FIELDS) { c->err = "Pedersen commit: nfields must be 0..4"; return JJ_ERR_INVALID; }
  if (nsrc < 0 || nsrc > PED_MAX_SRC || (nsrc == 0 && nfields > 0)) { c->err = "Pedersen commit: nsrc must be 1..4 (0 only without fields)"; return JJ_ERR_INVALID; }
  if ((nfields && (!fields || is_device_ptr(fields))) || (nsrc && (!srcs || !strides || is_device_ptr(srcs) || is_device_ptr(strides)))) {
    c->err = "Pedersen commit: srcs, strides and fields must be host arrays"; return JJ_ERR_INVALID;
  }
  for (int s = 0; s < nsrc; s++) {
    if (!srcs[s]) { c->err = "Pedersen commit: NULL source"; return JJ_ERR_INVALID; }
    if ((uint64_t)strides[s] > ((uint64_t)1 << 32) || (uint64_t)n * strides[s] > ((uint64_t)1 << 32)) { c->err = "Pedersen commit: more than 2^32 bytes of rows in one source"; return JJ_ERR_INVALID; }
    if (((uintptr_t)srcs[s] & 15u) && is_device_ptr(srcs[s])) { c->err = "device pointers must be 16-byte aligned"; return JJ_ERR_INVALID; }
  }
  uint64_t bits = (uint64_t)prefix_bits, cov[PED_MAX_SRC] = {0, 0, 0, 0};
  for (int f = 0; f < nfields; f++) {
    const uint64_t s = fields[3 * f], off = fields[3 * f + 1], nb = fields[3 * f + 2];
    if (s >= (uint64_t)nsrc) { c->err = "Pedersen commit: a field names a source that is not there"; return JJ_ERR_INVALID; }
    if (nb < 1 || off + (nb + 7) / 8 > (uint64_t)strides[s]) { c->err = "Pedersen commit: a field is empty or reaches past its source's stride"; return JJ_ERR_INVALID; }
    cov[s] = std::max(cov[s], off + (nb + 7) / 8);
    bits += nb;
  }
  if (bits > 3ull * (uint64_t)ped->ped.seg_chunks * (uint64_t)ped->ped.nseg) { c->err = "Pedersen commit: the message is longer than 3 * seg_chunks * nseg bits"; return JJ_ERR_INVALID; }
  if ((((uintptr_t)out & 15u) && is_device_ptr(out)) || (r32 && ((uintptr_t)r32 & 15u) && is_device_ptr(r32))) { c->err = "device pointers must be 16-byte aligned"; return JJ_ERR_INVALID; }
  PedSegs segs; PedSrcs S; memset(&S, 0, sizeof S);
  const std::vector<PedWinSrc> plan = ped_build_plan_src(ped->ped.nseg, ped->ped.seg_chunks, ped->ped.window_chunks, prefix, prefix_bits, nfields, fields, &segs, S.cover);
  const bool point = (flags & JJ_PEDERSEN_POINT) != 0;
  const int mode = !rbase ? PED_COMMIT_HASH : (rbase->window_bits >= 8 && COMMIT_FUSED) ? PED_COMMIT_FUSED : PED_COMMIT_CHAIN;
  const void *dplan, *dr = nullptr;
  OutRef o;
  if ((rc = ensure_ext(c, n, mode == PED_COMMIT_CHAIN ? 5 : 3)) || (!point && (rc = ensure(c, c->ws_tmp[2], 64 * n)))) return rc;
  for (int s = 0; s < nsrc; s++) {
    // a host source is staged up to the last covered byte of its last row: a row-strided view ends there.  A source no field reads is not read.
    const void* d;
    if ((rc = stage_in(c, PED_COMMIT_SRC_SLOT[s], srcs[s], cov[s] ? (n - 1) * strides[s] + (size_t)cov[s] : 0, &d))) return rc;
    S.rows[s] = (const uint8_t*)d; S.stride[s] = (u32)strides[s];
  }
  if ((rc = stage_in(c, 3, plan.data(), plan.size() * sizeof(PedWinSrc), &dplan)) || (rbase && (rc = stage_in(c, 5, r32, 32 * n, &dr))) ||
      (rc = stage_out(c, c->out[0], out, (point ? 64 : 32) * n, &o))) return rc;
  SoA ext = soa_of(c->ws->ext, n);
  prof_mark(c, 0);
  const unsigned gblocks = (unsigned)std::min((size_t)c->cus * c->fb_gather_blocks_per_cu, (n + 255) / 256);
  hipLaunchKernelGGL(k_pedersen_commit, dim3(gblocks), dim3(256), 0, c->stream, n, S, (const PedWinSrc*)dplan, (int)plan.size(), (const u32*)ped->dev, dr,
                     mode == PED_COMMIT_FUSED ? (const u32*)rbase->dev : nullptr, mode == PED_COMMIT_FUSED ? rbase->fp : FbParams{}, mode, ext);
  if (mode == PED_COMMIT_CHAIN && (rc = fixedbase_launch(c, rbase, n, dr, ext, /*chain=*/1))) return rc;
  prof_mark(c, 1);
  if ((rc = normalize_launch(c, n, ext, point ? o.dev : c->ws_tmp[2].p, 0))) return rc;
  if (!point) hipLaunchKernelGGL(k_affine_u, dim3(blocks_for(n)), dim3(256), 0, c->stream, n, (const void*)c->ws_tmp[2].p, o.dev);
  prof_mark(c, 2);
  bool sync = false;
  if ((rc = finish_out(c, o, &sync))) return rc;
  return finish(c, sync);
}
JJ_API int jj_batch_normalize(jj_ctx* c, size_t n, const void* ext160, void* out64) {
  if (!c) return JJ_ERR_INVALID;
  JJ_ENTER(c);
  return run_batch(c, n, {{ext160, 160, 0}}, {{out64, 64, &c->out[0]}}, 0, 0, [&](size_t n, const void* const* din, void* const* dout, bool) -> int {
    int rc;
    if ((rc = ensure_ext(c, n, 3))) return rc;
    SoA ext = soa_of(c->ws->ext, n);
    hipLaunchKernelGGL(k_ext160_to_soa, dim3(blocks_for(n)), dim3(256), 0, c->stream, n, din[0], ext);
    return normalize_launch(c, n, ext, dout[0], 0);
  });
}
