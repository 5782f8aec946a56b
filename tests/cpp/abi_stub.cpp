// A recording stand-in for the part of the C ABI (include/jubjub_hip.h) that tests/cpp/test_mirror_stub.cpp reaches through the C++ mirror:
// plain C++, no HIP, no device.  Linked with that program under -fsanitize=address,undefined it shows what a GPU run cannot:
//   - every data call READS every byte of each input over exactly the extent the header documents, so an input the mirror made too short is
//     a sanitizer report;
//   - it WRITES every byte of each output over exactly its documented extent -- byte i of output k is stub::pattern(i, k, tag), the tag
//     fixed per entry point -- so a result container that is too small is a sanitizer report and one that is too large keeps a tail that is
//     not the pattern;
//   - it appends one line per call to stub::log(): the entry point, every integer argument, which optional pointers were NULL, the values
//     of offsets and field arrays, and one short digest per row of every input array (the row order of a flattened buffer shows there).
// The extents are restated here from the header's text, one comment per function with the lines it rests on: this file is the one place
// where a second statement of the contract is wanted.  Handles are small heap objects, so a handle the mirror never releases is a leak report.
#include "abi_stub.h"

#include <cstdlib>
#include <cstring>

#include "jubjub_hip.h"

struct jj_ctx { int unused; };
struct jj_table { int nseg; };
struct jj_msm_basis { size_t n; };
struct jj_msm_job { int unused; };

namespace stub {
std::vector<std::string>& log() { static std::vector<std::string> lines; return lines; }
}
using stub::Line;
namespace tag = stub::tag;

static volatile uint8_t g_sink;
// reads every byte of [p, p + n)
static void touch(const void* p, size_t n) {
  const uint8_t* b = static_cast<const uint8_t*>(p);
  uint8_t x = 0;
  for (size_t i = 0; i < n; i++) x ^= b[i];
  g_sink = x;
}
// writes every byte of output k
static void fill(void* p, size_t n, int k, int t) {
  uint8_t* b = static_cast<uint8_t*>(p);
  for (size_t i = 0; i < n; i++) b[i] = stub::pattern(i, k, t);
}
static void put(const Line& l) { stub::log().push_back(l.str()); }
// rows of one strided input: the whole extent (count - 1) * stride + width is read, the digests are those of the rows
static size_t extent(size_t count, size_t stride, size_t width) { return count ? (count - 1) * stride + width : 0; }

extern "C" {

// jubjub_hip.h:60-62, 91
int jj_ctx_create(int, jj_ctx** out) { *out = new jj_ctx{0}; return JJ_OK; }
int jj_ctx_destroy(jj_ctx* c) { delete c; return JJ_OK; }
const char* jj_last_error(jj_ctx*) { return "stub"; }
// jubjub_hip.h:124-125, 135-136: *out = NULL for bytes = 0
int jj_host_alloc(size_t bytes, void** out) { *out = bytes ? std::malloc(bytes) : nullptr; return JJ_OK; }
int jj_host_free(void* p) { std::free(p); return JJ_OK; }

// jubjub_hip.h:227-238, 243-247: n x 32 scalars, n x 64 points -> n x 64
static int mul1(const char* name, int t, size_t n, const void* s, const void* p, void* out) {
  touch(s, 32 * n); touch(p, 64 * n);
  fill(out, 64 * n, 0, t);
  put(Line(name).i("n", (long long)n).rows("scalars32", s, n, 32, 32).rows("points64", p, n, 64, 64));
  return JJ_OK;
}
int jj_varbase_mul(jj_ctx*, size_t n, const void* s, const void* p, void* out) { return mul1("jj_varbase_mul", tag::varbase_mul, n, s, p, out); }
int jj_varbase_mul_vartime(jj_ctx*, size_t n, const void* s, const void* p, void* out) { return mul1("jj_varbase_mul_vartime", tag::varbase_mul_vartime, n, s, p, out); }
// jubjub_hip.h:253-271: a32, b32 n x 32, p64, q64 n x 64 -> n x 64
int jj_varbase_mul2_vartime(jj_ctx*, size_t n, const void* a, const void* p, const void* b, const void* q, void* out) {
  touch(a, 32 * n); touch(p, 64 * n); touch(b, 32 * n); touch(q, 64 * n);
  fill(out, 64 * n, 0, tag::varbase_mul2_vartime);
  put(Line("jj_varbase_mul2_vartime").i("n", (long long)n).rows("a32", a, n, 32, 32).rows("p64", p, n, 64, 64).rows("b32", b, n, 32, 32).rows("q64", q, n, 64, 64));
  return JJ_OK;
}
// jubjub_hip.h:273-275: ab64 = a then b, 64 bytes
int jj_varbase_mul2_scalars(jj_ctx*, size_t n, const void* ab, const void* p, const void* q, void* out) {
  touch(ab, 64); touch(p, 64 * n); touch(q, 64 * n);
  fill(out, 64 * n, 0, tag::varbase_mul2_scalars);
  put(Line("jj_varbase_mul2_scalars").i("n", (long long)n).rows("ab64", ab, 2, 32, 32).rows("p64", p, n, 64, 64).rows("q64", q, n, 64, 64));
  return JJ_OK;
}
// jubjub_hip.h:281-293: one base of 64 bytes
int jj_fixedbase_table_create(jj_ctx*, const void* base64, int window_bits, jj_table** out) {
  touch(base64, 64);
  *out = new jj_table{0};
  put(Line("jj_fixedbase_table_create").i("window_bits", window_bits).rows("base64", base64, 1, 64, 64));
  return JJ_OK;
}
int jj_fixedbase_table_destroy(jj_ctx*, jj_table* t) { delete t; return JJ_OK; }
// jubjub_hip.h:296-321: a32, b32 n x 32, q64 n x 64 -> n x 64
int jj_fixedvar_mul_vartime(jj_ctx*, const jj_table* t, size_t n, const void* a, const void* b, const void* q, void* out) {
  touch(a, 32 * n); touch(b, 32 * n); touch(q, 64 * n);
  fill(out, 64 * n, 0, tag::fixedvar_mul_vartime);
  put(Line("jj_fixedvar_mul_vartime").null("t", !t).i("n", (long long)n).rows("a32", a, n, 32, 32).rows("b32", b, n, 32, 32).rows("q64", q, n, 64, 64));
  return JJ_OK;
}
// jubjub_hip.h:875-878: n x 160 -> n x 64
int jj_batch_normalize(jj_ctx*, size_t n, const void* ext, void* out) {
  touch(ext, 160 * n);
  fill(out, 64 * n, 0, tag::batch_normalize);
  put(Line("jj_batch_normalize").i("n", (long long)n).rows("ext160", ext, n, 160, 160));
  return JJ_OK;
}

// jubjub_hip.h:830-837: nseg affine points
int jj_pedersen_table_create(jj_ctx*, int nseg, const void* gens, int seg_chunks, int window_chunks, jj_table** out) {
  touch(gens, 64 * (size_t)nseg);
  *out = new jj_table{nseg};
  put(Line("jj_pedersen_table_create").i("nseg", nseg).i("seg_chunks", seg_chunks).i("window_chunks", window_chunks).rows("gens64", gens, (size_t)nseg, 64, 64));
  return JJ_OK;
}
// jubjub_hip.h:838-845, 861-862: fields 2 * nfields values, rows n x row_stride (may be NULL when nfields = 0); flags 0: n x 32, JJ_PEDERSEN_POINT: n x 64
int jj_pedersen_hash_vartime(jj_ctx*, const jj_table* t, size_t n, unsigned prefix, int prefix_bits, const void* rows, size_t row_stride, int nfields,
                             const uint32_t* fields, unsigned flags, void* out) {
  if (nfields) { touch(fields, 8 * (size_t)nfields); touch(rows, n * row_stride); }
  const bool point = flags & JJ_PEDERSEN_POINT;
  fill(out, (point ? 64 : 32) * n, 0, point ? tag::pedersen_point : tag::pedersen_hash);
  put(Line("jj_pedersen_hash_vartime").null("t", !t).i("n", (long long)n).i("prefix", prefix).i("prefix_bits", prefix_bits).i("row_stride", (long long)row_stride)
          .i("nfields", nfields).null("fields", !fields).list("fields", fields, fields ? 2 * (size_t)nfields : 0).i("flags", flags)
          .rows("rows", rows, nfields ? n : 0, row_stride, row_stride));
  return JJ_OK;
}
// jubjub_hip.h:855-858, 863-864: the same message arguments; scalars32 is (nseg, n, 32)
int jj_pedersen_scalars(jj_ctx*, int nseg, int seg_chunks, size_t n, unsigned prefix, int prefix_bits, const void* rows, size_t row_stride, int nfields,
                        const uint32_t* fields, void* scalars32) {
  if (nfields) { touch(fields, 8 * (size_t)nfields); touch(rows, n * row_stride); }
  fill(scalars32, 32 * n * (size_t)nseg, 0, tag::pedersen_scalars);
  put(Line("jj_pedersen_scalars").i("nseg", nseg).i("seg_chunks", seg_chunks).i("n", (long long)n).i("prefix", prefix).i("prefix_bits", prefix_bits)
          .i("row_stride", (long long)row_stride).i("nfields", nfields).null("fields", !fields).list("fields", fields, fields ? 2 * (size_t)nfields : 0)
          .rows("rows", rows, nfields ? n : 0, row_stride, row_stride));
  return JJ_OK;
}

// jubjub_hip.h:367-381: scalars32 B x n x 32 row-major; points64 n x 64 when points_shared = 1, B x n x 64 when 0; out64 B x 64
int jj_msm_batch(jj_ctx*, size_t B, size_t n, const void* s, const void* p, int points_shared, void* out) {
  const size_t np = points_shared ? n : B * n;
  touch(s, 32 * B * n); touch(p, 64 * np);
  fill(out, 64 * B, 0, tag::msm_batch);
  put(Line("jj_msm_batch").i("B", (long long)B).i("n", (long long)n).i("points_shared", points_shared).rows("scalars32", s, B * n, 32, 32).rows("points64", p, np, 64, 64));
  return JJ_OK;
}
// jubjub_hip.h:382-391, 414: offsets S + 1 values, N = offsets[S]; scalars32 N x 32, points64 N x 64; out64 S x 64; S = 0 touches nothing
int jj_msm_ragged(jj_ctx*, size_t S, const uint64_t* offsets, const void* s, const void* p, void* out) {
  const size_t N = S ? (size_t)offsets[S] : 0;
  if (S) { touch(offsets, 8 * (S + 1)); touch(s, 32 * N); touch(p, 64 * N); }
  fill(out, 64 * S, 0, tag::msm_ragged);
  put(Line("jj_msm_ragged").i("S", (long long)S).null("offsets", !offsets).list("offsets", offsets, S ? S + 1 : 0).rows("scalars32", s, N, 32, 32).rows("points64", p, N, 64, 64));
  return JJ_OK;
}
// jubjub_hip.h:417-452: create copies n x 64 points; mul: scalars32 B x m x 32, out64 B x 64; info: four int64 values
int jj_msm_basis_create(jj_ctx*, size_t n, const void* p, int mode, int windows, jj_msm_basis** out) {
  touch(p, 64 * n);
  *out = new jj_msm_basis{n};
  put(Line("jj_msm_basis_create").i("n", (long long)n).i("mode", mode).i("windows", windows).rows("points64", p, n, 64, 64));
  return JJ_OK;
}
int jj_msm_basis_destroy(jj_ctx*, jj_msm_basis* b) { delete b; return JJ_OK; }
int jj_msm_basis_info(const jj_msm_basis* b, int64_t out[4]) {
  fill(out, 32, 0, tag::msm_basis_info);
  put(Line("jj_msm_basis_info").null("basis", !b));
  return JJ_OK;
}
int jj_msm_basis_mul(jj_ctx*, const jj_msm_basis* b, size_t B, size_t m, const void* s, void* out) {
  touch(s, 32 * B * m);
  fill(out, 64 * B, 0, tag::msm_basis_mul);
  put(Line("jj_msm_basis_mul").null("basis", !b).i("B", (long long)B).i("m", (long long)m).rows("scalars32", s, B * m, 32, 32));
  return JJ_OK;
}
// jubjub_hip.h:347-359: finish writes the 64-byte result and releases the job
int jj_msm_finish(jj_msm_job* job, void* out) {
  fill(out, 64, 0, tag::msm_finish);
  put(Line("jj_msm_finish").null("job", !job));
  delete job;
  return JJ_OK;
}

// jubjub_hip.h:498-523: base64 64 bytes; r32 a32 s32 c32 n x 32; z16 n x 16
int jj_sigbatch_begin(jj_ctx*, const void* base, size_t n, const void* r, const void* a, const void* s, const void* c, const void* z, unsigned flags, jj_msm_job** job) {
  touch(base, 64); touch(r, 32 * n); touch(a, 32 * n); touch(s, 32 * n); touch(c, 32 * n); touch(z, 16 * n);
  *job = new jj_msm_job{0};
  put(Line("jj_sigbatch_begin").i("n", (long long)n).i("flags", flags).rows("base64", base, 1, 64, 64).rows("r32", r, n, 32, 32).rows("a32", a, n, 32, 32).rows("s32", s, n, 32, 32)
          .rows("c32", c, n, 32, 32).rows("z16", z, n, 16, 16));
  return JJ_OK;
}
// jubjub_hip.h:524-550: a32 K keys; offsets K + 1 values, n = offsets[K]; r32 s32 c32 n x 32; z16 n x 16
int jj_sigbatch_keyed_begin(jj_ctx*, const void* base, size_t K, const void* a, const uint64_t* offsets, const void* r, const void* s, const void* c, const void* z, unsigned flags,
                            jj_msm_job** job) {
  touch(offsets, 8 * (K + 1));
  const size_t n = (size_t)offsets[K];
  touch(base, 64); touch(a, 32 * K); touch(r, 32 * n); touch(s, 32 * n); touch(c, 32 * n); touch(z, 16 * n);
  *job = new jj_msm_job{0};
  put(Line("jj_sigbatch_keyed_begin").i("K", (long long)K).i("flags", flags).list("offsets", offsets, K + 1).rows("base64", base, 1, 64, 64).rows("a32", a, K, 32, 32)
          .rows("r32", r, n, 32, 32).rows("s32", s, n, 32, 32).rows("c32", c, n, 32, 32).rows("z16", z, n, 16, 16));
  return JJ_OK;
}
// jubjub_hip.h:551-579: offsets S + 1 values, n = offsets[S]; the arrays of jj_sigbatch_begin; out64 S x 64; S = 0 touches nothing
int jj_sigbatch_ragged(jj_ctx*, const void* base, size_t S, const uint64_t* offsets, const void* r, const void* a, const void* s, const void* c, const void* z, unsigned flags,
                       void* out) {
  const size_t n = S ? (size_t)offsets[S] : 0;
  if (S) { touch(offsets, 8 * (S + 1)); touch(base, 64); touch(r, 32 * n); touch(a, 32 * n); touch(s, 32 * n); touch(c, 32 * n); touch(z, 16 * n); }
  fill(out, 64 * S, 0, tag::sigbatch_ragged);
  put(Line("jj_sigbatch_ragged").i("S", (long long)S).i("flags", flags).null("offsets", !offsets).list("offsets", offsets, S ? S + 1 : 0).rows("r32", r, n, 32, 32)
          .rows("a32", a, n, 32, 32).rows("s32", s, n, 32, 32).rows("c32", c, n, 32, 32).rows("z16", z, n, 16, 16));
  return JJ_OK;
}
// jubjub_hip.h:581-620: r32 a32 s32 c32 n x 32; verdict n bytes
int jj_sigverify_each(jj_ctx*, const jj_table* t, size_t n, const void* r, const void* a, const void* s, const void* c, unsigned flags, uint8_t* verdict) {
  touch(r, 32 * n); touch(a, 32 * n); touch(s, 32 * n); touch(c, 32 * n);
  fill(verdict, n, 0, tag::sigverify_each);
  put(Line("jj_sigverify_each").null("t", !t).i("n", (long long)n).i("flags", flags).rows("r32", r, n, 32, 32).rows("a32", a, n, 32, 32).rows("s32", s, n, 32, 32).rows("c32", c, n, 32, 32));
  return JJ_OK;
}
// jubjub_hip.h:622-668: personal16 16 bytes or NULL; r32 a32 n x 32 or NULL; offsets != NULL: n + 1 values, M_i = bytes offsets[i] .. offsets[i + 1] of
// msgs, msg_len 0; offsets == NULL: n x msg_len; c32 n x 32
int jj_sig_challenge(jj_ctx*, size_t n, const void* personal, const void* r, const void* a, const void* msgs, size_t msg_len, const uint64_t* offsets, void* c32) {
  if (personal) touch(personal, 16);
  if (r) touch(r, 32 * n);
  if (a) touch(a, 32 * n);
  Line l("jj_sig_challenge");
  l.i("n", (long long)n).null("personal16", !personal).null("r32", !r).null("a32", !a).i("msg_len", (long long)msg_len).null("offsets", !offsets);
  if (personal) l.rows("personal16", personal, 1, 16, 16);
  l.rows("r32", r, r ? n : 0, 32, 32).rows("a32", a, a ? n : 0, 32, 32);
  if (offsets) {
    touch(offsets, 8 * (n + 1));
    touch(msgs, (size_t)offsets[n]);
    l.list("offsets", offsets, n + 1);
    for (size_t i = 0; i < n; i++) l.rows("M", static_cast<const uint8_t*>(msgs) + offsets[i], 1, 0, (size_t)(offsets[i + 1] - offsets[i]));
  } else {
    touch(msgs, n * msg_len);
    l.rows("M", msgs, n, msg_len, msg_len);
  }
  fill(c32, 32 * n, 0, tag::sig_challenge);
  put(l);
  return JJ_OK;
}

// jubjub_hip.h:670-686, 725: sk32 32 bytes; p32 n x 32; personal16 16 bytes or NULL; key32 n x 32, ok n bytes
int jj_ka_kdf(jj_ctx*, size_t n, const void* sk, const void* p, unsigned flags, const void* personal, void* key32, uint8_t* ok) {
  touch(sk, 32); touch(p, 32 * n);
  if (personal) touch(personal, 16);
  fill(key32, 32 * n, 0, tag::ka_kdf);
  fill(ok, n, 1, tag::ka_kdf);
  Line l("jj_ka_kdf");
  l.i("n", (long long)n).i("flags", flags).null("personal16", !personal).rows("sk32", sk, 1, 32, 32).rows("p32", p, n, 32, 32);
  if (personal) l.rows("personal16", personal, 1, 16, 16);
  put(l);
  return JJ_OK;
}
// jubjub_hip.h:703-710, 726: keys32 n x 32; nonce12 12 bytes or NULL; rows of len bytes at in_stride: (n - 1) * in_stride + len bytes of in; out n x len
int jj_chacha20_xor(jj_ctx*, size_t n, const void* keys, const void* nonce, unsigned counter, const void* in, size_t len, size_t in_stride, void* out) {
  touch(keys, 32 * n); touch(in, extent(n, in_stride, len));
  if (nonce) touch(nonce, 12);
  fill(out, n * len, 0, tag::chacha20_xor);
  Line l("jj_chacha20_xor");
  l.i("n", (long long)n).null("nonce12", !nonce).i("counter", counter).i("len", (long long)len).i("in_stride", (long long)in_stride).rows("keys32", keys, n, 32, 32).rows("in", in, n, in_stride, len);
  if (nonce) l.rows("nonce12", nonce, 1, 12, 12);
  put(l);
  return JJ_OK;
}
// jubjub_hip.h:728-746, 773-776: keys32 n x 32; nonce12 12 bytes or NULL; aad aad_len bytes, NULL only with aad_len = 0; `in` is
// (n - 1) * in_stride + len bytes, plus 16 for jj_aead_open; tag16 n x 16; seal: out n x (len + 16); open: out n x len, ok n bytes
int jj_poly1305(jj_ctx*, size_t n, const void* keys, const void* in, size_t len, size_t in_stride, void* tag16) {
  touch(keys, 32 * n); touch(in, extent(n, in_stride, len));
  fill(tag16, 16 * n, 0, tag::poly1305);
  put(Line("jj_poly1305").i("n", (long long)n).i("len", (long long)len).i("in_stride", (long long)in_stride).rows("keys32", keys, n, 32, 32).rows("in", in, n, in_stride, len));
  return JJ_OK;
}
static Line aead_line(const char* name, size_t n, const void* keys, const void* nonce, const void* aad, size_t aad_len, const void* in, size_t len, size_t in_stride, size_t row) {
  touch(keys, 32 * n); touch(in, extent(n, in_stride, row));
  if (nonce) touch(nonce, 12);
  touch(aad, aad_len);
  Line l(name);
  l.i("n", (long long)n).null("nonce12", !nonce).null("aad", !aad).i("aad_len", (long long)aad_len).i("len", (long long)len).i("in_stride", (long long)in_stride)
      .rows("keys32", keys, n, 32, 32).rows("in", in, n, in_stride, row).rows("aad", aad, aad ? 1 : 0, 0, aad_len);
  if (nonce) l.rows("nonce12", nonce, 1, 12, 12);
  return l;
}
int jj_aead_open(jj_ctx*, size_t n, const void* keys, const void* nonce, const void* aad, size_t aad_len, const void* in, size_t len, size_t in_stride, void* out, uint8_t* ok) {
  const Line l = aead_line("jj_aead_open", n, keys, nonce, aad, aad_len, in, len, in_stride, len + 16);
  fill(out, n * len, 0, tag::aead_open);
  fill(ok, n, 1, tag::aead_open);
  put(l);
  return JJ_OK;
}
int jj_aead_seal(jj_ctx*, size_t n, const void* keys, const void* nonce, const void* aad, size_t aad_len, const void* in, size_t len, size_t in_stride, void* out) {
  const Line l = aead_line("jj_aead_seal", n, keys, nonce, aad, aad_len, in, len, in_stride, len);
  fill(out, n * (len + 16), 0, tag::aead_seal);
  put(l);
  return JJ_OK;
}

// jubjub_hip.h:778-794, 816-818: personal8 8 bytes or NULL; prefix prefix_len bytes, NULL only when prefix_len = 0; msgs rows of msg_len bytes at
// msg_stride, NULL only when msg_len = 0; out32 n x 32; out64 n x 64 and ok n bytes
static Line hash_line(const char* name, size_t n, const void* personal, const void* prefix, size_t prefix_len, const void* msgs, size_t msg_len, size_t msg_stride) {
  if (personal) touch(personal, 8);
  touch(prefix, prefix_len);
  if (msg_len) touch(msgs, extent(n, msg_stride, msg_len));
  Line l(name);
  l.i("n", (long long)n).null("personal8", !personal).null("prefix", !prefix).i("prefix_len", (long long)prefix_len).null("msgs", !msgs).i("msg_len", (long long)msg_len)
      .i("msg_stride", (long long)msg_stride).rows("prefix", prefix, prefix ? 1 : 0, 0, prefix_len).rows("msgs", msgs, msg_len ? n : 0, msg_stride, msg_len);
  if (personal) l.rows("personal8", personal, 1, 8, 8);
  return l;
}
int jj_blake2s(jj_ctx*, size_t n, const void* personal, const void* prefix, size_t prefix_len, const void* msgs, size_t msg_len, size_t msg_stride, void* out32) {
  const Line l = hash_line("jj_blake2s", n, personal, prefix, prefix_len, msgs, msg_len, msg_stride);
  fill(out32, 32 * n, 0, tag::blake2s);
  put(l);
  return JJ_OK;
}
int jj_group_hash(jj_ctx*, size_t n, const void* personal, const void* prefix, size_t prefix_len, const void* msgs, size_t msg_len, size_t msg_stride, unsigned flags, void* out64,
                  uint8_t* ok) {
  Line l = hash_line("jj_group_hash", n, personal, prefix, prefix_len, msgs, msg_len, msg_stride);
  l.i("flags", flags);
  fill(out64, 64 * n, 0, tag::group_hash);
  fill(ok, n, 1, tag::group_hash);
  put(l);
  return JJ_OK;
}

}  // extern "C"
