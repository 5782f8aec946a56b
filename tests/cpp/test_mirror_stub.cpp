// The wrappers of include/jubjub_hip.hpp that tests/cpp/test_mirror_calls.cpp runs on the GPU, here against the recording stub of the C ABI
// (tests/cpp/abi_stub.cpp) under -fsanitize=address,undefined: what the GPU program cannot see.  Every input vector has exactly the size its
// call needs (the stub reads all of it: a short one is a sanitizer report), and for every wrapper
//   (a) the returned container has the documented size and holds the stub's pattern over all of it;
//   (b) the stub's log line equals the one expected here: integers, flag bits, NULLs for empty and null arguments, offsets, and the row order
//       of every flattened buffer (each row has bytes of its own; the line carries a digest per row);
//   (c) every length-mismatch refusal throws jubjub::Error and leaves the log empty: nothing reached the C ABI.
// Built and run by tests/test_cpp_mirror_stub_cpu.py; a stand-alone program (exit code 0 = all passed, nothing on stderr).
#include <cstdio>
#include <cstring>
#include <set>

#include "abi_stub.h"
#include "jubjub_hip.hpp"

using namespace jubjub;
using stub::Line;
namespace tag = stub::tag;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("  FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

using Blob = std::vector<uint8_t>;
static std::set<std::string> RAN;
static void ran(const char* wrapper) { RAN.insert(wrapper); }

// n rows of N bytes, every row and every input with bytes of its own
template <size_t N>
static std::vector<std::array<uint8_t, N>> mk(size_t n, unsigned seed) {
  std::vector<std::array<uint8_t, N>> v(n);
  for (size_t r = 0; r < n; r++) for (size_t j = 0; j < N; j++) v[r][j] = (uint8_t)(seed * 29 + r * 7 + j * 3 + (r * j) % 5);
  return v;
}
static Blob mkb(size_t n, unsigned seed) {
  Blob v(n);
  for (size_t j = 0; j < n; j++) v[j] = (uint8_t)(seed * 31 + j * 5 + j / 7);
  return v;
}
static bool pattern_over(const void* p, size_t bytes, int k, int t) {
  const uint8_t* b = static_cast<const uint8_t*>(p);
  for (size_t i = 0; i < bytes; i++) if (b[i] != stub::pattern(i, k, t)) return false;
  return true;
}
// (a): the container is `rows` elements and all of it is the pattern
template <class T>
static bool holds(const std::vector<T>& v, size_t rows, int k, int t) { return v.size() == rows && pattern_over(v.data(), rows * sizeof(T), k, t); }
template <size_t N>
static bool holds(const std::array<uint8_t, N>& v, int k, int t) { return pattern_over(v.data(), N, k, t); }
// (b): the log is exactly these lines; it is emptied for the next step
static bool logged(std::initializer_list<std::string> want) {
  const std::vector<std::string> w(want);
  const bool ok = stub::log() == w;
  if (!ok) {
    std::printf("  the log differs:\n");
    for (const auto& l : stub::log()) std::printf("    got  %s\n", l.c_str());
    for (const auto& l : w) std::printf("    want %s\n", l.c_str());
  }
  stub::log().clear();
  return ok;
}
// (c): a refusal throws before the C call
template <class F>
static bool refused(F f) {
  bool threw = false;
  try { f(); } catch (const Error& e) { threw = e.status == JJ_ERR_INVALID; }
  const bool quiet = stub::log().empty();
  stub::log().clear();
  return threw && quiet;
}
template <class T>
static std::vector<T> cut(const std::vector<T>& v, size_t n) { return std::vector<T>(v.begin(), v.begin() + n); }
template <class T>
static std::vector<T> cat(const std::vector<std::vector<T>>& vs) { std::vector<T> o; for (const auto& v : vs) o.insert(o.end(), v.begin(), v.end()); return o; }
static std::string table_line(const Bytes64& base) { return Line("jj_fixedbase_table_create").i("window_bits", 0).rows("base64", base.data(), 1, 64, 64).str(); }
static const std::string FINISH = "jj_msm_finish job=set";

static void test_mul(const Context& c) {
  const size_t n = 5;
  const auto p = mk<64>(n, 1), q = mk<64>(n, 2);
  const auto a = mk<32>(n, 3), b = mk<32>(n, 4);
  const AffineBatch P(c, p), Q(c, q), P1(c, cut(p, 4)), Q1(c, cut(q, 4));
  const FrBatch A(c, a), B(c, b), A1(c, cut(a, 4)), B1(c, cut(b, 4));

  CHECK(holds(multiply_vartime(c, P, A).coords(), n, 0, tag::varbase_mul_vartime));
  CHECK(logged({Line("jj_varbase_mul_vartime").i("n", 5).rows("scalars32", a.data(), n, 32, 32).rows("points64", p.data(), n, 64, 64).str()}));
  CHECK(refused([&] { (void)multiply_vartime(c, P1, A); }) && refused([&] { (void)multiply_vartime(c, P, A1); }));
  ran("multiply_vartime");

  CHECK(holds(multiply2_vartime(c, P, A, Q, B).coords(), n, 0, tag::varbase_mul2_vartime));
  CHECK(logged({Line("jj_varbase_mul2_vartime").i("n", 5).rows("a32", a.data(), n, 32, 32).rows("p64", p.data(), n, 64, 64).rows("b32", b.data(), n, 32, 32)
                    .rows("q64", q.data(), n, 64, 64).str()}));
  CHECK(refused([&] { (void)multiply2_vartime(c, P1, A, Q, B); }) && refused([&] { (void)multiply2_vartime(c, P, A1, Q, B); }));
  CHECK(refused([&] { (void)multiply2_vartime(c, P, A, Q1, B); }) && refused([&] { (void)multiply2_vartime(c, P, A, Q, B1); }));
  CHECK(refused([&] { (void)multiply2_vartime(c, P1, A1, Q, B); }) && refused([&] { (void)multiply2_vartime(c, P, A, Q1, B1); }));
  ran("multiply2_vartime");

  const std::vector<Bytes32> ab = {a[1], b[2]};                                           // ab64 = a then b
  CHECK(holds(multiply2_scalars(c, P, a[1], Q, b[2]).coords(), n, 0, tag::varbase_mul2_scalars));
  CHECK(logged({Line("jj_varbase_mul2_scalars").i("n", 5).rows("ab64", ab.data(), 2, 32, 32).rows("p64", p.data(), n, 64, 64).rows("q64", q.data(), n, 64, 64).str()}));
  CHECK(refused([&] { (void)multiply2_scalars(c, P1, a[1], Q, b[2]); }) && refused([&] { (void)multiply2_scalars(c, P, a[1], Q1, b[2]); }));
  ran("multiply2_scalars");

  {
    const Bytes64 base = mk<64>(1, 5)[0];
    const FixedBase g(c, base);
    CHECK(logged({table_line(base)}));
    CHECK(holds(multiply_fixed_add_vartime(g, A, Q, B).coords(), n, 0, tag::fixedvar_mul_vartime));
    CHECK(logged({Line("jj_fixedvar_mul_vartime").null("t", false).i("n", 5).rows("a32", a.data(), n, 32, 32).rows("b32", b.data(), n, 32, 32).rows("q64", q.data(), n, 64, 64).str()}));
    CHECK(refused([&] { (void)multiply_fixed_add_vartime(g, A1, Q, B); }) && refused([&] { (void)multiply_fixed_add_vartime(g, A, Q1, B); }));
    CHECK(refused([&] { (void)multiply_fixed_add_vartime(g, A, Q, B1); }));
  }
  ran("multiply_fixed_add_vartime");

  const auto ext = mk<160>(3, 6);
  CHECK(holds(batch_normalize(c, ext).coords(), 3, 0, tag::batch_normalize));
  CHECK(logged({Line("jj_batch_normalize").i("n", 3).rows("ext160", ext.data(), 3, 160, 160).str()}));
  ran("batch_normalize");

  {
    HostBuffer hs(32 * n), hp(64 * n), ho(64 * n);                                        // exactly what the call reads and writes
    CHECK(hs.size() == 32 * n && hp.size() == 64 * n && ho.size() == 64 * n);
    std::memcpy(hs.data(), a.data(), 32 * n);
    std::memcpy(hp.data(), p.data(), 64 * n);
    multiply_raw(c, n, hs.data(), hp.data(), ho.data());
    CHECK(pattern_over(ho.data(), 64 * n, 0, tag::varbase_mul));
    CHECK(logged({Line("jj_varbase_mul").i("n", 5).rows("scalars32", a.data(), n, 32, 32).rows("points64", p.data(), n, 64, 64).str()}));
    const HostBuffer none(0);
    CHECK(none.size() == 0 && none.data() == nullptr);
  }
  ran("HostBuffer");
  ran("multiply_raw");
}

static void test_pedersen(const Context& c) {
  const auto gens = mk<64>(2, 7);
  const PedersenTable t(c, gens, 3, 2);
  CHECK(logged({Line("jj_pedersen_table_create").i("nseg", 2).i("seg_chunks", 3).i("window_chunks", 2).rows("gens64", gens.data(), 2, 64, 64).str()}));
  const size_t n = 5, stride = 3;
  const Blob rows = mkb(n * stride, 8);
  const std::vector<std::array<uint32_t, 2>> fields = {{0, 7}, {1, 9}};
  const uint32_t flat[4] = {0, 7, 1, 9};
  auto line = [&](Line& l) -> Line& { return l.i("row_stride", 3).i("nfields", 2).null("fields", false).list("fields", flat, 4); };
  CHECK(holds(t.hash(rows, stride, fields, 1, 1), n, 0, tag::pedersen_hash));
  CHECK(logged({line(Line("jj_pedersen_hash_vartime").null("t", false).i("n", 5).i("prefix", 1).i("prefix_bits", 1)).i("flags", 0).rows("rows", rows.data(), n, 3, 3).str()}));
  CHECK(holds(t.hash_points(rows, stride, fields, 1, 1).coords(), n, 0, tag::pedersen_point));
  CHECK(logged({line(Line("jj_pedersen_hash_vartime").null("t", false).i("n", 5).i("prefix", 1).i("prefix_bits", 1)).i("flags", JJ_PEDERSEN_POINT).rows("rows", rows.data(), n, 3, 3).str()}));
  CHECK(holds(t.scalars(rows, stride, fields, 1, 1), 2 * n, 0, tag::pedersen_scalars));          // (nseg, n): the table's own nseg and seg_chunks
  CHECK(logged({line(Line("jj_pedersen_scalars").i("nseg", 2).i("seg_chunks", 3).i("n", 5).i("prefix", 1).i("prefix_bits", 1)).rows("rows", rows.data(), n, 3, 3).str()}));
  // no fields: a NULL field array; the defaults: no prefix
  CHECK(holds(t.hash(Blob(4), 1, {}, 0xBEEF, 16), 4, 0, tag::pedersen_hash));
  CHECK(logged({"jj_pedersen_hash_vartime t=set n=4 prefix=48879 prefix_bits=16 row_stride=1 nfields=0 fields=NULL fields=[] flags=0 rows=[]"}));
  CHECK(holds(t.scalars(Blob(4), 1, {}), 8, 0, tag::pedersen_scalars));
  CHECK(logged({"jj_pedersen_scalars nseg=2 seg_chunks=3 n=4 prefix=0 prefix_bits=0 row_stride=1 nfields=0 fields=NULL fields=[] rows=[]"}));
  // the Merkle-layer call of the header's comment, on a table with the default chunk counts
  const auto gens3 = mk<64>(3, 9);
  const PedersenTable m(c, gens3);
  CHECK(logged({Line("jj_pedersen_table_create").i("nseg", 3).i("seg_chunks", 63).i("window_chunks", 0).rows("gens64", gens3.data(), 3, 64, 64).str()}));
  const Blob nodes = mkb(5 * 64, 10);
  const uint32_t mf[4] = {0, 255, 32, 255};
  CHECK(holds(m.hash(nodes, 64, {{0, 255}, {32, 255}}, 9, 6), 5, 0, tag::pedersen_hash));
  CHECK(logged({Line("jj_pedersen_hash_vartime").null("t", false).i("n", 5).i("prefix", 9).i("prefix_bits", 6).i("row_stride", 64).i("nfields", 2).null("fields", false)
                    .list("fields", mf, 4).i("flags", 0).rows("rows", nodes.data(), 5, 64, 64).str()}));
  CHECK(holds(m.scalars(nodes, 64, {{0, 255}, {32, 255}}, 9, 6), 15, 0, tag::pedersen_scalars));
  CHECK(logged({Line("jj_pedersen_scalars").i("nseg", 3).i("seg_chunks", 63).i("n", 5).i("prefix", 9).i("prefix_bits", 6).i("row_stride", 64).i("nfields", 2).null("fields", false)
                    .list("fields", mf, 4).rows("rows", nodes.data(), 5, 64, 64).str()}));
  ran("PedersenTable::hash");
  ran("PedersenTable::hash_points");
  ran("PedersenTable::scalars");
}

static void test_msm(const Context& c) {
  const size_t n = 3;
  const auto p = mk<64>(n, 11);
  const std::vector<std::vector<Bytes32>> s = {mk<32>(n, 12), mk<32>(n, 13)};
  const AffineBatch P(c, p);
  const std::vector<FrBatch> S = {FrBatch(c, s[0]), FrBatch(c, s[1])};
  const auto flat = cat(s);                                                               // B x n, row-major
  CHECK(holds(msm_batch(c, P, S).coords(), 2, 0, tag::msm_batch));
  CHECK(logged({Line("jj_msm_batch").i("B", 2).i("n", 3).i("points_shared", 1).rows("scalars32", flat.data(), 6, 32, 32).rows("points64", p.data(), 3, 64, 64).str()}));
  CHECK(refused([&] { (void)msm_batch(c, P, std::vector<FrBatch>{S[0], FrBatch(c, cut(s[1], 2))}); }));
  ran("msm_batch(shared)");

  const std::vector<std::vector<Bytes64>> pp = {mk<64>(n, 14), mk<64>(n, 15)};
  const std::vector<AffineBatch> PP = {AffineBatch(c, pp[0]), AffineBatch(c, pp[1])};
  const auto pflat = cat(pp);
  CHECK(holds(msm_batch(c, PP, S).coords(), 2, 0, tag::msm_batch));
  CHECK(logged({Line("jj_msm_batch").i("B", 2).i("n", 3).i("points_shared", 0).rows("scalars32", flat.data(), 6, 32, 32).rows("points64", pflat.data(), 6, 64, 64).str()}));
  CHECK(refused([&] { (void)msm_batch(c, PP, std::vector<FrBatch>{S[0]}); }));
  CHECK(refused([&] { (void)msm_batch(c, std::vector<AffineBatch>{PP[0], AffineBatch(c, cut(pp[1], 2))}, S); }));
  CHECK(refused([&] { (void)msm_batch(c, PP, std::vector<FrBatch>{S[0], FrBatch(c, cut(s[1], 2))}); }));
  ran("msm_batch(own)");

  const auto p5 = mk<64>(5, 16);
  const auto s5 = mk<32>(5, 17);
  const std::vector<uint64_t> off = {0, 0, 2, 5};
  CHECK(holds(msm_ragged(c, AffineBatch(c, p5), FrBatch(c, s5), off).coords(), 3, 0, tag::msm_ragged));
  CHECK(logged({Line("jj_msm_ragged").i("S", 3).null("offsets", false).list("offsets", off.data(), 4).rows("scalars32", s5.data(), 5, 32, 32).rows("points64", p5.data(), 5, 64, 64).str()}));
  CHECK(msm_ragged(c, AffineBatch(c, {}), FrBatch(c, {}), {}).len() == 0);                // no offsets: no rows
  CHECK(logged({"jj_msm_ragged S=0 offsets=NULL offsets=[] scalars32=[] points64=[]"}));
  CHECK(refused([&] { (void)msm_ragged(c, AffineBatch(c, p5), FrBatch(c, s5), {0, 0, 2, 4}); }));
  CHECK(refused([&] { (void)msm_ragged(c, AffineBatch(c, p5), FrBatch(c, cut(s5, 4)), off); }));
  ran("msm_ragged");

  const auto bp = mk<64>(6, 18);
  {
    const MsmBasis basis(c, AffineBatch(c, bp), 2, 17);
    CHECK(basis.len() == 6);
    CHECK(logged({Line("jj_msm_basis_create").i("n", 6).i("mode", 2).i("windows", 17).rows("points64", bp.data(), 6, 64, 64).str()}));
    CHECK(holds(basis.info(), 4, 0, tag::msm_basis_info));
    CHECK(logged({"jj_msm_basis_info basis=set"}));
    CHECK(holds(msm(basis, S).coords(), 2, 0, tag::msm_basis_mul));                       // rows of m = 3 < 6
    CHECK(logged({Line("jj_msm_basis_mul").null("basis", false).i("B", 2).i("m", 3).rows("scalars32", flat.data(), 6, 32, 32).str()}));
    CHECK(refused([&] { (void)msm(basis, std::vector<FrBatch>{S[0], FrBatch(c, cut(s[1], 2))}); }));
    const MsmBasis plain(c, AffineBatch(c, bp));
    CHECK(logged({Line("jj_msm_basis_create").i("n", 6).i("mode", 0).i("windows", 0).rows("points64", bp.data(), 6, 64, 64).str()}));
  }
  CHECK(logged({}));
  ran("MsmBasis");
  ran("msm(basis,rows)");
  ran("MsmBasis::info");
}

static void test_sig(const Context& c) {
  const size_t n = 3;
  const Bytes64 base = mk<64>(1, 20)[0];
  const auto R = mk<32>(n, 21), A = mk<32>(n, 22), s = mk<32>(n, 23), ch = mk<32>(n, 24);
  const auto z = mk<16>(n, 25);
  auto begin_line = [&](unsigned flags) {
    return Line("jj_sigbatch_begin").i("n", 3).i("flags", flags).rows("base64", base.data(), 1, 64, 64).rows("r32", R.data(), n, 32, 32).rows("a32", A.data(), n, 32, 32)
        .rows("s32", s.data(), n, 32, 32).rows("c32", ch.data(), n, 32, 32).rows("z16", z.data(), n, 16, 16).str();
  };
  {
    MsmJob job(c, base, R, A, s, ch, z, true);                                            // zip216 -> JJ_DECOMPRESS_ZIP216
    CHECK(holds(job.finish(), 0, tag::msm_finish));
    CHECK(logged({begin_line(JJ_DECOMPRESS_ZIP216), FINISH}));
    CHECK(refused([&] { (void)job.finish(); }));                                          // finished once
  }
  CHECK(logged({}));
  { MsmJob unfinished(c, base, R, A, s, ch, z, false); }                                   // the destructor finishes it (a leaked job: a sanitizer report)
  CHECK(logged({begin_line(0), FINISH}));
  CHECK(refused([&] { MsmJob j(c, base, R, cut(A, 2), s, ch, z, false); }) && refused([&] { MsmJob j(c, base, R, A, cut(s, 2), ch, z, false); }));
  CHECK(refused([&] { MsmJob j(c, base, R, A, s, cut(ch, 2), z, false); }) && refused([&] { MsmJob j(c, base, R, A, s, ch, cut(z, 2), false); }));
  ran("MsmJob(sig)");
  CHECK(holds(sigbatch_begin(c, base, R, A, s, ch, z)->finish(), 0, tag::msm_finish));
  CHECK(logged({begin_line(0), FINISH}));
  CHECK(holds(sigbatch_begin(c, base, R, A, s, ch, z, true)->finish(), 0, tag::msm_finish));
  CHECK(logged({begin_line(1), FINISH}));
  ran("sigbatch_begin");
  CHECK(sigbatch_verify(c, base, R, A, s, ch, z) == SigVerdict::Reject);                  // the pattern is no verdict point
  CHECK(logged({begin_line(0), FINISH}));
  CHECK(sigbatch_verify(c, base, R, A, s, ch, z, true) == SigVerdict::Reject);
  CHECK(logged({begin_line(1), FINISH}));
  CHECK(refused([&] { (void)sigbatch_verify(c, base, R, cut(A, 2), s, ch, z); }));
  ran("sigbatch_verify");

  const auto keys = mk<32>(2, 26);
  const std::vector<uint64_t> off = {0, 1, 3};
  auto keyed_line = [&](unsigned flags) {
    return Line("jj_sigbatch_keyed_begin").i("K", 2).i("flags", flags).list("offsets", off.data(), 3).rows("base64", base.data(), 1, 64, 64).rows("a32", keys.data(), 2, 32, 32)
        .rows("r32", R.data(), n, 32, 32).rows("s32", s.data(), n, 32, 32).rows("c32", ch.data(), n, 32, 32).rows("z16", z.data(), n, 16, 16).str();
  };
  {
    MsmJob job(c, base, keys, off, R, s, ch, z, true);
    CHECK(holds(job.finish(), 0, tag::msm_finish));
    CHECK(logged({keyed_line(1), FINISH}));
    CHECK(refused([&] { (void)job.finish(); }));
  }
  { MsmJob unfinished(c, base, keys, off, R, s, ch, z, false); }
  CHECK(logged({keyed_line(0), FINISH}));
  CHECK(refused([&] { MsmJob j(c, base, keys, {0, 1, 2}, R, s, ch, z, false); }) && refused([&] { MsmJob j(c, base, keys, {0, 3}, R, s, ch, z, false); }));
  CHECK(refused([&] { MsmJob j(c, base, keys, off, R, cut(s, 2), ch, z, false); }) && refused([&] { MsmJob j(c, base, keys, off, R, s, cut(ch, 2), z, false); }));
  CHECK(refused([&] { MsmJob j(c, base, keys, off, R, s, ch, cut(z, 2), false); }));
  ran("MsmJob(keyed)");
  CHECK(holds(sigbatch_keyed_begin(c, base, keys, off, R, s, ch, z)->finish(), 0, tag::msm_finish));
  CHECK(logged({keyed_line(0), FINISH}));
  CHECK(holds(sigbatch_keyed_begin(c, base, keys, off, R, s, ch, z, true)->finish(), 0, tag::msm_finish));
  CHECK(logged({keyed_line(1), FINISH}));
  ran("sigbatch_keyed_begin");
  CHECK(sigbatch_keyed_verify(c, base, keys, off, R, s, ch, z) == SigVerdict::Reject);
  CHECK(logged({keyed_line(0), FINISH}));
  CHECK(sigbatch_keyed_verify(c, base, keys, off, R, s, ch, z, true) == SigVerdict::Reject);
  CHECK(logged({keyed_line(1), FINISH}));
  CHECK(refused([&] { (void)sigbatch_keyed_verify(c, base, keys, {0, 1, 2}, R, s, ch, z); }));
  ran("sigbatch_keyed_verify");

  {
    Bytes64 ok{}, bad{}, other{}, off_curve{}, u_only{};
    ok[32] = 1;                                                                           // (0, 1)
    const uint8_t minus_one[32] = {0x00, 0x00, 0x00, 0x00, 0xff, 0xff, 0xff, 0xff, 0xfe, 0x5b, 0xfe, 0xff, 0x02, 0xa4, 0xbd, 0x53,
                                   0x05, 0xd8, 0xa1, 0x09, 0x08, 0xd8, 0x39, 0x33, 0x48, 0x7d, 0x9d, 0x29, 0x53, 0xa7, 0xed, 0x73};      // q - 1
    std::memcpy(bad.data() + 32, minus_one, 32);                                          // (0, -1)
    other = mk<64>(1, 27)[0];
    off_curve[32] = 2;                                                                    // u = 0 and neither of the two
    u_only[0] = 5; u_only[32] = 1;                                                        // v = 1 with u != 0
    CHECK(sigbatch_verdict(ok) == SigVerdict::Ok && sigbatch_verdict(bad) == SigVerdict::Malformed && sigbatch_verdict(other) == SigVerdict::Reject);
    CHECK(sigbatch_verdict(off_curve) == SigVerdict::Reject && sigbatch_verdict(u_only) == SigVerdict::Reject);
    Bytes64 near = bad; near[63] ^= 1;
    CHECK(sigbatch_verdict(near) == SigVerdict::Reject);
    Bytes64 high = ok; high[63] = 1;
    CHECK(sigbatch_verdict(high) == SigVerdict::Reject);
    CHECK(logged({}));
  }
  ran("sigbatch_verdict");

  const std::vector<uint64_t> seg = {0, 2, 2, 3};
  auto ragged_line = [&](unsigned flags) {
    return Line("jj_sigbatch_ragged").i("S", 3).i("flags", flags).null("offsets", false).list("offsets", seg.data(), 4).rows("r32", R.data(), n, 32, 32).rows("a32", A.data(), n, 32, 32)
        .rows("s32", s.data(), n, 32, 32).rows("c32", ch.data(), n, 32, 32).rows("z16", z.data(), n, 16, 16).str();
  };
  CHECK(holds(sigbatch_ragged(c, base, seg, R, A, s, ch, z), 3, 0, tag::sigbatch_ragged));
  CHECK(logged({ragged_line(0)}));
  CHECK(holds(sigbatch_ragged(c, base, seg, R, A, s, ch, z, true), 3, 0, tag::sigbatch_ragged));
  CHECK(logged({ragged_line(1)}));
  CHECK(sigbatch_ragged(c, base, {}, {}, {}, {}, {}, {}).empty());
  CHECK(logged({"jj_sigbatch_ragged S=0 flags=0 offsets=NULL offsets=[] r32=[] a32=[] s32=[] c32=[] z16=[]"}));
  CHECK(refused([&] { (void)sigbatch_ragged(c, base, {0, 2, 2, 4}, R, A, s, ch, z); }) && refused([&] { (void)sigbatch_ragged(c, base, {}, R, A, s, ch, z); }));
  CHECK(refused([&] { (void)sigbatch_ragged(c, base, seg, R, cut(A, 2), s, ch, z); }) && refused([&] { (void)sigbatch_ragged(c, base, seg, R, A, s, ch, cut(z, 2)); }));
  ran("sigbatch_ragged");
  CHECK(sigbatch_ragged_verify(c, base, seg, R, A, s, ch, z) == std::vector<SigVerdict>(3, SigVerdict::Reject));
  CHECK(logged({ragged_line(0)}));
  CHECK(sigbatch_ragged_verify(c, base, seg, R, A, s, ch, z, true).size() == 3);
  CHECK(logged({ragged_line(1)}));
  CHECK(refused([&] { (void)sigbatch_ragged_verify(c, base, {0, 2, 2, 4}, R, A, s, ch, z); }));
  ran("sigbatch_ragged_verify");

  {
    const FixedBase g(c, base);
    CHECK(logged({table_line(base)}));
    auto each_line = [&](unsigned flags) {
      return Line("jj_sigverify_each").null("t", false).i("n", 3).i("flags", flags).rows("r32", R.data(), n, 32, 32).rows("a32", A.data(), n, 32, 32).rows("s32", s.data(), n, 32, 32)
          .rows("c32", ch.data(), n, 32, 32).str();
    };
    CHECK(holds(sigverify_each(g, R, A, s, ch), n, 0, tag::sigverify_each));               // the defaults: no ZIP-216 rule, cofactored
    CHECK(logged({each_line(0)}));
    CHECK(holds(sigverify_each(g, R, A, s, ch, false, true), n, 0, tag::sigverify_each));
    CHECK(logged({each_line(0)}));
    CHECK(holds(sigverify_each(g, R, A, s, ch, false, false), n, 0, tag::sigverify_each)); // cofactored = false -> JJ_SIG_COFACTORLESS
    CHECK(logged({each_line(JJ_SIG_COFACTORLESS)}));
    CHECK(holds(sigverify_each(g, R, A, s, ch, true, true), n, 0, tag::sigverify_each));
    CHECK(logged({each_line(JJ_DECOMPRESS_ZIP216)}));
    CHECK(holds(sigverify_each(g, R, A, s, ch, true, false), n, 0, tag::sigverify_each));
    CHECK(logged({each_line(JJ_DECOMPRESS_ZIP216 | JJ_SIG_COFACTORLESS)}));
    CHECK(refused([&] { (void)sigverify_each(g, R, cut(A, 2), s, ch); }) && refused([&] { (void)sigverify_each(g, R, A, cut(s, 2), ch); }));
    CHECK(refused([&] { (void)sigverify_each(g, R, A, s, cut(ch, 2)); }));
  }
  ran("sigverify_each");

  {
    const size_t m = 5;
    const auto r5 = mk<32>(m, 28), a5 = mk<32>(m, 29);
    const std::vector<Blob> msgs = {Blob{}, mkb(1, 30), mkb(5, 31), Blob{}, mkb(3, 32)};
    const std::vector<uint64_t> sums = {0, 0, 1, 6, 6, 9};                                 // msg_len 0 and the prefix sums as offsets
    const std::array<uint8_t, 16> personal = mk<16>(1, 33)[0];
    auto ch_line = [&](bool with_personal, bool with_r, bool with_a) {
      Line l("jj_sig_challenge");
      l.i("n", 5).null("personal16", !with_personal).null("r32", !with_r).null("a32", !with_a).i("msg_len", 0).null("offsets", false);
      if (with_personal) l.rows("personal16", personal.data(), 1, 16, 16);
      l.rows("r32", r5.data(), with_r ? m : 0, 32, 32).rows("a32", a5.data(), with_a ? m : 0, 32, 32).list("offsets", sums.data(), 6);
      for (const Blob& M : msgs) l.rows("M", M.data(), 1, 0, M.size());
      return l.str();
    };
    CHECK(holds(sig_challenge(c, r5, a5, msgs, &personal), m, 0, tag::sig_challenge));
    CHECK(logged({ch_line(true, true, true)}));
    CHECK(holds(sig_challenge(c, {}, a5, msgs, &personal), m, 0, tag::sig_challenge));      // an empty R: NULL
    CHECK(logged({ch_line(true, false, true)}));
    CHECK(holds(sig_challenge(c, r5, {}, msgs, &personal), m, 0, tag::sig_challenge));      // an empty A: NULL
    CHECK(logged({ch_line(true, true, false)}));
    CHECK(holds(sig_challenge(c, r5, a5, msgs), m, 0, tag::sig_challenge));                 // personal == nullptr: NULL
    CHECK(logged({ch_line(false, true, true)}));
    CHECK(refused([&] { (void)sig_challenge(c, cut(r5, 4), a5, msgs); }) && refused([&] { (void)sig_challenge(c, r5, cut(a5, 4), msgs); }));
  }
  ran("sig_challenge");
}

static void test_ka(const Context& c) {
  const size_t n = 5;
  const auto P = mk<32>(n, 40);
  const Bytes32 sk = mk<32>(1, 41)[0];
  const std::array<uint8_t, 16> personal = mk<16>(1, 42)[0];
  const unsigned sapling = JJ_DECOMPRESS_ZIP216 | JJ_KA_COFACTOR | JJ_KA_HASH_INPUT;
  {
    const KaKeys r = ka_kdf(c, sk, P, sapling, &personal);
    CHECK(holds(r.keys, n, 0, tag::ka_kdf) && holds(r.ok, n, 1, tag::ka_kdf));
    CHECK(logged({Line("jj_ka_kdf").i("n", 5).i("flags", 97).null("personal16", false).rows("sk32", sk.data(), 1, 32, 32).rows("p32", P.data(), n, 32, 32)
                      .rows("personal16", personal.data(), 1, 16, 16).str()}));
  }
  {
    const KaKeys r = ka_kdf(c, sk, P, JJ_DECOMPRESS_ZIP216);
    CHECK(holds(r.keys, n, 0, tag::ka_kdf) && holds(r.ok, n, 1, tag::ka_kdf));
    CHECK(logged({Line("jj_ka_kdf").i("n", 5).i("flags", 1).null("personal16", true).rows("sk32", sk.data(), 1, 32, 32).rows("p32", P.data(), n, 32, 32).str()}));
  }
  ran("ka_kdf");

  const size_t m = 3, len = 8, stride = 12;
  const auto keys = mk<32>(m, 43);
  const Blob in = mkb((m - 1) * stride + len, 44);                                         // exactly the rows: nothing behind the last one
  const std::array<uint8_t, 12> nonce = mk<12>(1, 45)[0];
  CHECK(holds(chacha20_xor(c, keys, in, len, stride, 7, &nonce), m * len, 0, tag::chacha20_xor));
  CHECK(logged({Line("jj_chacha20_xor").i("n", 3).null("nonce12", false).i("counter", 7).i("len", 8).i("in_stride", 12).rows("keys32", keys.data(), m, 32, 32)
                    .rows("in", in.data(), m, stride, len).rows("nonce12", nonce.data(), 1, 12, 12).str()}));
  CHECK(holds(chacha20_xor(c, keys, in, len, stride), m * len, 0, tag::chacha20_xor));     // the defaults: counter 0, a null nonce
  CHECK(logged({Line("jj_chacha20_xor").i("n", 3).null("nonce12", true).i("counter", 0).i("len", 8).i("in_stride", 12).rows("keys32", keys.data(), m, 32, 32)
                    .rows("in", in.data(), m, stride, len).str()}));
  CHECK(holds(chacha20_xor(c, keys, in, len, stride, 0xFFFFFFFFu), m * len, 0, tag::chacha20_xor));
  CHECK(logged({Line("jj_chacha20_xor").i("n", 3).null("nonce12", true).i("counter", 4294967295ll).i("len", 8).i("in_stride", 12).rows("keys32", keys.data(), m, 32, 32)
                    .rows("in", in.data(), m, stride, len).str()}));
  CHECK(refused([&] { (void)chacha20_xor(c, keys, cut(in, in.size() - 1), len, stride); }));
  ran("chacha20_xor");
}

static void test_aead(const Context& c) {
  const size_t n = 3, len = 8;
  const auto keys = mk<32>(n, 50);
  const std::array<uint8_t, 12> nonce = mk<12>(1, 51)[0];
  const Blob aad = mkb(5, 52);
  {
    const size_t stride = 12;
    const Blob in = mkb((n - 1) * stride + len, 53);
    CHECK(holds(poly1305(c, keys, in, len, stride), n * 16, 0, tag::poly1305));
    CHECK(logged({Line("jj_poly1305").i("n", 3).i("len", 8).i("in_stride", 12).rows("keys32", keys.data(), n, 32, 32).rows("in", in.data(), n, stride, len).str()}));
    CHECK(refused([&] { (void)poly1305(c, keys, cut(in, in.size() - 1), len, stride); }));
    ran("poly1305");

    CHECK(holds(aead_seal(c, keys, in, len, stride, aad, &nonce), n * (len + 16), 0, tag::aead_seal));
    CHECK(logged({Line("jj_aead_seal").i("n", 3).null("nonce12", false).null("aad", false).i("aad_len", 5).i("len", 8).i("in_stride", 12).rows("keys32", keys.data(), n, 32, 32)
                      .rows("in", in.data(), n, stride, len).rows("aad", aad.data(), 1, 0, 5).rows("nonce12", nonce.data(), 1, 12, 12).str()}));
    CHECK(holds(aead_seal(c, keys, in, len, stride), n * (len + 16), 0, tag::aead_seal));   // the defaults: an empty aad and a null nonce are NULLs
    CHECK(logged({Line("jj_aead_seal").i("n", 3).null("nonce12", true).null("aad", true).i("aad_len", 0).i("len", 8).i("in_stride", 12).rows("keys32", keys.data(), n, 32, 32)
                      .rows("in", in.data(), n, stride, len).rows("aad", nullptr, 0, 0, 0).str()}));
    CHECK(refused([&] { (void)aead_seal(c, keys, cut(in, in.size() - 1), len, stride, aad, &nonce); }));
    ran("aead_seal");
  }
  {
    const size_t stride = 28;
    const Blob in = mkb((n - 1) * stride + len + 16, 54);                                   // the last row ends with its tag
    const AeadOpened r = aead_open(c, keys, in, len, stride, aad, &nonce);
    CHECK(holds(r.plain, n * len, 0, tag::aead_open) && holds(r.ok, n, 1, tag::aead_open));
    CHECK(logged({Line("jj_aead_open").i("n", 3).null("nonce12", false).null("aad", false).i("aad_len", 5).i("len", 8).i("in_stride", 28).rows("keys32", keys.data(), n, 32, 32)
                      .rows("in", in.data(), n, stride, len + 16).rows("aad", aad.data(), 1, 0, 5).rows("nonce12", nonce.data(), 1, 12, 12).str()}));
    const AeadOpened d = aead_open(c, keys, in, len, stride);
    CHECK(holds(d.plain, n * len, 0, tag::aead_open) && holds(d.ok, n, 1, tag::aead_open));
    CHECK(logged({Line("jj_aead_open").i("n", 3).null("nonce12", true).null("aad", true).i("aad_len", 0).i("len", 8).i("in_stride", 28).rows("keys32", keys.data(), n, 32, 32)
                      .rows("in", in.data(), n, stride, len + 16).rows("aad", nullptr, 0, 0, 0).str()}));
    CHECK(refused([&] { (void)aead_open(c, keys, cut(in, in.size() - 1), len, stride, aad, &nonce); }));   // one byte short of the last row's tag
    ran("aead_open");
  }
}

static void test_hash(const Context& c) {
  const size_t n = 3, len = 5, stride = 7;
  const Blob msgs = mkb((n - 1) * stride + len, 60);
  const Blob prefix = mkb(6, 61);
  const std::array<uint8_t, 8> personal = mk<8>(1, 62)[0];
  auto line = [&](const char* name, bool full) {
    Line l(name);
    l.i("n", 3).null("personal8", !full).null("prefix", !full).i("prefix_len", full ? 6 : 0).null("msgs", false).i("msg_len", 5).i("msg_stride", 7)
        .rows("prefix", prefix.data(), full ? 1 : 0, 0, 6).rows("msgs", msgs.data(), n, stride, len);
    if (full) l.rows("personal8", personal.data(), 1, 8, 8);
    return l;
  };
  CHECK(holds(blake2s(c, n, msgs, len, stride, prefix, &personal), n, 0, tag::blake2s));
  CHECK(logged({line("jj_blake2s", true).str()}));
  CHECK(holds(blake2s(c, n, msgs, len, stride), n, 0, tag::blake2s));                        // the defaults: an empty prefix and a null personal are NULLs
  CHECK(logged({line("jj_blake2s", false).str()}));
  CHECK(holds(blake2s(c, 4, {}, 0, 0, prefix), 4, 0, tag::blake2s));                          // empty messages: a NULL array
  CHECK(logged({Line("jj_blake2s").i("n", 4).null("personal8", true).null("prefix", false).i("prefix_len", 6).null("msgs", true).i("msg_len", 0).i("msg_stride", 0)
                    .rows("prefix", prefix.data(), 1, 0, 6).rows("msgs", nullptr, 0, 0, 0).str()}));
  CHECK(blake2s(c, 0, {}, 5, 7).empty());
  CHECK(logged({"jj_blake2s n=0 personal8=NULL prefix=NULL prefix_len=0 msgs=NULL msg_len=5 msg_stride=7 prefix=[] msgs=[]"}));
  CHECK(refused([&] { (void)blake2s(c, n, cut(msgs, msgs.size() - 1), len, stride); }) && refused([&] { (void)blake2s(c, n, msgs, len, 4); }));
  ran("blake2s");

  {
    const GroupHash r = group_hash(c, n, msgs, len, stride, 13, prefix, &personal);
    CHECK(holds(r.points, n, 0, tag::group_hash) && holds(r.ok, n, 1, tag::group_hash));
    CHECK(logged({line("jj_group_hash", true).i("flags", 13).str()}));
    const GroupHash d = group_hash(c, n, msgs, len, stride, JJ_DECOMPRESS_ZIP216);
    CHECK(holds(d.points, n, 0, tag::group_hash) && holds(d.ok, n, 1, tag::group_hash));
    CHECK(logged({line("jj_group_hash", false).i("flags", 1).str()}));
    const GroupHash e = group_hash(c, 0, {}, 5, 7, 0);
    CHECK(e.points.empty() && e.ok.empty());
    CHECK(logged({"jj_group_hash n=0 personal8=NULL prefix=NULL prefix_len=0 msgs=NULL msg_len=5 msg_stride=7 prefix=[] msgs=[] flags=0"}));
    CHECK(refused([&] { (void)group_hash(c, n, cut(msgs, msgs.size() - 1), len, stride, 0); }) && refused([&] { (void)group_hash(c, n, msgs, len, 4, 0); }));
  }
  ran("group_hash");
}

int main() {
  try {
    Context c(0);
    test_mul(c);
    test_pedersen(c);
    test_msm(c);
    test_sig(c);
    test_ka(c);
    test_aead(c);
    test_hash(c);
    CHECK(stub::log().empty());
  } catch (const Error& e) { std::printf("ERROR %d: %s\n", e.status, e.what()); return 3; }
  for (const std::string& w : RAN) std::printf("wrapper %s\n", w.c_str());
  std::printf("%s (%d failures)\n", failures ? "FAILED" : "ALL PASSED", failures);
  return failures ? 1 : 0;
}
