// Calls every wrapper of the C++ host mirror (include/jubjub_hip.hpp) that tests/cpp/test_reference_suite.cpp does not reach, on the GPU, and
// compares each whole result -- the size of the returned container and every byte of it -- with what the project's Python restatements
// (oracle/, tests/*_cases.py) give for the same inputs.  Inputs and expected bytes come from a text file written by tests/test_cpp_mirror.py:
// one `key hex` line per array (`-` for an empty one).  Everything goes through jubjub_hip.hpp; there is no direct jj_* call here.
// Usage: test_mirror_calls <vectors.txt> <group>      group: mul | msm | pedersen | sig | ka | aead | hash      (exit code 0 = all passed)
// One `wrapper <name>` line is printed per wrapper that was executed; the Python test holds the set of those lines to its own list.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <set>
#include <sstream>

#include "jubjub_hip.hpp"

using namespace jubjub;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("  FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

using Blob = std::vector<uint8_t>;
static std::map<std::string, Blob> G;
static void load(const char* path) {
  std::ifstream f(path);
  std::string line;
  while (std::getline(f, line)) {
    std::istringstream ss(line);
    std::string key, hex;
    if (!(ss >> key)) continue;
    Blob& o = G[key];
    while (ss >> hex) {
      if (hex == "-") continue;
      for (size_t i = 0; i + 1 < hex.size(); i += 2) o.push_back((uint8_t)std::stoi(hex.substr(i, 2), nullptr, 16));
    }
  }
}
static const Blob& blob(const std::string& key) {
  auto it = G.find(key);
  if (it == G.end()) { std::printf("missing key %s\n", key.c_str()); std::exit(2); }
  return it->second;
}
static bool has(const std::string& key) { return G.count(key) != 0; }
template <size_t N>
static std::vector<std::array<uint8_t, N>> arr(const std::string& key) {
  const Blob& b = blob(key);
  if (b.size() % N) { std::printf("bad size for %s\n", key.c_str()); std::exit(2); }
  std::vector<std::array<uint8_t, N>> o(b.size() / N);
  if (!b.empty()) std::memcpy(o.data(), b.data(), b.size());
  return o;
}
template <size_t N>
static std::array<uint8_t, N> one(const std::string& key) {
  const auto v = arr<N>(key);
  if (v.size() != 1) { std::printf("bad size for %s\n", key.c_str()); std::exit(2); }
  return v[0];
}
static std::vector<uint64_t> u64s(const std::string& key) {
  const auto v = arr<8>(key);
  std::vector<uint64_t> o(v.size());
  for (size_t i = 0; i < v.size(); i++) { o[i] = 0; for (int b = 0; b < 8; b++) o[i] |= (uint64_t)v[i][b] << (8 * b); }
  return o;
}
static uint64_t num(const std::string& key) { const auto v = u64s(key); if (v.size() != 1) { std::printf("bad size for %s\n", key.c_str()); std::exit(2); } return v[0]; }
// the whole result: the size of the container, then its bytes
template <size_t N>
static bool same(const std::vector<std::array<uint8_t, N>>& got, const std::string& key) {
  const Blob& w = blob(key);
  const bool ok = got.size() * N == w.size() && (w.empty() || std::memcmp(got.data(), w.data(), w.size()) == 0);
  if (!ok) std::printf("  differs from %s (%zu bytes against %zu)\n", key.c_str(), got.size() * N, w.size());
  return ok;
}
static bool same(const Blob& got, const std::string& key) {
  const bool ok = got == blob(key);
  if (!ok) std::printf("  differs from %s (%zu bytes against %zu)\n", key.c_str(), got.size(), blob(key).size());
  return ok;
}
template <size_t N>
static bool same(const std::array<uint8_t, N>& got, const std::string& key) { return same(std::vector<std::array<uint8_t, N>>{got}, key); }
template <class T>
static std::vector<T> cut(const std::vector<T>& v, size_t lo, size_t hi) { return std::vector<T>(v.begin() + lo, v.begin() + hi); }
template <class F>
static bool throws(F f) { try { f(); } catch (const Error&) { return true; } return false; }
static std::set<std::string> RAN;
static void ran(const char* wrapper) { RAN.insert(wrapper); }
static SigVerdict verdict_of(uint64_t v) { return v == 0 ? SigVerdict::Ok : v == 1 ? SigVerdict::Reject : SigVerdict::Malformed; }

// ---------------------------------------------------------------------------------------------------- mul
static void group_mul(const Context& c) {
  const AffineBatch P(c, arr<64>("mul.p")), Q(c, arr<64>("mul.q"));
  const FrBatch a(c, arr<32>("mul.a")), b(c, arr<32>("mul.b"));
  const size_t n = P.len();
  CHECK(n == 67 && Q.len() == n && a.len() == n && b.len() == n);
  const AffineBatch P1(c, cut(P.coords(), 0, n - 1)), Q1(c, cut(Q.coords(), 0, n - 1));
  const FrBatch a1(c, cut(a.to_bytes(), 0, n - 1)), b1(c, cut(b.to_bytes(), 0, n - 1));

  std::puts("multiply_vartime");
  CHECK(same(multiply_vartime(c, P, a).coords(), "mul.vartime"));
  CHECK(throws([&] { (void)multiply_vartime(c, P1, a); }) && throws([&] { (void)multiply_vartime(c, P, a1); }));
  ran("multiply_vartime");

  std::puts("multiply2_vartime");
  CHECK(same(multiply2_vartime(c, P, a, Q, b).coords(), "mul.mul2"));
  CHECK(throws([&] { (void)multiply2_vartime(c, P1, a, Q, b); }) && throws([&] { (void)multiply2_vartime(c, P, a1, Q, b); }));
  CHECK(throws([&] { (void)multiply2_vartime(c, P, a, Q1, b); }) && throws([&] { (void)multiply2_vartime(c, P, a, Q, b1); }));
  CHECK(throws([&] { (void)multiply2_vartime(c, P1, a1, Q, b); }) && throws([&] { (void)multiply2_vartime(c, P, a, Q1, b1); }));
  ran("multiply2_vartime");

  std::puts("multiply2_scalars");
  const Bytes32 sa = one<32>("mul.sa"), sb = one<32>("mul.sb");
  CHECK(same(multiply2_scalars(c, P, sa, Q, sb).coords(), "mul.mul2s"));
  CHECK(throws([&] { (void)multiply2_scalars(c, P1, sa, Q, sb); }) && throws([&] { (void)multiply2_scalars(c, P, sa, Q1, sb); }));
  ran("multiply2_scalars");

  std::puts("multiply_fixed_add_vartime");
  {
    const FixedBase g(c, one<64>("mul.fv.g"));
    const FrBatch fa(c, arr<32>("mul.fv.a")), fb(c, arr<32>("mul.fv.b"));
    const AffineBatch fq(c, arr<64>("mul.fv.q"));
    CHECK(fq.len() == 67);
    CHECK(same(multiply_fixed_add_vartime(g, fa, fq, fb).coords(), "mul.fv.want"));
    const FrBatch fa1(c, cut(fa.to_bytes(), 0, 66)), fb1(c, cut(fb.to_bytes(), 0, 66));
    const AffineBatch fq1(c, cut(fq.coords(), 0, 66));
    CHECK(throws([&] { (void)multiply_fixed_add_vartime(g, fa1, fq, fb); }) && throws([&] { (void)multiply_fixed_add_vartime(g, fa, fq1, fb); }));
    CHECK(throws([&] { (void)multiply_fixed_add_vartime(g, fa, fq, fb1); }));
  }
  ran("multiply_fixed_add_vartime");

  std::puts("batch_normalize");
  CHECK(same(batch_normalize(c, arr<160>("mul.ext")).coords(), "mul.norm"));
  CHECK(batch_normalize(c, {}).len() == 0);
  ran("batch_normalize");

  std::puts("HostBuffer + multiply_raw");
  {
    HostBuffer hs(32 * n), hp(64 * n), ho(64 * n);
    CHECK(hs.size() == 32 * n && hp.size() == 64 * n && ho.size() == 64 * n && hs.data() && hp.data() && ho.data());
    std::memcpy(hs.data(), a.to_bytes().data(), 32 * n);
    std::memcpy(hp.data(), P.coords().data(), 64 * n);
    std::memset(ho.data(), 0xA5, 64 * n);
    multiply_raw(c, n, hs.data(), hp.data(), ho.data());
    CHECK(same(Blob(ho.data(), ho.data() + 64 * n), "mul.raw"));
    const HostBuffer& ro = hs;                                 // the inputs were read, not written
    CHECK(std::memcmp(ro.data(), a.to_bytes().data(), 32 * n) == 0 && std::memcmp(hp.data(), P.coords().data(), 64 * n) == 0);
    HostBuffer none(0);
    CHECK(none.size() == 0);
  }
  ran("HostBuffer");
  ran("multiply_raw");
}

// ---------------------------------------------------------------------------------------------------- msm
static std::vector<FrBatch> fr_rows(const Context& c, const std::string& key, size_t B) {
  const auto flat = arr<32>(key);
  const size_t m = B ? flat.size() / B : 0;
  std::vector<FrBatch> rows;
  for (size_t b = 0; b < B; b++) rows.emplace_back(c, cut(flat, b * m, (b + 1) * m));
  return rows;
}
static void group_msm(const Context& c) {
  const AffineBatch P(c, arr<64>("msm.p"));
  const std::vector<FrBatch> S = fr_rows(c, "msm.s", 3);
  CHECK(P.len() == 40 && S.size() == 3 && S[0].len() == 40);

  std::puts("msm_batch, shared points");
  CHECK(same(msm_batch(c, P, S).coords(), "msm.shared"));
  CHECK(msm_batch(c, P, std::vector<FrBatch>{}).len() == 0);
  CHECK(throws([&] { (void)msm_batch(c, P, std::vector<FrBatch>{S[0], FrBatch(c, cut(S[1].to_bytes(), 0, 39)), S[2]}); }));
  ran("msm_batch(shared)");

  std::puts("msm_batch, own points");
  {
    const auto flat = arr<64>("msm.op");
    std::vector<AffineBatch> PP;
    for (size_t b = 0; b < 3; b++) PP.emplace_back(c, cut(flat, b * 40, (b + 1) * 40));
    const std::vector<FrBatch> SS = fr_rows(c, "msm.os", 3);
    CHECK(same(msm_batch(c, PP, SS).coords(), "msm.own"));
    CHECK(msm_batch(c, std::vector<AffineBatch>{}, std::vector<FrBatch>{}).len() == 0);
    CHECK(throws([&] { (void)msm_batch(c, PP, std::vector<FrBatch>{SS[0], SS[1]}); }));
    CHECK(throws([&] { (void)msm_batch(c, std::vector<AffineBatch>{PP[0], AffineBatch(c, cut(flat, 0, 39)), PP[2]}, SS); }));
    CHECK(throws([&] { (void)msm_batch(c, PP, std::vector<FrBatch>{SS[0], SS[1], FrBatch(c, cut(SS[2].to_bytes(), 0, 39))}); }));
  }
  ran("msm_batch(own)");

  std::puts("msm_ragged");
  {
    const std::vector<uint64_t> off = u64s("msm.offsets");
    CHECK(off.size() == 4 && off[1] == 0 && off[3] == 40);
    CHECK(same(msm_ragged(c, P, S[0], off).coords(), "msm.ragged"));
    CHECK(msm_ragged(c, P, S[0], {}).len() == 0);                                                      // no offsets: no rows
    CHECK(msm_ragged(c, AffineBatch(c, {}), FrBatch(c, {}), {}).len() == 0);
    CHECK(same(msm_ragged(c, AffineBatch(c, {}), FrBatch(c, {}), {0, 0, 0}).coords(), "msm.ragged_empty"));   // empty runs: identities
    CHECK(throws([&] { (void)msm_ragged(c, P, S[0], {0, 0, 5, 39}); }));
    CHECK(throws([&] { (void)msm_ragged(c, P, FrBatch(c, cut(S[0].to_bytes(), 0, 39)), off); }));
  }
  ran("msm_ragged");

  std::puts("MsmBasis, msm(basis, rows), info()");
  {
    const AffineBatch BP(c, arr<64>("msm.bp"));
    const std::vector<FrBatch> rows = fr_rows(c, "msm.bs", 2);
    CHECK(BP.len() == 64 && rows.size() == 2 && rows[0].len() == 40);
    for (int mode = 1; mode <= 2; mode++) {
      const MsmBasis basis(c, BP, mode);
      CHECK(basis.len() == 64);
      const std::vector<int64_t> info = basis.info();
      CHECK(info.size() == 4 && info[0] == 64 && info[1] == mode && info[3] > 0);
      CHECK(same(msm(basis, rows).coords(), "msm.basis"));
      CHECK(msm(basis, std::vector<FrBatch>{}).len() == 0);
      CHECK(throws([&] { (void)msm(basis, std::vector<FrBatch>{rows[0], FrBatch(c, cut(rows[1].to_bytes(), 0, 39))}); }));
    }
  }
  ran("MsmBasis");
  ran("msm(basis,rows)");
  ran("MsmBasis::info");
}

// ---------------------------------------------------------------------------------------------------- pedersen
// params: row_stride, prefix, prefix_bits, n; fields: byte_offset, nbits, ...
static void pedersen_case(const Context& c, const PedersenTable& t, const std::vector<const FixedBase*>& bases, const std::string& k) {
  std::printf("PedersenTable %s\n", k.c_str());
  const std::vector<uint64_t> par = u64s(k + ".params"), fl = u64s(k + ".fields");
  const size_t stride = par[0], n = par[3];
  const unsigned prefix = (unsigned)par[1];
  const int prefix_bits = (int)par[2];
  std::vector<std::array<uint32_t, 2>> fields;
  for (size_t i = 0; i + 1 < fl.size(); i += 2) fields.push_back({(uint32_t)fl[i], (uint32_t)fl[i + 1]});
  const Blob& rows = blob(k + ".rows");
  CHECK(rows.size() == n * stride);
  const AffineBatch pts = t.hash_points(rows, stride, fields, prefix, prefix_bits);
  CHECK(same(pts.coords(), k + ".points"));
  CHECK(same(t.hash(rows, stride, fields, prefix, prefix_bits), k + ".hash"));
  const std::vector<Bytes32> sc = t.scalars(rows, stride, fields, prefix, prefix_bits);
  CHECK(same(sc, k + ".scalars"));                                                                      // (nseg, n) segment-major
  CHECK(sc.size() == n * bases.size());
  if (sc.size() == n * bases.size()) {
    std::vector<std::vector<Bytes32>> by_seg;
    for (size_t j = 0; j < bases.size(); j++) by_seg.push_back(cut(sc, j * n, (j + 1) * n));
    CHECK(fixedbase_multi_mul(bases, by_seg) == pts);                                                   // the composed route gives hash_points' bytes
  }
}
static void group_pedersen(const Context& c) {
  {
    const auto gens = arr<64>("ped.gens2");
    CHECK(gens.size() == 2);
    const PedersenTable t(c, gens, 3);
    const FixedBase f0(c, gens[0]), f1(c, gens[1]);
    pedersen_case(c, t, {&f0, &f1}, "ped.one_segment");
    pedersen_case(c, t, {&f0, &f1}, "ped.both_segments");
    CHECK(t.hash({}, 2, {{0, 7}}).empty() && t.hash_points({}, 2, {{0, 7}}).len() == 0 && t.scalars({}, 2, {{0, 7}}).empty());
  }
  {
    const auto gens = arr<64>("ped.gens3");
    CHECK(gens.size() == 3);
    const PedersenTable t(c, gens);                                                                     // seg_chunks 63
    const FixedBase f0(c, gens[0]), f1(c, gens[1]), f2(c, gens[2]);
    // the Merkle-layer call as the header's comment writes it
    const Blob& nodes = blob("ped.merkle.rows");
    const unsigned layer = (unsigned)u64s("ped.merkle.params")[1];
    CHECK(u64s("ped.merkle.params")[0] == 64 && u64s("ped.merkle.params")[2] == 6 && nodes.size() == 5 * 64);
    CHECK(same(t.hash(nodes, 64, {{0, 255}, {32, 255}}, layer, 6), "ped.merkle.hash"));
    pedersen_case(c, t, {&f0, &f1, &f2}, "ped.merkle");
  }
  ran("PedersenTable::hash");
  ran("PedersenTable::hash_points");
  ran("PedersenTable::scalars");
}

// ---------------------------------------------------------------------------------------------------- sig
struct SigArrays {
  Bytes64 base;
  std::vector<Bytes32> R, A, s, ch;
  std::vector<Bytes16> z;
  bool zip216;
};
static SigArrays sig_arrays(const std::string& k) {
  SigArrays x{one<64>(k + ".base"), arr<32>(k + ".r"), has(k + ".a") ? arr<32>(k + ".a") : std::vector<Bytes32>{}, arr<32>(k + ".s"), arr<32>(k + ".c"),
              has(k + ".z") ? arr<16>(k + ".z") : std::vector<Bytes16>{}, num(k + ".zip216") != 0};
  return x;
}
static void group_sig(const Context& c) {
  std::puts("sigbatch_begin / sigbatch_verify / MsmJob");
  const uint64_t nb = num("sig.batches");
  for (uint64_t i = 0; i < nb; i++) {
    const std::string k = "sig.b" + std::to_string(i);
    const SigArrays x = sig_arrays(k);
    CHECK(x.R.size() == 9);
    CHECK(sigbatch_verify(c, x.base, x.R, x.A, x.s, x.ch, x.z, x.zip216) == verdict_of(num(k + ".verdict")));
    std::unique_ptr<MsmJob> job = sigbatch_begin(c, x.base, x.R, x.A, x.s, x.ch, x.z, x.zip216);
    CHECK(same(job->finish(), k + ".out"));
    CHECK(throws([&] { (void)job->finish(); }));                                                       // a job is finished once
    if (i == 0) {
      { std::unique_ptr<MsmJob> unfinished = sigbatch_begin(c, x.base, x.R, x.A, x.s, x.ch, x.z, x.zip216); }      // destroyed unfinished
      { MsmJob direct(c, x.base, x.R, x.A, x.s, x.ch, x.z, x.zip216); CHECK(same(direct.finish(), k + ".out")); }
      CHECK(sigbatch_verify(c, x.base, x.R, x.A, x.s, x.ch, x.z, x.zip216) == verdict_of(num(k + ".verdict")));   // the context still serves
      const auto A1 = cut(x.A, 0, 8); const auto s1 = cut(x.s, 0, 8); const auto c1 = cut(x.ch, 0, 8); const auto z1 = cut(x.z, 0, 8);
      CHECK(throws([&] { (void)sigbatch_verify(c, x.base, x.R, A1, x.s, x.ch, x.z); }) && throws([&] { (void)sigbatch_verify(c, x.base, x.R, x.A, s1, x.ch, x.z); }));
      CHECK(throws([&] { (void)sigbatch_begin(c, x.base, x.R, x.A, x.s, c1, x.z); }) && throws([&] { (void)sigbatch_begin(c, x.base, x.R, x.A, x.s, x.ch, z1); }));
    }
  }
  ran("sigbatch_begin"); ran("sigbatch_verify"); ran("MsmJob(sig)");

  std::puts("sigbatch_keyed_begin / sigbatch_keyed_verify / MsmJob");
  const uint64_t nk = num("sig.keyed");
  for (uint64_t i = 0; i < nk; i++) {
    const std::string k = "sig.k" + std::to_string(i);
    const SigArrays x = sig_arrays(k);
    const std::vector<Bytes32> keys = arr<32>(k + ".keys");
    const std::vector<uint64_t> off = u64s(k + ".offsets");
    CHECK(x.R.size() == 9);
    CHECK(sigbatch_keyed_verify(c, x.base, keys, off, x.R, x.s, x.ch, x.z, x.zip216) == verdict_of(num(k + ".verdict")));
    std::unique_ptr<MsmJob> job = sigbatch_keyed_begin(c, x.base, keys, off, x.R, x.s, x.ch, x.z, x.zip216);
    CHECK(same(job->finish(), k + ".out"));
    CHECK(throws([&] { (void)job->finish(); }));
    if (i == 0) {
      { std::unique_ptr<MsmJob> unfinished = sigbatch_keyed_begin(c, x.base, keys, off, x.R, x.s, x.ch, x.z, x.zip216); }
      { MsmJob direct(c, x.base, keys, off, x.R, x.s, x.ch, x.z, x.zip216); CHECK(same(direct.finish(), k + ".out")); }
      std::vector<uint64_t> bad = off; bad.back() -= 1;
      CHECK(throws([&] { (void)sigbatch_keyed_verify(c, x.base, keys, bad, x.R, x.s, x.ch, x.z); }));
      CHECK(throws([&] { (void)sigbatch_keyed_verify(c, x.base, keys, cut(off, 0, off.size() - 1), x.R, x.s, x.ch, x.z); }));
      CHECK(throws([&] { (void)sigbatch_keyed_begin(c, x.base, keys, off, x.R, cut(x.s, 0, 8), x.ch, x.z); }));
      CHECK(throws([&] { (void)sigbatch_keyed_begin(c, x.base, keys, off, x.R, x.s, cut(x.ch, 0, 8), x.z); }));
      CHECK(throws([&] { (void)sigbatch_keyed_begin(c, x.base, keys, off, x.R, x.s, x.ch, cut(x.z, 0, 8)); }));
    }
  }
  ran("sigbatch_keyed_begin"); ran("sigbatch_keyed_verify"); ran("MsmJob(keyed)");

  std::puts("sigbatch_verdict");
  {
    const auto pts = arr<64>("sig.verdict.points");
    const Blob& want = blob("sig.verdict.want");
    CHECK(pts.size() == want.size() && pts.size() >= 4);
    for (size_t i = 0; i < pts.size() && i < want.size(); i++) CHECK(sigbatch_verdict(pts[i]) == verdict_of(want[i]));
  }
  ran("sigbatch_verdict");

  std::puts("sigbatch_ragged / sigbatch_ragged_verify");
  const uint64_t nr = num("sig.ragged");
  for (uint64_t i = 0; i < nr; i++) {
    const std::string k = "sig.r" + std::to_string(i);
    const SigArrays x = sig_arrays(k);
    const std::vector<uint64_t> off = u64s(k + ".offsets");
    CHECK(same(sigbatch_ragged(c, x.base, off, x.R, x.A, x.s, x.ch, x.z, x.zip216), k + ".out"));
    const std::vector<SigVerdict> v = sigbatch_ragged_verify(c, x.base, off, x.R, x.A, x.s, x.ch, x.z, x.zip216);
    const Blob& want = blob(k + ".verdicts");
    CHECK(v.size() == want.size() && v.size() + 1 == off.size());
    for (size_t g = 0; g < v.size() && g < want.size(); g++) CHECK(v[g] == verdict_of(want[g]));
    if (i == 0) {
      std::vector<uint64_t> bad = off; bad.back() += 1;
      CHECK(throws([&] { (void)sigbatch_ragged(c, x.base, bad, x.R, x.A, x.s, x.ch, x.z); }) && throws([&] { (void)sigbatch_ragged(c, x.base, {}, x.R, x.A, x.s, x.ch, x.z); }));
      CHECK(throws([&] { (void)sigbatch_ragged_verify(c, x.base, off, x.R, cut(x.A, 0, x.A.size() - 1), x.s, x.ch, x.z); }));
      CHECK(sigbatch_ragged(c, x.base, {}, {}, {}, {}, {}, {}).empty() && sigbatch_ragged_verify(c, x.base, {}, {}, {}, {}, {}, {}).empty());
    }
  }
  ran("sigbatch_ragged"); ran("sigbatch_ragged_verify");

  std::puts("sigverify_each");
  const uint64_t ne = num("sig.each");
  for (uint64_t i = 0; i < ne; i++) {
    const std::string k = "sig.e" + std::to_string(i);
    const SigArrays x = sig_arrays(k);
    const FixedBase g(c, x.base);
    CHECK(x.R.size() == 67);
    CHECK(same(sigverify_each(g, x.R, x.A, x.s, x.ch, x.zip216, true), k + ".cofactored"));
    CHECK(same(sigverify_each(g, x.R, x.A, x.s, x.ch, x.zip216, false), k + ".cofactorless"));
    if (!x.zip216) CHECK(same(sigverify_each(g, x.R, x.A, x.s, x.ch), k + ".cofactored"));            // the defaults: no ZIP-216 rule, cofactored
    CHECK(blob(k + ".cofactored") != blob(k + ".cofactorless"));
    if (i == 0) {
      CHECK(throws([&] { (void)sigverify_each(g, x.R, cut(x.A, 0, 66), x.s, x.ch); }) && throws([&] { (void)sigverify_each(g, x.R, x.A, cut(x.s, 0, 66), x.ch); }));
      CHECK(throws([&] { (void)sigverify_each(g, x.R, x.A, x.s, cut(x.ch, 0, 66)); }));
      CHECK(sigverify_each(g, {}, {}, {}, {}).empty());
    }
  }
  ran("sigverify_each");

  std::puts("sig_challenge");
  {
    const std::vector<Bytes32> R = arr<32>("sig.ch.r"), A = arr<32>("sig.ch.a");
    const std::vector<uint64_t> lens = u64s("sig.ch.lens");
    const Blob& flat = blob("sig.ch.msgs");
    std::vector<Blob> msgs;
    size_t o = 0;
    for (uint64_t L : lens) { msgs.emplace_back(flat.begin() + o, flat.begin() + o + L); o += L; }
    CHECK(o == flat.size() && msgs.size() == 5 && msgs[0].empty() && msgs[4].size() == 129);
    const std::array<uint8_t, 16> personal = one<16>("sig.ch.personal");
    CHECK(same(sig_challenge(c, R, A, msgs, &personal), "sig.ch.both"));
    CHECK(same(sig_challenge(c, {}, A, msgs, &personal), "sig.ch.no_r"));
    CHECK(same(sig_challenge(c, R, {}, msgs, &personal), "sig.ch.no_a"));
    CHECK(same(sig_challenge(c, R, A, msgs), "sig.ch.null_personal"));
    CHECK(sig_challenge(c, {}, {}, {}).empty());
    CHECK(throws([&] { (void)sig_challenge(c, cut(R, 0, 4), A, msgs); }) && throws([&] { (void)sig_challenge(c, R, cut(A, 0, 4), msgs); }));
  }
  ran("sig_challenge");
}

// ---------------------------------------------------------------------------------------------------- ka
static void group_ka(const Context& c) {
  std::puts("ka_kdf");
  const std::vector<Bytes32> P = arr<32>("ka.p");
  const Bytes32 sk = one<32>("ka.sk");
  CHECK(P.size() == 67);
  const uint64_t nk = num("ka.cases");
  for (uint64_t i = 0; i < nk; i++) {
    const std::string k = "ka.k" + std::to_string(i);
    const unsigned flags = (unsigned)num(k + ".flags");
    KaKeys r;
    if (has(k + ".personal")) { const std::array<uint8_t, 16> personal = one<16>(k + ".personal"); r = ka_kdf(c, sk, P, flags, &personal); }
    else r = ka_kdf(c, sk, P, flags);
    CHECK(same(r.keys, k + ".keys"));
    CHECK(same(r.ok, k + ".ok"));
  }
  { const KaKeys r = ka_kdf(c, sk, {}, JJ_DECOMPRESS_ZIP216); CHECK(r.keys.empty() && r.ok.empty()); }
  ran("ka_kdf");

  std::puts("chacha20_xor");
  const uint64_t nc = num("ka.ciphers");
  for (uint64_t i = 0; i < nc; i++) {
    const std::string k = "ka.c" + std::to_string(i);
    const std::vector<Bytes32> keys = arr<32>(k + ".keys");
    const Blob& in = blob(k + ".in");
    const size_t len = num(k + ".len"), stride = num(k + ".stride");
    const uint32_t counter = (uint32_t)num(k + ".counter");
    CHECK(keys.size() == 67 && in.size() == 66 * stride + len);
    Blob out;
    if (has(k + ".nonce")) { const std::array<uint8_t, 12> nonce = one<12>(k + ".nonce"); out = chacha20_xor(c, keys, in, len, stride, counter, &nonce); }
    else out = chacha20_xor(c, keys, in, len, stride, counter);
    CHECK(same(out, k + ".out"));
    CHECK(throws([&] { (void)chacha20_xor(c, keys, Blob(in.begin(), in.end() - 1), len, stride, counter); }));
  }
  CHECK(chacha20_xor(c, {}, {}, 52, 60).empty());
  ran("chacha20_xor");
}

// ---------------------------------------------------------------------------------------------------- aead
static void group_aead(const Context& c) {
  const uint64_t nc = num("aead.cases");
  for (uint64_t i = 0; i < nc; i++) {
    const std::string k = "aead.c" + std::to_string(i);
    const size_t len = num(k + ".len"), stride = num(k + ".stride");
    const std::vector<Bytes32> keys = arr<32>(k + ".keys");
    const Blob& plain = blob(k + ".plain");
    const Blob& aad = blob(k + ".aad");
    const bool with_nonce = has(k + ".nonce");
    std::array<uint8_t, 12> nonce{};
    if (with_nonce) nonce = one<12>(k + ".nonce");
    const std::array<uint8_t, 12>* np = with_nonce ? &nonce : nullptr;
    const size_t n = keys.size();
    std::printf("aead len %zu stride %zu aad %zu nonce %s\n", len, stride, aad.size(), with_nonce ? "given" : "null");
    CHECK(n == 67 && plain.size() == (n - 1) * stride + len);
    if (has(k + ".tags")) {
      CHECK(same(poly1305(c, keys, plain, len, stride), k + ".tags"));
      CHECK(throws([&] { (void)poly1305(c, keys, Blob(plain.begin(), plain.end() - 1), len, stride); }));
    }
    CHECK(same(aad.empty() && !np ? aead_seal(c, keys, plain, len, stride) : aead_seal(c, keys, plain, len, stride, aad, np), k + ".sealed"));
    CHECK(throws([&] { (void)aead_seal(c, keys, Blob(plain.begin(), plain.end() - 1), len, stride, aad, np); }));
    const std::vector<Bytes32> okeys = arr<32>(k + ".open_keys");
    const Blob& rows = blob(k + ".open_in");
    CHECK(rows.size() == (n - 1) * stride + len + 16);
    const AeadOpened r = aad.empty() && !np ? aead_open(c, okeys, rows, len, stride) : aead_open(c, okeys, rows, len, stride, aad, np);
    CHECK(same(r.plain, k + ".opened"));
    CHECK(same(r.ok, k + ".ok"));
    CHECK(throws([&] { (void)aead_open(c, okeys, Blob(rows.begin(), rows.end() - 1), len, stride, aad, np); }));   // one byte short of the last row's tag
  }
  CHECK(poly1305(c, {}, {}, 64, 64).empty() && aead_seal(c, {}, {}, 64, 64).empty());
  { const AeadOpened r = aead_open(c, {}, {}, 64, 80); CHECK(r.plain.empty() && r.ok.empty()); }
  ran("poly1305"); ran("aead_seal"); ran("aead_open");
}

// ---------------------------------------------------------------------------------------------------- hash
static void group_hash(const Context& c) {
  const uint64_t nc = num("hash.cases");
  for (uint64_t i = 0; i < nc; i++) {
    const std::string k = "hash.c" + std::to_string(i);
    const size_t n = num(k + ".n"), len = num(k + ".len"), stride = num(k + ".stride");
    const unsigned flags = (unsigned)num(k + ".flags");
    const Blob& msgs = blob(k + ".msgs");
    const Blob& prefix = blob(k + ".prefix");
    const bool with_personal = has(k + ".personal");
    std::array<uint8_t, 8> personal{};
    if (with_personal) personal = one<8>(k + ".personal");
    const std::array<uint8_t, 8>* pp = with_personal ? &personal : nullptr;
    std::printf("blake2s / group_hash n %zu msg_len %zu stride %zu prefix %zu personal %s flags %u\n", n, len, stride, prefix.size(), with_personal ? "given" : "null", flags);
    CHECK(msgs.size() == (n && len ? (n - 1) * stride + len : 0));
    const bool defaults = prefix.empty() && !pp;
    CHECK(same(defaults ? blake2s(c, n, msgs, len, stride) : blake2s(c, n, msgs, len, stride, prefix, pp), k + ".digests"));
    const GroupHash r = defaults ? group_hash(c, n, msgs, len, stride, flags) : group_hash(c, n, msgs, len, stride, flags, prefix, pp);
    CHECK(same(r.points, k + ".points"));
    CHECK(same(r.ok, k + ".ok"));
    if (n && len) {
      CHECK(throws([&] { (void)blake2s(c, n, Blob(msgs.begin(), msgs.end() - 1), len, stride, prefix, pp); }));
      CHECK(throws([&] { (void)group_hash(c, n, Blob(msgs.begin(), msgs.end() - 1), len, stride, flags, prefix, pp); }));
      CHECK(throws([&] { (void)blake2s(c, n, msgs, len, len - 1, prefix, pp); }) && throws([&] { (void)group_hash(c, n, msgs, len, len - 1, flags, prefix, pp); }));
    }
  }
  ran("blake2s"); ran("group_hash");
}

int main(int argc, char** argv) {
  if (argc < 3) { std::puts("usage: test_mirror_calls vectors.txt group"); return 2; }
  load(argv[1]);
  const std::string group = argv[2];
  try {
    Context c(0);
    if (group == "mul") group_mul(c);
    else if (group == "msm") group_msm(c);
    else if (group == "pedersen") group_pedersen(c);
    else if (group == "sig") group_sig(c);
    else if (group == "ka") group_ka(c);
    else if (group == "aead") group_aead(c);
    else if (group == "hash") group_hash(c);
    else { std::printf("unknown group %s\n", group.c_str()); return 2; }
  } catch (const Error& e) { std::printf("ERROR %d: %s\n", e.status, e.what()); return 3; }
  for (const std::string& w : RAN) std::printf("wrapper %s\n", w.c_str());
  std::printf("%s (%d failures)\n", failures ? "FAILED" : "ALL PASSED", failures);
  return failures ? 1 : 0;
}
