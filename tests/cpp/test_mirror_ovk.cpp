// Calls ka_kdf_each and blake2b of the C++ host mirror (include/jubjub_hip.hpp) on the GPU and compares each whole result -- the size of the
// returned container and every byte of it -- with what the restatements of tests/ovk_cases.py give for the same inputs.  Inputs and expected
// bytes come from a text file written by tests/test_cpp_mirror_ovk.py: one `key hex` line per array (`-` for an empty one).  Everything goes
// through jubjub_hip.hpp; there is no direct jj_* call here.
// Usage: test_mirror_ovk <vectors.txt>      (exit code 0 = all passed)
// One `wrapper <name>` line is printed per wrapper that was executed; the Python test holds the set of those lines to its own list.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
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
template <size_t N>
static std::vector<std::array<uint8_t, N>> arr(const std::string& key) {
  const Blob& b = blob(key);
  if (b.size() % N) { std::printf("bad size for %s\n", key.c_str()); std::exit(2); }
  std::vector<std::array<uint8_t, N>> o(b.size() / N);
  if (!b.empty()) std::memcpy(o.data(), b.data(), b.size());
  return o;
}
static std::vector<uint64_t> u64s(const std::string& key) {
  const auto v = arr<8>(key);
  std::vector<uint64_t> o(v.size());
  for (size_t i = 0; i < v.size(); i++) { o[i] = 0; for (int b = 0; b < 8; b++) o[i] |= (uint64_t)v[i][b] << (8 * b); }
  return o;
}
// the whole result: the size of the container, then its bytes
template <size_t N>
static bool same(const std::vector<std::array<uint8_t, N>>& got, const std::string& key) {
  const Blob& w = blob(key);
  const bool ok = got.size() * N == w.size() && (w.empty() || std::memcmp(got.data(), w.data(), w.size()) == 0);
  if (!ok) std::printf("  differs from %s (%zu bytes against %zu)\n", key.c_str(), got.size() * N, w.size());
  return ok;
}
static bool same(const Blob& got, const std::string& key) {
  const Blob& w = blob(key);
  const bool ok = got == w;
  if (!ok) std::printf("  differs from %s (%zu bytes against %zu)\n", key.c_str(), got.size(), w.size());
  return ok;
}
template <class F>
static bool throws(F f) { try { f(); } catch (const Error&) { return true; } return false; }
static std::array<uint8_t, 16> personal_of(const std::string& key) {
  std::array<uint8_t, 16> p{};
  const Blob& b = blob(key);
  if (b.size() != 16) { std::printf("bad size for %s\n", key.c_str()); std::exit(2); }
  std::memcpy(p.data(), b.data(), 16);
  return p;
}

// ka.flags: one set of flags per sub-case j; ka.sk, ka.p, ka.h: n x 32; ka.keys<j>, ka.ok<j>: with h where the flags hash a second part and j is odd
static void ka_case(const Context& c) {
  std::printf("ka_kdf_each\n");
  const std::vector<Bytes32> sk = arr<32>("ka.sk"), P = arr<32>("ka.p"), h = arr<32>("ka.h");
  const std::array<uint8_t, 16> personal = personal_of("ka.personal");
  const std::vector<uint64_t> flags = u64s("ka.flags");
  for (size_t j = 0; j < flags.size(); j++) {
    const bool with_h = (flags[j] & JJ_KA_HASH_INPUT) && (j & 1);
    const KaKeys r = ka_kdf_each(c, sk, P, (unsigned)flags[j], with_h ? &h : nullptr, &personal);
    CHECK(same(r.keys, "ka.keys" + std::to_string(j)));
    CHECK(same(r.ok, "ka.ok" + std::to_string(j)));
  }
  const KaKeys z = ka_kdf_each(c, sk, P, (unsigned)flags[0]);                          // the default personalisation: sixteen zero bytes
  CHECK(same(z.keys, "ka.keys_null") && same(z.ok, "ka.ok0"));
  const KaKeys e = ka_kdf_each(c, {}, {}, (unsigned)flags[0]);                         // no units: empty containers
  CHECK(e.keys.empty() && e.ok.empty());
  CHECK(throws([&] { ka_kdf_each(c, std::vector<Bytes32>(sk.begin(), sk.end() - 1), P, (unsigned)flags[0]); }));      // fewer scalars than points
  CHECK(throws([&] { ka_kdf_each(c, sk, P, 0u, &h); }));                               // h without JJ_KA_HASH_INPUT: JJ_ERR_INVALID from the library
  CHECK(throws([&] { ka_kdf_each(c, sk, P, 8u); }));                                   // a flag that is not allowed
}

// b2b.<k>.params: digest_len, n, nsrc; .lens, .strides, .skews: one per source; .array<s>: the backing bytes; .prefix, .personal; .want
static void b2b_case(const Context& c, const std::string& k) {
  std::printf("blake2b %s\n", k.c_str());
  const std::vector<uint64_t> par = u64s(k + ".params"), ln = u64s(k + ".lens"), st = u64s(k + ".strides"), sk = u64s(k + ".skews");
  const int digest_len = (int)par[0];
  const size_t n = par[1], nsrc = par[2];
  std::vector<Blob> arrays;
  std::vector<const uint8_t*> sources;
  for (size_t s = 0; s < nsrc; s++) arrays.push_back(blob(k + ".array" + std::to_string(s)));
  for (size_t s = 0; s < nsrc; s++) sources.push_back(arrays[s].data() + sk[s]);
  const std::vector<size_t> lens(ln.begin(), ln.end()), strides(st.begin(), st.end());
  const std::array<uint8_t, 16> personal = personal_of(k + ".personal");
  CHECK(same(blake2b(c, n, digest_len, sources, lens, strides, blob(k + ".prefix"), &personal), k + ".want"));
  CHECK(same(blake2b(c, n, digest_len, sources, lens, strides, blob(k + ".prefix")), k + ".want_null"));
  CHECK(blake2b(c, 0, digest_len, sources, lens, strides, blob(k + ".prefix")).empty());
  CHECK(throws([&] { blake2b(c, n, 48, sources, lens, strides); }));                   // a digest length that is not allowed
  if (nsrc) {
    CHECK(throws([&] { blake2b(c, n, digest_len, sources, {lens[0]}, strides); }) == (nsrc > 1));      // fewer lengths than sources
    std::vector<size_t> odd = lens;
    odd[0] += 2;
    CHECK(throws([&] { blake2b(c, n, digest_len, sources, odd, strides); }));          // JJ_ERR_INVALID from the library: a length that is no multiple of 4
  }
}

int main(int argc, char** argv) {
  if (argc < 2) { std::puts("usage: test_mirror_ovk vectors.txt"); return 2; }
  load(argv[1]);
  try {
    Context c(0);
    ka_case(c);
    for (const uint64_t i : u64s("b2b.count")) for (uint64_t k = 0; k < i; k++) b2b_case(c, "b2b." + std::to_string(k));
  } catch (const Error& e) { std::printf("ERROR %d: %s\n", e.status, e.what()); return 3; }
  std::printf("wrapper ka_kdf_each\nwrapper blake2b\n");
  std::printf("%s (%d failures)\n", failures ? "FAILED" : "ALL PASSED", failures);
  return failures ? 1 : 0;
}
