// Calls PedersenTable::commit and PedersenTable::commit_points of the C++ host mirror (include/jubjub_hip.hpp) on the GPU and compares each whole
// result -- the size of the returned container and every byte of it -- with what the restatement of tests/commit_cases.py gives for the same
// inputs.  Inputs and expected bytes come from a text file written by tests/test_cpp_mirror_commit.py: one `key hex` line per array (`-` for an
// empty one).  Everything goes through jubjub_hip.hpp; there is no direct jj_* call here.
// Usage: test_mirror_commit <vectors.txt>      (exit code 0 = all passed)
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
template <class F>
static bool throws(F f) { try { f(); } catch (const Error&) { return true; } return false; }

// params: prefix, prefix_bits, n, seg_chunks; strides: one per source; fields: src, byte_offset, nbits, ...
static void commit_case(const Context& c, const std::string& k) {
  std::printf("PedersenTable::commit %s\n", k.c_str());
  const std::vector<uint64_t> par = u64s(k + ".params"), st = u64s(k + ".strides"), fl = u64s(k + ".fields");
  const unsigned prefix = (unsigned)par[0];
  const int prefix_bits = (int)par[1];
  const size_t n = par[2];
  const PedersenTable t(c, arr<64>(k + ".gens"), (int)par[3]);
  const auto base = arr<64>(k + ".rbase");
  CHECK(base.size() == 1);
  const FixedBase fb(c, base[0]);
  std::vector<std::vector<uint8_t>> sources;
  std::vector<size_t> strides(st.begin(), st.end());
  for (size_t s = 0; s < st.size(); s++) {
    sources.push_back(blob(k + ".src" + std::to_string(s)));
    CHECK(sources[s].size() == n * strides[s]);
  }
  std::vector<std::array<uint32_t, 3>> fields;
  for (size_t i = 0; i + 2 < fl.size(); i += 3) fields.push_back({(uint32_t)fl[i], (uint32_t)fl[i + 1], (uint32_t)fl[i + 2]});
  const std::vector<Bytes32> r = arr<32>(k + ".r");
  CHECK(r.size() == n);
  CHECK(same(t.commit(&fb, sources, strides, fields, r, 0, prefix, prefix_bits), k + ".commit"));
  CHECK(same(t.commit_points(&fb, sources, strides, fields, r, 0, prefix, prefix_bits).coords(), k + ".points"));
  // the hash-only form: no base, no r, the units counted by the caller
  CHECK(same(t.commit(nullptr, sources, strides, fields, {}, n, prefix, prefix_bits), k + ".hash"));
  CHECK(same(t.commit_points(nullptr, sources, strides, fields, {}, n, prefix, prefix_bits).coords(), k + ".hash_points"));
  // no units: empty containers, nothing read
  CHECK(t.commit(&fb, sources, strides, fields, {}).empty() && t.commit_points(nullptr, sources, strides, fields, {}).len() == 0);
  // what the wrapper refuses by itself, and what the library refuses through it
  CHECK(throws([&] { t.commit(nullptr, sources, strides, fields, r, n, prefix, prefix_bits); }));                        // r without a base
  CHECK(throws([&] { t.commit(&fb, sources, {strides[0]}, fields, r, 0, prefix, prefix_bits); }));                       // fewer strides than sources
  CHECK(throws([&] { t.commit(&fb, {sources[0], sources[1], Blob(sources[2].begin(), sources[2].end() - 1)}, strides, fields, r, 0, prefix, prefix_bits); }));      // a short source
  CHECK(throws([&] { t.commit(&fb, sources, strides, fields, r, 0, prefix, 33); }));                                     // JJ_ERR_INVALID from the library
}

int main(int argc, char** argv) {
  if (argc < 2) { std::puts("usage: test_mirror_commit vectors.txt"); return 2; }
  load(argv[1]);
  try {
    Context c(0);
    commit_case(c, "tiny3_two");
    commit_case(c, "tiny3_three");
  } catch (const Error& e) { std::printf("ERROR %d: %s\n", e.status, e.what()); return 3; }
  std::printf("wrapper PedersenTable::commit\nwrapper PedersenTable::commit_points\n");
  std::printf("%s (%d failures)\n", failures ? "FAILED" : "ALL PASSED", failures);
  return failures ? 1 : 0;
}
