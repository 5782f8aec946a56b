// What tests/cpp/abi_stub.cpp (a recording stand-in for the C ABI, no HIP and no device) and tests/cpp/test_mirror_stub.cpp share: the call
// log, the byte pattern the stub writes into every output, the tag of each entry point and the builder of a log line.
#pragma once
#include <cstddef>
#include <cstdint>
#include <sstream>
#include <string>
#include <vector>

namespace stub {

// one line per data call, in call order
std::vector<std::string>& log();

// byte i of output k of a call
inline uint8_t pattern(size_t i, int k, int tag) { return (uint8_t)(i * 131 + 17 * (size_t)k + (size_t)tag); }

namespace tag {
enum {
  varbase_mul = 1, varbase_mul_vartime, varbase_mul2_vartime, varbase_mul2_scalars, fixedvar_mul_vartime, fixedbase_multi_mul, batch_normalize,
  pedersen_hash, pedersen_point, pedersen_scalars, msm_batch, msm_ragged, msm_basis_mul, msm_basis_info, msm_finish, sigbatch_ragged,
  sigverify_each, sig_challenge, ka_kdf, chacha20_xor, poly1305, aead_open, aead_seal, blake2s, group_hash
};
}

// FNV-1a over a row: the short digest a log line carries per row of an input
inline uint32_t digest(const void* p, size_t n) {
  const uint8_t* b = static_cast<const uint8_t*>(p);
  uint32_t h = 2166136261u;
  for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 16777619u;
  return h;
}

// `name key=value ...`: the stub builds one from its arguments, the test from what the header documents for the call it made
class Line {
 public:
  explicit Line(const char* name) { s_ << name; }
  Line& i(const char* key, long long v) { s_ << ' ' << key << '=' << v; return *this; }
  Line& null(const char* key, bool is_null) { s_ << ' ' << key << '=' << (is_null ? "NULL" : "set"); return *this; }
  // `count` rows of `width` bytes, `stride` apart: one digest per row
  Line& rows(const char* key, const void* p, size_t count, size_t stride, size_t width) {
    s_ << ' ' << key << "=[";
    for (size_t r = 0; r < count; r++) s_ << (r ? "," : "") << std::hex << digest(static_cast<const uint8_t*>(p) + r * stride, width) << std::dec;
    s_ << ']';
    return *this;
  }
  template <class T>
  Line& list(const char* key, const T* p, size_t count) {
    s_ << ' ' << key << "=[";
    for (size_t r = 0; r < count; r++) s_ << (r ? "," : "") << (unsigned long long)p[r];
    s_ << ']';
    return *this;
  }
  std::string str() const { return s_.str(); }

 private:
  std::ostringstream s_;
};

}  // namespace stub
