// Host emulation of the functions behind jj_blake2b (Blake2bRows in jubjub_amd/csrc/jj_blake2b.h compiled with -DJJ_HOST_EMU): the host's
// midstate over the whole blocks of the prefix, the piece plan of the sources, and what one lane of k_blake2b does with them (the block loop
// over the prefix's tail and the lane's pieces), as a stand-alone program.  Test infrastructure only (tests/test_emu_blake2b_rows.py);
// nothing in jubjub_amd/ links or loads it.
//
// stdin, one case per line, numbers in decimal and bytes in hex ("-" for none):
//   digest_len personal|- prefix|- narrays { stride bytes }... nparts { array skew len }... n
// array a holds the bytes of n rows at `stride` apart, cut behind the last byte any part reads of its last row.  stdout: one line per case,
// the n digests in hex.  Every array and the prefix live in a fresh allocation of exactly their length, so a build with
// -fsanitize=address,undefined reports a read past the prefix and a dword read outside a part's own bytes of the last row.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include <iostream>
#include <sstream>
#define JJ_HOST_EMU 1
#include "../../jubjub_amd/csrc/jj_blake2b.h"

using namespace jj;

extern "C" void jj_emu_overflow(const char*) {}

static std::vector<uint8_t> unhex(const std::string& s) {
  std::vector<uint8_t> out;
  if (s == "-") return out;
  for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((uint8_t)strtoul(s.substr(i, 2).c_str(), nullptr, 16));
  return out;
}

template <int DIGEST>
static void run(const uint8_t* personal, const uint8_t* prefix, size_t prefix_len, int nparts, const uint8_t* const* base, const size_t* stride, const size_t* lens, size_t n) {
  size_t rest = 0;
  for (int k = 0; k < nparts; k++) rest += lens[k];
  B2bMid mid; B2bPlan plan;
  Blake2bRows<DIGEST>::midstate(mid, personal, prefix, prefix_len, rest);
  Blake2bRows<DIGEST>::plan_sources(plan, nparts, lens);
  for (size_t i = 0; i < n; i++) {
    u64 rowp[B2B_MAX_PIECES] = {0, 0, 0, 0};
    for (int k = 0; k < B2B_MAX_PIECES; k++)
      if (plan.nd[k]) rowp[k] = (u64)(uintptr_t)base[plan.src[k]] + (u64)i * stride[plan.src[k]] + plan.off[k];
    u32 d[DIGEST / 4];
    Blake2bRows<DIGEST>::finish(d, mid, plan, rowp);
    for (int j = 0; j < DIGEST / 4; j++) printf("%02x%02x%02x%02x", d[j] & 255, (d[j] >> 8) & 255, (d[j] >> 16) & 255, d[j] >> 24);
  }
  printf("\n");
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    int digest, narrays, nparts;
    std::string personal_hex, prefix_hex;
    in >> digest >> personal_hex >> prefix_hex >> narrays;
    std::vector<size_t> astride(narrays);
    std::vector<uint8_t*> arrays(narrays, nullptr);
    for (int a = 0; a < narrays; a++) {
      std::string hex;
      in >> astride[a] >> hex;
      const std::vector<uint8_t> bytes = unhex(hex);
      arrays[a] = (uint8_t*)malloc(bytes.size() ? bytes.size() : 1);      // malloc's alignment stands for the 16 bytes asked of a device pointer
      memcpy(arrays[a], bytes.data(), bytes.size());
    }
    in >> nparts;
    const uint8_t* base[4] = {nullptr, nullptr, nullptr, nullptr};
    size_t stride[4] = {0, 0, 0, 0}, lens[4] = {0, 0, 0, 0};
    for (int k = 0; k < nparts; k++) {
      size_t a, skew;
      in >> a >> skew >> lens[k];
      base[k] = arrays[a] + skew; stride[k] = astride[a];
    }
    size_t n;
    in >> n;
    if (!in || nparts > 4 || (digest != 32 && digest != 64)) { fprintf(stderr, "bad case line\n"); return 2; }
    const std::vector<uint8_t> personal = unhex(personal_hex), pre = unhex(prefix_hex);
    uint8_t* prefix = nullptr;
    if (!pre.empty()) { prefix = (uint8_t*)malloc(pre.size()); memcpy(prefix, pre.data(), pre.size()); }
    if (digest == 32) run<32>(personal.empty() ? nullptr : personal.data(), prefix, pre.size(), nparts, base, stride, lens, n);
    else run<64>(personal.empty() ? nullptr : personal.data(), prefix, pre.size(), nparts, base, stride, lens, n);
    free(prefix);
    for (uint8_t* a : arrays) free(a);
  }
  return 0;
}
