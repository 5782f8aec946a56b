// Host emulation of jj_sig_challenge's device functions (jubjub_amd/csrc/jj_blake2b.h compiled with -DJJ_HOST_EMU): what one lane of
// k_sig_challenge does -- Blake2b::hash over up to two 32-byte parts and a message, then Fr::from_words_wide and Fr::to_words -- as a stand-alone
// program.  Test infrastructure only (tests/test_emu_blake2b.py); nothing in jubjub_amd/ links or loads it.
//
// stdin: one record per line,  <personal: 32 hex digits or -> <part0: 64 hex digits or -> <part1: 64 hex digits or -> <message: hex or -> <skew>
// stdout: one line per record, <digest: 128 hex digits> <scalar: 64 hex digits>
// The message is copied to byte `skew` of a fresh allocation that ends with the dword of its last byte, so a build with -fsanitize=address
// reports a load of a dword that holds no byte of the message; an empty message is handed over as a null pointer.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#define JJ_HOST_EMU 1
#include "../../jubjub_amd/csrc/jj_blake2b.h"

using namespace jj;

static int g_overflow = 0;
extern "C" void jj_emu_overflow(const char*) { g_overflow++; }

static std::vector<uint8_t> unhex(const std::string& s) {
  std::vector<uint8_t> v;
  if (s == "-") return v;
  for (size_t i = 0; i + 1 < s.size(); i += 2) v.push_back((uint8_t)strtoul(s.substr(i, 2).c_str(), nullptr, 16));
  return v;
}
static void put(const uint8_t* p, size_t n) { for (size_t i = 0; i < n; i++) printf("%02x", p[i]); }

int main() {
  char* line = nullptr; size_t cap = 0;
  while (getline(&line, &cap, stdin) > 0) {
    std::vector<std::string> f;
    for (char* tok = strtok(line, " \n"); tok; tok = strtok(nullptr, " \n")) f.push_back(tok);
    if (f.size() != 5) { fprintf(stderr, "bad record\n"); return 2; }
    const std::vector<uint8_t> personal = unhex(f[0]), q0 = unhex(f[1]), q1 = unhex(f[2]), msg = unhex(f[3]);
    const size_t skew = strtoul(f[4].c_str(), nullptr, 10);
    if ((personal.size() != 0 && personal.size() != 16) || (q0.size() != 0 && q0.size() != 32) || (q1.size() != 0 && q1.size() != 32) || (q0.empty() && !q1.empty())) { fprintf(stderr, "bad record\n"); return 2; }
    u64 pl = 0, ph = 0;
    if (!personal.empty()) { memcpy(&pl, personal.data(), 8); memcpy(&ph, personal.data() + 8, 8); }
    u32 a[8] = {0}, b[8] = {0};
    if (!q0.empty()) memcpy(a, q0.data(), 32);
    if (!q1.empty()) memcpy(b, q1.data(), 32);
    uint8_t* buf = nullptr;
    if (!msg.empty()) {
      buf = (uint8_t*)malloc((skew + msg.size() + 3) & ~(size_t)3);      // malloc's alignment stands for the 16 bytes asked of a device pointer
      memset(buf, 0xA5, skew);
      memcpy(buf + skew, msg.data(), msg.size());
    }
    u32 lo[8], hi[8], w[8];
    const int parts = q0.empty() ? 0 : q1.empty() ? 1 : 2;
    if (parts == 0) Blake2b::hash<0>(lo, hi, pl, ph, a, b, buf, (u32)skew, (u64)msg.size());
    else if (parts == 1) Blake2b::hash<1>(lo, hi, pl, ph, a, b, buf, (u32)skew, (u64)msg.size());
    else Blake2b::hash<2>(lo, hi, pl, ph, a, b, buf, (u32)skew, (u64)msg.size());
    free(buf);
    Fr::to_words(w, Fr::from_words_wide(lo, hi));
    put((const uint8_t*)lo, 32); put((const uint8_t*)hi, 32); printf(" "); put((const uint8_t*)w, 32); printf("\n");
  }
  free(line);
  if (g_overflow) { fprintf(stderr, "%d column accumulators overflowed\n", g_overflow); return 3; }
  return 0;
}
