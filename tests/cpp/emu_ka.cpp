// Host emulation of the device functions behind jj_ka_kdf's hash and jj_chacha20_xor (jubjub_amd/csrc/jj_blake2b.h and jj_chacha20.h compiled
// with -DJJ_HOST_EMU): what one lane of k_ka_kdf does -- Blake2bT<32>::hash_parts over one or two 32-byte parts -- and what one lane of
// k_chacha20_xor does -- ChaCha20::xor_row over one row -- as a stand-alone program.  Test infrastructure only (tests/test_emu_ka.py); nothing
// in jubjub_amd/ links or loads it.
//
// stdin: one record per line,
//   H <personal: 32 hex digits or -> <part0: 64 hex digits> <part1: 64 hex digits or ->            -> <digest: 64 hex digits>
//   C <key: 64 hex digits> <nonce: 24 hex digits> <counter> <row: 2 * len hex digits>               -> <row xor keystream: 2 * len hex digits>
// A row is copied into a fresh allocation of exactly its length and the result is written into another, so a build with -fsanitize=address
// reports a dword read or written past the row's len bytes.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#define JJ_HOST_EMU 1
#include "../../jubjub_amd/csrc/jj_blake2b.h"
#include "../../jubjub_amd/csrc/jj_chacha20.h"

using namespace jj;

extern "C" void jj_emu_overflow(const char*) {}

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
    if (f.size() == 4 && f[0] == "H") {
      const std::vector<uint8_t> personal = unhex(f[1]), q0 = unhex(f[2]), q1 = unhex(f[3]);
      if ((personal.size() != 0 && personal.size() != 16) || q0.size() != 32 || (q1.size() != 0 && q1.size() != 32)) { fprintf(stderr, "bad record\n"); return 2; }
      u64 pl = 0, ph = 0;
      if (!personal.empty()) { memcpy(&pl, personal.data(), 8); memcpy(&ph, personal.data() + 8, 8); }
      u32 a[8], b[8] = {0}, w[8];
      memcpy(a, q0.data(), 32);
      if (!q1.empty()) memcpy(b, q1.data(), 32);
      if (q1.empty()) Blake2bT<32>::hash_parts<1>(w, pl, ph, a, b);
      else Blake2bT<32>::hash_parts<2>(w, pl, ph, a, b);
      put((const uint8_t*)w, 32); printf("\n");
    } else if (f.size() == 5 && f[0] == "C") {
      const std::vector<uint8_t> key = unhex(f[1]), nonce = unhex(f[2]), row = unhex(f[4]);
      const u32 counter = (u32)strtoul(f[3].c_str(), nullptr, 10);
      if (key.size() != 32 || nonce.size() != 12 || row.size() < 4 || row.size() > 1024 || (row.size() & 3)) { fprintf(stderr, "bad record\n"); return 2; }
      u32 k[8], nw[3];
      memcpy(k, key.data(), 32); memcpy(nw, nonce.data(), 12);
      uint8_t* in = (uint8_t*)malloc(row.size());       // malloc's alignment stands for the 4 bytes a row start has
      uint8_t* out = (uint8_t*)malloc(row.size());
      memcpy(in, row.data(), row.size());
      memset(out, 0xA5, row.size());
      ChaCha20::xor_row((const u32*)in, (u32*)out, (u32)(row.size() / 4), k, counter, nw);
      put(out, row.size()); printf("\n");
      free(in); free(out);
    } else { fprintf(stderr, "bad record\n"); return 2; }
  }
  free(line);
  return 0;
}
