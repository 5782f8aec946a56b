// Host emulation of the device functions behind jj_poly1305, jj_aead_open and jj_aead_seal (jubjub_amd/csrc/jj_poly1305.h and jj_chacha20.h
// compiled with -DJJ_HOST_EMU): what one lane of k_poly1305 does -- Poly1305::mac_row over one row -- and what one lane of k_aead<seal> does --
// Aead::row over one row -- as a stand-alone program.  Test infrastructure only (tests/test_emu_aead.py); nothing in jubjub_amd/ links or
// loads it.
//
// stdin: one record per line,
//   P <key: 64 hex digits> <row: 2 * len hex digits>                                                 -> <tag: 32 hex digits>
//   S <key: 64 hex digits> <nonce: 24 hex digits> <aad: hex digits or -> <row: 2 * len hex digits>   -> <ciphertext || tag>
//   O <key: 64 hex digits> <nonce: 24 hex digits> <aad: hex digits or -> <row: 2 * (len + 16)>       -> <ok: 00 or 01> <plaintext or zeros>
// A row is copied into a fresh allocation of exactly its length and the result is written into another of exactly its own, so a build with
// -fsanitize=address reports a dword read or written outside the row.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#define JJ_HOST_EMU 1
#include "../../jubjub_amd/csrc/jj_poly1305.h"

using namespace jj;

extern "C" void jj_emu_overflow(const char*) {}

static std::vector<uint8_t> unhex(const std::string& s) {
  std::vector<uint8_t> v;
  if (s == "-") return v;
  for (size_t i = 0; i + 1 < s.size(); i += 2) v.push_back((uint8_t)strtoul(s.substr(i, 2).c_str(), nullptr, 16));
  return v;
}
static void put(const uint8_t* p, size_t n) { for (size_t i = 0; i < n; i++) printf("%02x", p[i]); }
static bool legal(size_t len) { return len >= 4 && len <= 1024 && !(len & 3); }

int main() {
  char* line = nullptr; size_t cap = 0;
  while (getline(&line, &cap, stdin) > 0) {
    std::vector<std::string> f;
    for (char* tok = strtok(line, " \n"); tok; tok = strtok(nullptr, " \n")) f.push_back(tok);
    if (f.size() == 3 && f[0] == "P") {
      const std::vector<uint8_t> key = unhex(f[1]), row = unhex(f[2]);
      if (key.size() != 32 || !legal(row.size())) { fprintf(stderr, "bad record\n"); return 2; }
      u32 k[8], tag[4];
      memcpy(k, key.data(), 32);
      uint8_t* in = (uint8_t*)malloc(row.size());       // malloc's alignment stands for the 4 bytes a row start has
      memcpy(in, row.data(), row.size());
      Poly1305::mac_row(tag, (const u32*)in, (u32)(row.size() / 4), k);
      put((const uint8_t*)tag, 16); printf("\n");
      free(in);
    } else if (f.size() == 5 && (f[0] == "S" || f[0] == "O")) {
      const bool seal = f[0] == "S";
      const std::vector<uint8_t> key = unhex(f[1]), nonce = unhex(f[2]), aad = unhex(f[3]), row = unhex(f[4]);
      const size_t len = seal ? row.size() : row.size() - 16;
      if (key.size() != 32 || nonce.size() != 12 || aad.size() > 64 || row.size() < 20 - (seal ? 16 : 0) || !legal(len)) { fprintf(stderr, "bad record\n"); return 2; }
      u32 k[8], nw[3];
      memcpy(k, key.data(), 32); memcpy(nw, nonce.data(), 12);
      AeadAad a;
      memset(&a, 0, sizeof a);
      if (!aad.empty()) memcpy(a.w, aad.data(), aad.size());
      const size_t out_len = seal ? len + 16 : len;
      uint8_t* in = (uint8_t*)malloc(row.size());
      uint8_t* out = (uint8_t*)malloc(out_len);
      memcpy(in, row.data(), row.size());
      memset(out, 0xA5, out_len);
      if (seal) {
        Aead::row<true>((const u32*)in, (u32*)out, (u32)(len / 4), k, nw, a, (u32)aad.size());
      } else {
        const u32 ok = Aead::row<false>((const u32*)in, (u32*)out, (u32)(len / 4), k, nw, a, (u32)aad.size());
        printf("%02x ", ok);
      }
      put(out, out_len); printf("\n");
      free(in); free(out);
    } else { fprintf(stderr, "bad record\n"); return 2; }
  }
  free(line);
  return 0;
}
