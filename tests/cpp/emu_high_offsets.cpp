// Host emulation of the device functions that address a row with a 32-bit byte offset, AT the offsets the entry points accept: Blake2s::finish
// (k_blake2s), Blake2b::hash<PARTS> (k_sig_challenge) and ped_build_plan + Pedersen::raw_bits / index (k_pedersen_*) from
// jubjub_amd/csrc/jj_blake2s.h, jj_blake2b.h and jj_pedersen.h compiled with -DJJ_HOST_EMU, as a stand-alone program.  Test infrastructure only
// (tests/test_emu_high_offsets.py); nothing in jubjub_amd/ links or loads it.
//
// The row array is an anonymous mapping of 2^32 bytes that reserves nothing (MAP_NORESERVE): only the pages of the rows a record writes are
// ever touched, an inaccessible page lies directly in front of it and another directly behind.  A read past 2^32 or below 0 ends the program;
// an offset that lost a high bit or wrapped reads the zero pages near the bottom and gives another digest.
//
// argv[1]: a file of bytes the records copy from.  stdin: one record per line,
//   w <offset> <file offset> <len>        copy len bytes of the file to byte `offset` of the array
//   z                                     the array is all zeros again
//   s <personal: 16 hex digits or -> <prefix: hex or -> <offset> <len>
//                                         BLAKE2s: the host's midstate over the prefix, then one lane of k_blake2s at pos = (u32)offset
//   b <personal: 32 hex digits or -> <part0: 64 hex digits or -> <part1: 64 hex digits or -> <offset> <len>
//                                         BLAKE2b-512: one lane of k_sig_challenge at pos = (u32)offset (offset may be 2^32: an empty message)
//   p <nseg> <seg_chunks> <window_chunks> <prefix> <prefix_bits> <row_stride> <nfields> {<byte_offset> <nbits>} <unit>
//                                         one lane of k_pedersen_gather: pos = (u32)unit * (u32)row_stride, lastd from the plan's 32-bit cover
// stdout: one line per s, b and p record: the digest in hex, or for p "<segment> <window> <sub-table t> <entry0> <index> <sign>;" per window.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <string>
#include <vector>
#define JJ_HOST_EMU 1
#include "../../jubjub_amd/csrc/jj_blake2s.h"
#include "../../jubjub_amd/csrc/jj_pedersen.h"      // brings jj_blake2b.h

using namespace jj;

static int g_overflow = 0;
extern "C" void jj_emu_overflow(const char*) { g_overflow++; }

static const size_t SPAN = (size_t)1 << 32, PAGE = 4096;

static std::vector<uint8_t> unhex(const std::string& s) {
  std::vector<uint8_t> v;
  if (s == "-") return v;
  for (size_t i = 0; i + 1 < s.size(); i += 2) v.push_back((uint8_t)strtoul(s.substr(i, 2).c_str(), nullptr, 16));
  return v;
}
static void put(const void* p, size_t n) { for (size_t i = 0; i < n; i++) printf("%02x", ((const uint8_t*)p)[i]); }

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: emu_high_offsets FILE < records\n"); return 2; }
  FILE* df = fopen(argv[1], "rb");
  if (!df) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  uint8_t* map = (uint8_t*)mmap(nullptr, SPAN + 2 * PAGE, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
  if (map == (uint8_t*)MAP_FAILED) { perror("mmap of 2^32 bytes"); return 4; }
  if (mprotect(map, PAGE, PROT_NONE) || mprotect(map + PAGE + SPAN, PAGE, PROT_NONE)) { perror("mprotect"); return 4; }
  uint8_t* rows = map + PAGE;                      // page aligned: stands for the 16 bytes asked of a device pointer
  char* line = nullptr; size_t cap = 0;
  while (getline(&line, &cap, stdin) > 0) {
    std::vector<std::string> f;
    for (char* tok = strtok(line, " \n"); tok; tok = strtok(nullptr, " \n")) f.push_back(tok);
    if (f.empty()) continue;
    size_t k = 1;
    auto num = [&]() { return k < f.size() ? strtoull(f[k++].c_str(), nullptr, 10) : 0ull; };
    if (f[0] == "w" && f.size() == 4) {
      const u64 off = num(), from = num(), len = num();
      if (off > SPAN || len > SPAN - off) { fprintf(stderr, "bad record: w outside the array\n"); return 2; }
      if (fseek(df, (long)from, SEEK_SET) || fread(rows + off, 1, len, df) != len) { fprintf(stderr, "bad record: w past the file\n"); return 2; }
    } else if (f[0] == "z" && f.size() == 1) {
      if (madvise(rows, SPAN, MADV_DONTNEED)) { perror("madvise"); return 4; }
    } else if (f[0] == "s" && f.size() == 5) {
      const std::vector<uint8_t> personal = unhex(f[1]), prefix = unhex(f[2]);
      k = 3;
      const u64 off = num(), len = num();
      if ((personal.size() != 0 && personal.size() != 8) || off + len > SPAN || len > 65536) { fprintf(stderr, "bad record: s\n"); return 2; }
      const size_t B = Blake2s::midstate_blocks(prefix.size(), len);
      u32 h[8], tail[16], out[8];
      Blake2s::midstate(h, tail, personal.empty() ? nullptr : personal.data(), prefix.data(), prefix.size(), B);
      Blake2s::finish(out, h, tail, (u32)(64 * B), (u32)(prefix.size() - 64 * B), rows, (u32)off, (u32)len);
      put(out, 32); printf("\n");
    } else if (f[0] == "b" && f.size() == 6) {
      const std::vector<uint8_t> personal = unhex(f[1]), q0 = unhex(f[2]), q1 = unhex(f[3]);
      k = 4;
      const u64 off = num(), len = num();
      if ((personal.size() != 0 && personal.size() != 16) || (q0.size() != 0 && q0.size() != 32) || (q1.size() != 0 && q1.size() != 32) || (q0.empty() && !q1.empty()) ||
          off + len > SPAN) { fprintf(stderr, "bad record: b\n"); return 2; }
      u64 pl = 0, ph = 0;
      if (!personal.empty()) { memcpy(&pl, personal.data(), 8); memcpy(&ph, personal.data() + 8, 8); }
      u32 a[8] = {0}, b[8] = {0}, lo[8], hi[8];
      if (!q0.empty()) memcpy(a, q0.data(), 32);
      if (!q1.empty()) memcpy(b, q1.data(), 32);
      const u32 pos = (u32)off;                    // k_sig_challenge: pos = (u32)o
      if (q0.empty()) Blake2b::hash<0>(lo, hi, pl, ph, a, b, rows, pos, len);
      else if (q1.empty()) Blake2b::hash<1>(lo, hi, pl, ph, a, b, rows, pos, len);
      else Blake2b::hash<2>(lo, hi, pl, ph, a, b, rows, pos, len);
      put(lo, 32); put(hi, 32); printf("\n");
    } else if (f[0] == "p" && f.size() >= 9) {
      const int nseg = (int)num(), c = (int)num(), w = (int)num();
      const u32 prefix = (u32)num(); const int prefix_bits = (int)num();
      const u64 stride = num(); const int nfields = (int)num();
      if (nfields < 1 || nfields > PED_MAX_FIELDS || f.size() != 9 + 2 * (size_t)nfields || stride > SPAN) { fprintf(stderr, "bad record: p\n"); return 2; }
      uint32_t fields[2 * PED_MAX_FIELDS] = {0};
      for (int q = 0; q < 2 * nfields; q++) fields[q] = (uint32_t)num();
      const u64 unit = num();
      if ((unit + 1) * stride > SPAN) { fprintf(stderr, "bad record: p outside the array\n"); return 2; }
      PedSegs segs; u32 cover;
      const std::vector<PedWin> plan = ped_build_plan(nseg, c, w, prefix, prefix_bits, nfields, fields, &segs, &cover);
      const u32 pos = (u32)unit * (u32)stride, lastd = Pedersen::last_dword(pos, cover);      // the kernels' own expressions
      for (const PedWin& x : plan) {
        u32 neg;
        const u32 a = Pedersen::index(x, Pedersen::raw_bits(rows, pos, lastd, x), neg);
        printf("%u %u %u %u %u %u;", x.seg, x.chunk0 / (u32)w, x.t, x.entry0, a - x.entry0, neg & 1u);
      }
      printf("\n");
    } else { fprintf(stderr, "bad record: %s\n", f[0].c_str()); return 2; }
  }
  free(line); fclose(df);
  munmap(map, SPAN + 2 * PAGE);
  if (g_overflow) { fprintf(stderr, "%d column accumulators overflowed\n", g_overflow); return 3; }
  return 0;
}
