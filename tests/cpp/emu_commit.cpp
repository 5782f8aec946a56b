// Host emulation of the multi-source Pedersen plan and bit extraction (jubjub_amd/csrc/jj_pedersen.h compiled with -DJJ_HOST_EMU): what one lane
// of k_pedersen_commit does before it touches the Pedersen table -- the host-made plan with the source of every piece, the row position and the
// clamp dword formed per source, the bit extraction over aligned dwords, the window index, the sign and the choice of the sub-table -- as a
// stand-alone program.  Test infrastructure only (tests/test_emu_commit.py); nothing in jubjub_amd/ links or loads it.
//
// stdin: one record per line,
//   <nseg> <seg_chunks> <window_chunks> <prefix> <prefix_bits> <nsrc> {<stride>} <nfields> {<src> <byte_offset> <nbits>} <n> {<source: hex of n * stride bytes, or ->}
// stdout: one line per unit: for every window of the plan "<segment> <window> <sub-table t> <entry0> <index> <sign>;"
// Every source is copied into a fresh allocation of its own that ends with the dword of the last byte the fields cover in its LAST row, so a
// build with -fsanitize=address reports a load of a dword that holds no covered byte of that source; malloc's alignment stands for the 16 bytes
// asked of a device pointer.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#define JJ_HOST_EMU 1
#include "../../jubjub_amd/csrc/jj_pedersen.h"

using namespace jj;

static int g_overflow = 0;
extern "C" void jj_emu_overflow(const char*) { g_overflow++; }

int main() {
  char* line = nullptr; size_t cap = 0;
  while (getline(&line, &cap, stdin) > 0) {
    std::vector<std::string> f;
    for (char* tok = strtok(line, " \n"); tok; tok = strtok(nullptr, " \n")) f.push_back(tok);
    size_t k = 0;
    bool bad = false;
    auto num = [&]() -> unsigned long { if (k >= f.size()) { bad = true; return 0; } return strtoul(f[k++].c_str(), nullptr, 10); };
    const int nseg = (int)num(), c = (int)num(), w = (int)num();
    const u32 prefix = (u32)num(); const int prefix_bits = (int)num();
    const int nsrc = (int)num();
    if (bad || nsrc < 0 || nsrc > PED_MAX_SRC) { fprintf(stderr, "bad record\n"); return 2; }
    PedSrcs S; memset(&S, 0, sizeof S);
    for (int s = 0; s < nsrc; s++) S.stride[s] = (u32)num();
    const int nfields = (int)num();
    if (bad || nfields < 0 || nfields > PED_MAX_FIELDS) { fprintf(stderr, "bad record\n"); return 2; }
    uint32_t fields[3 * PED_MAX_FIELDS] = {0};
    for (int q = 0; q < 3 * nfields; q++) fields[q] = (uint32_t)num();
    const size_t n = num();
    if (bad || f.size() != k + (size_t)nsrc) { fprintf(stderr, "bad record\n"); return 2; }
    for (int q = 0; q < nfields; q++) if (fields[3 * q] >= (u32)nsrc) { fprintf(stderr, "bad record: source\n"); return 2; }
    PedSegs segs;
    const std::vector<PedWinSrc> plan = ped_build_plan_src(nseg, c, w, prefix, prefix_bits, nfields, fields, &segs, S.cover);
    uint8_t* buf[PED_MAX_SRC] = {nullptr, nullptr, nullptr, nullptr};
    for (int s = 0; s < nsrc; s++) {
      const std::string& hex = f[k++];
      if (!S.cover[s] || !n) continue;                             // a source no field reads is never touched
      if (hex.size() != 2 * n * S.stride[s]) { fprintf(stderr, "bad record: source %d\n", s); return 2; }
      const size_t used = (n - 1) * S.stride[s] + S.cover[s];      // up to the last covered byte of the last row
      buf[s] = (uint8_t*)malloc((used + 3) & ~(size_t)3);
      for (size_t b = 0; b < used; b++) buf[s][b] = (uint8_t)strtoul(hex.substr(2 * b, 2).c_str(), nullptr, 16);
      S.rows[s] = buf[s];
    }
    for (size_t i = 0; i < n; i++) {
      for (const PedWinSrc& x : plan) {
        u32 neg;
        const u32 a = Pedersen::index(x, Pedersen::raw_bits_src(S, (u32)i, x), neg);
        printf("%u %u %u %u %u %u;", x.seg, x.chunk0 / (u32)w, x.t, x.entry0, a - x.entry0, neg & 1u);
      }
      printf("\n");
    }
    for (int s = 0; s < nsrc; s++) free(buf[s]);
  }
  free(line);
  if (g_overflow) { fprintf(stderr, "%d column accumulators overflowed\n", g_overflow); return 3; }
  return 0;
}
