// Host emulation of the Pedersen hash's device functions (jubjub_amd/csrc/jj_pedersen.h compiled with -DJJ_HOST_EMU): what one lane of
// k_pedersen_gather does before it touches the table -- the host-made plan, the bit extraction over aligned dwords with its funnel shift and its
// clamp, the window index, the sign and the choice of the sub-table -- as a stand-alone program.  Test infrastructure only
// (tests/test_emu_pedersen.py); nothing in jubjub_amd/ links or loads it.
//
// stdin: one record per line,
//   <nseg> <seg_chunks> <window_chunks> <prefix> <prefix_bits> <row_stride> <nfields> {<byte_offset> <nbits>} <n> <rows: hex of n * row_stride bytes, or ->
// stdout: one line per unit: for every window of the plan "<segment> <window> <sub-table t> <entry0> <index> <sign>;"
// The rows are copied into a fresh allocation that ends with the dword of the last byte the fields cover in the LAST row, so a build with
// -fsanitize=address reports a load of a dword that holds no covered byte; malloc's alignment stands for the 16 bytes asked of a device pointer.
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
    if (f.size() < 9) { fprintf(stderr, "bad record\n"); return 2; }
    size_t k = 0;
    auto num = [&]() { return strtoul(f[k++].c_str(), nullptr, 10); };
    const int nseg = (int)num(), c = (int)num(), w = (int)num();
    const u32 prefix = (u32)num(); const int prefix_bits = (int)num();
    const u32 stride = (u32)num(); const int nfields = (int)num();
    if (nfields < 0 || nfields > PED_MAX_FIELDS || f.size() != 9 + 2 * (size_t)nfields) { fprintf(stderr, "bad record\n"); return 2; }
    uint32_t fields[2 * PED_MAX_FIELDS] = {0};
    for (int q = 0; q < 2 * nfields; q++) fields[q] = (uint32_t)num();
    const size_t n = num();
    const std::string hex = f[k++];
    PedSegs segs; u32 cover;
    const std::vector<PedWin> plan = ped_build_plan(nseg, c, w, prefix, prefix_bits, nfields, fields, &segs, &cover);
    uint8_t* buf = nullptr;
    if (nfields && n) {
      if (hex.size() != 2 * n * stride) { fprintf(stderr, "bad record: rows\n"); return 2; }
      const size_t used = (n - 1) * stride + cover;                // up to the last covered byte of the last row
      buf = (uint8_t*)malloc((used + 3) & ~(size_t)3);
      for (size_t b = 0; b < used; b++) buf[b] = (uint8_t)strtoul(hex.substr(2 * b, 2).c_str(), nullptr, 16);
    }
    for (size_t i = 0; i < n; i++) {
      const u32 pos = (u32)i * stride, lastd = Pedersen::last_dword(pos, cover);
      for (const PedWin& x : plan) {
        u32 neg;
        const u32 a = Pedersen::index(x, Pedersen::raw_bits(buf, pos, lastd, x), neg);
        printf("%u %u %u %u %u %u;", x.seg, x.chunk0 / (u32)w, x.t, x.entry0, a - x.entry0, neg & 1u);
      }
      printf("\n");
    }
    free(buf);
  }
  free(line);
  if (g_overflow) { fprintf(stderr, "%d column accumulators overflowed\n", g_overflow); return 3; }
  return 0;
}
