// Host emulation of ONE step of the Montgomery-form ladder (mont_xdbladd, jubjub_amd/csrc/jj_mont.h compiled with -DJJ_HOST_EMU) on states
// given limb by limb: the caller plants the extreme limb patterns of the state class that tools/bounds_check.py derives, which no scalar
// multiplication is known to reach, under the 128-bit shadow of every 64-bit column accumulator of jj_field.h.  Test infrastructure only
// (tests/test_emu_mont_step.py); nothing in jubjub_amd/ links or loads it.
#include <stdint.h>
#include <string.h>
#define JJ_HOST_EMU 1
#include "../../jubjub_amd/csrc/jj_mont.h"

using namespace jj;

static int g_overflow = 0;
extern "C" void jj_emu_overflow(const char*) { g_overflow++; }
extern "C" int emu_overflow_count(void) { return g_overflow; }
extern "C" void emu_overflow_reset(void) { g_overflow = 0; }

static Fe ld_limbs(const int32_t* p) { Fe r; for (int i = 0; i < NL; i++) r.l[i] = (u32)p[i]; return r; }

// n steps, each on its own state: st = (x2, z2, x3, z3) as 4 x 9 signed limbs, x1 as 9, sw = 0 or all-ones.  Out: the four coordinates that
// leave the step as canonical plain integers (value / R mod q, 4 x 32 little-endian bytes) and as the limbs the device would hold.
extern "C" void emu_mont_steps(int n, const int32_t* st, const int32_t* x1, const uint32_t* sw, uint8_t* out128, int32_t* out_limbs) {
  const Fe nqb = mont_neg_qbias();
  for (int s = 0; s < n; s++) {
    Fe c[4];
    for (int j = 0; j < 4; j++) c[j] = ld_limbs(st + 36 * s + 9 * j);
    mont_xdbladd(Fq::opaque(ld_limbs(x1 + 9 * s)), nqb, sw[s], c[0], c[1], c[2], c[3]);
    for (int j = 0; j < 4; j++) {
      u32 w[8];
      Fq::to_words(w, c[j]);
      memcpy(out128 + 128 * s + 32 * j, w, 32);
      for (int i = 0; i < NL; i++) out_limbs[36 * s + 9 * j + i] = (int32_t)c[j].l[i];
    }
  }
}
