// Host emulation of the Montgomery-form ladder of k_varbase_mont (jubjub_amd/csrc/jj_mont.h compiled with -DJJ_HOST_EMU): the same
// device functions, run on the CPU with the 128-bit shadow of every 64-bit column accumulator of jj_field.h.  Test infrastructure
// only (tests/test_emu_mont.py); nothing in jubjub_amd/ links or loads it.
#include <stdint.h>
#include <string.h>
#define JJ_HOST_EMU 1
#include "../../jubjub_amd/csrc/jj_mont.h"

using namespace jj;

static int g_overflow = 0;
extern "C" void jj_emu_overflow(const char*) { g_overflow++; }
extern "C" int emu_overflow_count(void) { return g_overflow; }
extern "C" void emu_overflow_reset(void) { g_overflow = 0; }

static void ld(u32 (&w)[8], const uint8_t* p) { memcpy(w, p, 32); }
static void st(uint8_t* p, const u32 (&w)[8]) { memcpy(p, w, 32); }
static Fe ld_fe(const uint8_t* p) { u32 w[8]; ld(w, p); return Fq::from_words(w); }

// n units: the batch inversion of k_varbase_mont_x1 over groups of MONT_X1_UNITS units (the kernel's order: prefix products forward,
// inverses backward), the ladder of k_varbase_mont, then the affine result through one inversion per unit
extern "C" void emu_varbase_mont(int n, const uint8_t* scalars, const uint8_t* points, uint8_t* out64) {
  Fe x1s[MONT_X1_UNITS], num;
  for (int g0 = 0; g0 < n; g0 += MONT_X1_UNITS) {
    const int m = n - g0 < MONT_X1_UNITS ? n - g0 : MONT_X1_UNITS;
    Fe acc = Fq::one();
    for (int s = 0; s < m; s++) { x1s[s] = acc; acc = Fq::mul(acc, mont_x1_den(ld_fe(points + 64 * (g0 + s) + 32), num)); }
    Fe inv = Fq::invert(acc);
    for (int s = m - 1; s >= 0; s--) {
      const Fe d = mont_x1_den(ld_fe(points + 64 * (g0 + s) + 32), num);
      const Fe di = Fq::mul(inv, x1s[s]);
      inv = Fq::mul(inv, d);
      x1s[s] = Fq::mul(Fq::carry(num), di);
    }
    for (int s = 0; s < m; s++) {
      const int i = g0 + s;
      u32 k[8]; ld(k, scalars + 32 * i);
      Affine P; P.u = ld_fe(points + 64 * i); P.v = ld_fe(points + 64 * i + 32);
      Fe U, V, W;
      varbase_mont(P, x1s[s], k, U, V, W);
      const Fe wi = Fq::invert(W);
      u32 w[8];
      Fq::to_words(w, Fq::mul(U, wi)); st(out64 + 64 * i, w);
      Fq::to_words(w, Fq::mul(V, wi)); st(out64 + 64 * i + 32, w);
    }
  }
}
// a24 * e through mont_a24, for e given as 9 signed limbs (any limb pattern the ladder can hand it); canonical result
extern "C" void emu_mont_a24(const int32_t* limbs9, uint8_t* out32) {
  Fe e; for (int i = 0; i < NL; i++) e.l[i] = (u32)limbs9[i];
  u32 w[8]; Fq::to_words(w, Fq::carry(mont_a24(e))); st(out32, w);
}
