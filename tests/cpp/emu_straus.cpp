// Host emulation of the two-term interleaved ladder of k_varbase_mul2 (jubjub_amd/csrc/jj_straus.h compiled with -DJJ_HOST_EMU): the same
// device functions, run on the CPU with the 128-bit shadow of every 64-bit column accumulator of jj_field.h.  Test infrastructure only
// (tests/test_emu_straus.py); nothing in jubjub_amd/ links or loads it.
#include <stdint.h>
#include <string.h>
#define JJ_HOST_EMU 1
#include "../../jubjub_amd/csrc/jj_straus.h"

using namespace jj;

static int g_overflow = 0;
extern "C" void jj_emu_overflow(const char*) { g_overflow++; }
extern "C" int emu_overflow_count(void) { return g_overflow; }
extern "C" void emu_overflow_reset(void) { g_overflow = 0; }

static Fe ld_fe(const uint8_t* p) { u32 w[8]; memcpy(w, p, 32); return Fq::from_words(w); }
static void st_fe(uint8_t* p, const Fe& x) { u32 w[8]; Fq::to_words(w, x); memcpy(p, w, 32); }

template <int W>
static void run(int n, const uint8_t* a, const uint8_t* p, const uint8_t* b, const uint8_t* q, uint8_t* out64) {
  static u32 slot[Straus<W>::LANE_WORDS];
  for (int i = 0; i < n; i++) {
    memset(slot, 0xA5, sizeof slot);                     // an entry the ladder reads must have been written by it
    u32 ka[8], kb[8];
    memcpy(ka, a + 32 * i, 32); memcpy(kb, b + 32 * i, 32);
    Affine P, Q;
    P.u = ld_fe(p + 64 * i); P.v = ld_fe(p + 64 * i + 32);
    Q.u = ld_fe(q + 64 * i); Q.v = ld_fe(q + 64 * i + 32);
    const Ext r = Straus<W>::mul2(P, Q, ka, kb, slot);
    const Fe zi = Fq::invert(r.z);
    st_fe(out64 + 64 * i, Fq::mul(r.u, zi));
    st_fe(out64 + 64 * i + 32, Fq::mul(r.v, zi));
  }
}
// n units of a[i] P[i] + b[i] Q[i] with signed w-bit windows (w = 4 or 5), the affine result through one inversion per unit; -1: bad width
extern "C" int emu_varbase_mul2(int w, int n, const uint8_t* a, const uint8_t* p, const uint8_t* b, const uint8_t* q, uint8_t* out64) {
  if (w == 5) run<5>(n, a, p, b, q, out64);
  else if (w == 4) run<4>(n, a, p, b, q, out64);
  else return -1;
  return 0;
}
// the signed digits of one scalar as the ladder sees them: out[i] = digit i (NWIN of them; the top one unsigned); returns NWIN
template <int W>
static int digits(const uint8_t* k32, int32_t* out) {
  u32 k[8]; memcpy(k, k32, 32);
  Straus<W>::recode(k);
  for (int i = 0; i < Straus<W>::NWIN - 1; i++) { u32 idx, neg; Straus<W>::digit(k, i, idx, neg); out[i] = neg ? -(int32_t)idx : (int32_t)idx; }
  out[Straus<W>::NWIN - 1] = (int32_t)Straus<W>::window(k, Straus<W>::NWIN - 1);
  return Straus<W>::NWIN;
}
extern "C" int emu_straus_digits(int w, const uint8_t* k32, int32_t* out64) { return w == 5 ? digits<5>(k32, out64) : w == 4 ? digits<4>(k32, out64) : -1; }
