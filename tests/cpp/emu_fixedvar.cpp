// Host emulation of the fused fixed + variable ladder of k_varbase_fixed (jubjub_amd/csrc/jj_fixedvar.h compiled with -DJJ_HOST_EMU): the same
// device functions, run on the CPU with the 128-bit shadow of every 64-bit column accumulator of jj_field.h.  Test infrastructure only
// (tests/test_emu_fixedvar.py); nothing in jubjub_amd/ links or loads it.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#define JJ_HOST_EMU 1
#include "../../jubjub_amd/csrc/jj_fixedvar.h"

using namespace jj;

static int g_overflow = 0;
extern "C" void jj_emu_overflow(const char*) { g_overflow++; }
extern "C" int emu_overflow_count(void) { return g_overflow; }
extern "C" void emu_overflow_reset(void) { g_overflow = 0; }

static Fe ld_fe(const uint8_t* p) { u32 w[8]; memcpy(w, p, 32); return Fq::from_words(w); }
static void st_fe(uint8_t* p, const Fe& x) { u32 w[8]; Fq::to_words(w, x); memcpy(p, w, 32); }

static FbParams params(int w) {
  FbParams fp;
  fp.w = w; fp.W = (253 + w - 1) / w; fp.E = 1u << (w - 1);
  memset(fp.recode, 0, sizeof fp.recode);
  for (int i = 0; i < fp.W - 1; i++) { const int bit = fp.w * i + fp.w - 1; fp.recode[bit >> 5] |= 1u << (bit & 31); }
  return fp;
}

// The gathered table of width w from its W * (E + 1) entries as canonical affine points (64 bytes each, entry i * (E + 1) + j = j 2^(w i) G):
// Curve::to_niels of each, 27 words at a stride of GNIELS_WORDS, the padding poisoned.  Returns the table (free with emu_table_free).
extern "C" u32* emu_table_create(int w, const uint8_t* entries64) {
  if (w < 8 || w > 16) return nullptr;
  const FbParams fp = params(w);
  const size_t ne = (size_t)fp.W * (fp.E + 1);
  u32* t = (u32*)malloc(ne * GNIELS_WORDS * sizeof(u32));
  if (!t) return nullptr;
  for (size_t e = 0; e < ne; e++) {
    Affine a;
    a.u = ld_fe(entries64 + 64 * e); a.v = ld_fe(entries64 + 64 * e + 32);
    const ANiels n = Curve::to_niels(a);
    u32* s = t + e * GNIELS_WORDS;
    for (int l = 0; l < NL; l++) { s[l] = n.vpu.l[l]; s[NL + l] = n.vmu.l[l]; s[2 * NL + l] = n.t2d.l[l]; }
    for (int l = 3 * NL; l < GNIELS_WORDS; l++) s[l] = 0xA5A5A5A5u;
  }
  return t;
}
extern "C" void emu_table_free(u32* t) { free(t); }

// n units of a[i] G + b[i] Q[i] over the table of width w, the affine result through one inversion per unit
extern "C" int emu_fixedvar_mul(int w, const u32* table, int n, const uint8_t* a, const uint8_t* b, const uint8_t* q, uint8_t* out64) {
  if (w < 8 || w > 16 || !table) return -1;
  const FbParams fp = params(w);
  static u32 slot[FixedVar<5>::LANE_WORDS];
  for (int i = 0; i < n; i++) {
    memset(slot, 0xA5, sizeof slot);                     // an entry the ladder reads must have been written by it
    u32 ka[8], kb[8];
    memcpy(ka, a + 32 * i, 32); memcpy(kb, b + 32 * i, 32);
    Affine Q;
    Q.u = ld_fe(q + 64 * i); Q.v = ld_fe(q + 64 * i + 32);
    const Ext r = FixedVar<5>::mul_add(table, fp, ka, Q, kb, slot);
    const Fe zi = Fq::invert(r.z);
    st_fe(out64 + 64 * i, Fq::mul(r.u, zi));
    st_fe(out64 + 64 * i + 32, Fq::mul(r.v, zi));
  }
  return 0;
}
// the digits of the fixed term as the kernel reads them: out[i] = signed digit i (fp.W of them; the top one unsigned); returns fp.W
extern "C" int emu_fixed_digits(int w, const uint8_t* k32, int32_t* out) {
  if (w < 8 || w > 16) return -1;
  const FbParams fp = params(w);
  u32 k[8]; memcpy(k, k32, 32);
  FixedVar<5>::recode_fixed(k, fp);
  for (int i = 0; i < fp.W - 1; i++) { u32 idx, neg; FixedVar<5>::fixed_digit(k, fp, i, idx, neg); out[i] = neg ? -(int32_t)idx : (int32_t)idx; }
  out[fp.W - 1] = (int32_t)fb_window(k, fp.w, fp.W - 1);
  return fp.W;
}
