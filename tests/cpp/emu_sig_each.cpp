// Host emulation of jj_sigverify_each's device functions (jubjub_amd/csrc/jj_sig_each.h compiled with -DJJ_HOST_EMU): what k_sig_each_prep,
// the ladder and k_sig_each_tail do per unit, run on the CPU with the 128-bit shadow of every 64-bit column accumulator of jj_field.h.  Test
// infrastructure only (tests/test_emu_sig_each.py); nothing in jubjub_amd/ links or loads it.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#define JJ_HOST_EMU 1
#include "../../jubjub_amd/csrc/jj_sig_each.h"

using namespace jj;

static int g_overflow = 0;
extern "C" void jj_emu_overflow(const char*) { g_overflow++; }
extern "C" int emu_overflow_count(void) { return g_overflow; }
extern "C" void emu_overflow_reset(void) { g_overflow = 0; }

static FbParams params(int w) {
  FbParams fp;
  fp.w = w; fp.W = (253 + w - 1) / w; fp.E = 1u << (w - 1);
  memset(fp.recode, 0, sizeof fp.recode);
  for (int i = 0; i < fp.W - 1; i++) { const int bit = fp.w * i + fp.w - 1; fp.recode[bit >> 5] |= 1u << (bit & 31); }
  return fp;
}
// the decoder's output row as load_affine (jj_kernels.h) reads it
static Affine ld_affine(const uint8_t* p) {
  u32 wu[8], wv[8];
  memcpy(wu, p, 32); memcpy(wv, p + 32, 32);
  Affine a; a.u = Fq::from_words(wu); a.v = Fq::from_words(wv);
  return a;
}

// The gathered table of width w from its W * (E + 1) entries as canonical affine points (64 bytes each, entry i * (E + 1) + j = j 2^(w i) B):
// Curve::to_niels of each, 27 words at a stride of GNIELS_WORDS, the padding poisoned.  Returns the table (free with emu_table_free).
extern "C" u32* emu_table_create(int w, const uint8_t* entries64) {
  if (w < 8 || w > 16) return nullptr;
  const FbParams fp = params(w);
  const size_t ne = (size_t)fp.W * (fp.E + 1);
  u32* t = (u32*)malloc(ne * GNIELS_WORDS * sizeof(u32));
  if (!t) return nullptr;
  for (size_t e = 0; e < ne; e++) {
    const ANiels n = Curve::to_niels(ld_affine(entries64 + 64 * e));
    u32* s = t + e * GNIELS_WORDS;
    for (int l = 0; l < NL; l++) { s[l] = n.vpu.l[l]; s[NL + l] = n.vmu.l[l]; s[2 * NL + l] = n.t2d.l[l]; }
    for (int l = 3 * NL; l < GNIELS_WORDS; l++) s[l] = 0xA5A5A5A5u;
  }
  return t;
}
extern "C" void emu_table_free(u32* t) { free(t); }

// n units.  points: the decoder's rows, R at [0, n) and A at [n, 2n) (64 bytes each; (0, 0) for a failed decode), ok: its 2n bytes -- both are
// rewritten as k_sig_each_prep rewrites them; s32, c32: the caller's arrays; cprime: n x 32 bytes of workspace.  route 0: mul_add's
// accumulator goes to the tail as it is; route 1: the three coordinates go through memory as 9-limb words and come back through from_uvz
// (k_sig_each_tail behind a ladder).  verdict: written as the kernels write it -- a malformed unit by the preparation only.
extern "C" int emu_sig_each(int w, const u32* table, int n, uint8_t* points, uint8_t* ok, const uint8_t* s32, const uint8_t* c32, uint8_t* cprime, int cofactored, int route,
                            uint8_t* verdict) {
  if (w < 8 || w > 16 || !table) return -1;
  const FbParams fp = params(w);
  typedef SigEach<5> SE;
  static u32 slot[FixedVar<5>::LANE_WORDS];
  static const uint8_t ident[64] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1};
  for (int i = 0; i < n; i++) {                            // k_sig_each_prep
    u32 x[8];
    memcpy(x, c32 + 32 * i, 32); SE::challenge(x); memcpy(cprime + 32 * i, x, 32);
    memcpy(x, s32 + 32 * i, 32);
    const bool s_ok = SE::scalar_ok(x), r_ok = ok[i] != 0, a_ok = ok[n + i] != 0;
    if (!r_ok) memcpy(points + 64 * i, ident, 64);
    if (!a_ok) memcpy(points + 64 * (n + i), ident, 64);
    else { memcpy(x, points + 64 * (n + i), 32); SE::neg_u(x); memcpy(points + 64 * (n + i), x, 32); }
    const bool good = r_ok && a_ok && s_ok;
    ok[i] = good ? 1 : 0;
    if (!good) verdict[i] = (uint8_t)SIG_EACH_MALFORMED;
  }
  for (int i = 0; i < n; i++) {                            // the ladder and SigEach::tail
    memset(slot, 0xA5, sizeof slot);                       // an entry the ladder reads must have been written by it
    u32 ka[8], kb[8];
    memcpy(ka, s32 + 32 * i, 32); memcpy(kb, cprime + 32 * i, 32);
    Ext acc = FixedVar<5>::mul_add(table, fp, ka, ld_affine(points + 64 * (n + i)), kb, slot);
    if (route == 1) {
      u32 mem[3][NL];
      for (int l = 0; l < NL; l++) { mem[0][l] = acc.u.l[l]; mem[1][l] = acc.v.l[l]; mem[2][l] = acc.z.l[l]; }
      Fe u, v, z;
      for (int l = 0; l < NL; l++) { u.l[l] = mem[0][l]; v.l[l] = mem[1][l]; z.l[l] = mem[2][l]; }
      acc = SE::from_uvz(u, v, z);
    }
    const bool good = SE::tail(acc, ld_affine(points + 64 * i), cofactored != 0);
    if (ok[i]) verdict[i] = (uint8_t)(good ? SIG_EACH_OK : SIG_EACH_REJECT);
  }
  return 0;
}
