// One fixed and one variable term per unit, a G + b Q, in ONE accumulator: the ladder of k_varbase_fixed -- device code, one unit per lane.
// G is the base of a gathered fixed-base table (jj_fixedbase_table_create, window_bits 8..16: FbParams and the entries k_fixedbase_gather
// reads), Q differs per lane.  Digit-dependent addresses in both terms: VARIABLE-TIME, public scalars.
// Included by jj_kernels.h after FbParams / fb_window / lds_aniels and, with -DJJ_HOST_EMU, by tests/cpp/emu_fixedvar.cpp.
//
// Variable term first: the signed w-bit ladder of k_varbase on (b, Q) -- Straus<W>'s recoding and its one-base table (17 extended-Niels
// entries in the lane's slot for w = 5), 51 windows, 250 doublings, 51 Curve::add_signed<true>, the next window's entry fetched ahead of
// the doublings.  Then, WITHOUT storing the accumulator, the fixed term: a is recoded with fp.recode and ceil(253 / fp.w) affine-Niels
// entries (i, |digit|) of the table are added with their signs, the top window unsigned -- the walk of k_fixedbase_gather over the same
// FbParams and the same table memory (one jj_table serves both calls), seven products per addition and no doubling: the entries already
// hold 2^(w i) G.  Entry i - 1 is fetched before addition i; the first fixed entry is fetched before the ladder's last addition.
// The Edwards law is complete, so Q = G, Q = -G, a G = -b Q, zero scalars, an identity Q and points with a cofactor component take the
// same path as everything else; the scalars are integers (low 252 bits), never reduced.
// Bounds: every add_signed<true> here meets the identity, the output of a doubling (the ladder's windows) or the output of an addition
// (every fixed window: the first one follows the ladder's last addition) -- the operand classes that the fixed point of
// tools/bounds_check.py check_curve iterates over; the fixed entries are Curve::to_niels of canonical affine points (k_affine_to_table).
// tests/test_emu_fixedvar.py runs this header on the host with the 128-bit shadow of every column accumulator.
#pragma once
#include "jj_straus.h"

namespace jj {

#ifdef JJ_HOST_EMU
// what jj_kernels.h gives the device build: the gathered table's entry stride and parameters, its entry as plain words, a window of k'
constexpr int ANIELS_WORDS = 28;
constexpr int GNIELS_WORDS = 32;
struct FbParams {
  int w, W;
  u32 E;
  u32 recode[8];
};
static JJ_DEV ANiels lds_aniels(const u32* e) {
  ANiels n;
  for (int l = 0; l < NL; l++) { n.vpu.l[l] = e[l]; n.vmu.l[l] = e[NL + l]; n.t2d.l[l] = e[2 * NL + l]; }
  return n;
}
static JJ_DEV u32 fb_window(const u32 (&k)[8], int w, int i) {
  const int bit = w * i, wi = bit >> 5, sh = bit & 31;
  const u64 both = ((u64)(wi < 7 ? k[wi + 1] : 0u) << 32) | k[wi];
  return (u32)(both >> sh) & ((1u << w) - 1u);
}
#endif

template <int W>
struct FixedVar {
  typedef Straus<W> S;
  static constexpr int LANE_WORDS = S::SLOTS * ENIELS_WORDS;   // one lane's slot: Q's table (k_varbase's slot)

  // a' = (a & (2^252 - 1)) + fp.recode
  static JJ_DEV void recode_fixed(u32 (&k)[8], const FbParams& fp) {
    k[7] &= 0x0fffffffu;
    u64 c = 0;
    _Pragma("unroll") for (int i = 0; i < 8; i++) { const u64 t = (u64)k[i] + fp.recode[i] + c; k[i] = (u32)t; c = t >> 32; }
  }
  // signed digit i (i < fp.W - 1) of a': entry index in [0, E] and sign mask
  static JJ_DEV void fixed_digit(const u32 (&k)[8], const FbParams& fp, int i, u32& idx, u32& negmask) {
    const int d = (int)fb_window(k, fp.w, i) - (int)fp.E;
    negmask = d < 0 ? ~0u : 0u; idx = (u32)(d < 0 ? -d : d);
  }
  static JJ_DEV const u32* fixed_entry(const u32* table, const FbParams& fp, int i, u32 idx) {
    return table + ((size_t)i * (fp.E + 1) + idx) * GNIELS_WORDS;
  }

  // a G + b Q; ka, kb: 32 little-endian bytes as 8 words each (recoded in place); table, fp: G's gathered table; slot: LANE_WORDS words
  // owned by this lane.  The ladder's last window is written out after its loop: there the entry in flight is the first FIXED entry
  // (27 words instead of the ladder's 36), so the loop itself is k_varbase's and carries nothing for the fixed term.
  static JJ_DEV Ext mul_add(const u32* table, const FbParams& fp, u32 (&ka)[8], const Affine& Q, u32 (&kb)[8], u32* slot) {
    S::table(Q, slot);
    S::recode(kb);
    u32 iq = S::window(kb, S::NWIN - 1), mq = 0;             // top window: unsigned digit
    ENiels e = load_eniels(slot + iq * ENIELS_WORDS);
    Ext acc = Curve::identity();
    #pragma unroll 1
    for (int i = S::NWIN - 1; i >= 1; i--) {
      const ENiels s = e;
      const u32 smask = mq;
      S::digit(kb, i - 1, iq, mq);                           // fetch the next window's entry before the doublings
      e = load_eniels(slot + iq * ENIELS_WORDS);
      acc = Curve::add_signed<true>(acc, s, smask);
      // two doublings per trip so that the results alternate between two register sets (varbase_windowed)
      #pragma unroll 1
      for (int d = 0; d < (W - 1) / 2; d++) acc = Curve::dbl(Curve::dbl(acc));
      if constexpr ((W - 1) % 2) acc = Curve::dbl(acc);
      acc = Curve::dbl(acc);
    }
    recode_fixed(ka, fp);
    u32 ig = fb_window(ka, fp.w, fp.W - 1), mg = 0;          // top window of a': unsigned digit (it holds the recoding carry)
    ANiels f = lds_aniels(fixed_entry(table, fp, fp.W - 1, ig));   // lands under the ladder's last addition
    acc = Curve::add_signed<true>(acc, e, mq);
    #pragma unroll 1
    for (int i = fp.W - 1; i >= 0; i--) {
      const ANiels s = f;
      const u32 smask = mg;
      if (i > 0) {                                           // fetch the next window's entry before this addition
        fixed_digit(ka, fp, i - 1, ig, mg);
        f = lds_aniels(fixed_entry(table, fp, i - 1, ig));
      }
      acc = Curve::add_signed<true>(acc, s, smask);
    }
    return acc;
  }
};

}  // namespace jj
