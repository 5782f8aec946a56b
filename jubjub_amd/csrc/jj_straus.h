// Two-term variable-base multiplication a P + b Q in ONE interleaved (Straus) ladder: the ladder of k_varbase_mul2 -- device code, one
// unit per lane, two per-lane tables of extended-Niels entries in memory (digit-dependent addresses: VARIABLE-TIME, public scalars).
// Included by jj_kernels.h after store_eniels / load_eniels and, with -DJJ_HOST_EMU, by tests/cpp/emu_straus.cpp.
//
// Both scalars (low 252 bits, integers, never reduced) are recoded as k_varbase recodes one: k' = k + sum_i 2^(w i + w - 1), digit_i =
// window_i(k') - 2^(w-1) in [-2^(w-1), 2^(w-1)), the top window unsigned (it holds the recoding carry).  One chain of doublings serves
// both terms: per window two Curve::add_signed<true> (the entry of P's digit, then the entry of Q's digit), then w doublings --
//   w = 5: 51 windows, 250 doublings, 102 additions, 2 x 17 entries (4896 B per lane);
//   w = 4: 64 windows, 252 doublings, 128 additions, 2 x  9 entries (2592 B per lane).
// The Edwards law is complete (d is not a square), so Q = P, Q = -P, a P = -b Q, identity bases, points with a cofactor component and
// zero digits (entry 0 = the identity entry) take the same path as everything else.
// Bounds: the tables are to_niels<true> of from_affine / add<true> results, and every add_signed<true> meets the output of a doubling
// or of an addition -- the operand classes that the fixed point of tools/bounds_check.py check_curve iterates over (add after add
// included); tests/test_emu_straus.py runs this header on the host with the 128-bit shadow of every column accumulator.
#pragma once
#include "jj_curve.h"

namespace jj {

#ifdef JJ_HOST_EMU
// the table slot as plain words (the device versions in jj_kernels.h move the same 36 words as nine 16-byte vectors)
constexpr int ENIELS_WORDS = 4 * NL;
static JJ_DEV void store_eniels(u32* slot, const ENiels& n) {
  for (int l = 0; l < NL; l++) { slot[l] = n.vpu.l[l]; slot[NL + l] = n.vmu.l[l]; slot[2 * NL + l] = n.z2.l[l]; slot[3 * NL + l] = n.t2d.l[l]; }
}
static JJ_DEV ENiels load_eniels(const u32* slot) {
  ENiels n;
  for (int l = 0; l < NL; l++) { n.vpu.l[l] = slot[l]; n.vmu.l[l] = slot[NL + l]; n.z2.l[l] = slot[2 * NL + l]; n.t2d.l[l] = slot[3 * NL + l]; }
  return n;
}
#endif

template <int W>
struct Straus {
  static_assert(W == 4 || W == 5, "signed window width of the two-term ladder: 4 or 5");
  static constexpr int TABLE = 1 << (W - 1);            // entries {1 .. 2^(w-1)} of one base
  static constexpr int SLOTS = TABLE + 1;               // ... and entry 0, the identity entry: a zero digit is a plain read
  static constexpr int NWIN = (253 + W - 1) / W;        // windows; the top one is unsigned
  static constexpr int LANE_WORDS = 2 * SLOTS * ENIELS_WORDS;   // one lane's slot: P's table, then Q's

  // k' = (k & (2^252 - 1)) + sum_{i < NWIN-1} 2^(w i + w - 1)
  static JJ_DEV void recode(u32 (&k)[8]) {
    k[7] &= 0x0fffffffu;
    u64 c = 0;
    _Pragma("unroll") for (int i = 0; i < 8; i++) {
      u32 rc = 0;
      _Pragma("unroll") for (int j = 0; j < NWIN - 1; j++) { const int bit = W * j + W - 1; if ((bit >> 5) == i) rc |= 1u << (bit & 31); }
      const u64 t = (u64)k[i] + rc + c;
      k[i] = (u32)t; c = t >> 32;
    }
  }
  // bits [w i, w i + w) of k'
  static JJ_DEV u32 window(const u32 (&k)[8], int i) {
    const int bit = W * i, wi = bit >> 5, sh = bit & 31;
    u32 lo = k[0], hi = k[1];
    _Pragma("unroll") for (int q = 1; q < 8; q++) { lo = (wi == q) ? k[q] : lo; hi = (wi == q) ? (q < 7 ? k[q + 1] : 0u) : hi; }
    const u64 both = ((u64)hi << 32) | lo;
    return (u32)(both >> sh) & ((1u << W) - 1u);
  }
  // signed digit i (i < NWIN - 1) of k': table index and sign mask
  static JJ_DEV void digit(const u32 (&k)[8], int i, u32& idx, u32& negmask) {
    const int d = (int)window(k, i) - TABLE;
    negmask = d < 0 ? ~0u : 0u; idx = (u32)(d < 0 ? -d : d);
  }
  // slot[0] = identity entry, slot[j] = j B for j = 1 .. 2^(w-1)
  static JJ_DEV void table(const Affine& B, u32* slot) {
    const ANiels bn = Curve::to_niels(B);
    Ext cur = Curve::from_affine(B);
    store_eniels(slot, Curve::eniels_identity());
    store_eniels(slot + ENIELS_WORDS, Curve::to_niels<true>(cur));
    #pragma unroll 1
    for (int j = 2; j <= TABLE; j++) {
      cur = Curve::add<true>(cur, bn);
      store_eniels(slot + j * ENIELS_WORDS, Curve::to_niels<true>(cur));
    }
  }

  // a P + b Q; ka, kb: 32 little-endian bytes as 8 words each (recoded in place); slot: LANE_WORDS words owned by this lane.
  // P's entry for a window is fetched before the w doublings that precede its use (as varbase_windowed fetches its one entry); Q's
  // entry for the same window is fetched under P's addition, so one entry is in flight during the doublings and the loop carries 36
  // registers of prefetch, not 72: with both entries fetched ahead of the doublings the kernel needs 256 VGPRs and 92 bytes of scratch
  // per lane (22 spilled registers), this form 218 and none.
  static JJ_DEV Ext mul2(const Affine& P, const Affine& Q, u32 (&ka)[8], u32 (&kb)[8], u32* slot) {
    u32* const tp = slot;
    u32* const tq = slot + SLOTS * ENIELS_WORDS;
    table(P, tp);
    table(Q, tq);
    recode(ka);
    recode(kb);
    u32 ip = window(ka, NWIN - 1), mp = 0;               // top window: unsigned digit
    u32 iq = window(kb, NWIN - 1), mq = 0;
    ENiels ep = load_eniels(tp + ip * ENIELS_WORDS);
    Ext acc = Curve::identity();
    #pragma unroll 1
    for (int i = NWIN - 1; i >= 0; i--) {
      const ENiels eq = load_eniels(tq + iq * ENIELS_WORDS);   // lands under P's addition
      acc = Curve::add_signed<true>(acc, ep, mp);
      const u32 mq_now = mq;
      if (i > 0) {                                             // P's next entry: under Q's addition and the doublings
        digit(ka, i - 1, ip, mp);
        digit(kb, i - 1, iq, mq);
        ep = load_eniels(tp + ip * ENIELS_WORDS);
      }
      acc = Curve::add_signed<true>(acc, eq, mq_now);
      if (i > 0) {
        // two doublings per trip so that the results alternate between two register sets (varbase_windowed)
        #pragma unroll 1
        for (int d = 0; d < (W - 1) / 2; d++) acc = Curve::dbl(Curve::dbl(acc));
        if constexpr ((W - 1) % 2) acc = Curve::dbl(acc);
        acc = Curve::dbl(acc);
      }
    }
    return acc;
  }
};

}  // namespace jj
