// One Schnorr verdict per signature: the tail of jj_sigverify_each's kernels -- device code, one unit per lane.
//   cofactored (default):  OK  iff  [8]([s]B - [c mod r]A - R) = O        cofactorless:  OK  iff  [s]B - [c mod r]A - R = O
// Everything is public: VARIABLE-TIME (the ladder of jj_fixedvar.h reads digit-dependent addresses).
// Included by jj_kernels.h after jj_fixedvar.h and, with -DJJ_HOST_EMU, by tests/cpp/emu_sig_each.cpp.
//
// k_sig_each_prep (jj_kernels.h) has reduced c, tested s < r, written -A over A and the identity over a failed decode.  fixedvar_to_ext
// (jj_abi.hip), unchanged, then leaves [s]B + [c'](-A) as three coordinates in memory -- FixedVar<W>::mul_add in k_varbase_fixed for a gathered
// table above vb_quad_max units, a ladder and the table's own kernel otherwise -- and k_sig_each_tail rebuilds the accumulator from them
// (from_uvz) and runs tail(): R enters as an affine-Niels operand (Curve::to_niels of the decoder's canonical point, what k_affine_to_table
// makes of a table entry) through Curve::add_signed<true> with the sign mask set; three doublings unless the call is cofactorless;
// Curve::is_identity on the extended coordinates.  One byte is stored; nothing is inverted, nothing is compressed.
// tail() takes any accumulator of the class below, so a kernel may also hand it mul_add's result without leaving the registers: that kernel
// (k_sig_each) was built, ran 2 % behind the route above at 2^20 units (profiles/sig_each_ab.txt) and was removed
// (experiments/sig_each_fused); the host emulation still runs both forms.
// Bounds: tail() adds to the output of an addition (mul_add's last fixed window) or to from_uvz()'s point and doubles the output of an
// addition; then doublings of doublings.  add-after-add, dbl-after-add and dbl-after-dbl are all in the set that the fixed point of
// tools/bounds_check.py check_curve iterates over (its accumulator class is the union over both producers and feeds add_signed<true> and dbl
// alike), and the affine-Niels operand is the class of the gathered table's entries.  from_uvz() hands on products (u z, v z, z z) as u, v, z
// and the stored products u, v as t1, t2: tools/bounds_check.py check_kernel_formulas holds that point and its sum with an affine-Niels
// operand inside the accumulator class, for coordinates fresh from a kernel and for coordinates that went through memory.
// tests/test_emu_sig_each.py runs both forms on the host with the 128-bit shadow of every column accumulator.
#pragma once
#include "jj_fixedvar.h"

namespace jj {

constexpr u32 SIG_EACH_REJECT = 0u, SIG_EACH_OK = 1u, SIG_EACH_MALFORMED = 2u;     // = JJ_SIG_REJECT / _OK / _MALFORMED (include/jubjub_hip.h)

template <int W>
struct SigEach {
  typedef FixedVar<W> FV;

  // acc - R is the identity (cofactorless) or of small order (cofactored: [8](acc - R) = O)
  static JJ_DEV bool tail(const Ext& acc, const Affine& R, bool cofactored) {
    Ext d = Curve::add_signed<true>(acc, Curve::to_niels(R), ~0u);
    if (cofactored) d = Curve::mul_by_cofactor(d);
    return Curve::is_identity(d);
  }
  // (U : V : Z) as stored by the ladders, without T1, T2 -> the same point as (U Z : V Z : Z^2) with T1 T2 = U V = (U Z)(V Z) / Z^2
  static JJ_DEV Ext from_uvz(const Fe& u, const Fe& v, const Fe& z) {
    Ext e;
    e.u = Fq::mul(u, z); e.v = Fq::mul(v, z); e.z = Fq::sqr(z); e.t1 = u; e.t2 = v;
    return e;
  }

  // ---- what k_sig_each_prep does per unit, on 8-word little-endian integers
  // c mod r for any 256-bit c, canonical: Fr::from_words reduces (as k_sig_terms reads a challenge), to_words leaves Montgomery form
  static JJ_DEV void challenge(u32 (&c)[8]) { Fr::to_words(c, Fr::from_words(c)); }
  // s < r
  static JJ_DEV bool scalar_ok(const u32 (&s)[8]) {
    const Fe x = Fr::unpack(s);
    i32 borrow = 0;
    _Pragma("unroll") for (int i = 0; i < NL; i++) { const i32 t = (i32)x.l[i] - (i32)FrP::P[i] + borrow; borrow = t >> LB; }
    return borrow != 0;
  }
  // u -> q - u for a canonical u (0 stays 0): the u coordinate of -A
  static JJ_DEV void neg_u(u32 (&u)[8]) {
    const Fe x = Fq::unpack(u);
    u32 nz = 0; _Pragma("unroll") for (int i = 0; i < NL; i++) nz |= x.l[i];
    Fe d; _Pragma("unroll") for (int i = 0; i < NL; i++) d.l[i] = (nz ? FqP::P[i] : 0u) - x.l[i];
    Fq::pack(u, Fq::carry_full(d));
  }
};

}  // namespace jj
