// Constant-time variable-base multiplication on the Montgomery form of Jubjub: the x-only ladder of k_varbase_mont -- device code, one
// scalar multiplication per lane, no table, no LDS.  Included by jj_kernels.h and, with -DJJ_HOST_EMU, by tests/cpp/emu_mont.cpp.
//
// Jubjub (-u^2 + v^2 = 1 + d u^2 v^2, a = -1, d = -10240/10241) is birationally equivalent to the Montgomery curve
// B y^2 = x^3 + A x^2 + x with A = 2(a + d)/(a - d) = 40962 and B = 4/(a - d) = -40964:  x = (1 + v)/(1 - v), y = x/u, and back
// u = x/y, v = (x - 1)/(x + 1).  The map sends the identity (0, 1) to the point at infinity and (0, -1) to (0, 0), the one point of
// order 2 (the group is cyclic of order 8r); d is not a square, so no other point is exceptional.
//
// Ladder: RFC 7748 section 5 (xDBLADD with a24 = (A - 2)/4 = 10240), bits 251..0 of the scalar (the reference's ladder skips the top
// four, src/lib.rs:357-379), from (1 : 0) and (x1 : 1).  Per bit one masked select of the doubling's two inputs keyed on bit_i ^ bit_(i+1) -- the bits of the Gray
// code k ^ (k >> 1), shifted out of eight registers -- then 4S + 5M and one multiplication by a24 (mont_a24: 9 + 9 multiply-adds and
// a carry, no product).  No load, store, branch or address of the loop depends on the scalar.
// The three sums of the step (x2 + z2, x3 + z3, DA + CB) are formed as x + z - q with q written in limbs near 2^29 (MontK::QBIAS): the
// same residue with limbs centred on zero, so that they can be squared and multiplied without a carry step (mont_xdbladd).
// The kernel runs the ladder (varbase_mont_ladder) before it loads the base point for the y-recovery (varbase_mont_recover): the
// point's 18 registers are not live across the 252 iterations.
// y-recovery: Okeya-Sakurai in the projective form of Costello-Smith ("Montgomery curves and their arithmetic", Algorithm 5), every
// coordinate scaled by u instead of divided by y1 = x1/u, then (X : Y : Z) -> Edwards (X (X + Z) : Y (X - Z) : Y (X + Z)).
// Exceptional inputs and results are masked, never branched on.  tests/mont_ladder_model.py is the same algorithm over integers.
#pragma once
#include "jj_curve.h"

namespace jj {

// Montgomery-form constants (R = 2^261): 2A, 2B, -1 (tests/test_mont_ladder_cpu.py recomputes them)
// QBIAS: q itself (FqP::P) with its low eight limbs moved next to 2^29: from limb 0 up, a limb below 2^28 borrows 2^29 from the limb
// above it.  sum QBIAS[i] 2^(29 i) = q and limbs 0..7 lie in [1.32 * 2^28, 2.76 * 2^28] (tests/test_mont_qbias_cpu.py recomputes it).
struct MontK {
  static constexpr u32 QBIAS[9] = {0x20000001u, 0x1ffffff7u, 0x1f96ffbfu, 0x1b4805ffu, 0x1d80553bu, 0x2c0404d0u, 0x1520cce6u, 0x2a6533afu, 0x0073eda6u};
  static constexpr u32 TWO_A[9] = {0x1fa7aa4fu, 0x02c2ad87u, 0x1bae6c40u, 0x0936fbd9u, 0x11652c16u, 0x13ce2c45u, 0x10c0760eu, 0x117bd639u, 0x006b8a64u};
  static constexpr u32 TWO_B[9] = {0x005856cdu, 0x1d3d4998u, 0x0fd54cbfu, 0x1aafac22u, 0x08f9624fu, 0x00a72b80u, 0x1fa2daa0u, 0x16c980a5u, 0x00301b3bu};
  static constexpr u32 NEG_ONE[9] = {0x00000047u, 0x1ffffdc8u, 0x02e0ee3fu, 0x10f9a9ffu, 0x0e97a399u, 0x151d55f1u, 0x1c18d42bu, 0x021155b7u, 0x0026e968u};
};
constexpr int MONT_NBITS = 252;
constexpr i32 MONT_A24 = 10240;
constexpr i32 MONT_A24_QMUL = 0x58549745;     // round(a24 * 2^272 / q): q-digit of a24 * e from its top limb, (e_8 * QMUL) >> 40
constexpr int MONT_X1_UNITS = 16;             // k_varbase_mont_x1: units per lane (one inversion per 16 units)

// a24 * e (any value with limbs in (-2^31, 2^31) and a top limb < 2^26): limb-wise 64-bit products minus qd * q, where qd estimates
// a24 * e_8 * 2^232 / q to within (-2^-15, 1 + 2^-15), then one parallel carry.  Value in (a24 * e_low - q, a24 * e_low + 2q),
// e_low = the part of e below 2^232; limbs 0..7 in (-2^15, 2^29 + 2^15).  tools/bounds_check.py: FieldModel.mul_a24.
static JJ_DEV Fe mont_a24(const Fe& e) {
  const i32 qd = (i32)(((i64)(i32)e.l[NL - 1] * (i64)MONT_A24_QMUL) >> 40);
  i64 t[NL];
  _Pragma("unroll") for (int i = 0; i < NL; i++) t[i] = (i64)(i32)e.l[i] * (i64)MONT_A24 - (i64)qd * (i64)FqP::P[i];
  Fe r;
  r.l[0] = (u32)t[0] & LMASK;
  _Pragma("unroll") for (int i = 1; i < NL; i++) r.l[i] = (i < NL - 1 ? ((u32)t[i] & LMASK) : (u32)t[i]) + (u32)(t[i - 1] >> LB);
#ifdef JJ_HOST_EMU
  if (t[NL - 1] + (t[NL - 2] >> LB) != (i64)(i32)r.l[NL - 1]) jj_emu_overflow("a24 top limb");
#endif
  return r;
}

// One ladder step without swapping the state: with sw all-ones the roles of (x2 : z2) and (x3 : z3) are exchanged, which exchanges
// DA = (x3 - z3)(x2 + z2) and CB = (x3 + z3)(x2 - z2) and so leaves DA + CB and (DA - CB)^2 as they are: only the doubling reads the
// swap bit, through two selects (the sum and the difference it squares).  (x2 : z2) <- 2 (sw ? (x3 : z3) : (x2 : z2)),
// (x3 : z3) <- (x2 : z2) + (x3 : z3), difference (ox1 : 1); ox1 is already hidden (Field::opaque).  The state that leaves is the one a
// masked swap of all four coordinates followed by RFC 7748's xDBLADD leaves.  Inputs and outputs are products ("N").
// Bounds: a product has limbs 0..7 in [0, 2^29), so a plain sum of two has them in [0, 2^30) and the nine-term middle column of its
// square could reach 9 * 2^60 > 2^63.  The sums are therefore biased by q: x + z - QBIAS is the same residue, its limbs 0..7 lie in
// (-0.69 * 2^30, 0.67 * 2^30) and the columns of its square stay below 0.63 * 2^63 before the reduction terms; DA and CB multiply a
// difference (limbs in (-2^29, 2^29)) by such a sum.  No carry step is left in the loop (tools/bounds_check.py check_mont_ladder;
// tests/cpp/emu_mont_step.cpp plants the extreme limb patterns under the 128-bit shadow accumulators).
// nqb = -QBIAS, limb by limb, held in scalar registers by the caller (mont_neg_qbias): a VOP3 instruction of gfx950 takes no 32-bit
// literal, so for x + z - constant hipcc emits a literal v_subrev_u32 per limb next to the v_add_u32 (1 740 instructions per bit); from a
// register the biased sum is one v_add3_u32 per limb, what the plain sum cost (1 711; profiles/r11_vb_bias_census.txt).
// The four sums and differences are hidden once and multiplied as they are (mul_hidden), and so is the select: hipcc otherwise
// re-expands it (v_and + two v_bitop3_b32 per limb), or spills (tests/test_codegen_trim.py, tests/test_codegen_bias.py hold the census).
// -QBIAS limb by limb (two's complement), pinned to scalar registers on the device (see mont_xdbladd)
static JJ_DEV Fe mont_neg_qbias() {
  Fe r;
  _Pragma("unroll") for (int i = 0; i < NL; i++) {
    u32 c = 0u - MontK::QBIAS[i];
#ifndef JJ_HOST_EMU
    asm("" : "+s"(c));
#endif
    r.l[i] = c;
  }
  return r;
}
static JJ_DEV void mont_xdbladd(const Fe& ox1, const Fe& nqb, u32 sw, Fe& x2, Fe& z2, Fe& x3, Fe& z3) {
  typedef Fq F;
  const Fe s2 = F::opaque(F::add(F::add(x2, z2), nqb)), d2 = F::opaque(F::sub(x2, z2));
  const Fe s3 = F::opaque(F::add(F::add(x3, z3), nqb)), d3 = F::opaque(F::sub(x3, z3));
  const Fe oa = F::opaque(F::select(s2, s3, sw));
  const Fe ob = F::opaque(F::select(d2, d3, sw));
  const Fe da = F::mul_hidden(d3, s2), cb = F::mul_hidden(s3, d2);
  const Fe aa = F::sqr_hidden(oa), bb = F::sqr_hidden(ob);
  const Fe e = F::sub(aa, bb);
  const Fe w = F::add(aa, mont_a24(e));
  x3 = F::sqr(F::add(F::add(da, cb), nqb));
  z3 = F::mul_hidden(ox1, F::opaque(F::sqr(F::sub(da, cb))));
  z2 = F::mul(e, w);
  x2 = F::mul(aa, bb);
}

// denominator 1 - v of x1 = (1 + v)/(1 - v) for the batch inversion of k_varbase_mont_x1, 1 in place of 0 (v = 1: the identity); num = 1 + v
static JJ_DEV Fe mont_x1_den(const Fe& v, Fe& num) {
  num = Fq::add(Fq::one(), v);
  const Fe d = Fq::sub(Fq::one(), v);
  return Fq::select(d, Fq::one(), 0u - (u32)Fq::is_zero(d));
}

// masks of the canonical zero test of a product-form value (Field::is_zero_product, no product)
static JJ_DEV u32 mont_zero_mask(const Fe& t) { return 0u - (u32)Fq::is_zero_product(t); }

// The ladder of k P: x1 = (1 + v)/(1 - v) of the base (a product; any value when v = 1), k: 32 little-endian bytes as 8 words, bits
// 251..0 are used.  Leaves k P = (xq : zq) and (k + 1) P = (xp : zp), products, and returns the mask of the final swap (bit 0 of k).
static JJ_DEV u32 varbase_mont_ladder(const Fe& x1, const u32 (&k_in)[8], Fe& xq, Fe& zq, Fe& xp, Fe& zp) {
  typedef Fq F;
  u32 k[8];
  _Pragma("unroll") for (int q = 0; q < 8; q++) k[q] = k_in[q];
  k[7] &= 0x0fffffffu;
  // swap keys: the Gray code k ^ (k >> 1) (bit 252 is zero), left-aligned so that bit 251 sits at bit 255
  u32 g[8];
  _Pragma("unroll") for (int q = 0; q < 8; q++) g[q] = k[q] ^ ((k[q] >> 1) | (q < 7 ? k[q + 1] << 31 : 0u));
  _Pragma("unroll") for (int q = 7; q >= 1; q--) g[q] = (g[q] << 4) | (g[q - 1] >> 28);
  g[0] <<= 4;
  const Fe ox1 = F::opaque(x1);
  const Fe nqb = mont_neg_qbias();
  Fe x2 = F::one(), z2 = F::zero(), x3 = x1, z3 = F::one();
  #pragma unroll 1
  for (int i = 0; i < MONT_NBITS; i++) {
    u32 sw = (u32)((i32)g[7] >> 31);                  // all-ones iff bit_i != bit_(i+1)
    _Pragma("unroll") for (int q = 7; q >= 1; q--) g[q] = (g[q] << 1) | (g[q - 1] >> 31);
    g[0] <<= 1;
    mont_xdbladd(ox1, nqb, sw, x2, z2, x3, z3);
  }
  const u32 last = 0u - (k[0] & 1u);                  // the final swap: bit 0
  xq = F::select(x2, x3, last); zq = F::select(z2, z3, last);
  xp = F::select(x3, x2, last); zp = F::select(z3, z2, last);
  return last;
}

// k P as a projective Edwards point (U : V : Z), products, from what the ladder left: P = (u, v) (products, as load_affine gives
// them), its x1, last = the ladder's return value.
static JJ_DEV void varbase_mont_recover(const Affine& P, const Fe& x1, u32 last, const Fe& xq, const Fe& zq, const Fe& xp, const Fe& zp,
                                        Fe& ou, Fe& ov, Fe& oz) {
  typedef Fq F;

  // y-recovery (Costello-Smith Algorithm 5), scaled by u
  const Fe v1 = F::mul(x1, zq);
  const Fe v3 = F::mul(F::sqr(F::sub(xq, v1)), xp);
  const Fe t = F::mul(F::konst(MontK::TWO_A), zq);
  const Fe v4 = F::add(F::mul(x1, xq), zq);
  Fe v2 = F::mul(F::carry(F::add(F::add(xq, v1), t)), v4);
  v2 = F::mul(F::sub(v2, F::mul(t, zq)), zp);
  const Fe Y = F::mul(P.u, F::sub(v2, v3));
  const Fe w = F::mul(F::mul(F::mul(F::konst(MontK::TWO_B), x1), zq), zp);
  const Fe X = F::mul(w, xq), Z = F::mul(w, zq);
  const Fe xpz = F::add(X, Z);
  Fe U = F::mul(X, xpz), V = F::mul(Y, F::sub(X, Z)), W = F::mul(Y, xpz);

  // exceptional cases, later selects win (tests/mont_ladder_model.py varbase)
  const Fe one = F::one(), zero = F::zero(), negone = F::konst(MontK::NEG_ONE);
  const u32 zp0 = mont_zero_mask(zp), zq0 = mont_zero_mask(zq), xq0 = mont_zero_mask(xq) & ~zq0;
  const u32 x10 = mont_zero_mask(x1);
  const u32 ident = 0u - (u32)F::is_zero(F::sub(P.v, one));
  const u32 odd = last;
  U = F::select(U, F::mul(P.u, negone), zp0); V = F::select(V, P.v, zp0); W = F::select(W, one, zp0);   // (k + 1) P = O: -P
  U = F::select(U, zero, xq0); V = F::select(V, negone, xq0); W = F::select(W, one, xq0);                // k P = (0, 0): (0, -1)
  const u32 to_id = zq0 | (x10 & ~odd) | ident;                                                          // k P = O
  const u32 to_t2 = x10 & odd & ~ident;                                                                  // P = (0, -1), k odd
  U = F::select(U, zero, to_id | to_t2); V = F::select(F::select(V, one, to_id), negone, to_t2); W = F::select(W, one, to_id | to_t2);
  ou = U; ov = V; oz = W;
}

// ladder and y-recovery in one call (the host emulation; k_varbase_mont loads P between the two)
static JJ_DEV void varbase_mont(const Affine& P, const Fe& x1, const u32 (&k_in)[8], Fe& ou, Fe& ov, Fe& oz) {
  Fe xq, zq, xp, zp;
  const u32 last = varbase_mont_ladder(x1, k_in, xq, zq, xp, zp);
  varbase_mont_recover(P, x1, last, xq, zq, xp, zp, ou, ov, oz);
}

}  // namespace jj
