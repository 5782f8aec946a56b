// Kernels of jj_sigbatch_ragged (jj_msm.hip): S batch Schnorr checks over consecutive runs (CSR offsets) of one signature array, one verdict point
// per run.  Segment g with L_g = offsets[g + 1] - offsets[g] signatures owns the terms
//   T_g = 2 offsets[g] + g  ..  T_g + 2 L_g :   [z_i] R_i (L_g terms) | [z_i c_i mod r] A_i (L_g terms) | [r - sum_{i in g} z_i s_i mod r] B
// of ONE term array that the ragged MSM sums segment by segment (term offsets 2 offsets[g] + g); an empty segment is the single term [0] B.
// The decoder has run over r32 | a32 with JJ_DECOMPRESS_CLEAR_COFACTOR: `dec` holds [8] R_0 .. [8] R_{n-1} | [8] A_0 .. [8] A_{n-1} (a failed
// decode: (0, 0)) and ok[0, 2n) their ok bytes; b8 holds [8] B.  Every point of a sum then lies in the image of [8] and the sum IS the verdict
// point: no doublings behind the MSM.
// k_sig_seg_terms, one signature per lane, writes the signature's two scalars and two points to its segment's term positions (the identity in
// place of a failed decode), stores 1 to bad[g] for a unit that fails (decode, or s >= r) and adds z_i s_i over the lanes of its wave that share a
// segment; each run's first lane stores the sum to its 32-byte head slot.  A run starts where a segment starts or where a wave starts, so
//   heads(g) = { offsets[g] } + { every multiple of 64 strictly inside (offsets[g], offsets[g + 1]) }
// -- a pure function of the offsets, as in jj_sig_keyed_kernels.h: k_sig_seg_close reads only slots written in this call.  k_sig_seg_close, one
// segment per lane, adds heads(g) (a whole wave strides over a segment with several) and writes the segment's last term.  k_sig_seg_verdict, one
// segment per lane, runs behind the sums and writes (0, q - 1) over the rows with bad[g] set.  bad[] is cleared by a memset before the first
// kernel; every writer stores the same value.  Everything is public (VARIABLE-TIME is allowed).  Plain vector stores; no atomics.
#pragma once
#include "jj_sig_keyed_kernels.h"

namespace jj {

// points / scalars: the 2n + S terms;  heads: 32 bytes per signature (see above);  bad: one word per segment
__global__ void __launch_bounds__(SIG_THREADS) k_sig_seg_terms(size_t n, u32 S, const unsigned long long* offs, const void* s32, const void* c32, const void* z16, const uint8_t* ok,
                                                               const void* dec, void* points, void* scalars, void* heads, u32* bad) {
  const size_t i = (size_t)blockIdx.x * SIG_THREADS + threadIdx.x;
  const int lane = threadIdx.x & 63;
  Fe zs = Fr::zero();
  u32 seg = 0xffffffffu;                                               // lanes past n: no segment matches theirs (S <= 2^24)
  bool head = false;
  if (i < n) {
    u32 z[8], w[8];
    const Fe zp = sig_weight(z16, i, z);
    seg = sig_key_of(offs, S, i);
    const unsigned long long lo = offs[seg];
    const size_t len = (size_t)(offs[seg + 1] - lo), at = 2 * (size_t)lo + seg + (size_t)(i - lo);      // term of R_i; A_i is len terms further
    bool c_ok, s_ok;                                                   // c is taken mod r: c_ok is not read
    const Fe t = sig_product(zp, c32, i, c_ok);
    store8(scalars, at, z);
    Fr::pack(w, t);
    store8(scalars, at + len, w);
    zs = sig_product(zp, s32, i, s_ok);
    const bool r_ok = ok[i] != 0, a_ok = ok[n + i] != 0;
    if (r_ok) sig_copy64(points, at, dec, i); else sig_store_identity(points, at);
    if (a_ok) sig_copy64(points, at + len, dec, n + i); else sig_store_identity(points, at + len);
    if (!(r_ok && a_ok && s_ok)) bad[seg] = 1u;
    head = lane == 0 || lo == i;
  }
  sig_run_sum(zs, seg, lane);
  if (head) {
    u32 w[8];
    Fr::pack(w, zs);
    store8(heads, i, w);
  }
}

// One segment per lane: sigma_g = the sum of heads(g) (sig_heads_sum), then scalar T_g + 2 L_g = r - sigma_g mod r and point T_g + 2 L_g = [8] B.
__global__ void __launch_bounds__(SIG_THREADS) k_sig_seg_close(u32 S, const unsigned long long* offs, const void* heads, const void* b8, void* points, void* scalars) {
  const u32 g = blockIdx.x * SIG_THREADS + threadIdx.x;
  unsigned long long lo = 0, hi = 0;
  if (g < S) { lo = offs[g]; hi = offs[g + 1]; }
  const Fe acc = sig_heads_sum(lo, hi, heads, threadIdx.x & 63);
  if (g < S) {
    const size_t at = 2 * (size_t)hi + g;                              // T_g + 2 L_g
    u32 w[8];
    Fr::pack(w, sig_neg(acc));
    store8(scalars, at, w);
    sig_copy64(points, at, b8, 0);
  }
}

// One segment per lane, behind the sums: the order-2 point (0, q - 1) over the row of a segment that holds a malformed unit.
__global__ void __launch_bounds__(SIG_THREADS) k_sig_seg_verdict(u32 S, const u32* bad, void* out64) {
  const u32 g = blockIdx.x * SIG_THREADS + threadIdx.x;
  if (g >= S || !bad[g]) return;
  Fe m; _Pragma("unroll") for (int k = 0; k < NL; k++) m.l[k] = FqP::P[k];
  m.l[0] -= 1u;                                                        // q is odd: no borrow
  u32 u[8], v[8];
  zero8(u);
  Fq::pack(v, m);
  store8(out64, 2 * (size_t)g, u); store8(out64, 2 * (size_t)g + 1, v);
}

}  // namespace jj
