// Kernels of jj_sigbatch_begin (jj_msm.hip): the scalars of a batch Schnorr check, prepared on the device for ONE multi-scalar multiplication.
//   sum_i [z_i] R_i + sum_i [z_i c_i mod r] A_i - [sum_i z_i s_i mod r] B        (2n + 1 terms; the cofactor is cleared by the host tail)
// k_decompress (jj_kernels.h, launched by decompress_dev) has written R_i and A_i to slots [0, n) and [n, 2n) of the points workspace and their ok
// bytes to ok[0, n) and ok[n, 2n).  k_sig_terms, one signature per lane, writes the 2n scalars, replaces the points of failed units by the identity
// and leaves ONE partial of sum z_i s_i per workgroup; k_sig_close, one workgroup, adds the partials and writes term 2n and the malformed flag.
// Everything is public (VARIABLE-TIME is allowed; nothing here branches on data except the identity stores).  Results leave through plain vector
// stores; no atomics.
#pragma once

namespace jj {

constexpr int SIG_THREADS = 256;             // k_sig_terms: signatures per workgroup
constexpr int SIG_CLOSE_THREADS = 256;       // k_sig_close: partials per pass of its loop (one pass covers SIG_THREADS * SIG_CLOSE_THREADS signatures)
constexpr int SIG_PART_WORDS = 12;           // a workgroup's partial: 9 limbs (canonical plain integer below r), failed units, 2 words of padding

// a + b mod r for canonical plain integers (limbs in [0, 2^29), value in [0, r)): one conditional subtraction
static JJ_DEV Fe sig_add(const Fe& a, const Fe& b) {
  const Fe s = Fr::add(a, b);
  Fe d; _Pragma("unroll") for (int i = 0; i < NL; i++) d.l[i] = s.l[i] - FrP::P[i];
  d = Fr::carry_full(d);
  const u32 neg = (u32)((i32)d.l[NL - 1] >> 31);
  return Fr::select(d, Fr::carry_full(s), neg);
}
// Sum of v and of bad over the workgroup (every thread calls it; 64-lane waves): butterflies through the wave's lanes, then the waves' sums
// through LDS.  Thread 0 returns the totals.
template <int THREADS>
static JJ_DEV void sig_block_sum(Fe& v, u32& bad, u32 (*lds)[NL + 1]) {
  _Pragma("unroll") for (int m = 32; m >= 1; m >>= 1) {
    Fe o; _Pragma("unroll") for (int i = 0; i < NL; i++) o.l[i] = (u32)__shfl_xor((int)v.l[i], m, 64);
    v = sig_add(v, o);
    bad += (u32)__shfl_xor((int)bad, m, 64);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { _Pragma("unroll") for (int i = 0; i < NL; i++) lds[wave][i] = v.l[i]; lds[wave][NL] = bad; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < THREADS / 64; w++) {
      Fe o; _Pragma("unroll") for (int i = 0; i < NL; i++) o.l[i] = lds[w][i];
      v = sig_add(v, o);
      bad += lds[w][NL];
    }
  }
}

// scalars: z_i at i, t_i = z_i c_i mod r at n + i (32 bytes each);  part: SIG_PART_WORDS words per workgroup
__global__ void __launch_bounds__(SIG_THREADS) k_sig_terms(size_t n, const void* s32, const void* c32, const void* z16, const uint8_t* ok, void* points, void* scalars, u32* part) {
  __shared__ u32 lds[SIG_THREADS / 64][NL + 1];
  const size_t i = (size_t)blockIdx.x * SIG_THREADS + threadIdx.x;
  Fe zs = Fr::zero();
  u32 bad = 0;
  if (i < n) {
    u32 z[8], w[8];
    const uint4 zz = reinterpret_cast<const uint4*>(z16)[i];
    z[0] = zz.x; z[1] = zz.y; z[2] = zz.z; z[3] = zz.w; z[4] = 0; z[5] = 0; z[6] = 0; z[7] = 0;
    const Fe zp = Fr::unpack(z);                                       // the plain integer z < 2^128
    // z (plain) times c R (from_words reduces any 256-bit pattern): the Montgomery product is z c mod r as a plain value in (-r - 1, 1)
    load8(w, c32, i);
    const Fe t = Fr::canon_plain_product(Fr::mul(zp, Fr::from_words(w)));
    store8(scalars, i, z);
    Fr::pack(w, t);
    store8(scalars, n + i, w);
    load8(w, s32, i);
    bool s_ok;
    const Fe sm = Fr::from_words_checked(w, s_ok);                     // s_ok: s < r
    zs = Fr::canon_plain_product(Fr::mul(zp, sm));
    const bool r_ok = ok[i] != 0, a_ok = ok[n + i] != 0;
    // a failed decode left (0, 0), which is not on the curve: its term becomes [x] O
    u32 id_u[8], id_v[8];
    zero8(id_u); zero8(id_v); id_v[0] = 1;
    if (!r_ok) { store8(points, 2 * i, id_u); store8(points, 2 * i + 1, id_v); }
    if (!a_ok) { store8(points, 2 * (n + i), id_u); store8(points, 2 * (n + i) + 1, id_v); }
    bad = (r_ok && a_ok && s_ok) ? 0u : 1u;
  }
  sig_block_sum<SIG_THREADS>(zs, bad, lds);
  if (threadIdx.x == 0) {
    u32* p = part + (size_t)blockIdx.x * SIG_PART_WORDS;
    _Pragma("unroll") for (int k = 0; k < NL; k++) p[k] = zs.l[k];
    p[NL] = bad;
  }
}

// One workgroup: sigma = the sum of the nblk partials (a loop when there are more partials than threads); scalar 2n = r - sigma mod r, point 2n = B,
// *flag = 1 when any unit failed (a bad encoding or s >= r), else 0.  flag points into the job's page-locked buffer, next to the records.
__global__ void __launch_bounds__(SIG_CLOSE_THREADS) k_sig_close(size_t n, u32 nblk, const u32* part, const u32* base64, void* points, void* scalars, u32* flag) {
  __shared__ u32 lds[SIG_CLOSE_THREADS / 64][NL + 1];
  Fe acc = Fr::zero();
  u32 bad = 0;
  for (u32 b = threadIdx.x; b < nblk; b += SIG_CLOSE_THREADS) {
    const u32* p = part + (size_t)b * SIG_PART_WORDS;
    Fe v; _Pragma("unroll") for (int k = 0; k < NL; k++) v.l[k] = p[k];
    acc = sig_add(acc, v);
    bad += p[NL];
  }
  sig_block_sum<SIG_CLOSE_THREADS>(acc, bad, lds);
  if (threadIdx.x == 0) {
    u32 nz = 0; _Pragma("unroll") for (int k = 0; k < NL; k++) nz |= acc.l[k];
    Fe d; _Pragma("unroll") for (int k = 0; k < NL; k++) d.l[k] = (nz ? FrP::P[k] : 0u) - acc.l[k];
    u32 w[8];
    Fr::pack(w, Fr::carry_full(d));
    store8(scalars, 2 * n, w);
    *flag = bad ? 1u : 0u;
  }
  if (threadIdx.x < 16) reinterpret_cast<u32*>(points)[(size_t)2 * n * 16 + threadIdx.x] = base64[threadIdx.x];
}

}  // namespace jj
