// Kernels of jj_sigbatch_keyed_begin (jj_msm.hip): the batch Schnorr check of jj_sig_kernels.h for signatures grouped by key (CSR offsets), with
// the terms of equal keys folded into one:
//   sum_i [z_i] R_i + sum_k [sum_{i in group k} z_i c_i mod r] A_k - [sum_i z_i s_i mod r] B        (n + K + 1 terms)
// k_decompress has written R_0..R_{n-1} | A_0..A_{K-1} to slots [0, n + K) of the points workspace and their ok bytes to ok[0, n + K).
// k_sig_keyed_terms, one signature per lane, writes scalar i = z_i, replaces a failed R by the identity, adds t_i = z_i c_i mod r over the lanes
// of its wave that hold the same key and stores each run's sum to the 32-byte head slot of the run's first lane; it leaves ONE partial of
// sum z_i s_i per workgroup, like k_sig_terms.  A run starts where a group starts or where a wave starts, so the slots that hold a sum are
//   heads(k) = { offsets[k] } + { every multiple of 64 strictly inside (offsets[k], offsets[k+1]) }
// -- a pure function of the offsets: k_sig_keyed_close reads only slots written in this call (the workspace is pooled).  k_sig_keyed_close, one
// key per lane, writes scalar n + k = the sum of heads(k) (0 for an empty group), the identity in place of a key that did not decode, and one
// partial (zero sum, failed keys) per workgroup behind those of the terms kernel; k_sig_close (jj_sig_kernels.h, unchanged) then closes sigma over
// all partials and writes term n + K and the malformed flag.  Everything is public (VARIABLE-TIME is allowed).  Plain vector stores; no atomics.
#pragma once
#include "jj_sig_kernels.h"

namespace jj {

// the group of signature i: the k with offs[k] <= i < offs[k + 1] (i < offs[K]; empty groups are skipped)
static JJ_DEV u32 sig_key_of(const unsigned long long* offs, u32 K, unsigned long long i) {
  u32 lo = 0, hi = K;                                                  // offs[lo] <= i < offs[hi]
  while (hi - lo > 1) {
    const u32 mid = lo + ((hi - lo) >> 1);
    if (offs[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}
static JJ_DEV Fe sig_load_plain(const void* base, size_t idx) {
  u32 w[8];
  load8(w, base, idx);
  return Fr::unpack(w);
}

// scalars: z_i at i;  heads: 32 bytes per signature (see above);  part: SIG_PART_WORDS words per workgroup
__global__ void __launch_bounds__(SIG_THREADS) k_sig_keyed_terms(size_t n, u32 K, const unsigned long long* offs, const void* s32, const void* c32, const void* z16, const uint8_t* ok,
                                                                 void* points, void* scalars, void* heads, u32* part) {
  __shared__ u32 lds[SIG_THREADS / 64][NL + 1];
  const size_t i = (size_t)blockIdx.x * SIG_THREADS + threadIdx.x;
  const int lane = threadIdx.x & 63;
  Fe zs = Fr::zero(), t = Fr::zero();
  u32 bad = 0, key = 0xffffffffu;                                      // lanes past n: no key matches theirs (K <= 2^24)
  bool head = false;
  if (i < n) {
    u32 z[8], w[8];
    const uint4 zz = reinterpret_cast<const uint4*>(z16)[i];
    z[0] = zz.x; z[1] = zz.y; z[2] = zz.z; z[3] = zz.w; z[4] = 0; z[5] = 0; z[6] = 0; z[7] = 0;
    const Fe zp = Fr::unpack(z);                                       // the plain integer z < 2^128
    load8(w, c32, i);
    t = Fr::canon_plain_product(Fr::mul(zp, Fr::from_words(w)));       // z c mod r, canonical plain (as in k_sig_terms)
    store8(scalars, i, z);
    load8(w, s32, i);
    bool s_ok;
    const Fe sm = Fr::from_words_checked(w, s_ok);                     // s_ok: s < r
    zs = Fr::canon_plain_product(Fr::mul(zp, sm));
    const bool r_ok = ok[i] != 0;
    if (!r_ok) {                                                       // a failed decode left (0, 0): its term becomes [z] O
      u32 id_u[8], id_v[8];
      zero8(id_u); zero8(id_v); id_v[0] = 1;
      store8(points, 2 * i, id_u); store8(points, 2 * i + 1, id_v);
    }
    bad = (r_ok && s_ok) ? 0u : 1u;
    key = sig_key_of(offs, K, i);
    head = lane == 0 || offs[key] == i;
  }
  // segmented sum: after the step of width m a lane holds the sum of its run's lanes in [lane, lane + 2m).  Runs are contiguous, so equal keys
  // at distance m mean every lane between belongs to the run too.
  _Pragma("unroll") for (int m = 1; m <= 32; m <<= 1) {
    Fe o; _Pragma("unroll") for (int k = 0; k < NL; k++) o.l[k] = (u32)__shfl_down((int)t.l[k], m, 64);
    const u32 okey = (u32)__shfl_down((int)key, m, 64);
    const Fe sum = sig_add(t, o);
    const u32 take = (lane + m < 64 && okey == key) ? 0xffffffffu : 0u;
    t = Fr::select(t, sum, take);
  }
  if (head) {
    u32 w[8];
    Fr::pack(w, t);
    store8(heads, i, w);
  }
  sig_block_sum<SIG_THREADS>(zs, bad, lds);
  if (threadIdx.x == 0) {
    u32* p = part + (size_t)blockIdx.x * SIG_PART_WORDS;
    _Pragma("unroll") for (int k = 0; k < NL; k++) p[k] = zs.l[k];
    p[NL] = bad;
  }
}

// One key per lane.  A key whose group lies in one wave of the terms kernel has one head: its lane copies it.  A key with more heads is summed by
// its whole wave, one such key after the other (lanes stride over the heads, a butterfly finishes), so one key that holds all n signatures costs
// n / 4096 additions per lane, not n / 64 in one.  part: this kernel's partials (zero sum, failed key decodes).
__global__ void __launch_bounds__(SIG_THREADS) k_sig_keyed_close(size_t n, u32 K, const unsigned long long* offs, const uint8_t* ok, const void* heads, void* points, void* scalars,
                                                                 u32* part) {
  __shared__ u32 lds[SIG_THREADS / 64][NL + 1];
  const u32 k = blockIdx.x * SIG_THREADS + threadIdx.x;
  const int lane = threadIdx.x & 63;
  unsigned long long lo = 0;
  u32 cnt = 0, bad = 0;
  Fe acc = Fr::zero();
  if (k < K) {
    lo = offs[k];
    const unsigned long long hi = offs[k + 1];
    cnt = hi > lo ? 1u + (u32)(((hi - 1) >> 6) - (lo >> 6)) : 0u;      // heads(k)
    if (cnt) acc = sig_load_plain(heads, (size_t)lo);
    if (ok[n + k] == 0) {
      u32 id_u[8], id_v[8];
      zero8(id_u); zero8(id_v); id_v[0] = 1;
      store8(points, 2 * (n + k), id_u); store8(points, 2 * (n + k) + 1, id_v);
      bad = 1;
    }
  }
  unsigned long long many = __ballot(cnt > 1);                         // wave-uniform
  while (many) {
    const int src = __ffsll((long long)many) - 1;
    many &= many - 1;
    const u32 first = (u32)__shfl((int)(u32)(lo >> 6), src, 64);       // n <= 2^24: the wave index fits a word
    const u32 scnt = (u32)__shfl((int)cnt, src, 64);
    Fe v = Fr::zero();
    for (u32 j = 1 + (u32)lane; j < scnt; j += 64) v = sig_add(v, sig_load_plain(heads, (size_t)(first + j) << 6));
    _Pragma("unroll") for (int m = 32; m >= 1; m >>= 1) {
      Fe o; _Pragma("unroll") for (int q = 0; q < NL; q++) o.l[q] = (u32)__shfl_xor((int)v.l[q], m, 64);
      v = sig_add(v, o);
    }
    if (lane == src) acc = sig_add(acc, v);
  }
  if (k < K) {
    u32 w[8];
    Fr::pack(w, acc);
    store8(scalars, n + k, w);
  }
  Fe none = Fr::zero();
  sig_block_sum<SIG_THREADS>(none, bad, lds);
  if (threadIdx.x == 0) {
    u32* p = part + (size_t)blockIdx.x * SIG_PART_WORDS;
    _Pragma("unroll") for (int q = 0; q < NL; q++) p[q] = none.l[q];
    p[NL] = bad;
  }
}

}  // namespace jj
