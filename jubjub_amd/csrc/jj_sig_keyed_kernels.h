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
    u32 z[8];
    const Fe zp = sig_weight(z16, i, z);
    bool c_ok, s_ok;                                                   // c is taken mod r: c_ok is not read
    t = sig_product(zp, c32, i, c_ok);
    store8(scalars, i, z);
    zs = sig_product(zp, s32, i, s_ok);
    const bool r_ok = ok[i] != 0;
    if (!r_ok) sig_store_identity(points, i);                          // its term becomes [z] O
    bad = (r_ok && s_ok) ? 0u : 1u;
    key = sig_key_of(offs, K, i);
    head = lane == 0 || offs[key] == i;
  }
  sig_run_sum(t, key, lane);
  if (head) {
    u32 w[8];
    Fr::pack(w, t);
    store8(heads, i, w);
  }
  sig_block_sum<SIG_THREADS>(zs, bad, lds);
  sig_store_partial(part, zs, bad);
}

// One key per lane: scalar n + k = the sum of heads(k) (sig_heads_sum).  part: this kernel's partials (zero sum, failed key decodes).
__global__ void __launch_bounds__(SIG_THREADS) k_sig_keyed_close(size_t n, u32 K, const unsigned long long* offs, const uint8_t* ok, const void* heads, void* points, void* scalars,
                                                                 u32* part) {
  __shared__ u32 lds[SIG_THREADS / 64][NL + 1];
  const u32 k = blockIdx.x * SIG_THREADS + threadIdx.x;
  unsigned long long lo = 0, hi = 0;
  u32 bad = 0;
  if (k < K) {
    lo = offs[k]; hi = offs[k + 1];
    if (ok[n + k] == 0) { sig_store_identity(points, n + k); bad = 1; }
  }
  const Fe acc = sig_heads_sum(lo, hi, heads, threadIdx.x & 63);
  if (k < K) {
    u32 w[8];
    Fr::pack(w, acc);
    store8(scalars, n + k, w);
  }
  Fe none = Fr::zero();
  sig_block_sum<SIG_THREADS>(none, bad, lds);
  sig_store_partial(part, none, bad);
}

}  // namespace jj
