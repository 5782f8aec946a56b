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
// Sum of v over the wave (every lane calls it; 64-lane waves): a butterfly, every lane ends with the total
static JJ_DEV void sig_wave_sum(Fe& v) {
  _Pragma("unroll") for (int m = 32; m >= 1; m >>= 1) {
    Fe o; _Pragma("unroll") for (int i = 0; i < NL; i++) o.l[i] = (u32)__shfl_xor((int)v.l[i], m, 64);
    v = sig_add(v, o);
  }
}
// Sum of v and of bad over the workgroup (every thread calls it): sig_wave_sum, then the waves' sums through LDS.  Thread 0 returns the totals.
template <int THREADS>
static JJ_DEV void sig_block_sum(Fe& v, u32& bad, u32 (*lds)[NL + 1]) {
  sig_wave_sum(v);
  _Pragma("unroll") for (int m = 32; m >= 1; m >>= 1) bad += (u32)__shfl_xor((int)bad, m, 64);
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
// thread 0 stores the workgroup's partial (the totals of sig_block_sum) to its SIG_PART_WORDS words of part
static JJ_DEV void sig_store_partial(u32* part, const Fe& zs, u32 bad) {
  if (threadIdx.x != 0) return;
  u32* p = part + (size_t)blockIdx.x * SIG_PART_WORDS;
  _Pragma("unroll") for (int k = 0; k < NL; k++) p[k] = zs.l[k];
  p[NL] = bad;
}
// r - acc mod r for a canonical plain integer; zero stays zero
static JJ_DEV Fe sig_neg(const Fe& acc) {
  u32 nz = 0; _Pragma("unroll") for (int k = 0; k < NL; k++) nz |= acc.l[k];
  Fe d; _Pragma("unroll") for (int k = 0; k < NL; k++) d.l[k] = (nz ? FrP::P[k] : 0u) - acc.l[k];
  return Fr::carry_full(d);
}
// The weight of signature i: its 16 bytes of z16 zero-extended to the eight words z[] (the scalar of R_i as it is stored), and z < 2^128 as a
// plain integer
static JJ_DEV Fe sig_weight(const void* z16, size_t i, u32 (&z)[8]) {
  const uint4 zz = reinterpret_cast<const uint4*>(z16)[i];
  z[0] = zz.x; z[1] = zz.y; z[2] = zz.z; z[3] = zz.w; z[4] = 0; z[5] = 0; z[6] = 0; z[7] = 0;
  return Fr::unpack(z);
}
// z x mod r as a canonical plain integer, x the 32 bytes at index i of x32; below_r: x < r (asked of s, not of c).  z (plain) times x R
// (from_words_checked reduces any 256-bit pattern): the Montgomery product is z x mod r as a plain value in (-r - 1, 1).  One product per call:
// the kernels store what they have of c before they load s, which keeps them below 64 VGPRs.
static JJ_DEV Fe sig_product(const Fe& zp, const void* x32, size_t i, bool& below_r) {
  u32 w[8];
  load8(w, x32, i);
  return Fr::canon_plain_product(Fr::mul(zp, Fr::from_words_checked(w, below_r)));
}
// a failed decode left (0, 0), which is not on the curve: the identity (0, 1) to slot `at` of points makes its term [x] O
static JJ_DEV void sig_store_identity(void* points, size_t at) {
  u32 id_u[8], id_v[8];
  zero8(id_u); zero8(id_v); id_v[0] = 1;
  store8(points, 2 * at, id_u); store8(points, 2 * at + 1, id_v);
}
static JJ_DEV void sig_copy64(void* dst, size_t to, const void* src, size_t from) {
  u32 w[8];
  load8(w, src, 2 * from); store8(dst, 2 * to, w);
  load8(w, src, 2 * from + 1); store8(dst, 2 * to + 1, w);
}
static JJ_DEV Fe sig_load_plain(const void* base, size_t idx) {
  u32 w[8];
  load8(w, base, idx);
  return Fr::unpack(w);
}

// ---- signatures in consecutive runs (CSR offsets): the groups of jj_sig_keyed_kernels.h, the segments of jj_sig_seg_kernels.h
// the run of signature i: the k with offs[k] <= i < offs[k + 1] (i < offs[K]; empty runs are skipped)
static JJ_DEV u32 sig_key_of(const unsigned long long* offs, u32 K, unsigned long long i) {
  u32 lo = 0, hi = K;                                                  // offs[lo] <= i < offs[hi]
  while (hi - lo > 1) {
    const u32 mid = lo + ((hi - lo) >> 1);
    if (offs[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}
// Segmented sum over the wave (every lane calls it): v becomes the sum over the lanes from this one to the last of its run, a run being
// consecutive lanes with equal keys.  After the step of width m a lane holds the sum of its run's lanes in [lane, lane + 2m); runs are
// contiguous, so equal keys at distance m mean every lane between belongs to the run too.
static JJ_DEV void sig_run_sum(Fe& v, u32 key, int lane) {
  _Pragma("unroll") for (int m = 1; m <= 32; m <<= 1) {
    Fe o; _Pragma("unroll") for (int k = 0; k < NL; k++) o.l[k] = (u32)__shfl_down((int)v.l[k], m, 64);
    const u32 okey = (u32)__shfl_down((int)key, m, 64);
    const Fe sum = sig_add(v, o);
    const u32 take = (lane + m < 64 && okey == key) ? 0xffffffffu : 0u;
    v = Fr::select(v, sum, take);
  }
}
// The sum of the head slots of the run [lo, hi) of this lane's key or segment: heads = { lo } + { every multiple of 64 strictly inside (lo, hi) },
// the slots sig_run_sum's first lanes stored (0 for an empty run).  A run with one head: its lane copies it.  A run with more is summed by
// the whole wave, one such run after the other (lanes stride over the heads, a butterfly finishes), so one run that holds all n signatures costs
// n / 4096 additions per lane, not n / 64 in one.  EVERY lane of the wave must call it, lanes without a run with lo = hi = 0: it votes and
// shuffles over the wave, so the call stands outside any divergent branch.
static JJ_DEV Fe sig_heads_sum(unsigned long long lo, unsigned long long hi, const void* heads, int lane) {
  const u32 cnt = hi > lo ? 1u + (u32)(((hi - 1) >> 6) - (lo >> 6)) : 0u;
  Fe acc = Fr::zero();
  if (cnt) acc = sig_load_plain(heads, (size_t)lo);
  unsigned long long many = __ballot(cnt > 1);                         // wave-uniform
  while (many) {
    const int src = __ffsll((long long)many) - 1;
    many &= many - 1;
    const u32 first = (u32)__shfl((int)(u32)(lo >> 6), src, 64);       // n <= 2^24: the wave index fits a word
    const u32 scnt = (u32)__shfl((int)cnt, src, 64);
    Fe v = Fr::zero();
    for (u32 j = 1 + (u32)lane; j < scnt; j += 64) v = sig_add(v, sig_load_plain(heads, (size_t)(first + j) << 6));
    sig_wave_sum(v);
    if (lane == src) acc = sig_add(acc, v);
  }
  return acc;
}

// scalars: z_i at i, t_i = z_i c_i mod r at n + i (32 bytes each);  part: SIG_PART_WORDS words per workgroup
__global__ void __launch_bounds__(SIG_THREADS) k_sig_terms(size_t n, const void* s32, const void* c32, const void* z16, const uint8_t* ok, void* points, void* scalars, u32* part) {
  __shared__ u32 lds[SIG_THREADS / 64][NL + 1];
  const size_t i = (size_t)blockIdx.x * SIG_THREADS + threadIdx.x;
  Fe zs = Fr::zero();
  u32 bad = 0;
  if (i < n) {
    u32 z[8], w[8];
    const Fe zp = sig_weight(z16, i, z);
    bool c_ok, s_ok;                                                   // c is taken mod r: c_ok is not read
    const Fe t = sig_product(zp, c32, i, c_ok);
    store8(scalars, i, z);
    Fr::pack(w, t);
    store8(scalars, n + i, w);
    zs = sig_product(zp, s32, i, s_ok);
    const bool r_ok = ok[i] != 0, a_ok = ok[n + i] != 0;
    if (!r_ok) sig_store_identity(points, i);
    if (!a_ok) sig_store_identity(points, n + i);
    bad = (r_ok && a_ok && s_ok) ? 0u : 1u;
  }
  sig_block_sum<SIG_THREADS>(zs, bad, lds);
  sig_store_partial(part, zs, bad);
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
    u32 w[8];
    Fr::pack(w, sig_neg(acc));
    store8(scalars, 2 * n, w);
    *flag = bad ? 1u : 0u;
  }
  if (threadIdx.x < 16) reinterpret_cast<u32*>(points)[(size_t)2 * n * 16 + threadIdx.x] = base64[threadIdx.x];
}

}  // namespace jj
