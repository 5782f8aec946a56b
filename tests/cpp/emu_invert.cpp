// Host emulation of Field::invert_divsteps (jubjub_amd/csrc/jj_field.h compiled with -DJJ_HOST_EMU) against Field::invert, the power
// chain it stands in for in k_normalize and k_varbase_mont_x1: the same device function, run on the CPU with a 128-bit shadow of every
// 64-bit accumulator and, after every batch of divsteps, the check that d and e still lie in (-2p, p).  Test infrastructure only
// (tests/test_emu_invert.py); nothing in jubjub_amd/ links or loads it.  With -DEMU_INVERT_MAIN it is a stand-alone program (its own
// seeded inputs, exit status 0 iff every inverse agrees and nothing overflowed): the form to run under a host sanitizer.
#include <stdint.h>
#include <string.h>
#include <atomic>
#include <thread>
#include <vector>
#define JJ_HOST_EMU 1
#include "../../jubjub_amd/csrc/jj_field.h"

using namespace jj;

static std::atomic<int> g_overflow{0};
extern "C" void jj_emu_overflow(const char*) { g_overflow++; }
extern "C" int emu_overflow_count(void) { return g_overflow.load(); }
extern "C" void emu_overflow_reset(void) { g_overflow = 0; }

// the input of case `op` from two 32-byte little-endian integers a, b:
//   0: a as a product (from_words)          1: sub of two products          2: add of two products
//   3: the canonical Montgomery digits of a, minus p, minus the plain integer b (b < 0.2 p: a value in (-1.2p, 0))
template <class F, class P>
static Fe make_input(int op, const uint8_t* a, const uint8_t* b) {
  u32 wa[8], wb[8];
  memcpy(wa, a, 32); memcpy(wb, b, 32);
  const Fe x = F::from_words(wa);
  switch (op) {
    case 1: return F::sub(x, F::from_words(wb));
    case 2: return F::add(x, F::from_words(wb));
    case 3: return F::sub(F::sub(F::canon(x), F::konst(P::P)), F::unpack(wb));
    default: return x;
  }
}

template <class F, class P>
static void run_range(size_t lo, size_t hi, const uint8_t* ops, const uint8_t* a, const uint8_t* b, uint8_t* out_div, uint8_t* out_ref) {
  for (size_t i = lo; i < hi; i++) {
    const Fe x = make_input<F, P>(ops[i], a + 32 * i, b + 32 * i);
    u32 w[8];
    F::pack(w, F::canon(F::invert_divsteps(x))); memcpy(out_div + 32 * i, w, 32);
    F::pack(w, F::canon(F::invert(x))); memcpy(out_ref + 32 * i, w, 32);
  }
}

// field: 0 = Fq, 1 = Fr.  out_div / out_ref: canon(invert_divsteps(x)) and canon(invert(x)) as 32-byte integers (Montgomery form, in [0, p))
extern "C" void emu_invert_both(int field, size_t n, const uint8_t* ops, const uint8_t* a, const uint8_t* b, uint8_t* out_div, uint8_t* out_ref, int threads) {
  std::vector<std::thread> pool;
  if (threads < 1) threads = 1;
  for (int t = 0; t < threads; t++) {
    const size_t lo = n * t / threads, hi = n * (t + 1) / threads;
    if (field == 0) pool.emplace_back(run_range<Fq, FqP>, lo, hi, ops, a, b, out_div, out_ref);
    else pool.emplace_back(run_range<Fr, FrP>, lo, hi, ops, a, b, out_div, out_ref);
  }
  for (auto& th : pool) th.join();
}

#ifdef EMU_INVERT_MAIN
#include <stdio.h>
int main() {
  uint64_t s = 0x9e3779b97f4a7c15ull;
  auto next = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
  const size_t n = 4000;
  std::vector<uint8_t> ops(n), a(32 * n), b(32 * n), d(32 * n), r(32 * n);
  int bad = 0;
  for (int field = 0; field < 2; field++) {
    for (size_t i = 0; i < n; i++) {
      ops[i] = (uint8_t)(i & 3);
      for (int k = 0; k < 32; k++) { a[32 * i + k] = (uint8_t)next(); b[32 * i + k] = (uint8_t)next(); }
      if (ops[i] == 3) { b[32 * i + 31] = 0; b[32 * i + 30] &= 0x7f; }          // b < 2^247 < 0.2 p for both fields
      if (i < 8) memset(&a[32 * i], 0, 32), a[32 * i] = (uint8_t)(i >> 2);     // 0 and 1
    }
    emu_invert_both(field, n, ops.data(), a.data(), b.data(), d.data(), r.data(), 1);
    bad += memcmp(d.data(), r.data(), 32 * n) != 0;
  }
  printf("emu_invert: %s, %d overflow reports\n", bad ? "MISMATCH" : "all inverses agree", emu_overflow_count());
  return bad || emu_overflow_count();
}
#endif
