// ChaCha20 (RFC 8439 section 2.3: 32-bit block counter, 96-bit nonce), one key and one row per lane: the block function and "xor a row with
// the keystream" -- device code, everything in registers.  Included by jj_kernels.h (k_chacha20_xor, jj_chacha20_xor) and, with -DJJ_HOST_EMU,
// by tests/cpp/emu_ka.cpp.
//
// The 16 state words (four constants, eight key words, the counter, three nonce words) and the 16 working words stay in registers; the 20
// rounds are written out (ten double rounds, unrolled), every index a constant, so nothing goes to scratch (tests/test_codegen_ka.py).  A
// rotation to the left by n is the funnel shift (x : x) >> (32 - n): one v_alignbit_b32 for each of 16, 12, 8 and 7.  Per block: 320 add, 320
// xor, 320 alignbit and the 16 final additions.
// A row is `nwords` dwords (the entry point asks len = 4 * nwords, a multiple of 4 in 4..1024, and rows that start on a multiple of 4 from a
// 16-byte aligned base: every access is an aligned dword at every skew of the row).  Block b of the keystream covers words 16 b .. 16 b + 15
// of the row; a word at or past nwords is neither read nor written, so nothing is touched past the row's len bytes.  The block counter is
// counter + b modulo 2^32 (plain 32-bit addition).  nwords, nonce and counter are the same in every lane: the block loop and the predicate on
// the word index are uniform.
#pragma once
#include "jj_field.h"

namespace jj {

struct ChaCha20 {
  static constexpr u32 SIGMA[4] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u};      // "expand 32-byte k"

  template <int N>
  static JJ_DEV u32 rotl(u32 x) {
#ifdef JJ_HOST_EMU
    return (x << N) | (x >> (32 - N));
#else
    return __builtin_amdgcn_alignbit(x, x, 32 - N);
#endif
  }
  static JJ_DEV void quarter(u32& a, u32& b, u32& c, u32& d) {
    a += b; d = rotl<16>(d ^ a);
    c += d; b = rotl<12>(b ^ c);
    a += b; d = rotl<8>(d ^ a);
    c += d; b = rotl<7>(b ^ c);
  }
  // x <- the keystream block of (key, counter, nonce) as 16 little-endian words
  static JJ_DEV void block(u32 (&x)[16], const u32 (&key)[8], u32 counter, const u32 (&nonce)[3]) {
    u32 s[16];
    _Pragma("unroll") for (int i = 0; i < 4; i++) s[i] = SIGMA[i];
    _Pragma("unroll") for (int i = 0; i < 8; i++) s[4 + i] = key[i];
    s[12] = counter; s[13] = nonce[0]; s[14] = nonce[1]; s[15] = nonce[2];
    _Pragma("unroll") for (int i = 0; i < 16; i++) x[i] = s[i];
    _Pragma("unroll") for (int r = 0; r < 10; r++) {
      quarter(x[0], x[4], x[8], x[12]); quarter(x[1], x[5], x[9], x[13]); quarter(x[2], x[6], x[10], x[14]); quarter(x[3], x[7], x[11], x[15]);
      quarter(x[0], x[5], x[10], x[15]); quarter(x[1], x[6], x[11], x[12]); quarter(x[2], x[7], x[8], x[13]); quarter(x[3], x[4], x[9], x[14]);
    }
    _Pragma("unroll") for (int i = 0; i < 16; i++) x[i] += s[i];
  }
  // out[j] = in[j] ^ keystream word j for j < nwords, the block counter starting at `counter`
  static JJ_DEV void xor_row(const u32* in, u32* out, u32 nwords, const u32 (&key)[8], u32 counter, const u32 (&nonce)[3]) {
    #pragma unroll 1
    for (u32 w0 = 0; w0 < nwords; w0 += 16, counter++) {
      u32 x[16];
      block(x, key, counter, nonce);
      if (nwords - w0 >= 16) {
        _Pragma("unroll") for (int j = 0; j < 16; j++) out[w0 + j] = in[w0 + j] ^ x[j];
      } else {
        _Pragma("unroll") for (int j = 0; j < 15; j++) if (w0 + j < nwords) out[w0 + j] = in[w0 + j] ^ x[j];
      }
    }
  }
};

}  // namespace jj
