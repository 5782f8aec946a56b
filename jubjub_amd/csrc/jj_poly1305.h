// Poly1305 (RFC 8439 section 2.5) and the ChaCha20-Poly1305 AEAD built on it (section 2.8), one key and one row per lane -- device code,
// everything in registers, every index a constant.  Included by jj_kernels.h (k_poly1305, k_aead: jj_poly1305, jj_aead_open, jj_aead_seal) and,
// with -DJJ_HOST_EMU, by tests/cpp/emu_aead.cpp.
//
// Limbs: r, the accumulator h and every block as five limbs of 26 bits (bit 26 i of the number is bit 0 of limb i); s as four dwords.
// r is clamped (r &= 0x0ffffffc0ffffffc0ffffffc0fffffff) by masking its limbs: r0 <= 0x3ffffff, r1 <= 0x3ffff03, r2 <= 0x3ffc0ff,
// r3 <= 0x3f03fff, r4 <= 0x00fffff.  s_i = 5 r_i (i = 1..4) < 5 * 2^26 is kept beside it, so the wrap of 2^130 = 5 (mod p) costs no
// multiplication per block: column k of h * r is  sum_{i <= k} h_i r_{k-i} + sum_{i > k} h_i s_{5+k-i},  five products a column, 25 a block,
// each one v_mad_u64_u32 into the column's 64-bit sum.
//
// Why no column overflows.  Between two blocks h0, h2, h3, h4 < 2^26 and h1 < 2^26 + 2^8 (shown below).  A block adds limbs below 2^26 (the
// top one below 2^24, plus 2^24 for the bit behind a whole block), so every factor h_i < 2^27 + 2^8 < 2^28.  A product is below
// 2^28 * 5 * 2^26 < 2^57, five of them below 2^60, and the carry that comes in from the column below is below 2^60 / 2^26 = 2^34: every column
// stays below 2^61 in a u64.  The top column holds no s_i (h0 r4 + h1 r3 + h2 r2 + h3 r1 + h4 r0 < 5 * 2^28 * 2^26 < 2^57 with its carry), so
// what leaves it is c < 2^31; it comes back into limb 0 as 5 c through one more 64-bit multiply-add, t = 5 c + (column 0 mod 2^26) < 2^34,
// which leaves h0 = t mod 2^26 and adds t >> 26 < 2^8 to h1 < 2^26: the bounds this paragraph started from.
//
// finish() is complete.  First one carry pass h1 -> h2 -> h3 -> h4, the bit that leaves limb 4 (the value was below 2^130 + 2^35, so it is 0 or
// 1) times 5 into h0 and h0's carry into h1: if the bit was 1 the limbs 2..4 are now 0 and h1 < 2^9, if it was 0 nothing moved into h0; either
// way every limb is below 2^26 and h < 2^130 as a number.  Then g = h + 5 with a full carry chain: bit 26 of g4 is set exactly when h >= p =
// 2^130 - 5, and g mod 2^130 = h - p then.  h is replaced by g under the all-ones-or-zero mask made from that bit (and / andn / or on the limbs:
// no compare, no select), so h in [p, 2^130) comes out as h - p.  The tag is (h mod 2^128) + s mod 2^128: one dword addition and three with
// carry (the carry stays in the carry bit on the device, in a u64 on the host), the carry out of the top dropped.
//
// TIMING: no branch, no select and no address depends on r, s, h, the data or a tag.  The only predicates are on the block count and on the
// hibit argument, both the same in every lane and functions of the public lengths.
//
// The AEAD (Aead::row): the one-time key is words 0..7 of ChaCha20 block 0 of (key, nonce); the data stream starts at block 1; the MAC runs over
// aad || pad16 || ciphertext || pad16 || le64(aad_len) || le64(len), every block a whole 16 bytes.  It is walked in STEPS of up to 16 words, so
// that one ChaCha20 block (seal) or 16 loads in flight (open) stand in front of up to four absorbed blocks: step 0 is the aad (at most 64 bytes =
// 16 words, zero-padded by the caller), steps 1 .. ceil(nwords / 16) the ciphertext, the last step the two lengths.  The four absorbs of a step
// are written once, in ONE loop, under a uniform predicate on the step's block count.
// seal: ciphertext words are absorbed as they are produced and stored; the tag goes behind them (dst: nwords + 4 dwords).
// open: the MAC runs over the ciphertext first; the tag is compared as an OR over the four xored words, without an early exit; then the keystream
// pass stores (ciphertext ^ keystream) & (0 - ok) -- a failed row is written as zeros, never as plaintext, and the verdict costs no divergence.
// The row is read twice (the second read comes from the cache where the row still is there; profiles/aead_ab.txt has the measured cost).
// A word at or past nwords is neither read nor written, except the four tag words of open's source row.
#pragma once
#include "jj_chacha20.h"

namespace jj {

// A row's dwords, one at a time.  On the device each is a relaxed atomic of wavefront scope: the instruction is the plain global_load_dword /
// global_store_dword (no cache bits, no wait), but the compiler does not fuse neighbours into the 8-, 12- and 16-byte accesses that a row on a
// multiple of 4 is not aligned for.
static JJ_DEV u32 row_ld(const u32* p) {
#ifdef JJ_HOST_EMU
  return *p;
#else
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
#endif
}
static JJ_DEV void row_st(u32* p, u32 v) {
#ifdef JJ_HOST_EMU
  *p = v;
#else
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
#endif
}
// x, with its history hidden from the compiler: a mask made from a secret stays a mask (and / or), it is not turned back into the compare and
// the select it came from
static JJ_DEV u32 opaque(u32 x) {
#ifndef JJ_HOST_EMU
  asm volatile("" : "+v"(x));
#endif
  return x;
}

struct Poly1305 {
  static constexpr u32 M26 = 0x3ffffffu;
  u32 r0, r1, r2, r3, r4, s1, s2, s3, s4;     // r clamped, s_i = 5 r_i
  u32 h0, h1, h2, h3, h4;                     // the accumulator
  u32 pad[4];                                 // s of the one-time key

  // the one-time key: r in k[0..3], s in k[4..7] (little-endian dwords)
  JJ_DEV void init(u32 k0, u32 k1, u32 k2, u32 k3, u32 k4, u32 k5, u32 k6, u32 k7) {
    r0 = k0 & 0x3ffffffu;
    r1 = ((k0 >> 26) | (k1 << 6)) & 0x3ffff03u;
    r2 = ((k1 >> 20) | (k2 << 12)) & 0x3ffc0ffu;
    r3 = ((k2 >> 14) | (k3 << 18)) & 0x3f03fffu;
    r4 = (k3 >> 8) & 0x00fffffu;
    s1 = r1 * 5; s2 = r2 * 5; s3 = r3 * 5; s4 = r4 * 5;
    h0 = h1 = h2 = h3 = h4 = 0;
    pad[0] = k4; pad[1] = k5; pad[2] = k6; pad[3] = k7;
  }
  static JJ_DEV u64 mad(u32 a, u32 b, u64 c) { return (u64)a * b + c; }
  // h <- (h + block) r mod 2^130 - 5, partially reduced; the block is w0..w3 (little-endian dwords) plus hibit * 2^128
  JJ_DEV void absorb(u32 w0, u32 w1, u32 w2, u32 w3, u32 hibit) {
    const u32 a0 = h0 + (w0 & M26);
    const u32 a1 = h1 + (((w0 >> 26) | (w1 << 6)) & M26);
    const u32 a2 = h2 + (((w1 >> 20) | (w2 << 12)) & M26);
    const u32 a3 = h3 + (((w2 >> 14) | (w3 << 18)) & M26);
    const u32 a4 = h4 + ((w3 >> 8) | (hibit << 24));
    u64 d0 = mad(a0, r0, mad(a1, s4, mad(a2, s3, mad(a3, s2, mad(a4, s1, 0)))));
    u64 d1 = mad(a0, r1, mad(a1, r0, mad(a2, s4, mad(a3, s3, mad(a4, s2, d0 >> 26)))));
    u64 d2 = mad(a0, r2, mad(a1, r1, mad(a2, r0, mad(a3, s4, mad(a4, s3, d1 >> 26)))));
    u64 d3 = mad(a0, r3, mad(a1, r2, mad(a2, r1, mad(a3, r0, mad(a4, s4, d2 >> 26)))));
    u64 d4 = mad(a0, r4, mad(a1, r3, mad(a2, r2, mad(a3, r1, mad(a4, r0, d3 >> 26)))));
    const u64 t = mad((u32)(d4 >> 26), 5u, (u64)((u32)d0 & M26));
    h0 = (u32)t & M26;
    h1 = ((u32)d1 & M26) + (u32)(t >> 26);
    h2 = (u32)d2 & M26; h3 = (u32)d3 & M26; h4 = (u32)d4 & M26;
  }
  // tag <- ((h mod 2^130 - 5) + s) mod 2^128
  JJ_DEV void finish(u32 (&tag)[4]) const {
    u32 c, a0 = h0, a1 = h1, a2, a3, a4;
    c = a1 >> 26; a1 &= M26;
    a2 = h2 + c; c = a2 >> 26; a2 &= M26;
    a3 = h3 + c; c = a3 >> 26; a3 &= M26;
    a4 = h4 + c; c = a4 >> 26; a4 &= M26;
    a0 += c * 5; c = a0 >> 26; a0 &= M26;
    a1 += c;
    u32 g0 = a0 + 5; c = g0 >> 26; g0 &= M26;
    u32 g1 = a1 + c; c = g1 >> 26; g1 &= M26;
    u32 g2 = a2 + c; c = g2 >> 26; g2 &= M26;
    u32 g3 = a3 + c; c = g3 >> 26; g3 &= M26;
    const u32 g4 = a4 + c;
    const u32 take = opaque(0u - (g4 >> 26));   // all ones where h >= p
    a0 = (a0 & ~take) | (g0 & take); a1 = (a1 & ~take) | (g1 & take); a2 = (a2 & ~take) | (g2 & take); a3 = (a3 & ~take) | (g3 & take);
    a4 = (a4 & ~take) | (g4 & M26 & take);
    const u32 v0 = a0 | (a1 << 26), v1 = (a1 >> 6) | (a2 << 20), v2 = (a2 >> 12) | (a3 << 14), v3 = (a3 >> 18) | (a4 << 8);
#ifdef JJ_HOST_EMU
    u64 f = (u64)v0 + pad[0]; tag[0] = (u32)f;
    f = (u64)v1 + pad[1] + (f >> 32); tag[1] = (u32)f;
    f = (u64)v2 + pad[2] + (f >> 32); tag[2] = (u32)f;
    f = (u64)v3 + pad[3] + (f >> 32); tag[3] = (u32)f;
#else
    u32 cy;                                      // one add and three add-with-carry: the carry stays in the carry bit
    tag[0] = __builtin_addc(v0, pad[0], 0u, &cy);
    tag[1] = __builtin_addc(v1, pad[1], cy, &cy);
    tag[2] = __builtin_addc(v2, pad[2], cy, &cy);
    tag[3] = __builtin_addc(v3, pad[3], cy, &cy);
#endif
  }
  // tag <- Poly1305(key; the nwords dwords at src): whole blocks, then a last block of 1..3 words with the 0x01 byte behind the data.  The
  // absorb is written once; the predicates are on nwords alone.
  static JJ_DEV void mac_row(u32 (&tag)[4], const u32* src, u32 nwords, const u32 (&key)[8]) {
    Poly1305 p;
    p.init(key[0], key[1], key[2], key[3], key[4], key[5], key[6], key[7]);
    #pragma unroll 1
    for (u32 w0 = 0; w0 < nwords; w0 += 4) {
      const u32 rem = nwords - w0;
      u32 w[4];
      if (rem >= 4) {
        _Pragma("unroll") for (int j = 0; j < 4; j++) w[j] = row_ld(src + w0 + j);
      } else {
        w[0] = row_ld(src + w0);
        w[1] = rem > 1 ? row_ld(src + w0 + 1) : 1u;
        w[2] = rem > 2 ? row_ld(src + w0 + 2) : (rem == 2 ? 1u : 0u);
        w[3] = rem == 3 ? 1u : 0u;
      }
      p.absorb(w[0], w[1], w[2], w[3], rem >= 4 ? 1u : 0u);
    }
    p.finish(tag);
  }
};

struct AeadAad { u32 w[16]; };              // the aad, zero-padded to 64 bytes: the same in every lane, a kernel argument

struct Aead {
  // SEAL: dst[0 .. nwords) = src ^ keystream from block 1, dst[nwords .. nwords + 4) = the tag.  Returns 1.
  // open: src[nwords .. nwords + 4) is the tag; dst[0 .. nwords) = (src ^ keystream) & (0 - ok).  Returns ok (0 or 1).
  template <bool SEAL>
  static JJ_DEV u32 row(const u32* src, u32* dst, u32 nwords, const u32 (&key)[8], const u32 (&nonce)[3], const AeadAad& aad, u32 aad_len) {
    u32 x[16];
    ChaCha20::block(x, key, 0, nonce);
    Poly1305 mac;
    mac.init(x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7]);
    const u32 csteps = (nwords + 15) >> 4;
    #pragma unroll 1
    for (u32 st = 0; st < csteps + 2; st++) {
      u32 m[16], nb;
      if (st == 0) {
        _Pragma("unroll") for (int j = 0; j < 16; j++) m[j] = aad.w[j];
        nb = (aad_len + 15) >> 4;
      } else if (st <= csteps) {
        const u32 w0 = (st - 1) << 4, rem = nwords - w0;
        if (rem >= 16) {
          _Pragma("unroll") for (int j = 0; j < 16; j++) m[j] = row_ld(src + w0 + j);
        } else {
          _Pragma("unroll") for (int j = 0; j < 16; j++) m[j] = 0;
          _Pragma("unroll") for (int j = 0; j < 15; j++) if (j < rem) m[j] = row_ld(src + w0 + j);
        }
        if constexpr (SEAL) {
          ChaCha20::block(x, key, st, nonce);
          if (rem >= 16) {
            _Pragma("unroll") for (int j = 0; j < 16; j++) { m[j] ^= x[j]; row_st(dst + w0 + j, m[j]); }
          } else {
            _Pragma("unroll") for (int j = 0; j < 15; j++) if (j < rem) { m[j] ^= x[j]; row_st(dst + w0 + j, m[j]); }
          }
        }
        nb = rem >= 16 ? 4u : (rem + 3) >> 2;
      } else {
        _Pragma("unroll") for (int j = 0; j < 16; j++) m[j] = 0;
        m[0] = aad_len; m[2] = nwords << 2;
        nb = 1;
      }
      _Pragma("unroll") for (int q = 0; q < 4; q++) if ((u32)q < nb) mac.absorb(m[4 * q], m[4 * q + 1], m[4 * q + 2], m[4 * q + 3], 1u);
    }
    u32 tag[4];
    mac.finish(tag);
    if constexpr (SEAL) {
      _Pragma("unroll") for (int j = 0; j < 4; j++) row_st(dst + nwords + j, tag[j]);
      return 1u;
    } else {
      const u32 diff = (tag[0] ^ row_ld(src + nwords)) | (tag[1] ^ row_ld(src + nwords + 1)) | (tag[2] ^ row_ld(src + nwords + 2)) | (tag[3] ^ row_ld(src + nwords + 3));
      const u32 okm = opaque(((diff | opaque(0u - diff)) >> 31) - 1u);          // all ones where the four words agree
      u32 counter = 1;
      #pragma unroll 1
      for (u32 w0 = 0; w0 < nwords; w0 += 16, counter++) {
        // the loads first: they are in flight while the block is computed, and no store of this row stands between them (dst may alias src
        // for all the compiler knows, so a load behind a store would wait for it)
        u32 m[16];
        if (nwords - w0 >= 16) {
          _Pragma("unroll") for (int j = 0; j < 16; j++) m[j] = row_ld(src + w0 + j);
        } else {
          _Pragma("unroll") for (int j = 0; j < 16; j++) m[j] = 0;
          _Pragma("unroll") for (int j = 0; j < 15; j++) if (w0 + j < nwords) m[j] = row_ld(src + w0 + j);
        }
        ChaCha20::block(x, key, counter, nonce);
        if (nwords - w0 >= 16) {
          _Pragma("unroll") for (int j = 0; j < 16; j++) row_st(dst + w0 + j, (m[j] ^ x[j]) & okm);
        } else {
          _Pragma("unroll") for (int j = 0; j < 15; j++) if (w0 + j < nwords) row_st(dst + w0 + j, (m[j] ^ x[j]) & okm);
        }
      }
      return okm & 1u;
    }
  }
};

}  // namespace jj
