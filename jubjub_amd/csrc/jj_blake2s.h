// BLAKE2s-256 (RFC 7693), one message per lane: the compression function, the host's midstate over a prefix that all lanes share, and "finish
// from the midstate over the prefix's tail and the lane's own message" -- device code, everything in registers.  Unkeyed, 32-byte digest, zero
// salt, an 8-byte personalisation: parameter block word 0 = 0x01010020 xored into h[0], the personalisation into h[6] and h[7]; t counts bytes
// as a 64-bit number whose high word stays 0 (a prefix of at most 4096 and a message of at most 65536 bytes); f0 is set on the last block, and
// the last block of an empty input is one zero block with t = 0.
// Included by jj_kernels.h (k_blake2s: jj_blake2s, jj_group_hash), by jj_abi.hip for the host's midstate, and, with -DJJ_HOST_EMU, by
// tests/cpp/emu_blake2s.cpp.
//
// Number format: uint32_t throughout.  Per G: 6 v_add_u32 (or 2 v_add3_u32 + 2 v_add_u32), 4 v_xor_b32, 4 rotations -- by 16, 12, 8 and 7, one
// v_alignbit_b32 (x : x) >> n each; 80 G per compression (10 rounds), 320 alignbits.  The message schedule is resolved at compile time
// (round<R> reads m[SIGMA[R][k]] with constant indices), so v, m and h never leave the registers: a run-time-indexed m[] would send the 16
// message words to scratch (tests/test_codegen_group_hash.py pins scratch = 0).
//
// The hashed string is  prefix || message.  The prefix is the same in every lane, so the host compresses its whole blocks once (midstate: B
// blocks, B = min(prefix_len / 64, (prefix_len + msg_len - 1) / 64), never a block that could be the final one) and the kernel gets the eight
// words of h, t = 64 B and the prefix's tail -- prefix_len - 64 B bytes, 0..64, zero-padded to 16 words, the same in every lane (kernel
// arguments: scalar registers).  The lane's message follows the tail at byte `tail_len` of the first block, which is any value: the message is
// `len` bytes at msgs + pos, may start at ANY byte address, and is read as aligned dwords through a funnel shift (v_alignbit_b32 by
// 8 * (address mod 4)) from a VIRTUAL start at pos - tail_len, so that word j of a block is always m[j].  Only dwords that hold at least one
// byte of the lane's own message are read: the index of every load is clamped between the message's first and last dword of the block, a block
// that takes no message byte loads nothing, and the bytes of a word that lie outside the message -- in front of it in the first block, behind
// it in the last -- are masked to zero before the word is ORed over the tail's.  `msgs` must be 4-byte aligned (the entry point asks 16 of a
// device pointer).  len, tail_len and t are the same in every lane: the block loop and the masks are uniform, only the addresses and the shift
// differ between lanes.  ONE loop holds the one inlined compression: the first block differs from the others by values (the tail's words, the
// offset of the message in the block), not by code.
#pragma once
#include "jj_field.h"

#ifdef JJ_HOST_EMU
#define JJ_B2S_FN inline
#else
#define JJ_B2S_FN __host__ __device__ __forceinline__        // the midstate runs on the host (jj_abi.hip), the rest in k_blake2s
#endif

namespace jj {

struct Blake2s {
  static constexpr u32 IV[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
  static constexpr uint8_t SIGMA[10][16] = {
      {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
      {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
      {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
      {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
      {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0}};
  static constexpr u32 PARAM0 = 0x01010020u;      // digest length 32, key length 0, fanout 1, depth 1
  static constexpr u32 BLOCK = 64;

  // (hi : lo) >> sh for sh in [0, 32): v_alignbit_b32
  static JJ_B2S_FN u32 funnel(u32 hi, u32 lo, u32 sh) {
#if defined(JJ_HOST_EMU) || !defined(__HIP_DEVICE_COMPILE__)
    return (u32)(((((u64)hi) << 32) | lo) >> (sh & 31u));
#else
    return __builtin_amdgcn_alignbit(hi, lo, sh);
#endif
  }
  template <int N>
  static JJ_B2S_FN u32 rotr(u32 x) { return funnel(x, x, N); }
  static JJ_B2S_FN void g(u32& a, u32& b, u32& c, u32& d, u32 x, u32 y) {
    a = a + b + x; d = rotr<16>(d ^ a);
    c = c + d;     b = rotr<12>(b ^ c);
    a = a + b + y; d = rotr<8>(d ^ a);
    c = c + d;     b = rotr<7>(b ^ c);
  }
  template <int R>
  static JJ_B2S_FN void round(u32 (&v)[16], const u32 (&m)[16]) {
    static_assert(R >= 0 && R < 10, "BLAKE2s has 10 rounds");
    constexpr int s0 = SIGMA[R][0], s1 = SIGMA[R][1], s2 = SIGMA[R][2], s3 = SIGMA[R][3], s4 = SIGMA[R][4], s5 = SIGMA[R][5], s6 = SIGMA[R][6], s7 = SIGMA[R][7];
    constexpr int s8 = SIGMA[R][8], s9 = SIGMA[R][9], s10 = SIGMA[R][10], s11 = SIGMA[R][11], s12 = SIGMA[R][12], s13 = SIGMA[R][13], s14 = SIGMA[R][14], s15 = SIGMA[R][15];
    g(v[0], v[4], v[8], v[12], m[s0], m[s1]);
    g(v[1], v[5], v[9], v[13], m[s2], m[s3]);
    g(v[2], v[6], v[10], v[14], m[s4], m[s5]);
    g(v[3], v[7], v[11], v[15], m[s6], m[s7]);
    g(v[0], v[5], v[10], v[15], m[s8], m[s9]);
    g(v[1], v[6], v[11], v[12], m[s10], m[s11]);
    g(v[2], v[7], v[8], v[13], m[s12], m[s13]);
    g(v[3], v[4], v[9], v[14], m[s14], m[s15]);
  }
  // F of RFC 7693 section 3.2: h <- F(h, m, t, last), t the number of bytes hashed so far including this block
  static JJ_B2S_FN void compress(u32 (&h)[8], const u32 (&m)[16], u64 t, bool last) {
    u32 v[16];
    _Pragma("unroll") for (int i = 0; i < 8; i++) { v[i] = h[i]; v[8 + i] = IV[i]; }
    v[12] ^= (u32)t; v[13] ^= (u32)(t >> 32);
    v[14] ^= last ? ~(u32)0 : (u32)0;
    round<0>(v, m); round<1>(v, m); round<2>(v, m); round<3>(v, m); round<4>(v, m);
    round<5>(v, m); round<6>(v, m); round<7>(v, m); round<8>(v, m); round<9>(v, m);
    _Pragma("unroll") for (int i = 0; i < 8; i++) h[i] ^= v[i] ^ v[8 + i];
  }
  // h of an unkeyed 32-byte digest with the 8 bytes of personalisation given as two little-endian words
  static JJ_B2S_FN void init(u32 (&h)[8], u32 personal_lo, u32 personal_hi) {
    _Pragma("unroll") for (int i = 0; i < 8; i++) h[i] = IV[i];
    h[0] ^= PARAM0; h[6] ^= personal_lo; h[7] ^= personal_hi;
  }

  // ---- the host's part: plain C++, no load through a funnel.
  // Number of whole prefix blocks the host absorbs: never one that could be the final block of prefix || message.
  static inline size_t midstate_blocks(size_t prefix_len, size_t msg_len) {
    if (prefix_len + msg_len == 0) return 0;
    const size_t a = prefix_len / BLOCK, b = (prefix_len + msg_len - 1) / BLOCK;
    return a < b ? a : b;
  }
  // h <- the state behind the first `blocks` blocks of prefix; tail <- the prefix's remaining prefix_len - 64 blocks bytes (0..64), zero-padded.
  // personal8 == nullptr: eight zero bytes.
  static inline void midstate(u32 (&h)[8], u32 (&tail)[16], const uint8_t* personal8, const uint8_t* prefix, size_t prefix_len, size_t blocks) {
    u32 pl = 0, ph = 0;
    if (personal8) { pl = le32(personal8); ph = le32(personal8 + 4); }
    init(h, pl, ph);
    u32 m[16];
    for (size_t k = 0; k < blocks; k++) {
      for (int j = 0; j < 16; j++) m[j] = le32(prefix + BLOCK * k + 4 * j);
      compress(h, m, (u64)BLOCK * (k + 1), false);
    }
    uint8_t pad[BLOCK] = {0};
    for (size_t j = BLOCK * blocks; j < prefix_len; j++) pad[j - BLOCK * blocks] = prefix[j];
    for (int j = 0; j < 16; j++) tail[j] = le32(pad + 4 * j);
  }
  static inline u32 le32(const uint8_t* p) { return (u32)p[0] | ((u32)p[1] << 8) | ((u32)p[2] << 16) | ((u32)p[3] << 24); }

  // ---- the lane's part
  // all ones for x >= 4, the low x bytes for x in 1..3, nothing for x <= 0
  static JJ_B2S_FN u32 byte_mask(i32 x) {
    const u32 c = (u32)(x < 0 ? 0 : x > 4 ? 4 : x);
    return c >= 4u ? ~0u : ((1u << (8u * c)) - 1u);
  }
  // w[j] <- word j of a block whose bytes at .. at + take - 1 are the `take` (1..64 - at) bytes at msgs + pos and whose other bytes are zero.
  // The virtual start of the block is pos - at; the arithmetic on offsets is modulo 2^32 and only differences of at most 128 are compared.
  static JJ_B2S_FN void fill(u32 (&w)[16], const uint8_t* msgs, u32 pos, u32 at, u32 take) {
    const u32 vstart = pos - at;
    const u32 sh = 8u * (vstart & 3u);
    const u32 first = pos & ~3u, lastd = (pos + take - 1u) & ~3u;      // byte offsets of the first and last dword that hold a byte of these `take`
    const i32 rel0 = (i32)((vstart & ~3u) - first);                    // where the virtual block's dword 0 lies from `first`: -64 .. 0
    const i32 maxd = (i32)(lastd - first);                             // 0 .. 64
    u32 d[17];
    _Pragma("unroll") for (int q = 0; q <= 16; q++) {
      i32 rel = rel0 + 4 * q;
      rel = rel < 0 ? 0 : rel > maxd ? maxd : rel;                     // every load inside first .. lastd
      d[q] = *reinterpret_cast<const u32*>(msgs + ((size_t)first + (size_t)(u32)rel));
    }
    _Pragma("unroll") for (int q = 0; q < 16; q++)
      w[q] = funnel(d[q + 1], d[q], sh) & byte_mask((i32)(at + take) - 4 * q) & ~byte_mask((i32)at - 4 * q);
  }

  // out <- BLAKE2s-256 finished from the midstate h (t0 = 64 B bytes absorbed) over  the tail's tail_len bytes || the len bytes at msgs + pos,
  // as 8 little-endian words.  h, tail, t0, tail_len and len are the same in every lane.
  static JJ_B2S_FN void finish(u32 (&out)[8], const u32 (&h0)[8], const u32 (&tail)[16], u32 t0, u32 tail_len, const uint8_t* msgs, u32 pos, u32 len) {
    u32 h[8], m[16];
    _Pragma("unroll") for (int i = 0; i < 8; i++) h[i] = h0[i];
    _Pragma("unroll") for (int j = 0; j < 16; j++) m[j] = tail[j];
    u64 t = t0;
    u32 at = tail_len;
    for (;;) {
      const u32 room = BLOCK - at, take = len < room ? len : room;
      if (take != 0) {
        u32 w[16];
        fill(w, msgs, pos, at, take);
        for (int j = 0; j < 16; j++) m[j] |= w[j];
      }
      pos += take; len -= take; t += at + take;
      compress(h, m, t, len == 0);
      if (len == 0) break;
      for (int j = 0; j < 16; j++) m[j] = 0;
      at = 0;
    }
    _Pragma("unroll") for (int i = 0; i < 8; i++) out[i] = h[i];
  }
};

}  // namespace jj
