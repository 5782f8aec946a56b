// BLAKE2b (RFC 7693; BLAKE2b-512 unless told otherwise), one message per lane: the compression function and a streaming "absorb up to three parts, finish" routine -- device
// code, everything in registers.  Unkeyed, 64-byte digest, zero salt, a 16-byte personalisation: parameter block word 0 = 0x01010040 xored into
// h[0], the personalisation into h[6] and h[7]; t counts bytes in its low 64-bit word only (t1 = 0: inputs stay far below 2^64 bytes); f0 is set
// on the last block, and the last block of an empty input is one zero block with t = 0.
// Included by jj_kernels.h (k_sig_challenge, jj_sig_challenge; k_ka_kdf, jj_ka_kdf, jj_ka_kdf_each; k_blake2b, jj_blake2b: Blake2bRows at the
// end of this file), by jj_abi.hip for that host midstate, and, with -DJJ_HOST_EMU, by tests/cpp/emu_blake2b.cpp, tests/cpp/emu_ka.cpp and
// tests/cpp/emu_blake2b_rows.cpp.
// The digest length is a compile-time parameter (Blake2bT<DIGEST>, 1..64 bytes; Blake2b = Blake2bT<64>): it enters the parameter word only --
// BLAKE2b-256 is another hash than BLAKE2b-512 cut short -- and the first DIGEST bytes of h are the digest.  hash_parts is the one-compression
// form jj_ka_kdf uses: one or two 32-byte parts and nothing else.
//
// Number format: uint64_t for the state, the message words, the additions and the xors; hipcc lowers a 64-bit add to v_add_co_u32 +
// v_addc_co_u32 and an xor to two v_xor_b32, which is what code on explicit register pairs would be.  The rotations are NOT left to the 64-bit
// form -- (x >> n) | (x << (64 - n)) becomes two 64-bit shifts and an or -- but written on the two halves: 24 and 16 and 63 are two
// v_alignbit_b32 each, 32 is a register rename.  Per G: 12 add / add-with-carry, 8 xor, 6 alignbit; 96 G per compression.
// The message schedule is resolved at compile time (round<R> reads m[SIGMA[R % 10][k]] with constant indices), so v, m and h never leave the
// registers: a run-time-indexed m[] would send the 16 message words to scratch (tests/test_codegen_sig_challenge.py pins scratch = 0).
//
// Streaming: the hashed string is  part0 (32 bytes) || part1 (32 bytes) || message, the parts optional and their NUMBER a template argument, so
// that every index into m[] is a constant: block 0 starts with PARTS * 4 words of the parts, and message word j of a block is always the same
// m[k].  The message is `len` bytes at msgs + pos and may start at ANY byte address; it is read as aligned dwords through a funnel shift
// (v_alignbit_b32 by 8 * (address mod 4)).  Only dwords that hold at least one byte of the message are read: the index of every load is clamped
// to the message's last dword, a lane whose message has ended (or is empty) loads nothing, and the bytes of the boundary dwords that lie
// outside the message are masked to zero before they reach m[].  `msgs` must be 4-byte aligned (the entry point asks 16 of a device pointer).
// In a wave whose lanes hold messages of different lengths the block loop runs while any lane has blocks left; the lanes that are done are
// masked by the loop's own exit condition and neither compress nor load.
#pragma once
#include "jj_field.h"

namespace jj {

template <int DIGEST = 64>
struct Blake2bT {
  static_assert(DIGEST >= 1 && DIGEST <= 64, "BLAKE2b digest length");
  static constexpr u64 IV[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull,
                                0x510e527fade682d1ull, 0x9b05688c2b3e6c1full, 0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
  static constexpr uint8_t SIGMA[10][16] = {
      {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
      {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
      {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
      {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
      {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0}};
  static constexpr u32 PARAM0 = 0x01010000u | (u32)DIGEST;      // digest length (0x01010040 for 64, 0x01010020 for 32), key length 0, fanout 1, depth 1

  // (hi : lo) >> sh for sh in [0, 32): v_alignbit_b32
  static JJ_DEV u32 funnel(u32 hi, u32 lo, u32 sh) {
#ifdef JJ_HOST_EMU
    return (u32)(((((u64)hi) << 32) | lo) >> (sh & 31u));
#else
    return __builtin_amdgcn_alignbit(hi, lo, sh);
#endif
  }
  static JJ_DEV u64 pair(u32 lo, u32 hi) { return ((u64)hi << 32) | lo; }
  // rotate right by N on the halves: two alignbits, or a rename for 32
  template <int N>
  static JJ_DEV u64 rotr(u64 x) {
    const u32 lo = (u32)x, hi = (u32)(x >> 32);
    if constexpr (N == 32) return pair(hi, lo);
    else if constexpr (N < 32) return pair(funnel(hi, lo, N), funnel(lo, hi, N));
    else return pair(funnel(lo, hi, N - 32), funnel(hi, lo, N - 32));
  }
  static JJ_DEV void g(u64& a, u64& b, u64& c, u64& d, u64 x, u64 y) {
    a = a + b + x; d = rotr<32>(d ^ a);
    c = c + d;     b = rotr<24>(b ^ c);
    a = a + b + y; d = rotr<16>(d ^ a);
    c = c + d;     b = rotr<63>(b ^ c);
  }
  template <int R>
  static JJ_DEV void round(u64 (&v)[16], const u64 (&m)[16]) {
    constexpr int s = R % 10;
    constexpr int s0 = SIGMA[s][0], s1 = SIGMA[s][1], s2 = SIGMA[s][2], s3 = SIGMA[s][3], s4 = SIGMA[s][4], s5 = SIGMA[s][5], s6 = SIGMA[s][6], s7 = SIGMA[s][7];
    constexpr int s8 = SIGMA[s][8], s9 = SIGMA[s][9], s10 = SIGMA[s][10], s11 = SIGMA[s][11], s12 = SIGMA[s][12], s13 = SIGMA[s][13], s14 = SIGMA[s][14], s15 = SIGMA[s][15];
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
  static JJ_DEV void compress(u64 (&h)[8], const u64 (&m)[16], u64 t, bool last) {
    u64 v[16];
    _Pragma("unroll") for (int i = 0; i < 8; i++) { v[i] = h[i]; v[8 + i] = IV[i]; }
    v[12] ^= t;
    v[14] ^= last ? ~(u64)0 : (u64)0;
    round<0>(v, m); round<1>(v, m); round<2>(v, m); round<3>(v, m); round<4>(v, m); round<5>(v, m);
    round<6>(v, m); round<7>(v, m); round<8>(v, m); round<9>(v, m); round<10>(v, m); round<11>(v, m);
    _Pragma("unroll") for (int i = 0; i < 8; i++) h[i] ^= v[i] ^ v[8 + i];
  }
  // h of an unkeyed DIGEST-byte digest with the 16 bytes of personalisation given as two little-endian words
  static JJ_DEV void init(u64 (&h)[8], u64 personal_lo, u64 personal_hi) {
    _Pragma("unroll") for (int i = 0; i < 8; i++) h[i] = IV[i];
    h[0] ^= PARAM0; h[6] ^= personal_lo; h[7] ^= personal_hi;
  }

  // all ones for x >= 4, the low x bytes for x in 1..3, nothing for x <= 0
  static JJ_DEV u32 byte_mask(i32 x) {
    const u32 c = (u32)(x < 0 ? 0 : x > 4 ? 4 : x);
    return c >= 4u ? ~0u : ((1u << (8u * c)) - 1u);
  }
  // m[K0 .. 15] <- the `take` (<= 8 * (16 - K0)) bytes at msgs + pos, zero-padded.  take = 0 reads nothing.
  template <int K0>
  static JJ_DEV void fill(u64 (&m)[16], const uint8_t* msgs, u32 pos, u32 take) {
    constexpr int NW = 16 - K0;                  // 64-bit words to fill
    if (take == 0) { _Pragma("unroll") for (int k = K0; k < 16; k++) m[k] = 0; return; }
    const u32 sh = 8u * (pos & 3u);
    const u32 first = pos & ~3u, lastd = (pos + take - 1u) & ~3u;      // byte offsets of the message's first and last dword in this block
    u32 d[2 * NW + 1];
    _Pragma("unroll") for (int q = 0; q <= 2 * NW; q++) {
      // (first + 4 q cannot wrap: the dwords up to lastd exist, and beyond it the offset is clamped before the add can matter -- the clamp
      // compares distances from `first`, not absolute offsets)
      const u32 dist = 4u * (u32)q, maxd = lastd - first;
      d[q] = *reinterpret_cast<const u32*>(msgs + (size_t)(first + (dist < maxd ? dist : maxd)));
    }
    u32 w[2 * NW];
    _Pragma("unroll") for (int q = 0; q < 2 * NW; q++) w[q] = funnel(d[q + 1], d[q], sh);
    if (take != 8u * NW) {                       // a partial block: the bytes past the message read as zero
      _Pragma("unroll") for (int q = 0; q < 2 * NW; q++) w[q] &= byte_mask((i32)take - 4 * q);
    }
    _Pragma("unroll") for (int k = 0; k < NW; k++) m[K0 + k] = pair(w[2 * k], w[2 * k + 1]);
  }
  static JJ_DEV void words32(u64 (&m)[16], int k, const u32 (&w)[8]) {
    m[k] = pair(w[0], w[1]); m[k + 1] = pair(w[2], w[3]); m[k + 2] = pair(w[4], w[5]); m[k + 3] = pair(w[6], w[7]);
  }

  // digest <- BLAKE2b-512(personal; part0 || part1 || the len bytes at msgs + pos) as 16 little-endian 32-bit words.
  // PARTS = 0: no part; 1: part0 only; 2: both.  pos is a 32-bit byte offset: the entry point bounds the bytes of a call by 2^32.
  template <int PARTS>
  static JJ_DEV void hash(u32 (&lo)[8], u32 (&hi)[8], u64 personal_lo, u64 personal_hi, const u32 (&part0)[8], const u32 (&part1)[8], const uint8_t* msgs, u32 pos, u64 len) {
    constexpr int K0 = 4 * PARTS;
    constexpr u32 ROOM0 = 128u - 8u * K0;
    u64 h[8], m[16];
    init(h, personal_lo, personal_hi);
    if constexpr (PARTS >= 1) words32(m, 0, part0);
    if constexpr (PARTS >= 2) words32(m, 4, part1);
    u32 take = len < ROOM0 ? (u32)len : ROOM0;
    fill<K0>(m, msgs, pos, take);
    pos += take; len -= take;
    u64 t = 8u * K0 + take;
    compress(h, m, t, len == 0);
    while (len != 0) {
      take = len < 128u ? (u32)len : 128u;
      fill<0>(m, msgs, pos, take);
      pos += take; len -= take; t += take;
      compress(h, m, t, len == 0);
    }
    _Pragma("unroll") for (int i = 0; i < 4; i++) { lo[2 * i] = (u32)h[i]; lo[2 * i + 1] = (u32)(h[i] >> 32); hi[2 * i] = (u32)h[4 + i]; hi[2 * i + 1] = (u32)(h[4 + i] >> 32); }
  }

  // out <- the first 32 bytes of h after ONE compression over part0 (PARTS = 1: 32 bytes hashed) or part0 || part1 (PARTS = 2: 64 bytes): the
  // whole digest when DIGEST = 32.  Straight-line code: no load, no branch, nothing indexed at run time.
  template <int PARTS>
  static JJ_DEV void hash_parts(u32 (&out)[8], u64 personal_lo, u64 personal_hi, const u32 (&part0)[8], const u32 (&part1)[8]) {
    static_assert(PARTS == 1 || PARTS == 2, "one or two 32-byte parts");
    u64 h[8], m[16];
    init(h, personal_lo, personal_hi);
    words32(m, 0, part0);
    if constexpr (PARTS == 2) words32(m, 4, part1);
    _Pragma("unroll") for (int k = 4 * PARTS; k < 16; k++) m[k] = 0;
    compress(h, m, 32u * PARTS, true);
    _Pragma("unroll") for (int i = 0; i < 4; i++) { out[2 * i] = (u32)h[i]; out[2 * i + 1] = (u32)(h[i] >> 32); }
  }
};
typedef Blake2bT<64> Blake2b;

// ---- rows gathered from several arrays (jj_blake2b, k_blake2b; with -DJJ_HOST_EMU tests/cpp/emu_blake2b_rows.cpp): the hashed string of row i
// is  prefix || piece_0[i] || .. || piece_{np-1}[i].  The prefix is the same in every lane, so the host compresses its whole blocks once
// (midstate: B = min(prefix_len / 128, (prefix_len + rest - 1) / 128) blocks, never a block that could be the final one) and the kernel gets
// h, t0 = 128 B and the prefix's tail -- 0..128 bytes, zero-padded to 32 dwords -- as arguments: scalar registers.  A piece is `nd` dwords at
// byte `off` of a row of source `src`; every length is a multiple of 4 and the same in every lane, so dword j of block b is EITHER a word of
// the tail OR one aligned dword of one piece, the same piece in every lane: no funnel shift, no mask, and the block loop, the piece
// boundaries and the final-block flag are uniform.  Every index into m[] is a compile-time constant (the 32 dwords of a block are an unrolled
// loop; which piece serves dword j is a chain of uniform compares that selects one of four per-lane addresses): a run-time-indexed m[] would
// go to scratch.  A dword that lies past the hashed string is not loaded at all.  Nothing in the instruction stream or in an address depends
// on the data: the prefix may be a secret.
constexpr int B2B_MAX_PIECES = 4;
struct B2bMid { u64 h[8]; u64 t0; u32 tail[32]; u32 tail_len; };
struct B2bPlan { u32 npieces; u32 src[B2B_MAX_PIECES], off[B2B_MAX_PIECES], nd[B2B_MAX_PIECES]; };     // unused pieces: nd = 0

template <int DIGEST>
struct Blake2bRows {
  static_assert(DIGEST == 32 || DIGEST == 64, "jj_blake2b: digests of 32 or 64 bytes");
  typedef Blake2bT<DIGEST> H;
  static constexpr u32 BLOCK = 128;

  // ---- the host's part: plain C++ (the device's compression is device code; this one never sees a final block)
  static inline u64 le64(const uint8_t* p) { u64 x = 0; for (int i = 7; i >= 0; i--) x = (x << 8) | p[i]; return x; }
  static inline u64 host_rotr(u64 x, int r) { return (x >> r) | (x << (64 - r)); }
  static inline void host_compress(u64 (&h)[8], const u64 (&m)[16], u64 t) {
    u64 v[16];
    for (int i = 0; i < 8; i++) { v[i] = h[i]; v[8 + i] = H::IV[i]; }
    v[12] ^= t;
    static const uint8_t LANES[8][4] = {{0, 4, 8, 12}, {1, 5, 9, 13}, {2, 6, 10, 14}, {3, 7, 11, 15}, {0, 5, 10, 15}, {1, 6, 11, 12}, {2, 7, 8, 13}, {3, 4, 9, 14}};
    for (int r = 0; r < 12; r++)
      for (int q = 0; q < 8; q++) {
        u64 &a = v[LANES[q][0]], &b = v[LANES[q][1]], &c = v[LANES[q][2]], &d = v[LANES[q][3]];
        a = a + b + m[H::SIGMA[r % 10][2 * q]];     d = host_rotr(d ^ a, 32);
        c = c + d;                                  b = host_rotr(b ^ c, 24);
        a = a + b + m[H::SIGMA[r % 10][2 * q + 1]]; d = host_rotr(d ^ a, 16);
        c = c + d;                                  b = host_rotr(b ^ c, 63);
      }
    for (int i = 0; i < 8; i++) h[i] ^= v[i] ^ v[8 + i];
  }
  // Number of whole prefix blocks the host absorbs; `rest` = the bytes every row adds behind the prefix
  static inline size_t midstate_blocks(size_t prefix_len, size_t rest) {
    if (prefix_len + rest == 0) return 0;
    const size_t a = prefix_len / BLOCK, b = (prefix_len + rest - 1) / BLOCK;
    return a < b ? a : b;
  }
  // mid <- the state behind those blocks, t0, and the prefix's remaining bytes (0..128) zero-padded.  personal16 == nullptr: sixteen zero bytes.
  static inline void midstate(B2bMid& mid, const uint8_t* personal16, const uint8_t* prefix, size_t prefix_len, size_t rest) {
    const size_t blocks = midstate_blocks(prefix_len, rest);
    for (int i = 0; i < 8; i++) mid.h[i] = H::IV[i];
    mid.h[0] ^= H::PARAM0;
    if (personal16) { mid.h[6] ^= le64(personal16); mid.h[7] ^= le64(personal16 + 8); }
    u64 m[16];
    for (size_t k = 0; k < blocks; k++) {
      for (int j = 0; j < 16; j++) m[j] = le64(prefix + BLOCK * k + 8 * j);
      host_compress(mid.h, m, (u64)BLOCK * (k + 1));
    }
    uint8_t pad[BLOCK] = {0};
    for (size_t j = BLOCK * blocks; j < prefix_len; j++) pad[j - BLOCK * blocks] = prefix[j];
    for (int j = 0; j < 32; j++) mid.tail[j] = (u32)pad[4 * j] | ((u32)pad[4 * j + 1] << 8) | ((u32)pad[4 * j + 2] << 16) | ((u32)pad[4 * j + 3] << 24);
    mid.t0 = (u64)BLOCK * blocks; mid.tail_len = (u32)(prefix_len - BLOCK * blocks);
  }
  // one piece per source, in order: source s whole (lens[s] bytes from byte 0 of its rows)
  static inline void plan_sources(B2bPlan& plan, int nsrc, const size_t* lens) {
    plan.npieces = (u32)nsrc;
    for (int k = 0; k < B2B_MAX_PIECES; k++) { plan.src[k] = k < nsrc ? (u32)k : 0u; plan.off[k] = 0; plan.nd[k] = k < nsrc ? (u32)(lens[k] / 4) : 0u; }
  }

  // ---- the lane's part
  // the aligned dword at a 64-bit address of global memory (an address formed as an integer would otherwise be read with flat_load)
  static JJ_DEV u32 load_dword(u64 addr) {
#ifdef JJ_HOST_EMU
    return *reinterpret_cast<const u32*>((uintptr_t)addr);
#else
    return *(const __attribute__((address_space(1))) u32*)addr;
#endif
  }
  // out <- the digest finished from the midstate over  tail || piece_0 || .. || piece_3  as DIGEST / 4 little-endian words.  rowp[k] = the
  // address of the first byte of piece k in THIS lane's row (unused where nd[k] = 0); everything else is the same in every lane.
  static JJ_DEV void finish(u32 (&out)[DIGEST / 4], const B2bMid& mid, const B2bPlan& plan, const u64 (&rowp)[B2B_MAX_PIECES]) {
    u64 h[8], m[16];
    _Pragma("unroll") for (int i = 0; i < 8; i++) h[i] = mid.h[i];
    const u32 c1 = plan.nd[0], c2 = c1 + plan.nd[1], c3 = c2 + plan.nd[2], total = c3 + plan.nd[3];      // stream dwords in front of pieces 1, 2, 3; all
    // rowp[k] - 4 c_k: what 4 g is added to for a stream dword g of piece k (integers: the difference may lie in front of the array)
    const u64 v0 = rowp[0], v1 = rowp[1] - 4ull * c1, v2 = rowp[2] - 4ull * c2, v3 = rowp[3] - 4ull * c3;
    const u32 tail_dw = mid.tail_len / 4u;
    const u32 bytes = mid.tail_len + 4u * total;                  // behind t0: at most 128 + 4 * 65536 bytes
    const u32 nblocks = bytes ? (bytes + BLOCK - 1u) / BLOCK : 1u;
    _Pragma("unroll 1") for (u32 blk = 0; blk < nblocks; blk++) {
      u32 w[32];
      _Pragma("unroll") for (int j = 0; j < 32; j++) {
        w[j] = blk == 0 ? mid.tail[j] : 0u;
        const u32 pos = 32u * blk + (u32)j;                       // dword of  tail || pieces
        if (pos >= tail_dw && pos - tail_dw < total) {            // uniform
          const u32 g = pos - tail_dw;
          const u64 vb = g < c1 ? v0 : g < c2 ? v1 : g < c3 ? v2 : v3;
          w[j] = load_dword(vb + 4ull * g);
        }
      }
      _Pragma("unroll") for (int k = 0; k < 16; k++) m[k] = H::pair(w[2 * k], w[2 * k + 1]);
      const bool last = blk + 1u == nblocks;
      H::compress(h, m, mid.t0 + (last ? (u64)bytes : (u64)BLOCK * (blk + 1u)), last);
    }
    _Pragma("unroll") for (int i = 0; i < DIGEST / 8; i++) { out[2 * i] = (u32)h[i]; out[2 * i + 1] = (u32)(h[i] >> 32); }
  }
};

}  // namespace jj
