// Windowed Pedersen hashes (jj_pedersen_table_create, jj_pedersen_hash_vartime, jj_pedersen_scalars, jj_pedersen_commit_vartime): the table
// layout, the per-window plan of a call and the device functions that turn a unit's row into table indices.  Kernels: k_pedersen_gather,
// k_pedersen_scalars and k_pedersen_commit in jj_kernels.h.
// Included by jj_kernels.h and, with -DJJ_HOST_EMU, by tests/cpp/emu_pedersen.cpp and tests/cpp/emu_commit.cpp.
//
// The function.  A message M is `prefix_bits` bits of a call constant followed by up to four fields of the unit's row, every bit taken LSB-first
// within its byte.  M is padded with zero bits to a multiple of 3 and cut into chunks (s0, s1, s2), enc = (1 - 2 s2)(1 + s0 + 2 s1) in +-{1..4};
// segment j takes chunks j c .. j c + c - 1 (c = seg_chunks <= 63), <M_j> = sum_i enc(m_i) 16^i, H(M) = sum_j [<M_j>] P_j.  A chunk that is
// not there contributes nothing (it is NOT a zero chunk: 000 encodes +1), the empty message gives the identity.
//
// Table.  A window is w = window_chunks consecutive chunks of one segment and never straddles a segment: ceil(c / w) windows per segment, the
// last one of c - w (nw - 1) chunks.  A window that may hold up to T chunks carries sub-tables for t = 1 .. T present chunks -- the message
// length is one per call, so which sub-table the message's LAST window uses is a call constant and every other window uses its full one.
// Sub-table t has 2^(3t - 1) entries: the sign bit of the window's last present chunk is taken out of the index and applied by
// Curve::add_signed, and since negating an entry negates EVERY chunk of it, a set sign also flips the sign bits of the chunks below it:
//     raw  = the 3t message bits of the window, chunk i at bits 3i .. 3i + 2
//     neg  = bit 3t - 1 of raw
//     idx  = (raw mod 2^(3t - 1)) xor (neg ? FLIP_t : 0),  FLIP_t = the bits 2, 5, 8 below bit 3t - 3
//     entry(t, idx) = [sum_{i < t - 1} enc(idx bits 3i .. 3i + 2) 16^(i + w k) + (1 + idx_{3t-3} + 2 idx_{3t-2}) 16^(t - 1 + w k)] P_j
// Entries are GNIELS_WORDS apart (one 128-byte line, the format of k_fixedbase_gather's tables); segment j, window k, sub-table t starts at
// entry j * ped_seg_entries(c, w) + k * ped_window_entries(w) + ped_sub_offset(t).
//
// Plan.  The layout (prefix, fields) is the same for every unit of a call, so which bytes a window's bits come from, by what shift, and where a
// field ends are wave-uniform: the host cuts every window's bit range along the field boundaries into at most four pieces (the prefix's bits
// are folded into a constant) and the kernels read the plan with uniform addresses.  A piece is at most 12 bits starting at bit `shift` of byte
// `byte` of the row; a lane reads the aligned dword of that byte and the next one, joins them with a funnel shift (v_alignbit_b32) and masks.
// The second load is clamped to the last dword that holds a byte the fields cover in the lane's OWN row: the last row of the caller's array may
// end in the middle of a dword directly in front of memory that is not the caller's, and no dword beyond that one is ever read.
//
// Several sources (jj_pedersen_commit_vartime).  The message's fields may lie in up to four row arrays, each with its own stride; a field is a
// triple (src, byte_offset, nbits).  The plan of such a call is a PedWinSrc per window: the PedWin of the same message plus the source of every
// piece.  A lane forms pos and the clamp dword from the source's OWN stride and cover, so the rule above holds for every source separately.
#pragma once
#include "jj_blake2b.h"      // Blake2b::funnel
#include <string.h>
#include <algorithm>
#include <vector>

namespace jj {

constexpr int PED_DEFAULT_WINDOW = 4;      // what window_chunks = 0 means
constexpr int PED_MAX_SEG = 8, PED_MAX_CHUNKS = 63, PED_MAX_WINDOW = 4, PED_MAX_FIELDS = 4, PED_MAX_PIECES = 4, PED_MAX_SRC = 4;

struct PedPiece { u32 byte, shift, mask, dst; };      // bits [shift, shift + popcount(mask)) from byte `byte` of the row, placed at bit `dst` of raw
struct PedWin {
  u32 entry0;        // first entry of the window's sub-table for `t` chunks
  u32 konst;         // the prefix's bits of this window, in place
  u32 t;             // chunks present: 1 .. window_chunks
  u32 np;            // pieces in use
  u32 top;           // 3t - 1: the sign bit
  u32 flip;          // FLIP_t
  u32 seg, chunk0;   // the segment, and the position in it of the window's first chunk (a multiple of window_chunks)
  PedPiece pc[PED_MAX_PIECES];
};
struct PedSegs { int first[PED_MAX_SEG + 1]; };       // segment j owns windows first[j] .. first[j + 1] - 1 of the plan
struct PedWinSrc : PedWin { u32 src[PED_MAX_PIECES]; };                                   // src[p]: the source that piece p reads
struct PedSrcs { const uint8_t* rows[PED_MAX_SRC]; u32 stride[PED_MAX_SRC], cover[PED_MAX_SRC]; };      // a call's row arrays (4-byte aligned bases), their strides and covered bytes per row

// ---- layout arithmetic, host and device
constexpr u32 ped_sub_entries(int t) { return 1u << (3 * t - 1); }
constexpr u32 ped_sub_offset(int t) { return t <= 1 ? 0u : ped_sub_offset(t - 1) + ped_sub_entries(t - 1); }      // 0, 4, 36, 292
constexpr u32 ped_window_entries(int T) { return ped_sub_offset(T + 1); }                                            // 4, 36, 292, 2340
constexpr int ped_windows(int c, int w) { return (c + w - 1) / w; }
constexpr u32 ped_seg_entries(int c, int w) { return (u32)(ped_windows(c, w) - 1) * ped_window_entries(w) + ped_window_entries(c - (ped_windows(c, w) - 1) * w); }
constexpr u32 ped_flip(int t) { return 0x124u & ((1u << (3 * t - 3)) - 1u); }

struct Pedersen {
  // the bits of one piece, in place.  pos: byte offset of the unit's row in `rows` (4-byte aligned base); lastd: byte offset of the last dword
  // that holds a covered byte of this row
  static JJ_DEV u32 piece(const uint8_t* rows, u32 pos, u32 lastd, const PedPiece& p) {
    const u32 a = pos + p.byte, d0 = a & ~3u, d1 = d0 < lastd ? d0 + 4u : lastd;
    const u32 lo = *reinterpret_cast<const u32*>(rows + (size_t)d0), hi = *reinterpret_cast<const u32*>(rows + (size_t)d1);
    return (Blake2b::funnel(hi, lo, 8u * (a & 3u) + p.shift) & p.mask) << p.dst;
  }
  // the 3t message bits of a window
  static JJ_DEV u32 raw_bits(const uint8_t* rows, u32 pos, u32 lastd, const PedWin& w) {
    u32 raw = w.konst;
    for (u32 p = 0; p < w.np; p++) raw |= piece(rows, pos, lastd, w.pc[p]);
    return raw;
  }
  // raw -> entry number in the table and the mask add_signed takes
  static JJ_DEV u32 index(const PedWin& w, u32 raw, u32& negmask) {
    negmask = 0u - ((raw >> w.top) & 1u);
    return w.entry0 + ((raw & ((1u << w.top) - 1u)) ^ (negmask & w.flip));
  }
  static JJ_DEV u32 last_dword(u32 pos, u32 cover) { return (pos + cover - 1u) & ~3u; }
  // element s of a four-entry array by compares: s is wave-uniform, and an indexed read of a kernel argument would park the array in scratch
  template <class T> static JJ_DEV T pick(const T (&a)[PED_MAX_SRC], u32 s) {
    T r = a[0];
    _Pragma("unroll") for (u32 q = 1; q < (u32)PED_MAX_SRC; q++) r = s == q ? a[q] : r;
    return r;
  }
  // raw_bits over several sources: pos and the clamp dword of unit `unit` are formed per piece from the piece's own source
  static JJ_DEV u32 raw_bits_src(const PedSrcs& S, u32 unit, const PedWinSrc& w) {
    u32 raw = w.konst;
    for (u32 p = 0; p < w.np; p++) {
      const u32 s = w.src[p], pos = unit * pick(S.stride, s);
      raw |= piece(pick(S.rows, s), pos, last_dword(pos, pick(S.cover, s)), w.pc[p]);
    }
    return raw;
  }
};

// ---- the plan of one call (host).  fields: nfields pairs (byte_offset, nbits), checked by the caller.  Returns the windows the message
// reaches, in message order; segs->first gets the window ranges of the segments (empty for a segment the message does not reach) and *cover
// the bytes of a row the fields cover (0 without fields).
inline std::vector<PedWin> ped_build_plan(int nseg, int c, int w, u32 prefix, int prefix_bits, int nfields, const uint32_t* fields, PedSegs* segs, u32* cover) {
  u32 start[PED_MAX_FIELDS + 1];
  u32 L = (u32)prefix_bits; u64 cov = 0;
  for (int f = 0; f < nfields; f++) {
    start[f] = L; L += fields[2 * f + 1];
    const u64 end = (u64)fields[2 * f] + ((u64)fields[2 * f + 1] + 7u) / 8u;      // up to 2^32: a 32-bit sum would wrap
    if (end > cov) cov = end;
  }
  start[nfields] = L;
  // cover travels as 32 bits.  A cover of exactly 2^32 (row_stride = 2^32, so n = 1 and pos = 0) becomes 0, and last_dword(0, 0) =
  // (0 - 1) & ~3 = 2^32 - 4 is the dword of the row's byte 2^32 - 1: the arithmetic is modulo 2^32 throughout and only the sum pos + cover - 1,
  // which is below 2^32 for every row, is used.  Without fields no piece exists and lastd is never looked at.
  *cover = (u32)cov;
  const u32 chunks = (L + 2u) / 3u, seg_e = ped_seg_entries(c, w);
  std::vector<PedWin> plan;
  for (int j = 0; j <= PED_MAX_SEG; j++) segs->first[j] = 0;
  for (int j = 0; j < nseg; j++) {
    segs->first[j] = (int)plan.size();
    for (int k = 0; k < ped_windows(c, w); k++) {
      const u32 c0 = (u32)j * c + (u32)k * w;                       // first chunk of the window, in message chunks
      if (c0 >= chunks) break;
      const int T = std::min(w, c - k * w);
      PedWin x; memset(&x, 0, sizeof x);
      x.t = std::min<u32>((u32)T, chunks - c0);
      x.entry0 = (u32)j * seg_e + (u32)k * ped_window_entries(w) + ped_sub_offset((int)x.t);
      x.top = 3 * x.t - 1; x.flip = ped_flip((int)x.t); x.seg = (u32)j; x.chunk0 = (u32)k * w;
      const u32 b0 = 3 * c0, b1 = std::min(b0 + 3 * x.t, L);       // beyond L: the padding's zero bits
      if (b0 < (u32)prefix_bits) {
        const u32 hi = std::min(b1, (u32)prefix_bits);
        x.konst = (u32)(((uint64_t)prefix >> b0) & ((1ull << (hi - b0)) - 1ull));
      }
      for (int f = 0; f < nfields; f++) {
        const u32 lo = std::max(b0, start[f]), hi = std::min(b1, start[f + 1]);
        if (lo >= hi) continue;
        // the piece's first bit within the field.  byte_offset + rel / 8 < 2^32 since the field ends inside row_stride <= 2^32; the bit number
        // 8 * byte_offset + rel would not fit 32 bits from byte_offset = 2^29 on
        const u32 rel = lo - start[f];
        x.pc[x.np++] = PedPiece{fields[2 * f] + (rel >> 3), rel & 7u, (1u << (hi - lo)) - 1u, lo - b0};

      }
      plan.push_back(x);
    }
    segs->first[j + 1] = (int)plan.size();
  }
  for (int j = nseg; j < PED_MAX_SEG; j++) segs->first[j + 1] = (int)plan.size();
  return plan;
}
// The plan of a call over several sources.  fields: nfields triples (src, byte_offset, nbits), checked by the caller.  The windows are those of
// ped_build_plan over the pairs (byte_offset, nbits); a window's pieces come in field order, one for every field that meets the window's bits,
// which is how their sources are found again here.  cover[s]: the bytes of a row of source s that its fields cover (0 for an unused source).
inline std::vector<PedWinSrc> ped_build_plan_src(int nseg, int c, int w, u32 prefix, int prefix_bits, int nfields, const uint32_t* fields, PedSegs* segs, u32 cover[PED_MAX_SRC]) {
  uint32_t pairs[2 * PED_MAX_FIELDS] = {0};
  u32 start[PED_MAX_FIELDS + 1];
  u64 cov[PED_MAX_SRC] = {0, 0, 0, 0};
  u32 L = (u32)prefix_bits;
  for (int f = 0; f < nfields; f++) {
    const u32 s = fields[3 * f], off = fields[3 * f + 1], nb = fields[3 * f + 2];
    pairs[2 * f] = off; pairs[2 * f + 1] = nb;
    start[f] = L; L += nb;
    cov[s] = std::max(cov[s], (u64)off + ((u64)nb + 7u) / 8u);
  }
  start[nfields] = L;
  for (int s = 0; s < PED_MAX_SRC; s++) cover[s] = (u32)cov[s];               // 2^32 travels as 0, as in ped_build_plan
  u32 one;
  const std::vector<PedWin> base = ped_build_plan(nseg, c, w, prefix, prefix_bits, nfields, pairs, segs, &one);
  std::vector<PedWinSrc> plan(base.size());
  for (size_t k = 0; k < base.size(); k++) {
    PedWinSrc& x = plan[k];
    memset(&x, 0, sizeof x);
    static_cast<PedWin&>(x) = base[k];
    const u32 b0 = 3u * (x.seg * (u32)c + x.chunk0), b1 = std::min(b0 + 3u * x.t, L);
    u32 p = 0;
    for (int f = 0; f < nfields; f++)
      if (std::max(b0, start[f]) < std::min(b1, start[f + 1])) x.src[p++] = fields[3 * f];
  }
  return plan;
}

}  // namespace jj
