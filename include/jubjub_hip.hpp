// jubjub_hip.hpp — C++17 host-side mirror of the zkcrypto/jubjub public API for the batched MI355X engine.
//
// Header-only layer above the C ABI (jubjub_hip.h).  It keeps the reference crate's names, argument meaning and
// error behaviour for the scalar-multiplication path, lifted from one element to a batch (std::vector of wire
// encodings).  The reference is Rust; no Rust toolchain exists in this image, so this C++ mirror (plus the Python
// one in jubjub_amd/) is the host side that is compiled and tested here.
//
//   reference (src/lib.rs, src/fr.rs)                          here
//   ---------------------------------------------------------  -----------------------------------------------
//   Fr / Fq   (to_bytes, from_bytes, add, sub, mul, ...)        jubjub::FrBatch / jubjub::FqBatch
//   AffinePoint::{to_bytes, from_bytes, batch_from_bytes,       jubjub::AffineBatch::{to_bytes, from_bytes,
//     from_bytes_pre_zip216_compatibility, to_niels,              from_bytes_pre_zip216_compatibility, to_niels,
//     mul_by_cofactor, is_small_order, is_torsion_free,           mul_by_cofactor, is_small_order, is_torsion_free,
//     is_prime_order, is_identity}                                is_prime_order, is_identity, is_on_curve}
//   &ExtendedPoint * &Fr  (lib.rs:873-879)                      operator*(const AffineBatch&, const FrBatch&)
//   ExtendedPoint::{double, +, -, neg}                          AffineBatch::{double_, operator+, operator-, neg}
//   AffineNielsPoint::multiply_bits (lib.rs:297-301)            FixedBase::multiply_bits / operator*
//   batch_normalize (lib.rs:1084-1107)                          jubjub::batch_normalize
//   iter.sum() (lib.rs:183-193)                                 AffineBatch::sum ; jubjub::msm
//   SubgroupPoint::from_bytes (lib.rs:1427-1429)                AffineBatch::from_bytes(..., DecodeFlags::subgroup())
//
// Results cross the boundary as the crate's own public encodings, so they can be fed straight back into the Rust
// types with Fq::from_bytes / AffinePoint::from_raw_unchecked.
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "jubjub_hip.h"

namespace jubjub {

using Bytes32 = std::array<uint8_t, 32>;
using Bytes64 = std::array<uint8_t, 64>;

class Error : public std::runtime_error {
 public:
  Error(int status, const std::string& what) : std::runtime_error(what), status(status) {}
  int status;
};

// Owns one device context (one per GPU; one process per GPU is the intended deployment).
class Context {
 public:
  explicit Context(int device = 0) {
    const int rc = jj_ctx_create(device, &ctx_);
    if (rc != JJ_OK) throw Error(rc, rc == JJ_ERR_NODEVICE ? "no gfx950 GPU visible (there is no CPU fallback)" : "jj_ctx_create failed");
  }
  ~Context() { if (ctx_) jj_ctx_destroy(ctx_); }
  Context(const Context&) = delete;
  Context& operator=(const Context&) = delete;
  jj_ctx* raw() const { return ctx_; }
  void check(int rc) const { if (rc != JJ_OK) throw Error(rc, std::string("libjubjub_hip: ") + jj_last_error(ctx_)); }

 private:
  jj_ctx* ctx_ = nullptr;
};

// `CtOption<T>` for a batch: values plus one Choice byte each (1 = Some).  Values of None entries are zero.
template <class T>
struct CtOptionBatch {
  T value;
  std::vector<uint8_t> is_some;
  bool all_some() const { for (auto b : is_some) if (!b) return false; return true; }
};

// ------------------------------------------------------------------------------------------------ fields
template <bool IS_FR>
class FieldBatch {
 public:
  FieldBatch(const Context& c, std::vector<Bytes32> v) : c_(&c), v_(std::move(v)) {}
  static FieldBatch from_u64(const Context& c, const std::vector<uint64_t>& xs) {   // From<u64> for Fr (fr.rs:42-46)
    std::vector<Bytes32> v(xs.size());
    for (size_t i = 0; i < xs.size(); i++) { v[i].fill(0); for (int b = 0; b < 8; b++) v[i][b] = (uint8_t)(xs[i] >> (8 * b)); }
    return FieldBatch(c, std::move(v));
  }
  // from_bytes (fr.rs:268-292): None when the integer is not below the modulus
  static CtOptionBatch<FieldBatch> from_bytes(const Context& c, const std::vector<Bytes32>& in) {
    CtOptionBatch<FieldBatch> r{FieldBatch(c, std::vector<Bytes32>(in.size())), std::vector<uint8_t>(in.size())};
    c.check((IS_FR ? jj_fr_from_bytes : jj_fq_from_bytes)(c.raw(), in.size(), in.data(), r.value.v_.data(), r.is_some.data()));
    return r;
  }
  // from_bytes_wide (fr.rs:312-343)
  static FieldBatch from_bytes_wide(const Context& c, const std::vector<Bytes64>& in) {
    FieldBatch r(c, std::vector<Bytes32>(in.size()));
    c.check((IS_FR ? jj_fr_from_bytes_wide : jj_fq_from_bytes_wide)(c.raw(), in.size(), in.data(), r.v_.data()));
    return r;
  }
  const std::vector<Bytes32>& to_bytes() const { return v_; }   // fr.rs:296-308 (already canonical)
  size_t len() const { return v_.size(); }
  // PrimeFieldBits::to_le_bits (fr.rs:746-773): 256 bytes of 0/1 per element, bit 0 first
  std::vector<std::array<uint8_t, 256>> to_le_bits() const {
    std::vector<std::array<uint8_t, 256>> out(len());
    c_->check((IS_FR ? jj_fr_to_le_bits : jj_fq_to_le_bits)(c_->raw(), len(), v_.data(), out.data()));
    return out;
  }
  // Field::random (fr.rs:684-688; bls12_381::Scalar likewise): 64 PRNG bytes per element through from_bytes_wide, for both
  // fields.  The two 32-byte halves come from two decorrelated streams of the library's counter-based generator (the seed
  // hashed with a domain tag per half; jubjub_amd/group.py random_stream_seeds is the same function).  Test data only: the
  // generator is reproducible by design and not a source of secret scalars.
  static uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  static FieldBatch random(const Context& c, size_t n, uint64_t seed, uint64_t first_index = 0) {
    std::vector<Bytes32> lo(n), hi(n);
    c.check(jj_synth_bytes32(c.raw(), n, splitmix64(seed ^ 0x6F4C646E72466A6Aull), first_index, lo.data()));
    c.check(jj_synth_bytes32(c.raw(), n, splitmix64(seed ^ 0x6948646E72466A6Aull), first_index, hi.data()));
    std::vector<std::array<uint8_t, 64>> wide(n);
    for (size_t i = 0; i < n; i++) { std::memcpy(wide[i].data(), lo[i].data(), 32); std::memcpy(wide[i].data() + 32, hi[i].data(), 32); }
    FieldBatch r(c, std::vector<Bytes32>(n));
    c.check((IS_FR ? jj_fr_from_bytes_wide : jj_fq_from_bytes_wide)(c.raw(), n, wide.data(), r.v_.data()));
    return r;
  }

  FieldBatch operator+(const FieldBatch& o) const { return bin(IS_FR ? jj_fr_add : jj_fq_add, o); }
  FieldBatch operator-(const FieldBatch& o) const { return bin(IS_FR ? jj_fr_sub : jj_fq_sub, o); }
  FieldBatch operator*(const FieldBatch& o) const { return bin(IS_FR ? jj_fr_mul : jj_fq_mul, o); }
  FieldBatch operator-() const { return un(IS_FR ? jj_fr_neg : jj_fq_neg); }
  FieldBatch square() const { return un(IS_FR ? jj_fr_square : jj_fq_square); }
  FieldBatch double_() const { return un(IS_FR ? jj_fr_double : jj_fq_double); }
  CtOptionBatch<FieldBatch> invert() const { return opt(IS_FR ? jj_fr_invert : jj_fq_invert); }   // fr.rs:438-540
  CtOptionBatch<FieldBatch> sqrt() const { return opt(IS_FR ? jj_fr_sqrt : jj_fq_sqrt); }         // fr.rs:384-399
  bool operator==(const FieldBatch& o) const { return v_ == o.v_; }

 private:
  using Bin = int (*)(jj_ctx*, size_t, const void*, const void*, void*);
  using Un = int (*)(jj_ctx*, size_t, const void*, void*);
  using Opt = int (*)(jj_ctx*, size_t, const void*, void*, uint8_t*);
  FieldBatch bin(Bin f, const FieldBatch& o) const {
    if (o.len() != len()) throw Error(JJ_ERR_INVALID, "length mismatch");
    FieldBatch r(*c_, std::vector<Bytes32>(len()));
    c_->check(f(c_->raw(), len(), v_.data(), o.v_.data(), r.v_.data()));
    return r;
  }
  FieldBatch un(Un f) const { FieldBatch r(*c_, std::vector<Bytes32>(len())); c_->check(f(c_->raw(), len(), v_.data(), r.v_.data())); return r; }
  CtOptionBatch<FieldBatch> opt(Opt f) const {
    CtOptionBatch<FieldBatch> r{FieldBatch(*c_, std::vector<Bytes32>(len())), std::vector<uint8_t>(len())};
    c_->check(f(c_->raw(), len(), v_.data(), r.value.v_.data(), r.is_some.data()));
    return r;
  }
  const Context* c_;
  std::vector<Bytes32> v_;
};
using FrBatch = FieldBatch<true>;
using FqBatch = FieldBatch<false>;

// ------------------------------------------------------------------------------------------------ points
struct DecodeFlags {
  unsigned bits = JJ_DECOMPRESS_ZIP216;
  static DecodeFlags zip216() { return DecodeFlags{JJ_DECOMPRESS_ZIP216}; }                          // AffinePoint::from_bytes
  static DecodeFlags pre_zip216() { return DecodeFlags{0}; }                                          // from_bytes_pre_zip216_compatibility
  static DecodeFlags subgroup() { return DecodeFlags{JJ_DECOMPRESS_ZIP216 | JJ_DECOMPRESS_TORSION_FREE}; }  // SubgroupPoint::from_bytes
};

class AffineBatch {
 public:
  AffineBatch(const Context& c, std::vector<Bytes64> p) : c_(&c), p_(std::move(p)) {}
  // AffinePoint::from_raw_unchecked (lib.rs:662-664)
  static AffineBatch from_raw_unchecked(const Context& c, std::vector<Bytes64> uv) { return AffineBatch(c, std::move(uv)); }
  static AffineBatch identity(const Context& c, size_t n) {                                           // lib.rs:416-421
    std::vector<Bytes64> p(n); for (auto& e : p) { e.fill(0); e[32] = 1; } return AffineBatch(c, std::move(p));
  }
  static AffineBatch generator(const Context& c, size_t n) {                                          // lib.rs:1380-1396
    static const uint8_t U[32] = {0xfe, 0xad, 0xa7, 0xf1, 0x5d, 0xd3, 0xb3, 0xe4, 0xaf, 0x81, 0xbf, 0x29, 0x1b, 0x5d, 0xf5, 0xca,
                                  0x87, 0x81, 0x0a, 0xd6, 0xdd, 0x03, 0x0f, 0x8b, 0xc8, 0x87, 0x37, 0xbf, 0xb8, 0xcb, 0xed, 0x62};
    std::vector<Bytes64> p(n); for (auto& e : p) { e.fill(0); std::memcpy(e.data(), U, 32); e[32] = 11; } return AffineBatch(c, std::move(p));
  }
  // ExtendedPoint::random / SubgroupPoint::random (lib.rs:1244-1267, 1290-1298) over the library's counter-based stream
  static AffineBatch random(const Context& c, size_t n, uint64_t seed, uint64_t first_index = 0, bool subgroup = false) {
    std::vector<Bytes64> p(n);
    c.check(jj_random_points(c.raw(), n, seed, first_index, subgroup ? 1 : 0, p.data(), nullptr));
    return AffineBatch(c, std::move(p));
  }
  // AffinePoint::from_bytes / batch_from_bytes / from_bytes_pre_zip216_compatibility (lib.rs:469-627)
  static CtOptionBatch<AffineBatch> from_bytes(const Context& c, const std::vector<Bytes32>& enc, DecodeFlags f = DecodeFlags::zip216()) {
    CtOptionBatch<AffineBatch> r{AffineBatch(c, std::vector<Bytes64>(enc.size())), std::vector<uint8_t>(enc.size())};
    c.check(jj_decompress(c.raw(), enc.size(), enc.data(), f.bits, r.value.p_.data(), r.is_some.data()));
    return r;
  }
  static CtOptionBatch<AffineBatch> batch_from_bytes(const Context& c, const std::vector<Bytes32>& enc) { return from_bytes(c, enc); }
  static CtOptionBatch<AffineBatch> from_bytes_pre_zip216_compatibility(const Context& c, const std::vector<Bytes32>& enc) {
    return from_bytes(c, enc, DecodeFlags::pre_zip216());
  }
  std::vector<Bytes32> to_bytes() const {                                                             // lib.rs:455-464
    std::vector<Bytes32> out(len()); c_->check(jj_compress(c_->raw(), len(), p_.data(), out.data())); return out;
  }
  const std::vector<Bytes64>& coords() const { return p_; }                                           // get_u / get_v (lib.rs:630-637)
  size_t len() const { return p_.size(); }

  AffineBatch double_() const { return un(jj_point_double); }                                          // lib.rs:739-828
  AffineBatch neg() const { return un(jj_point_neg); }                                                 // lib.rs:92-104
  AffineBatch mul_by_cofactor() const { return un(jj_point_mul_by_cofactor); }                         // lib.rs:722-724
  AffineBatch operator+(const AffineBatch& o) const { return bin(jj_point_add, o); }                   // lib.rs:1012-1019
  AffineBatch operator-(const AffineBatch& o) const { return bin(jj_point_sub, o); }                   // lib.rs:1021-1028
  std::vector<std::array<uint8_t, 96>> to_niels() const {                                              // lib.rs:652-658
    std::vector<std::array<uint8_t, 96>> out(len()); c_->check(jj_point_to_niels(c_->raw(), len(), p_.data(), out.data())); return out;
  }
  std::vector<uint8_t> is_identity() const { return pred(jj_is_identity); }                            // lib.rs:424-426
  std::vector<uint8_t> is_small_order() const { return pred(jj_is_small_order); }                      // lib.rs:435-437
  std::vector<uint8_t> is_torsion_free() const { return pred(jj_is_torsion_free); }                    // lib.rs:441-443
  std::vector<uint8_t> is_prime_order() const { return pred(jj_is_prime_order); }                      // lib.rs:449-452
  std::vector<uint8_t> is_on_curve() const { return pred(jj_is_on_curve); }                            // lib.rs:670-675
  // ExtendedPoint::multiply / multiply_bits: raw 32-byte patterns, low 252 bits used (lib.rs:357-385, 831-833); constant-time like the reference (jj_varbase_mul)
  AffineBatch multiply_bits(const std::vector<Bytes32>& by) const {
    if (by.size() != len()) throw Error(JJ_ERR_INVALID, "length mismatch");
    AffineBatch r(*c_, std::vector<Bytes64>(len()));
    c_->check(jj_varbase_mul(c_->raw(), len(), by.data(), p_.data(), r.p_.data()));
    return r;
  }
  AffineBatch operator*(const FrBatch& k) const { return multiply_bits(k.to_bytes()); }                // lib.rs:873-879, 1109-1115
  // Sum (lib.rs:183-193): one point
  Bytes64 sum() const { Bytes64 out; c_->check(jj_point_sum(c_->raw(), len(), p_.data(), out.data())); return out; }
  bool operator==(const AffineBatch& o) const { return p_ == o.p_; }

 private:
  using Un = int (*)(jj_ctx*, size_t, const void*, void*);
  using Bin = int (*)(jj_ctx*, size_t, const void*, const void*, void*);
  using Pred = int (*)(jj_ctx*, size_t, const void*, uint8_t*);
  AffineBatch un(Un f) const { AffineBatch r(*c_, std::vector<Bytes64>(len())); c_->check(f(c_->raw(), len(), p_.data(), r.p_.data())); return r; }
  AffineBatch bin(Bin f, const AffineBatch& o) const {
    if (o.len() != len()) throw Error(JJ_ERR_INVALID, "length mismatch");
    AffineBatch r(*c_, std::vector<Bytes64>(len()));
    c_->check(f(c_->raw(), len(), p_.data(), o.p_.data(), r.p_.data()));
    return r;
  }
  std::vector<uint8_t> pred(Pred f) const { std::vector<uint8_t> out(len()); c_->check(f(c_->raw(), len(), p_.data(), out.data())); return out; }
  const Context* c_;
  std::vector<Bytes64> p_;
};

// `AffineNielsPoint * Fr` / multiply_bits for ONE base point (lib.rs:272-310): the window table lives on the device
class FixedBase {
 public:
  FixedBase(const Context& c, const Bytes64& base) : c_(&c) { c.check(jj_fixedbase_table_create(c.raw(), base.data(), 0, &t_)); }
  ~FixedBase() { if (t_) jj_fixedbase_table_destroy(c_->raw(), t_); }
  FixedBase(const FixedBase&) = delete;
  FixedBase& operator=(const FixedBase&) = delete;
  AffineBatch multiply_bits(const std::vector<Bytes32>& by) const {
    std::vector<Bytes64> out(by.size());
    c_->check(jj_fixedbase_mul(c_->raw(), t_, by.size(), by.data(), out.data()));
    return AffineBatch(*c_, std::move(out));
  }
  AffineBatch operator*(const FrBatch& k) const { return multiply_bits(k.to_bytes()); }
  const jj_table* raw() const { return t_; }
  const Context& context() const { return *c_; }

 private:
  const Context* c_;
  jj_table* t_ = nullptr;
};
// sum_j bases[j] * scalars[j][i] for every i: sums of AffineNielsPoint::multiply_bits over several fixed generators
inline AffineBatch fixedbase_multi_mul(const std::vector<const FixedBase*>& bases, const std::vector<std::vector<Bytes32>>& scalars) {
  if (bases.empty() || bases.size() != scalars.size()) throw Error(JJ_ERR_INVALID, "bases / scalars mismatch");
  const size_t n = scalars[0].size();
  std::vector<const jj_table*> tabs;
  std::vector<Bytes32> flat;
  flat.reserve(n * bases.size());
  for (size_t j = 0; j < bases.size(); j++) {
    if (scalars[j].size() != n) throw Error(JJ_ERR_INVALID, "length mismatch");          // cf. lib.rs:841
    tabs.push_back(bases[j]->raw());
    flat.insert(flat.end(), scalars[j].begin(), scalars[j].end());
  }
  const Context& c = bases[0]->context();
  std::vector<Bytes64> out(n);
  c.check(jj_fixedbase_multi_mul(c.raw(), tabs.data(), (int)tabs.size(), n, flat.data(), out.data()));
  return AffineBatch(c, std::move(out));
}

// Windowed Pedersen hashes (jj_pedersen_*; the function and its arguments: jubjub_hip.h).  The table of `gens` (each on the curve and
// torsion-free), seg_chunks chunks per generator; hash(): one message per row of `rows` -- `prefix_bits` bits of `prefix`, then the fields
// (byte_offset, nbits) of the row -- as the canonical u-coordinate.  VARIABLE-TIME: public inputs.  A Merkle layer over node u-coordinates is
// hash(nodes, 64, {{0, 255}, {32, 255}}, layer, 6).
class PedersenTable {
 public:
  PedersenTable(const Context& c, const std::vector<Bytes64>& gens, int seg_chunks = 63, int window_chunks = 0) : c_(&c), nseg_((int)gens.size()), seg_chunks_(seg_chunks) {
    c.check(jj_pedersen_table_create(c.raw(), nseg_, gens.data(), seg_chunks, window_chunks, &t_));
  }
  ~PedersenTable() { if (t_) jj_fixedbase_table_destroy(c_->raw(), t_); }
  PedersenTable(const PedersenTable&) = delete;
  PedersenTable& operator=(const PedersenTable&) = delete;
  std::vector<Bytes32> hash(const std::vector<uint8_t>& rows, size_t row_stride, const std::vector<std::array<uint32_t, 2>>& fields, unsigned prefix = 0, int prefix_bits = 0) const {
    const size_t n = row_stride ? rows.size() / row_stride : 0;
    std::vector<Bytes32> out(n);
    c_->check(jj_pedersen_hash_vartime(c_->raw(), t_, n, prefix, prefix_bits, rows.data(), row_stride, (int)fields.size(), fields.empty() ? nullptr : fields[0].data(), 0, out.data()));
    return out;
  }
  AffineBatch hash_points(const std::vector<uint8_t>& rows, size_t row_stride, const std::vector<std::array<uint32_t, 2>>& fields, unsigned prefix = 0, int prefix_bits = 0) const {
    const size_t n = row_stride ? rows.size() / row_stride : 0;
    std::vector<Bytes64> out(n);
    c_->check(jj_pedersen_hash_vartime(c_->raw(), t_, n, prefix, prefix_bits, rows.data(), row_stride, (int)fields.size(), fields.empty() ? nullptr : fields[0].data(), JJ_PEDERSEN_POINT, out.data()));
    return AffineBatch(*c_, std::move(out));
  }
  // <M_j> mod r, segment-major (nseg x n): what fixedbase_multi_mul reads -- the route for secret inputs, over the constant-time LDS tables
  std::vector<Bytes32> scalars(const std::vector<uint8_t>& rows, size_t row_stride, const std::vector<std::array<uint32_t, 2>>& fields, unsigned prefix = 0, int prefix_bits = 0) const {
    const size_t n = row_stride ? rows.size() / row_stride : 0;
    std::vector<Bytes32> out(n * (size_t)nseg_);
    c_->check(jj_pedersen_scalars(c_->raw(), nseg_, seg_chunks_, n, prefix, prefix_bits, rows.data(), row_stride, (int)fields.size(), fields.empty() ? nullptr : fields[0].data(), out.data()));
    return out;
  }
  // H(M) + [r] R per unit (jj_pedersen_commit_vartime): the message's fields (src, byte_offset, nbits) lie in up to four row arrays, sources[s]
  // holding n rows of strides[s] bytes; R is the base of `rbase`, r one scalar per unit.  rbase = nullptr with an empty r: the plain hash, n
  // units.  -> canonical u-coordinates.  VARIABLE-TIME in the message; r is constant-time with an LDS table (FixedBase's default).
  std::vector<Bytes32> commit(const FixedBase* rbase, const std::vector<std::vector<uint8_t>>& sources, const std::vector<size_t>& strides,
                              const std::vector<std::array<uint32_t, 3>>& fields, const std::vector<Bytes32>& r, size_t n = 0, unsigned prefix = 0, int prefix_bits = 0) const {
    std::vector<Bytes32> out(commit_units(rbase, sources, strides, r, n));
    commit_call(rbase, sources, strides, fields, r, out.size(), prefix, prefix_bits, 0, out.data());
    return out;
  }
  AffineBatch commit_points(const FixedBase* rbase, const std::vector<std::vector<uint8_t>>& sources, const std::vector<size_t>& strides,
                            const std::vector<std::array<uint32_t, 3>>& fields, const std::vector<Bytes32>& r, size_t n = 0, unsigned prefix = 0, int prefix_bits = 0) const {
    std::vector<Bytes64> out(commit_units(rbase, sources, strides, r, n));
    commit_call(rbase, sources, strides, fields, r, out.size(), prefix, prefix_bits, JJ_PEDERSEN_POINT, out.data());
    return AffineBatch(*c_, std::move(out));
  }
  const jj_table* raw() const { return t_; }

 private:
  // the units of a commit call: r's length with a blinding term, else `n`; every source must hold that many rows
  size_t commit_units(const FixedBase* rbase, const std::vector<std::vector<uint8_t>>& sources, const std::vector<size_t>& strides, const std::vector<Bytes32>& r, size_t n) const {
    if (!rbase && !r.empty()) throw Error(JJ_ERR_INVALID, "r without rbase");
    if (sources.size() != strides.size() || sources.size() > 4) throw Error(JJ_ERR_INVALID, "sources / strides mismatch");
    const size_t units = rbase ? r.size() : n;
    for (size_t s = 0; s < sources.size(); s++)
      if (sources[s].size() < units * strides[s]) throw Error(JJ_ERR_INVALID, "a source holds fewer rows than there are units");
    return units;
  }
  void commit_call(const FixedBase* rbase, const std::vector<std::vector<uint8_t>>& sources, const std::vector<size_t>& strides, const std::vector<std::array<uint32_t, 3>>& fields,
                   const std::vector<Bytes32>& r, size_t n, unsigned prefix, int prefix_bits, unsigned flags, void* out) const {
    std::vector<const void*> ptrs;
    for (const auto& s : sources) ptrs.push_back(s.data());
    c_->check(jj_pedersen_commit_vartime(c_->raw(), t_, rbase ? rbase->raw() : nullptr, n, prefix, prefix_bits, (int)sources.size(), ptrs.data(), strides.data(), (int)fields.size(),
                                         fields.empty() ? nullptr : fields[0].data(), rbase ? r.data() : nullptr, flags, out));
  }
  const Context* c_;
  int nseg_, seg_chunks_;
  jj_table* t_ = nullptr;
};

// batch_normalize (lib.rs:1084-1107): (U,V,Z,T1,T2) canonical 160-byte records -> affine
inline AffineBatch batch_normalize(const Context& c, const std::vector<std::array<uint8_t, 160>>& ext) {
  std::vector<Bytes64> out(ext.size());
  c.check(jj_batch_normalize(c.raw(), ext.size(), ext.data(), out.data()));
  return AffineBatch(c, std::move(out));
}
// sum_i points[i] * scalars[i]   (iterator Sum of p * k, lib.rs:183-193 + 873-879)
inline Bytes64 msm(const Context& c, const AffineBatch& points, const FrBatch& scalars) {
  if (points.len() != scalars.len()) throw Error(JJ_ERR_INVALID, "length mismatch");
  Bytes64 out;
  c.check(jj_msm(c.raw(), points.len(), scalars.to_bytes().data(), points.coords().data(), out.data()));
  return out;
}

// B independent sums in one call (jj_msm_batch): row b = sum_i points[i] * scalars[b][i], every row over the SAME points ...
inline AffineBatch msm_batch(const Context& c, const AffineBatch& points, const std::vector<FrBatch>& scalars) {
  const size_t n = points.len();
  std::vector<Bytes32> flat;
  flat.reserve(scalars.size() * n);
  for (const FrBatch& s : scalars) {
    if (s.len() != n) throw Error(JJ_ERR_INVALID, "length mismatch");
    flat.insert(flat.end(), s.to_bytes().begin(), s.to_bytes().end());
  }
  std::vector<Bytes64> out(scalars.size());
  c.check(jj_msm_batch(c.raw(), scalars.size(), n, flat.data(), points.coords().data(), 1, out.data()));
  return AffineBatch(c, std::move(out));
}
// ... or row b = sum_i points[b][i] * scalars[b][i], every row over its own points (all rows of one length)
inline AffineBatch msm_batch(const Context& c, const std::vector<AffineBatch>& points, const std::vector<FrBatch>& scalars) {
  if (points.size() != scalars.size()) throw Error(JJ_ERR_INVALID, "one point batch per scalar batch");
  const size_t n = points.empty() ? 0 : points[0].len();
  std::vector<Bytes32> fs;
  std::vector<Bytes64> fp;
  fs.reserve(scalars.size() * n);
  fp.reserve(points.size() * n);
  for (size_t b = 0; b < points.size(); b++) {
    if (points[b].len() != n || scalars[b].len() != n) throw Error(JJ_ERR_INVALID, "length mismatch");
    fs.insert(fs.end(), scalars[b].to_bytes().begin(), scalars[b].to_bytes().end());
    fp.insert(fp.end(), points[b].coords().begin(), points[b].coords().end());
  }
  std::vector<Bytes64> out(points.size());
  c.check(jj_msm_batch(c.raw(), points.size(), n, fs.data(), fp.data(), 0, out.data()));
  return AffineBatch(c, std::move(out));
}
// Sums of DIFFERENT lengths in one call (jj_msm_ragged): row s = sum of points[i] * scalars[i] over offsets[s] <= i < offsets[s + 1];
// offsets: S + 1 values, offsets[0] = 0, non-decreasing, offsets[S] = points.len().  An empty run gives the identity; no offsets: no rows.
inline AffineBatch msm_ragged(const Context& c, const AffineBatch& points, const FrBatch& scalars, const std::vector<uint64_t>& offsets) {
  if (points.len() != scalars.len()) throw Error(JJ_ERR_INVALID, "length mismatch");
  if (!offsets.empty() && offsets.back() != points.len()) throw Error(JJ_ERR_INVALID, "the last offset must be the number of terms");
  const size_t S = offsets.empty() ? 0 : offsets.size() - 1;
  std::vector<Bytes64> out(S);
  c.check(jj_msm_ragged(c.raw(), S, offsets.data(), scalars.to_bytes().data(), points.coords().data(), out.data()));
  return AffineBatch(c, std::move(out));
}

// Many scalar vectors against ONE set of points (jj_msm_basis_*): the points go to the device once (tables owned by this object), every
// msm(basis, rows) brings scalars only.  Mode: 0 = auto, 1 = points, 2 = windows; windows: 0 = auto or 16 .. 36 (jubjub_hip.h).
class MsmBasis {
 public:
  MsmBasis(const Context& c, const AffineBatch& points, int mode = 0, int windows = 0) : c_(&c), n_(points.len()) {
    c.check(jj_msm_basis_create(c.raw(), n_, points.coords().data(), mode, windows, &b_));
  }
  MsmBasis(const MsmBasis&) = delete;
  MsmBasis& operator=(const MsmBasis&) = delete;
  ~MsmBasis() { if (b_) (void)jj_msm_basis_destroy(c_->raw(), b_); }
  size_t len() const { return n_; }
  const jj_msm_basis* raw() const { return b_; }
  const Context& context() const { return *c_; }
  // {n, mode in use, windows of the layout, bytes of device memory}
  std::vector<int64_t> info() const { std::vector<int64_t> v(4); c_->check(jj_msm_basis_info(b_, v.data())); return v; }
 private:
  const Context* c_;
  size_t n_;
  jj_msm_basis* b_ = nullptr;
};
// row b = sum_{i < m} basis point i * rows[b][i]; every row has the same length m <= basis.len()
inline AffineBatch msm(const MsmBasis& basis, const std::vector<FrBatch>& rows) {
  const Context& c = basis.context();
  const size_t m = rows.empty() ? 0 : rows[0].len();
  std::vector<Bytes32> flat;
  flat.reserve(rows.size() * m);
  for (const FrBatch& s : rows) {
    if (s.len() != m) throw Error(JJ_ERR_INVALID, "length mismatch");
    flat.insert(flat.end(), s.to_bytes().begin(), s.to_bytes().end());
  }
  std::vector<Bytes64> out(rows.size());
  c.check(jj_msm_basis_mul(c.raw(), basis.raw(), rows.size(), m, flat.data(), out.data()));
  return AffineBatch(c, std::move(out));
}

// The same sum with the host tail of one MSM overlapping the kernels of the next (jj_msm_begin / jj_msm_finish): the job owns copies
// of its inputs until it is finished
struct AllRanks { bool by_windows = false; };      // MsmJob over every rank of the communicator lent with set_comm (jj_msm_allgather_begin)
class MsmJob {
 public:
  MsmJob(const Context& c, const AffineBatch& points, const FrBatch& scalars) : c_(&c), s_(scalars.to_bytes()), p_(points.coords()) {
    if (p_.size() != s_.size()) throw Error(JJ_ERR_INVALID, "length mismatch");
    c.check(jj_msm_begin(c.raw(), p_.size(), s_.data(), p_.data(), &job_));
  }
  // this rank's terms of a sum over all ranks: window sums, ncclAllGather and the fold of the gathered records queued behind one another;
  // every rank constructs the same jobs in the same order
  MsmJob(const Context& c, const AffineBatch& my_points, const FrBatch& my_scalars, AllRanks how) : c_(&c), s_(my_scalars.to_bytes()), p_(my_points.coords()) {
    if (p_.size() != s_.size()) throw Error(JJ_ERR_INVALID, "length mismatch");
    c.check(jj_msm_allgather_begin(c.raw(), p_.size(), s_.data(), p_.data(), how.by_windows ? 1 : 0, &job_));
  }
  // the batch check of n Schnorr signatures as one MSM job (jj_sigbatch_begin; sigbatch_begin below): host arrays, staged at begin
  MsmJob(const Context& c, const Bytes64& base, const std::vector<Bytes32>& R, const std::vector<Bytes32>& A, const std::vector<Bytes32>& s,
         const std::vector<Bytes32>& ch, const std::vector<std::array<uint8_t, 16>>& z, bool zip216) : c_(&c) {
    const size_t n = R.size();
    if (A.size() != n || s.size() != n || ch.size() != n || z.size() != n) throw Error(JJ_ERR_INVALID, "length mismatch");
    c.check(jj_sigbatch_begin(c.raw(), base.data(), n, R.data(), A.data(), s.data(), ch.data(), z.data(), zip216 ? JJ_DECOMPRESS_ZIP216 : 0u, &job_));
  }
  // the same check for signatures grouped by key (jj_sigbatch_keyed_begin; sigbatch_keyed_begin below): offsets.size() == keys.size() + 1
  MsmJob(const Context& c, const Bytes64& base, const std::vector<Bytes32>& keys, const std::vector<uint64_t>& offsets, const std::vector<Bytes32>& R,
         const std::vector<Bytes32>& s, const std::vector<Bytes32>& ch, const std::vector<std::array<uint8_t, 16>>& z, bool zip216) : c_(&c) {
    const size_t n = R.size();
    if (offsets.size() != keys.size() + 1 || offsets.back() != n || s.size() != n || ch.size() != n || z.size() != n) throw Error(JJ_ERR_INVALID, "length mismatch");
    c.check(jj_sigbatch_keyed_begin(c.raw(), base.data(), keys.size(), keys.data(), offsets.data(), R.data(), s.data(), ch.data(), z.data(), zip216 ? JJ_DECOMPRESS_ZIP216 : 0u, &job_));
  }
  MsmJob(const MsmJob&) = delete;
  MsmJob& operator=(const MsmJob&) = delete;
  ~MsmJob() { if (job_) { Bytes64 sink; (void)jj_msm_finish(job_, sink.data()); } }
  Bytes64 finish() {
    if (!job_) throw Error(JJ_ERR_INVALID, "MSM job already finished");
    Bytes64 out;
    jj_msm_job* j = job_;
    job_ = nullptr;
    c_->check(jj_msm_finish(j, out.data()));
    return out;
  }

 private:
  const Context* c_;
  std::vector<Bytes32> s_;
  std::vector<Bytes64> p_;
  jj_msm_job* job_ = nullptr;
};
// Batch verification of Schnorr signatures (jj_sigbatch_begin): R, A compressed, s canonical responses, ch raw challenges (reduced mod r),
// z the caller's 128-bit random weights.  The job's finish() is [8] (sum [z_i] R_i + sum [z_i c_i] A_i - [sum z_i s_i] B).
enum class SigVerdict { Ok, Reject, Malformed };      // (0, 1) | any other point | (0, -1)
using Bytes16 = std::array<uint8_t, 16>;
inline std::unique_ptr<MsmJob> sigbatch_begin(const Context& c, const Bytes64& base, const std::vector<Bytes32>& R, const std::vector<Bytes32>& A,
                                              const std::vector<Bytes32>& s, const std::vector<Bytes32>& ch, const std::vector<Bytes16>& z, bool zip216 = false) {
  return std::unique_ptr<MsmJob>(new MsmJob(c, base, R, A, s, ch, z, zip216));
}
// The same for signatures grouped by key (jj_sigbatch_keyed_begin): signatures offsets[k] .. offsets[k+1] are checked under keys[k]; n + K + 1
// terms.  The same 64 bytes as sigbatch_begin on the expanded arrays whenever every key has a signature.
inline std::unique_ptr<MsmJob> sigbatch_keyed_begin(const Context& c, const Bytes64& base, const std::vector<Bytes32>& keys, const std::vector<uint64_t>& offsets,
                                                    const std::vector<Bytes32>& R, const std::vector<Bytes32>& s, const std::vector<Bytes32>& ch, const std::vector<Bytes16>& z,
                                                    bool zip216 = false) {
  return std::unique_ptr<MsmJob>(new MsmJob(c, base, keys, offsets, R, s, ch, z, zip216));
}
inline SigVerdict sigbatch_verdict(const Bytes64& out) {
  static const Bytes32 minus_one = {{0x00, 0x00, 0x00, 0x00, 0xff, 0xff, 0xff, 0xff, 0xfe, 0x5b, 0xfe, 0xff, 0x02, 0xa4, 0xbd, 0x53, 0x05, 0xd8, 0xa1, 0x09, 0x08, 0xd8, 0x39, 0x33,
                                     0x48, 0x7d, 0x9d, 0x29, 0x53, 0xa7, 0xed, 0x73}};      // q - 1
  for (int i = 0; i < 32; i++) if (out[i]) return SigVerdict::Reject;
  if (out[32] == 1 && std::all_of(out.begin() + 33, out.end(), [](uint8_t b) { return b == 0; })) return SigVerdict::Ok;
  return std::equal(minus_one.begin(), minus_one.end(), out.begin() + 32) ? SigVerdict::Malformed : SigVerdict::Reject;
}
inline SigVerdict sigbatch_verify(const Context& c, const Bytes64& base, const std::vector<Bytes32>& R, const std::vector<Bytes32>& A,
                                  const std::vector<Bytes32>& s, const std::vector<Bytes32>& ch, const std::vector<Bytes16>& z, bool zip216 = false) {
  return sigbatch_verdict(sigbatch_begin(c, base, R, A, s, ch, z, zip216)->finish());
}
inline SigVerdict sigbatch_keyed_verify(const Context& c, const Bytes64& base, const std::vector<Bytes32>& keys, const std::vector<uint64_t>& offsets,
                                        const std::vector<Bytes32>& R, const std::vector<Bytes32>& s, const std::vector<Bytes32>& ch, const std::vector<Bytes16>& z,
                                        bool zip216 = false) {
  return sigbatch_verdict(sigbatch_keyed_begin(c, base, keys, offsets, R, s, ch, z, zip216)->finish());
}
// S batch checks over consecutive runs of one signature array, one verdict per run (jj_sigbatch_ragged): segment g holds signatures
// offsets[g] .. offsets[g+1]; row g is what sigbatch_begin + finish give for that segment alone (an empty segment: the identity).
inline std::vector<Bytes64> sigbatch_ragged(const Context& c, const Bytes64& base, const std::vector<uint64_t>& offsets, const std::vector<Bytes32>& R, const std::vector<Bytes32>& A,
                                            const std::vector<Bytes32>& s, const std::vector<Bytes32>& ch, const std::vector<Bytes16>& z, bool zip216 = false) {
  const size_t n = R.size();
  if (A.size() != n || s.size() != n || ch.size() != n || z.size() != n || (!offsets.empty() && offsets.back() != n) || (offsets.empty() && n)) throw Error(JJ_ERR_INVALID, "length mismatch");
  const size_t S = offsets.empty() ? 0 : offsets.size() - 1;
  std::vector<Bytes64> out(S);
  c.check(jj_sigbatch_ragged(c.raw(), base.data(), S, offsets.data(), R.data(), A.data(), s.data(), ch.data(), z.data(), zip216 ? JJ_DECOMPRESS_ZIP216 : 0u, out.data()));
  return out;
}
inline std::vector<SigVerdict> sigbatch_ragged_verify(const Context& c, const Bytes64& base, const std::vector<uint64_t>& offsets, const std::vector<Bytes32>& R,
                                                      const std::vector<Bytes32>& A, const std::vector<Bytes32>& s, const std::vector<Bytes32>& ch, const std::vector<Bytes16>& z,
                                                      bool zip216 = false) {
  std::vector<SigVerdict> v;
  for (const Bytes64& row : sigbatch_ragged(c, base, offsets, R, A, s, ch, z, zip216)) v.push_back(sigbatch_verdict(row));
  return v;
}
// One verdict per signature in one call (jj_sigverify_each): JJ_SIG_OK iff [8]([s]B - [c]A - R) = O, B the base of `g` -- the cofactored equation
// of every sigbatch_* call; cofactored = false: iff [s]B - [c]A - R = O --, JJ_SIG_MALFORMED for an R or A that does not decode or s >= r, else
// JJ_SIG_REJECT.  Variable-time; everything is public.
inline std::vector<uint8_t> sigverify_each(const FixedBase& g, const std::vector<Bytes32>& R, const std::vector<Bytes32>& A, const std::vector<Bytes32>& s,
                                           const std::vector<Bytes32>& ch, bool zip216 = false, bool cofactored = true) {
  const size_t n = R.size();
  if (A.size() != n || s.size() != n || ch.size() != n) throw Error(JJ_ERR_INVALID, "length mismatch");
  const Context& c = g.context();
  std::vector<uint8_t> v(n);
  c.check(jj_sigverify_each(c.raw(), g.raw(), n, R.data(), A.data(), s.data(), ch.data(), (zip216 ? JJ_DECOMPRESS_ZIP216 : 0u) | (cofactored ? 0u : JJ_SIG_COFACTORLESS), v.data()));
  return v;
}
// The challenges of the signature family, hashed on the device (jj_sig_challenge): c_i = Fr::from_bytes_wide(BLAKE2b-512(personal; R_i || A_i || M_i))
// as canonical bytes.  An EMPTY R or A leaves that part out of the hash; personal == nullptr is sixteen zero bytes (RedJubjub: "Zcash_RedJubjubH").
// The messages are packed here and may differ in length; meant for short ones (one lane hashes one message).
inline std::vector<Bytes32> sig_challenge(const Context& c, const std::vector<Bytes32>& R, const std::vector<Bytes32>& A, const std::vector<std::vector<uint8_t>>& msgs,
                                          const std::array<uint8_t, 16>* personal = nullptr) {
  const size_t n = msgs.size();
  if ((!R.empty() && R.size() != n) || (!A.empty() && A.size() != n)) throw Error(JJ_ERR_INVALID, "length mismatch");
  std::vector<uint64_t> offsets(n + 1, 0);
  for (size_t i = 0; i < n; i++) offsets[i + 1] = offsets[i] + msgs[i].size();
  std::vector<uint8_t> flat;
  flat.reserve((size_t)offsets[n]);
  for (const auto& m : msgs) flat.insert(flat.end(), m.begin(), m.end());
  std::vector<Bytes32> out(n);
  c.check(jj_sig_challenge(c.raw(), n, personal ? personal->data() : nullptr, R.empty() ? nullptr : R.data(), A.empty() ? nullptr : A.data(), flat.data(), 0, offsets.data(), out.data()));
  return out;
}
// Key agreement with ONE secret scalar and its KDF (jj_ka_kdf): keys[i] = BLAKE2b-256(personal; to_bytes(share_i) [|| P[i]]), share_i = [sk]P_i or
// [8]([sk]P_i); flags: the decoder's JJ_DECOMPRESS_ZIP216 | _TORSION_FREE | _NOT_SMALL_ORDER bits | JJ_KA_COFACTOR | JJ_KA_HASH_INPUT.  ok[i] = 0
// and a zero key where P[i] does not decode.  CONSTANT-TIME in sk and in the shares.  personal == nullptr is sixteen zero bytes (the Sapling
// recipient: "Zcash_SaplingKDF" with JJ_DECOMPRESS_ZIP216 | JJ_KA_COFACTOR | JJ_KA_HASH_INPUT).
struct KaKeys { std::vector<Bytes32> keys; std::vector<uint8_t> ok; };
inline KaKeys ka_kdf(const Context& c, const Bytes32& sk, const std::vector<Bytes32>& P, unsigned flags, const std::array<uint8_t, 16>* personal = nullptr) {
  KaKeys r{std::vector<Bytes32>(P.size()), std::vector<uint8_t>(P.size())};
  c.check(jj_ka_kdf(c.raw(), P.size(), sk.data(), P.data(), flags, personal ? personal->data() : nullptr, r.keys.data(), r.ok.data()));
  return r;
}
// The same with one secret scalar PER ROW (jj_ka_kdf_each: the sender's side of a note): sk[i] is read as jj_varbase_mul reads a scalar; with
// JJ_KA_HASH_INPUT the second hashed part is (*hash_input)[i] when hash_input is given and P[i] when it is nullptr.  CONSTANT-TIME in the
// scalars and in the shares.
inline KaKeys ka_kdf_each(const Context& c, const std::vector<Bytes32>& sk, const std::vector<Bytes32>& P, unsigned flags, const std::vector<Bytes32>* hash_input = nullptr,
                          const std::array<uint8_t, 16>* personal = nullptr) {
  if (sk.size() != P.size() || (hash_input && hash_input->size() != P.size())) throw Error(JJ_ERR_INVALID, "length mismatch");
  KaKeys r{std::vector<Bytes32>(P.size()), std::vector<uint8_t>(P.size())};
  c.check(jj_ka_kdf_each(c.raw(), P.size(), sk.data(), P.data(), hash_input ? hash_input->data() : nullptr, flags, personal ? personal->data() : nullptr, r.keys.data(), r.ok.data()));
  return r;
}
// Raw BLAKE2b digests over rows gathered from up to four arrays (jj_blake2b): out[i] = BLAKE2b-digest_len(personal; prefix || S_0[i] || ..),
// S_s[i] the lens[s] bytes at sources[s] + i * strides[s]; digest_len 32 or 64; lengths, strides and the prefix's length multiples of 4.
// The result is n x digest_len bytes, dense.  personal == nullptr is sixteen zero bytes.  The library knows no protocol: personalisation,
// prefix and layout are the caller's (Sapling's ock: digest_len 32, prefix = ovk, the sources cv, cmu, epk).
inline std::vector<uint8_t> blake2b(const Context& c, size_t n, int digest_len, const std::vector<const uint8_t*>& sources, const std::vector<size_t>& lens,
                                    const std::vector<size_t>& strides, const std::vector<uint8_t>& prefix = {}, const std::array<uint8_t, 16>* personal = nullptr) {
  if (sources.size() != lens.size() || sources.size() != strides.size() || sources.size() > 4 || (digest_len != 32 && digest_len != 64)) throw Error(JJ_ERR_INVALID, "length mismatch");
  std::vector<const void*> ptrs(sources.begin(), sources.end());
  std::vector<uint8_t> out(n * (size_t)digest_len);
  c.check(jj_blake2b(c.raw(), n, digest_len, personal ? personal->data() : nullptr, prefix.empty() ? nullptr : prefix.data(), prefix.size(), (int)sources.size(),
                     ptrs.empty() ? nullptr : ptrs.data(), lens.empty() ? nullptr : lens.data(), strides.empty() ? nullptr : strides.data(), out.data()));
  return out;
}
// One RFC 8439 ChaCha20 key per row (jj_chacha20_xor): rows of `len` bytes at a stride of in_stride in `in`, a dense n x len result; len and
// in_stride multiples of 4, len in 4..1024; nonce == nullptr is twelve zero bytes.
inline std::vector<uint8_t> chacha20_xor(const Context& c, const std::vector<Bytes32>& keys, const std::vector<uint8_t>& in, size_t len, size_t in_stride, uint32_t counter = 0,
                                         const std::array<uint8_t, 12>* nonce = nullptr) {
  const size_t n = keys.size();
  if (n && in.size() < (n - 1) * in_stride + len) throw Error(JJ_ERR_INVALID, "length mismatch");
  std::vector<uint8_t> out(n * len);
  c.check(jj_chacha20_xor(c.raw(), n, keys.data(), nonce ? nonce->data() : nullptr, counter, in.data(), len, in_stride, out.data()));
  return out;
}
// One Poly1305 one-time key per row (jj_poly1305; r in key bytes 0..15, s in bytes 16..31): the tags of rows of `len` bytes at a stride of
// in_stride in `in`, n x 16 bytes, dense; len and in_stride multiples of 4, len in 4..1024.
inline std::vector<uint8_t> poly1305(const Context& c, const std::vector<Bytes32>& keys, const std::vector<uint8_t>& in, size_t len, size_t in_stride) {
  const size_t n = keys.size();
  if (n && in.size() < (n - 1) * in_stride + len) throw Error(JJ_ERR_INVALID, "length mismatch");
  std::vector<uint8_t> out(n * 16);
  c.check(jj_poly1305(c.raw(), n, keys.data(), in.data(), len, in_stride, out.data()));
  return out;
}
// RFC 8439 ChaCha20-Poly1305 with one key per row, the tag checked on the device (jj_aead_open): a row of `in` is `len` ciphertext bytes and the
// 16 tag bytes; ok[i] = 1 and the plaintext, or ok[i] = 0 and a zero row where the tag does not verify.  One nonce (nullptr: twelve zero bytes)
// and one aad (at most 64 bytes) for all rows.
struct AeadOpened { std::vector<uint8_t> plain; std::vector<uint8_t> ok; };
inline AeadOpened aead_open(const Context& c, const std::vector<Bytes32>& keys, const std::vector<uint8_t>& in, size_t len, size_t in_stride, const std::vector<uint8_t>& aad = {},
                            const std::array<uint8_t, 12>* nonce = nullptr) {
  const size_t n = keys.size();
  if (n && in.size() < (n - 1) * in_stride + len + 16) throw Error(JJ_ERR_INVALID, "length mismatch");
  AeadOpened r{std::vector<uint8_t>(n * len), std::vector<uint8_t>(n)};
  c.check(jj_aead_open(c.raw(), n, keys.data(), nonce ? nonce->data() : nullptr, aad.empty() ? nullptr : aad.data(), aad.size(), in.data(), len, in_stride, r.plain.data(), r.ok.data()));
  return r;
}
// The sealing direction (jj_aead_seal): n x (len + 16) bytes, each row its ciphertext followed by its tag.
inline std::vector<uint8_t> aead_seal(const Context& c, const std::vector<Bytes32>& keys, const std::vector<uint8_t>& in, size_t len, size_t in_stride, const std::vector<uint8_t>& aad = {},
                                      const std::array<uint8_t, 12>* nonce = nullptr) {
  const size_t n = keys.size();
  if (n && in.size() < (n - 1) * in_stride + len) throw Error(JJ_ERR_INVALID, "length mismatch");
  std::vector<uint8_t> out(n * (len + 16));
  c.check(jj_aead_seal(c.raw(), n, keys.data(), nonce ? nonce->data() : nullptr, aad.empty() ? nullptr : aad.data(), aad.size(), in.data(), len, in_stride, out.data()));
  return out;
}
// BLAKE2s-256(personal; prefix || M_i) for n messages of msg_len bytes, msg_stride apart in `msgs` (jj_blake2s); personal == nullptr is eight
// zero bytes.  The library knows no protocol's personalisation or prefix: both are the caller's.
inline std::vector<Bytes32> blake2s(const Context& c, size_t n, const std::vector<uint8_t>& msgs, size_t msg_len, size_t msg_stride, const std::vector<uint8_t>& prefix = {},
                                    const std::array<uint8_t, 8>* personal = nullptr) {
  if (n && msg_len && (msg_stride < msg_len || msgs.size() < (n - 1) * msg_stride + msg_len)) throw Error(JJ_ERR_INVALID, "length mismatch");
  std::vector<Bytes32> out(n);
  c.check(jj_blake2s(c.raw(), n, personal ? personal->data() : nullptr, prefix.empty() ? nullptr : prefix.data(), prefix.size(), msgs.empty() ? nullptr : msgs.data(), msg_len, msg_stride,
                     out.data()));
  return out;
}
// Hash to the curve (jj_group_hash): the digest of blake2s decoded exactly as jj_decompress decodes it under `flags` (the four JJ_DECOMPRESS_*
// bits; JJ_DECOMPRESS_ZIP216 | JJ_DECOMPRESS_NOT_SMALL_ORDER | JJ_DECOMPRESS_CLEAR_COFACTOR is [8] * decode(digest), small order refused).
// ok[i] = 0 and 64 zero bytes where digest_i is refused.
struct GroupHash { std::vector<std::array<uint8_t, 64>> points; std::vector<uint8_t> ok; };
inline GroupHash group_hash(const Context& c, size_t n, const std::vector<uint8_t>& msgs, size_t msg_len, size_t msg_stride, unsigned flags, const std::vector<uint8_t>& prefix = {},
                            const std::array<uint8_t, 8>* personal = nullptr) {
  if (n && msg_len && (msg_stride < msg_len || msgs.size() < (n - 1) * msg_stride + msg_len)) throw Error(JJ_ERR_INVALID, "length mismatch");
  GroupHash r{std::vector<std::array<uint8_t, 64>>(n), std::vector<uint8_t>(n)};
  c.check(jj_group_hash(c.raw(), n, personal ? personal->data() : nullptr, prefix.empty() ? nullptr : prefix.data(), prefix.size(), msgs.empty() ? nullptr : msgs.data(), msg_len, msg_stride,
                        flags, r.points.data(), r.ok.data()));
  return r;
}
// MSM cut into parts (jj_msm_partial / jj_msm_combine): part g of G by windows (every part sees all terms) or all windows of a slice
// of the terms; the records are combined in one host tail
using MsmRecord = std::array<uint8_t, JJ_MSM_PARTIAL_BYTES>;
inline MsmRecord msm_partial(const Context& c, const AffineBatch& points, const FrBatch& scalars, int part_index = 0, int part_count = 1) {
  if (points.len() != scalars.len()) throw Error(JJ_ERR_INVALID, "length mismatch");
  MsmRecord rec;
  c.check(jj_msm_partial(c.raw(), points.len(), scalars.to_bytes().data(), points.coords().data(), part_index, part_count, rec.data()));
  return rec;
}
inline Bytes64 msm_combine(const std::vector<MsmRecord>& records) {
  Bytes64 out;
  const int rc = jj_msm_combine(records.size(), records.empty() ? nullptr : records.data(), out.data());
  if (rc) throw Error(rc, "jj_msm_combine: damaged or mismatched records");
  return out;
}
// Round 4: page-locked host memory for batches that come back call after call (jj_host_alloc); the raw entry points then copy straight
// from and to it.  (std::vector arguments are pageable: the library moves them through its own page-locked staging buffers.)
class HostBuffer {
 public:
  explicit HostBuffer(size_t bytes) : n_(bytes) { const int rc = jj_host_alloc(bytes, &p_); if (rc) throw Error(rc, "jj_host_alloc failed"); }
  ~HostBuffer() { (void)jj_host_free(p_); }
  HostBuffer(const HostBuffer&) = delete;
  HostBuffer& operator=(const HostBuffer&) = delete;
  uint8_t* data() { return static_cast<uint8_t*>(p_); }
  const uint8_t* data() const { return static_cast<const uint8_t*>(p_); }
  size_t size() const { return n_; }
 private:
  void* p_ = nullptr;
  size_t n_ = 0;
};
// points[i] * scalars[i] on raw wire-format buffers (any kind of host memory, e.g. HostBuffers kept by the caller): out = n x 64 bytes
inline void multiply_raw(const Context& c, size_t n, const uint8_t* scalars32, const uint8_t* points64, uint8_t* out64) {
  c.check(jj_varbase_mul(c.raw(), n, scalars32, points64, out64));
}
// One process per GPU: the Sum over the terms of every rank of an RCCL communicator the application created (jj_ctx_set_comm +
// jj_msm_allgather; examples/msm_rccl.cpp).  all_gather_fn: address of that RCCL library's ncclAllGather, or nullptr (looked up).
inline void set_comm(const Context& c, void* nccl_comm, int rank, int nranks, void* all_gather_fn = nullptr) {
  c.check(jj_ctx_set_comm(c.raw(), nccl_comm, rank, nranks, all_gather_fn));
}
inline Bytes64 msm_all_ranks(const Context& c, const AffineBatch& my_points, const FrBatch& my_scalars, bool by_windows = false) {
  if (my_points.len() != my_scalars.len()) throw Error(JJ_ERR_INVALID, "length mismatch");
  Bytes64 out;
  c.check(jj_msm_allgather(c.raw(), my_points.len(), my_scalars.to_bytes().data(), my_points.coords().data(), by_windows ? 1 : 0, out.data()));
  return out;
}
// `ExtendedPoint * Fr` as operator* computes it: the reference's constant-time discipline (lib.rs:334-343, 357-379), no scalar-dependent
// address or branch (jj_varbase_mul; multiply_ct is the name rounds 3-4 gave it)
inline AffineBatch multiply_ct(const Context& c, const AffineBatch& points, const FrBatch& scalars) {
  if (points.len() != scalars.len()) throw Error(JJ_ERR_INVALID, "length mismatch");
  std::vector<Bytes64> out(points.len());
  c.check(jj_varbase_mul_ct(c.raw(), points.len(), scalars.to_bytes().data(), points.coords().data(), out.data()));
  return AffineBatch(c, std::move(out));
}
// the same product by the variable-time ladder (per-lane window table in memory, digit-dependent addresses): for PUBLIC scalars only
inline AffineBatch multiply_vartime(const Context& c, const AffineBatch& points, const FrBatch& scalars) {
  if (points.len() != scalars.len()) throw Error(JJ_ERR_INVALID, "length mismatch");
  std::vector<Bytes64> out(points.len());
  c.check(jj_varbase_mul_vartime(c.raw(), points.len(), scalars.to_bytes().data(), points.coords().data(), out.data()));
  return AffineBatch(c, std::move(out));
}
// p[i] * a[i] + q[i] * b[i] in one interleaved ladder per unit (jj_varbase_mul2_vartime): variable-time, for PUBLIC scalars only; the same points as
// multiply_vartime twice and a sum
inline AffineBatch multiply2_vartime(const Context& c, const AffineBatch& p, const FrBatch& a, const AffineBatch& q, const FrBatch& b) {
  if (p.len() != a.len() || q.len() != b.len() || p.len() != q.len()) throw Error(JJ_ERR_INVALID, "length mismatch");
  std::vector<Bytes64> out(p.len());
  c.check(jj_varbase_mul2_vartime(c.raw(), p.len(), a.to_bytes().data(), p.coords().data(), b.to_bytes().data(), q.coords().data(), out.data()));
  return AffineBatch(c, std::move(out));
}
// p[i] * a + q[i] * b for one pair of scalars (jj_varbase_mul2_scalars)
inline AffineBatch multiply2_scalars(const Context& c, const AffineBatch& p, const Bytes32& a, const AffineBatch& q, const Bytes32& b) {
  if (p.len() != q.len()) throw Error(JJ_ERR_INVALID, "length mismatch");
  Bytes32 ab[2] = {a, b};
  std::vector<Bytes64> out(p.len());
  c.check(jj_varbase_mul2_scalars(c.raw(), p.len(), ab, p.coords().data(), q.coords().data(), out.data()));
  return AffineBatch(c, std::move(out));
}
// g * a[i] + q[i] * b[i], g the base of a FixedBase (jj_fixedvar_mul_vartime): variable-time, for PUBLIC scalars only; the same points as
// g * a, multiply_vartime(q, b) and a sum
inline AffineBatch multiply_fixed_add_vartime(const FixedBase& g, const FrBatch& a, const AffineBatch& q, const FrBatch& b) {
  if (a.len() != b.len() || q.len() != b.len()) throw Error(JJ_ERR_INVALID, "length mismatch");
  const Context& c = g.context();
  std::vector<Bytes64> out(q.len());
  c.check(jj_fixedvar_mul_vartime(c.raw(), g.raw(), q.len(), a.to_bytes().data(), b.to_bytes().data(), q.coords().data(), out.data()));
  return AffineBatch(c, std::move(out));
}
// several fixed bases with short scalars through one LDS table set, one pass (sums of multiply_bits, lib.rs:297-301)
class CompositeBase {
 public:
  CompositeBase(const Context& c, const std::vector<Bytes64>& bases, const std::vector<int>& scalar_bits) : c_(&c), nb_(bases.size()) {
    if (bases.empty() || bases.size() != scalar_bits.size()) throw Error(JJ_ERR_INVALID, "one bit length per base");
    c.check(jj_fixedbase_composite_create(c.raw(), (int)bases.size(), bases.data(), scalar_bits.data(), &t_));
  }
  ~CompositeBase() { if (t_) jj_fixedbase_table_destroy(c_->raw(), t_); }
  CompositeBase(const CompositeBase&) = delete;
  CompositeBase& operator=(const CompositeBase&) = delete;
  // scalars[b][i]: only the low scalar_bits[b] bits are used
  AffineBatch multiply_bits(const std::vector<std::vector<Bytes32>>& scalars) const {
    if (scalars.size() != nb_) throw Error(JJ_ERR_INVALID, "bases / scalars mismatch");
    const size_t n = scalars[0].size();
    std::vector<Bytes32> flat;
    for (const auto& v : scalars) { if (v.size() != n) throw Error(JJ_ERR_INVALID, "length mismatch"); flat.insert(flat.end(), v.begin(), v.end()); }
    std::vector<Bytes64> out(n);
    c_->check(jj_fixedbase_composite_mul(c_->raw(), t_, n, flat.data(), out.data()));
    return AffineBatch(*c_, std::move(out));
  }

 private:
  const Context* c_;
  size_t nb_;
  jj_table* t_ = nullptr;
};

}  // namespace jubjub
