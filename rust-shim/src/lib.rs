//! jubjub-hip: batched Jubjub arithmetic on AMD MI355X (gfx950) behind the `jubjub` crate's own types.
//!
//! A thin, safe layer over `libjubjub_hip.so` (C ABI: `include/jubjub_hip.h`; raw declarations: `ffi.rs`, generated from that header by
//! `tools/gen_rust_ffi.py` and held to it by `tests/test_rust_shim_signatures.py`).  It marshals through the crate's PUBLIC byte APIs only
//! (`Fr::to_bytes / from_bytes`, `Fq::to_bytes / from_bytes`, `AffinePoint::{get_u, get_v, from_raw_unchecked, to_bytes}`), so it builds next
//! to an unmodified `jubjub` 0.10.  The build image of the GPU library has no Rust toolchain: this crate has not been compiled there; what IS
//! checked mechanically is every `extern "C"` signature against the header.
//!
//! Reference interface replaced, by entry point: see INTEGRATION.md section 2 (`/root/reference/src/lib.rs`, `src/fr.rs` line numbers).
use jubjub::{AffinePoint, ExtendedPoint, Fq, Fr, SubgroupPoint};
use group::{cofactor::CofactorGroup, Curve};
use std::os::raw::{c_int, c_void};

pub mod ffi;
use ffi::*;


pub const ZIP216: u32 = 1; pub const TORSION_FREE: u32 = 2; pub const NOT_SMALL_ORDER: u32 = 4; pub const CLEAR_COFACTOR: u32 = 8;

/// A byte buffer in page-locked host memory (jj_host_alloc) for callers that multiply batch after batch: allocated ONCE (page-locking
/// a gigabyte takes longer than the call it serves), reused by every call (`PinnedBatch` below), it lets the copies run straight from
/// and to the caller's memory: 0.89-0.91 of the device-resident rate at 2^24 fixed-base units (profiles/r4_pcie_inclusive.txt).
/// One-shot callers just pass `Vec<u8>`s: the library moves pageable memory through its own page-locked staging buffers with a few copy
/// threads (within 2-3 % of the page-locked rate, and a freshly allocated result vector costs only its page faults).
pub struct HostBuf { p: *mut u8, len: usize }
impl HostBuf {
    pub fn new(len: usize) -> Self {
        let mut p: *mut c_void = std::ptr::null_mut();
        assert_eq!(unsafe { jj_host_alloc(len.max(1), &mut p) }, 0);
        HostBuf { p: p as *mut u8, len }
    }
    pub fn as_slice(&self) -> &[u8] { unsafe { std::slice::from_raw_parts(self.p, self.len) } }
    pub fn as_mut_slice(&mut self) -> &mut [u8] { unsafe { std::slice::from_raw_parts_mut(self.p, self.len) } }
    pub fn as_ptr(&self) -> *const c_void { self.p as _ }
    pub fn as_mut_ptr(&mut self) -> *mut c_void { self.p as _ }
}
impl Drop for HostBuf { fn drop(&mut self) { unsafe { jj_host_free(self.p as _); } } }
unsafe impl Send for HostBuf {}

/// an MSM in flight (jj_msm_begin): finished exactly once by `GpuBatch::msm_finish`
pub struct MsmJob { job: *mut JjMsmJob, _keep: (Vec<u8>, Vec<u8>) }

fn write_points(p: &mut [u8], points: &[AffinePoint]) {
    for (i, q) in points.iter().enumerate() {
        p[64 * i..64 * i + 32].copy_from_slice(&q.get_u().to_bytes());        // src/lib.rs:630-637
        p[64 * i + 32..64 * i + 64].copy_from_slice(&q.get_v().to_bytes());
    }
}
fn write_scalars(s: &mut [u8], scalars: &[Fr]) {
    for (i, k) in scalars.iter().enumerate() { s[32 * i..32 * i + 32].copy_from_slice(&k.to_bytes()); }   // src/fr.rs:296-308
}
fn put_points(points: &[AffinePoint]) -> Vec<u8> { let mut p = vec![0u8; 64 * points.len()]; write_points(&mut p, points); p }
fn put_scalars(scalars: &[Fr]) -> Vec<u8> { let mut s = vec![0u8; 32 * scalars.len()]; write_scalars(&mut s, scalars); s }

/// Marshalling buffers of a caller that multiplies batch after batch: page-locked once, reused by every call.
pub struct PinnedBatch { cap: usize, s: HostBuf, p: HostBuf, out: HostBuf }
impl PinnedBatch {
    pub fn new(cap: usize) -> Self { PinnedBatch { cap, s: HostBuf::new(32 * cap), p: HostBuf::new(64 * cap), out: HostBuf::new(64 * cap) } }
}
fn get_point(b: &[u8]) -> AffinePoint {
    let u = Fq::from_bytes(b[..32].try_into().unwrap()).unwrap();                 // the library only emits canonical encodings
    let v = Fq::from_bytes(b[32..64].try_into().unwrap()).unwrap();
    AffinePoint::from_raw_unchecked(u, v)                                         // src/lib.rs:662-664
}

/// A page-locked result buffer out of the context's pool (jj_result_acquire); goes back to the pool when dropped.
pub struct Pooled<'a> { gpu: &'a Gpu, p: *mut u8, len: usize }
impl Pooled<'_> {
    pub fn bytes(&self) -> &[u8] { unsafe { std::slice::from_raw_parts(self.p, self.len) } }
}
impl Drop for Pooled<'_> { fn drop(&mut self) { unsafe { jj_result_release(self.gpu.0, self.p as _); } } }

pub struct Gpu(*mut JjCtx);
unsafe impl Send for Gpu {}    // the library serialises the entry points of one context on a lock
unsafe impl Sync for Gpu {}

impl Gpu {
    pub fn new(device: i32) -> Option<Self> {
        let mut p = std::ptr::null_mut();
        if unsafe { jj_ctx_create(device, &mut p) } == 0 { Some(Gpu(p)) } else { None }   // JJ_ERR_NODEVICE: no gfx950, no CPU fallback
    }

    /// Per-context tuning by key (jj_ctx_set_option; the library reads no environment variable).  No key touches the timing discipline.
    pub fn set_option(&self, key: &str, value: i64) -> bool {
        let k = std::ffi::CString::new(key).unwrap();
        unsafe { jj_ctx_set_option(self.0, k.as_ptr(), value) == 0 }
    }

    /// Batched `points[i] * scalars[i]`  (reference: `Mul<&Fr> for &ExtendedPoint`, src/lib.rs:873-879).  CONSTANT-TIME like the reference's
    /// ladder (`conditional_select`, src/lib.rs:334-343, 357-379): `jj_varbase_mul` has no scalar-dependent address or branch.
    pub fn mul_batch(&self, points: &[AffinePoint], scalars: &[Fr]) -> Vec<AffinePoint> {
        assert_eq!(points.len(), scalars.len());                                  // cf. src/lib.rs:841
        let (n, s, p) = (points.len(), put_scalars(scalars), put_points(points)); // pageable inputs: through the library's staging slots (bounce path)
        let out = self.result(64 * n);                                            // a page-locked buffer from the library's pool: no page faults of a fresh
                                                                                  // Vec inside the call, no registration; a different buffer per call in flight
        assert_eq!(unsafe { jj_varbase_mul(self.0, n, s.as_ptr() as _, p.as_ptr() as _, out.p as _) }, 0);
        out.bytes().chunks_exact(64).map(get_point).collect()                     // the `-> Vec` the caller sees; `out` goes back to the pool when it drops here
    }

    /// Result buffers for the `-> Vec<..>`-shaped functions (reference: `batch_from_bytes` src/lib.rs:541-627, `batch_normalize` 1084-1107): see
    /// `jj_result_acquire` in include/jubjub_hip.h.  Measured (bench.py --host-buffers pooled, 2^24 fixed-base units): 559 M/s against 195 M/s with a fresh `Vec`.
    fn result(&self, bytes: usize) -> Pooled<'_> {
        let mut p = std::ptr::null_mut();
        assert_eq!(unsafe { jj_result_acquire(self.0, bytes, &mut p) }, 0);
        Pooled { gpu: self, p: p as *mut u8, len: bytes }
    }

    /// The same with the caller's page-locked, reused buffers: the copies run straight from and to them.
    pub fn mul_batch_pinned(&self, b: &mut PinnedBatch, points: &[AffinePoint], scalars: &[Fr]) -> Vec<AffinePoint> {
        assert!(points.len() == scalars.len() && points.len() <= b.cap);
        let n = points.len();
        write_scalars(b.s.as_mut_slice(), scalars);
        write_points(b.p.as_mut_slice(), points);
        assert_eq!(unsafe { jj_varbase_mul(self.0, n, b.s.as_ptr(), b.p.as_ptr(), b.out.as_mut_ptr()) }, 0);
        b.out.as_slice()[..64 * n].chunks_exact(64).map(get_point).collect()
    }

    /// One scalar, many bases: the `Wnaf::new().scalar(k)` then `.base(p)` reuse pattern (WnafGroup, src/lib.rs:1318-1336).
    pub fn mul_scalar(&self, k: &Fr, points: &[AffinePoint]) -> Vec<AffinePoint> {
        let (n, p) = (points.len(), put_points(points));
        let mut out = vec![0u8; 64 * n];
        assert_eq!(unsafe { jj_varbase_mul_scalar(self.0, n, k.to_bytes().as_ptr() as _, p.as_ptr() as _, out.as_mut_ptr() as _) }, 0);
        out.chunks_exact(64).map(get_point).collect()
    }

    /// `sum_i points[i] * scalars[i]` (the `Sum` of `p * k`, src/lib.rs:183-193).
    pub fn msm(&self, points: &[AffinePoint], scalars: &[Fr]) -> ExtendedPoint {
        assert_eq!(points.len(), scalars.len());
        let (n, s, p) = (points.len(), put_scalars(scalars), put_points(points));
        let mut out = [0u8; 64];
        assert_eq!(unsafe { jj_msm(self.0, n, s.as_ptr() as _, p.as_ptr() as _, out.as_mut_ptr() as _) }, 0);
        get_point(&out).into()
    }

    /// `B` independent sums in one call (`jj_msm_batch`): row `b` is `sum_i points[i] * scalars[b][i]` when `points` holds `n` points shared
    /// by every row, or `sum_i points[b n + i] * scalars[b][i]` when it holds `B n` (one run of `n` per row).  Every row has `n` scalars.
    pub fn msm_batch(&self, points: &[AffinePoint], scalars: &[Vec<Fr>]) -> Vec<ExtendedPoint> {
        let (b, n) = (scalars.len(), scalars.first().map_or(0, |r| r.len()));
        assert!(scalars.iter().all(|r| r.len() == n));
        let shared = points.len() == n;
        assert!(shared || points.len() == b * n);
        let flat: Vec<Fr> = scalars.iter().flatten().copied().collect();
        let (s, p) = (put_scalars(&flat), put_points(points));
        let mut out = vec![0u8; 64 * b];
        assert_eq!(unsafe { jj_msm_batch(self.0, b, n, s.as_ptr() as _, p.as_ptr() as _, shared as c_int, out.as_mut_ptr() as _) }, 0);
        out.chunks_exact(64).map(|r| get_point(r).into()).collect()
    }

    /// Sums of different lengths in one call (`jj_msm_ragged`): row `s` is `sum_i points[i] * scalars[i]` over `offsets[s] <= i < offsets[s + 1]`.
    /// `offsets` holds `S + 1` values, starts at 0, never decreases and ends at `points.len()`; an empty run gives the identity.
    pub fn msm_ragged(&self, points: &[AffinePoint], scalars: &[Fr], offsets: &[u64]) -> Vec<ExtendedPoint> {
        assert_eq!(points.len(), scalars.len());
        if offsets.is_empty() { return Vec::new(); }
        assert!(offsets[0] == 0 && offsets.windows(2).all(|w| w[0] <= w[1]) && *offsets.last().unwrap() == points.len() as u64);
        let (rows, s, p) = (offsets.len() - 1, put_scalars(scalars), put_points(points));
        let mut out = vec![0u8; 64 * rows];
        assert_eq!(unsafe { jj_msm_ragged(self.0, rows, offsets.as_ptr(), s.as_ptr() as _, p.as_ptr() as _, out.as_mut_ptr() as _) }, 0);
        out.chunks_exact(64).map(|r| get_point(r).into()).collect()
    }

    /// `AffinePoint::batch_from_bytes` (src/lib.rs:541-627); `flags`: ZIP216 (from_bytes vs from_bytes_pre_zip216_compatibility,
    /// src/lib.rs:469-489), TORSION_FREE (SubgroupPoint::from_bytes, 1427-1429), NOT_SMALL_ORDER (699-705), CLEAR_COFACTOR (722-724).
    pub fn batch_from_bytes(&self, enc: &[[u8; 32]], flags: u32) -> Vec<Option<AffinePoint>> {
        let n = enc.len();
        let (mut out, mut ok) = (vec![0u8; 64 * n], vec![0u8; n]);                // `enc` is already the wire format: passed as it is
        assert_eq!(unsafe { jj_decompress(self.0, n, enc.as_ptr() as _, flags, out.as_mut_ptr() as _, ok.as_mut_ptr()) }, 0);
        (0..n).map(|i| if ok[i] == 1 { Some(get_point(&out[64 * i..64 * i + 64])) } else { None }).collect()   // CtOption -> Option
    }

    /// `SubgroupPoint::from_bytes` for a whole vector (decode + `[r]P == O`, src/lib.rs:1427-1429).
    pub fn subgroup_points_from_bytes(&self, enc: &[[u8; 32]]) -> Vec<Option<SubgroupPoint>> {
        self.batch_from_bytes(enc, ZIP216 | TORSION_FREE).into_iter()
            .map(|p| p.map(|a| ExtendedPoint::from(a).into_subgroup().unwrap())).collect()   // the check already ran on the GPU
    }

    /// `AffinePoint::to_bytes` for a whole vector (src/lib.rs:455-464).
    pub fn to_bytes_batch(&self, points: &[AffinePoint]) -> Vec<[u8; 32]> {
        let (n, p) = (points.len(), put_points(points));
        let mut out = vec![[0u8; 32]; n];
        assert_eq!(unsafe { jj_compress(self.0, n, p.as_ptr() as _, out.as_mut_ptr() as _) }, 0);
        out
    }

    /// `ExtendedPoint::batch_normalize` (src/lib.rs:1084-1107).  NOT BOUND to `jj_batch_normalize` from outside the crate:
    /// `ExtendedPoint`'s five coordinates are private (src/lib.rs:138-145) and the crate exposes no accessor, so a shim that lives
    /// next to the crate cannot hand (U, V, Z, T1, T2) to the GPU; it falls back to the crate's own per-point `to_affine()`.
    /// Inside the crate (a `pub(crate)` accessor, three lines) the entry point takes the 160-byte `(U,V,Z,T1,T2)` records as they are;
    /// that binding is exercised by the C++ mirror (`batch_normalize` in include/jubjub_hip.hpp) and the Python one, not from Rust.
    pub fn batch_normalize(&self, pts: &[ExtendedPoint]) -> Vec<AffinePoint> {
        pts.iter().map(|p| p.to_affine()).collect()
    }

    /// MSM with the host tail of one call overlapping the kernels of the next: `begin` queues the device work, `finish` waits for
    /// that job only (iterator `Sum` of `p * k`, src/lib.rs:183-193 + 873-879).
    pub fn msm_begin(&self, scalars: &[Fr], points: &[AffinePoint]) -> MsmJob {
        assert_eq!(scalars.len(), points.len());
        let (s, p) = (put_scalars(scalars), put_points(points));
        let mut job: *mut JjMsmJob = std::ptr::null_mut();
        assert_eq!(unsafe { jj_msm_begin(self.0, scalars.len(), s.as_ptr() as _, p.as_ptr() as _, &mut job) }, 0);
        MsmJob { job, _keep: (s, p) }                       // host arrays are staged at begin; kept alive until finish anyway
    }
    /// Batch verification of `n` Schnorr signatures as one MSM job (`jj_sigbatch_begin`): `r`, `a` compressed points, `s` responses,
    /// `c` raw challenges (reduced mod r by the library), `z` the caller's 128-bit random weights.  `msm_finish` returns
    /// `[8] (sum [z_i] R_i + sum [z_i c_i] A_i - [sum z_i s_i] B)`: the identity when every signature passes the cofactored check, `(0, -1)`
    /// for malformed input, any other point when one fails.  Variable-time; everything is public.
    pub fn sigbatch_begin(&self, base: &AffinePoint, r: &[[u8; 32]], a: &[[u8; 32]], s: &[Fr], c: &[[u8; 32]], z: &[[u8; 16]], zip216: bool) -> MsmJob {
        let n = r.len();
        assert!(a.len() == n && s.len() == n && c.len() == n && z.len() == n);
        let (b, ss) = (put_points(std::slice::from_ref(base)), put_scalars(s));
        let mut job: *mut JjMsmJob = std::ptr::null_mut();
        assert_eq!(unsafe { jj_sigbatch_begin(self.0, b.as_ptr() as _, n, r.as_ptr() as _, a.as_ptr() as _, ss.as_ptr() as _, c.as_ptr() as _, z.as_ptr() as _, if zip216 { 1 } else { 0 }, &mut job) }, 0);
        MsmJob { job, _keep: (b, ss) }                      // host arrays are staged at begin
    }
    /// The same check for signatures grouped by key (`jj_sigbatch_keyed_begin`): `keys` the `K` compressed verification keys, `offsets` the
    /// `K + 1` CSR offsets (`offsets[0] = 0`, non-decreasing, `offsets[K] = n`); signatures `offsets[k] .. offsets[k+1]` of `r`, `s`, `c`, `z` are
    /// checked under `keys[k]`.  The terms of equal keys are folded: `n + K + 1` MSM terms and `n + K` decodes.  `msm_finish` returns the same
    /// point as `sigbatch_begin` on the expanded arrays whenever every key has a signature.  Variable-time; everything is public.
    pub fn sigbatch_keyed_begin(&self, base: &AffinePoint, keys: &[[u8; 32]], offsets: &[u64], r: &[[u8; 32]], s: &[Fr], c: &[[u8; 32]], z: &[[u8; 16]], zip216: bool) -> MsmJob {
        let n = r.len();
        assert!(offsets.len() == keys.len() + 1 && offsets[keys.len()] as usize == n && s.len() == n && c.len() == n && z.len() == n);
        let (b, ss) = (put_points(std::slice::from_ref(base)), put_scalars(s));
        let mut job: *mut JjMsmJob = std::ptr::null_mut();
        assert_eq!(unsafe { jj_sigbatch_keyed_begin(self.0, b.as_ptr() as _, keys.len(), keys.as_ptr() as _, offsets.as_ptr(), r.as_ptr() as _, ss.as_ptr() as _, c.as_ptr() as _, z.as_ptr() as _, if zip216 { 1 } else { 0 }, &mut job) }, 0);
        MsmJob { job, _keep: (b, ss) }                      // host arrays and the offsets are staged at begin
    }
    /// One batch check per run of one signature array (`jj_sigbatch_ragged`): segment `g` holds signatures `offsets[g] .. offsets[g+1]`
    /// (`offsets[0] = 0`, non-decreasing, the last one `n`); row `g` is the point `sigbatch_begin` + `msm_finish` give for that segment alone:
    /// the identity to accept (also an empty segment), `(0, -1)` for a malformed unit in it, any other point a failing signature.
    /// Variable-time; everything is public.
    pub fn sigbatch_ragged(&self, base: &AffinePoint, offsets: &[u64], r: &[[u8; 32]], a: &[[u8; 32]], s: &[Fr], c: &[[u8; 32]], z: &[[u8; 16]], zip216: bool) -> Vec<AffinePoint> {
        let n = r.len();
        if offsets.is_empty() { assert_eq!(n, 0); return Vec::new(); }
        assert!(*offsets.last().unwrap() as usize == n && a.len() == n && s.len() == n && c.len() == n && z.len() == n);
        let (rows, b, ss) = (offsets.len() - 1, put_points(std::slice::from_ref(base)), put_scalars(s));
        let mut out = vec![0u8; 64 * rows];
        assert_eq!(unsafe { jj_sigbatch_ragged(self.0, b.as_ptr() as _, rows, offsets.as_ptr(), r.as_ptr() as _, a.as_ptr() as _, ss.as_ptr() as _, c.as_ptr() as _, z.as_ptr() as _, if zip216 { 1 } else { 0 }, out.as_mut_ptr() as _) }, 0);
        out.chunks_exact(64).map(get_point).collect()
    }
    /// One verdict per signature in one call (`jj_sigverify_each`): `1` iff `[8]([s]B - [c]A - R) = O`, `B` the base of `g` -- the cofactored
    /// equation of every `sigbatch_*` call; `cofactored = false`: iff `[s]B - [c]A - R = O` --, `2` for an `R` or `A` that does not decode,
    /// else `0` (`s` is an `Fr`, so it is in range).  Variable-time; everything is public.
    pub fn sigverify_each(&self, g: &FixedBase, r: &[[u8; 32]], a: &[[u8; 32]], s: &[Fr], c: &[[u8; 32]], zip216: bool, cofactored: bool) -> Vec<u8> {
        let n = r.len();
        assert!(a.len() == n && s.len() == n && c.len() == n);
        let ss = put_scalars(s);
        let mut out = vec![0u8; n];
        let flags = (if zip216 { 1 } else { 0 }) | (if cofactored { 0 } else { 16 });
        assert_eq!(unsafe { jj_sigverify_each(self.0, g.t, n, r.as_ptr() as _, a.as_ptr() as _, ss.as_ptr() as _, c.as_ptr() as _, flags, out.as_mut_ptr()) }, 0);
        out
    }
    /// The challenges of the signature family, hashed on the device (`jj_sig_challenge`):
    /// `c_i = Fr::from_bytes_wide(BLAKE2b-512(personal; r_i || a_i || msgs[i]))` as canonical bytes.  `r` / `a`: `None` leaves that part out of the
    /// hash; `personal`: `None` is sixteen zero bytes (RedJubjub: `b"Zcash_RedJubjubH"`).  The messages are packed here and may differ in length.
    pub fn sig_challenge(&self, personal: Option<&[u8; 16]>, r: Option<&[[u8; 32]]>, a: Option<&[[u8; 32]]>, msgs: &[&[u8]]) -> Vec<[u8; 32]> {
        let n = msgs.len();
        assert!(r.map_or(true, |x| x.len() == n) && a.map_or(true, |x| x.len() == n));
        let mut offsets = vec![0u64; n + 1];
        for (i, m) in msgs.iter().enumerate() { offsets[i + 1] = offsets[i] + m.len() as u64; }
        let flat: Vec<u8> = msgs.concat();
        let mut out = vec![[0u8; 32]; n];
        let ptr = |x: Option<&[[u8; 32]]>| x.map_or(std::ptr::null(), |v| v.as_ptr() as *const c_void);
        assert_eq!(unsafe { jj_sig_challenge(self.0, n, personal.map_or(std::ptr::null(), |p| p.as_ptr() as *const c_void), ptr(r), ptr(a), flat.as_ptr() as _, 0, offsets.as_ptr(), out.as_mut_ptr() as _) }, 0);
        out
    }
    /// Key agreement with ONE secret scalar and its KDF (`jj_ka_kdf`): `keys[i] = BLAKE2b-256(personal; to_bytes(share_i) [|| p[i]])` with
    /// `share_i = [sk]P_i` or `[8]([sk]P_i)`; `flags`: the decoder's bits 1 | 2 | 4, 32 = cofactor, 64 = hash the encoding too.  `ok[i] == 0` and a
    /// zero key where `p[i]` does not decode.  Constant-time in `sk` and in the shares.  `personal`: `None` is sixteen zero bytes (the Sapling
    /// recipient: `b"Zcash_SaplingKDF"` with flags 1 | 32 | 64).
    pub fn ka_kdf(&self, sk: &[u8; 32], p: &[[u8; 32]], flags: u32, personal: Option<&[u8; 16]>) -> (Vec<[u8; 32]>, Vec<u8>) {
        let n = p.len();
        let mut keys = vec![[0u8; 32]; n];
        let mut ok = vec![0u8; n];
        assert_eq!(unsafe { jj_ka_kdf(self.0, n, sk.as_ptr() as _, p.as_ptr() as _, flags, personal.map_or(std::ptr::null(), |x| x.as_ptr() as *const c_void), keys.as_mut_ptr() as _, ok.as_mut_ptr()) }, 0);
        (keys, ok)
    }
    /// The same with one secret scalar PER ROW (`jj_ka_kdf_each`: the sender's side of a note): `sk[i]` is read as `jj_varbase_mul` reads a
    /// scalar; with flag 64 the second hashed part is `hash_input[i]` when `hash_input` is given and `p[i]` when it is `None`.  Constant-time in
    /// the scalars and in the shares.
    pub fn ka_kdf_each(&self, sk: &[[u8; 32]], p: &[[u8; 32]], hash_input: Option<&[[u8; 32]]>, flags: u32, personal: Option<&[u8; 16]>) -> (Vec<[u8; 32]>, Vec<u8>) {
        let n = p.len();
        assert!(sk.len() == n && hash_input.map_or(true, |h| h.len() == n));
        let mut keys = vec![[0u8; 32]; n];
        let mut ok = vec![0u8; n];
        assert_eq!(unsafe { jj_ka_kdf_each(self.0, n, sk.as_ptr() as _, p.as_ptr() as _, hash_input.map_or(std::ptr::null(), |h| h.as_ptr() as *const c_void), flags, personal.map_or(std::ptr::null(), |x| x.as_ptr() as *const c_void), keys.as_mut_ptr() as _, ok.as_mut_ptr()) }, 0);
        (keys, ok)
    }
    /// Raw BLAKE2b digests over rows gathered from up to four arrays (`jj_blake2b`): `out[i] = BLAKE2b-digest_len(personal; prefix || S_0[i] || ..)`,
    /// `S_s[i]` the `lens[s]` bytes at byte `i * strides[s]` of `sources[s]`; `digest_len` 32 or 64; lengths, strides and the prefix's length
    /// multiples of 4.  Returns `n x digest_len` bytes, dense.  `personal`: `None` is sixteen zero bytes.  The library knows no protocol
    /// (Sapling's ock: `digest_len` 32, `prefix` = ovk, the sources cv, cmu, epk).
    pub fn blake2b(&self, n: usize, digest_len: c_int, personal: Option<&[u8; 16]>, prefix: &[u8], sources: &[&[u8]], lens: &[usize], strides: &[usize]) -> Vec<u8> {
        assert!(sources.len() == lens.len() && sources.len() == strides.len() && sources.len() <= 4 && (digest_len == 32 || digest_len == 64));
        assert!(n == 0 || sources.iter().zip(lens.iter().zip(strides)).all(|(s, (l, st))| st >= l && s.len() >= (n - 1) * st + l));
        let ptrs: Vec<*const c_void> = sources.iter().map(|s| s.as_ptr() as *const c_void).collect();
        let mut out = vec![0u8; n * digest_len as usize];
        assert_eq!(unsafe { jj_blake2b(self.0, n, digest_len, personal.map_or(std::ptr::null(), |x| x.as_ptr() as *const c_void), if prefix.is_empty() { std::ptr::null() } else { prefix.as_ptr() as _ }, prefix.len(), sources.len() as c_int, ptrs.as_ptr(), lens.as_ptr(), strides.as_ptr(), out.as_mut_ptr() as _) }, 0);
        out
    }
    /// One RFC 8439 ChaCha20 key per row (`jj_chacha20_xor`): rows of `len` bytes at a stride of `in_stride` in `input`, a dense `n x len` result;
    /// `len` and `in_stride` multiples of 4, `len` in 4..=1024; `nonce`: `None` is twelve zero bytes.
    pub fn chacha20_xor(&self, keys: &[[u8; 32]], nonce: Option<&[u8; 12]>, counter: u32, input: &[u8], len: usize, in_stride: usize) -> Vec<u8> {
        let n = keys.len();
        assert!(n == 0 || input.len() >= (n - 1) * in_stride + len);
        let mut out = vec![0u8; n * len];
        assert_eq!(unsafe { jj_chacha20_xor(self.0, n, keys.as_ptr() as _, nonce.map_or(std::ptr::null(), |x| x.as_ptr() as *const c_void), counter, input.as_ptr() as _, len, in_stride, out.as_mut_ptr() as _) }, 0);
        out
    }
    /// One Poly1305 one-time key per row (`jj_poly1305`; `r` in key bytes 0..16, `s` in bytes 16..32): the tags of rows of `len` bytes at a
    /// stride of `in_stride` in `input`, `n x 16` bytes, dense; `len` and `in_stride` multiples of 4, `len` in 4..=1024.
    pub fn poly1305(&self, keys: &[[u8; 32]], input: &[u8], len: usize, in_stride: usize) -> Vec<[u8; 16]> {
        let n = keys.len();
        assert!(n == 0 || input.len() >= (n - 1) * in_stride + len);
        let mut out = vec![[0u8; 16]; n];
        assert_eq!(unsafe { jj_poly1305(self.0, n, keys.as_ptr() as _, input.as_ptr() as _, len, in_stride, out.as_mut_ptr() as _) }, 0);
        out
    }
    /// RFC 8439 ChaCha20-Poly1305 with one key per row, the tag checked on the device (`jj_aead_open`): a row of `input` is `len` ciphertext
    /// bytes and the 16 tag bytes; returns the dense `n x len` plaintext and `ok`, with `ok[i] == 0` and a zero row where the tag does not
    /// verify.  One `nonce` (`None`: twelve zero bytes) and one `aad` (at most 64 bytes) for all rows.
    pub fn aead_open(&self, keys: &[[u8; 32]], nonce: Option<&[u8; 12]>, aad: &[u8], input: &[u8], len: usize, in_stride: usize) -> (Vec<u8>, Vec<u8>) {
        let n = keys.len();
        assert!(n == 0 || input.len() >= (n - 1) * in_stride + len + 16);
        let mut out = vec![0u8; n * len];
        let mut ok = vec![0u8; n];
        assert_eq!(unsafe { jj_aead_open(self.0, n, keys.as_ptr() as _, nonce.map_or(std::ptr::null(), |x| x.as_ptr() as *const c_void), if aad.is_empty() { std::ptr::null() } else { aad.as_ptr() as _ }, aad.len(), input.as_ptr() as _, len, in_stride, out.as_mut_ptr() as _, ok.as_mut_ptr()) }, 0);
        (out, ok)
    }
    /// The sealing direction (`jj_aead_seal`): `n x (len + 16)` bytes, each row its ciphertext followed by its tag.
    pub fn aead_seal(&self, keys: &[[u8; 32]], nonce: Option<&[u8; 12]>, aad: &[u8], input: &[u8], len: usize, in_stride: usize) -> Vec<u8> {
        let n = keys.len();
        assert!(n == 0 || input.len() >= (n - 1) * in_stride + len);
        let mut out = vec![0u8; n * (len + 16)];
        assert_eq!(unsafe { jj_aead_seal(self.0, n, keys.as_ptr() as _, nonce.map_or(std::ptr::null(), |x| x.as_ptr() as *const c_void), if aad.is_empty() { std::ptr::null() } else { aad.as_ptr() as _ }, aad.len(), input.as_ptr() as _, len, in_stride, out.as_mut_ptr() as _) }, 0);
        out
    }
    /// `BLAKE2s-256(personal; prefix || M_i)` for `n` messages of `msg_len` bytes, `msg_stride` apart in `msgs` (`jj_blake2s`); `personal`:
    /// `None` is eight zero bytes.  The library knows no protocol's personalisation or prefix: both are the caller's.
    pub fn blake2s(&self, n: usize, personal: Option<&[u8; 8]>, prefix: &[u8], msgs: &[u8], msg_len: usize, msg_stride: usize) -> Vec<[u8; 32]> {
        assert!(n == 0 || msg_len == 0 || (msg_stride >= msg_len && msgs.len() >= (n - 1) * msg_stride + msg_len));
        let mut out = vec![[0u8; 32]; n];
        assert_eq!(unsafe { jj_blake2s(self.0, n, personal.map_or(std::ptr::null(), |x| x.as_ptr() as *const c_void), if prefix.is_empty() { std::ptr::null() } else { prefix.as_ptr() as _ }, prefix.len(), if msgs.is_empty() { std::ptr::null() } else { msgs.as_ptr() as _ }, msg_len, msg_stride, out.as_mut_ptr() as _) }, 0);
        out
    }
    /// Hash to the curve (`jj_group_hash`): the digest of `blake2s` decoded exactly as `jj_decompress` decodes it under `flags` (the decoder's
    /// bits 1 | 2 | 4 | 8; 1 | 4 | 8 is `[8] * decode(digest)` with small order refused).  `ok[i] == 0` and 64 zero bytes where the digest is refused.
    pub fn group_hash(&self, n: usize, personal: Option<&[u8; 8]>, prefix: &[u8], msgs: &[u8], msg_len: usize, msg_stride: usize, flags: u32) -> (Vec<[u8; 64]>, Vec<u8>) {
        assert!(n == 0 || msg_len == 0 || (msg_stride >= msg_len && msgs.len() >= (n - 1) * msg_stride + msg_len));
        let mut pts = vec![[0u8; 64]; n];
        let mut ok = vec![0u8; n];
        assert_eq!(unsafe { jj_group_hash(self.0, n, personal.map_or(std::ptr::null(), |x| x.as_ptr() as *const c_void), if prefix.is_empty() { std::ptr::null() } else { prefix.as_ptr() as _ }, prefix.len(), if msgs.is_empty() { std::ptr::null() } else { msgs.as_ptr() as _ }, msg_len, msg_stride, flags, pts.as_mut_ptr() as _, ok.as_mut_ptr()) }, 0);
        (pts, ok)
    }
    pub fn msm_finish(&self, j: MsmJob) -> AffinePoint {
        let mut out = [0u8; 64];
        assert_eq!(unsafe { jj_msm_finish(j.job, out.as_mut_ptr() as _) }, 0);
        get_point(&out)
    }

    /// The same product for PUBLIC scalars only (verification keys, public randomisers): the variable-time ladder, whose per-lane window
    /// table is read at digit-dependent addresses -- ~1.6 % faster.  Not a drop-in for `Mul<Fr>` (the reference's `multiply` is constant-time,
    /// src/lib.rs:357-379); it stands where a caller would reach for the group crate's `Wnaf`, which is variable-time by design.
    pub fn multiply_batch_vartime(&self, scalars: &[Fr], points: &[AffinePoint]) -> Vec<AffinePoint> {
        assert_eq!(scalars.len(), points.len());
        let (n, s, p) = (scalars.len(), put_scalars(scalars), put_points(points));
        let mut out = vec![0u8; 64 * n];
        assert_eq!(unsafe { jj_varbase_mul_vartime(self.0, n, s.as_ptr() as _, p.as_ptr() as _, out.as_mut_ptr() as _) }, 0);
        (0..n).map(|i| get_point(&out[64 * i..64 * i + 64])).collect()
    }

    /// `p[i] * a[i] + q[i] * b[i]` for PUBLIC scalars (the two-term combination of a verifier equation) in one interleaved ladder per unit
    /// (`jj_varbase_mul2_vartime`): the same points as `multiply_batch_vartime` twice and a sum, variable-time like it.
    pub fn multiply2_batch_vartime(&self, a: &[Fr], p: &[AffinePoint], b: &[Fr], q: &[AffinePoint]) -> Vec<AffinePoint> {
        assert!(a.len() == p.len() && b.len() == q.len() && a.len() == b.len());
        let (n, sa, pp, sb, pq) = (a.len(), put_scalars(a), put_points(p), put_scalars(b), put_points(q));
        let mut out = vec![0u8; 64 * n];
        assert_eq!(unsafe { jj_varbase_mul2_vartime(self.0, n, sa.as_ptr() as _, pp.as_ptr() as _, sb.as_ptr() as _, pq.as_ptr() as _, out.as_mut_ptr() as _) }, 0);
        out.chunks_exact(64).map(get_point).collect()
    }

    /// `g * a[i] + q[i] * b[i]` for PUBLIC scalars, `g` the base of a `FixedBase` (`[s]G - [c]A` of a Schnorr / RedJubjub check with `A` negated
    /// by the caller) (`jj_fixedvar_mul_vartime`): the same points as `FixedBase::mul_batch`, `multiply_batch_vartime` and a sum, variable-time.
    pub fn fixedvar_mul_vartime(&self, g: &FixedBase, a: &[Fr], b: &[Fr], q: &[AffinePoint]) -> Vec<AffinePoint> {
        assert!(a.len() == b.len() && b.len() == q.len());
        let (n, sa, sb, pq) = (a.len(), put_scalars(a), put_scalars(b), put_points(q));
        let mut out = vec![0u8; 64 * n];
        assert_eq!(unsafe { jj_fixedvar_mul_vartime(self.0, g.t, n, sa.as_ptr() as _, sb.as_ptr() as _, pq.as_ptr() as _, out.as_mut_ptr() as _) }, 0);
        out.chunks_exact(64).map(get_point).collect()
    }

    /// `is_torsion_free` (src/lib.rs:709-711) for a whole vector.
    pub fn is_torsion_free_batch(&self, points: &[AffinePoint]) -> Vec<bool> {
        let (n, p) = (points.len(), put_points(points));
        let mut out = vec![0u8; n];
        assert_eq!(unsafe { jj_is_torsion_free(self.0, n, p.as_ptr() as _, out.as_mut_ptr()) }, 0);
        out.into_iter().map(|b| b == 1).collect()
    }

    /// `PrimeFieldBits::to_le_bits` (src/fr.rs:746-773) for a whole vector: 256 bits (one byte each) per scalar.
    pub fn to_le_bits_batch(&self, scalars: &[Fr]) -> Vec<[u8; 256]> {
        let (n, s) = (scalars.len(), put_scalars(scalars));
        let mut out = vec![[0u8; 256]; n];
        assert_eq!(unsafe { jj_fr_to_le_bits(self.0, n, s.as_ptr() as _, out.as_mut_ptr() as _) }, 0);
        out
    }
}
impl Drop for Gpu { fn drop(&mut self) { unsafe { jj_ctx_destroy(self.0); } } }

/// `AffineNielsPoint * Fr` / `multiply_bits` (src/lib.rs:272-310) for one fixed base: the table lives on the device.
pub struct FixedBase<'a> { gpu: &'a Gpu, t: *mut JjTable }
impl<'a> FixedBase<'a> {
    pub fn new(gpu: &'a Gpu, base: &AffinePoint) -> Self {
        let (b, mut t) = (put_points(std::slice::from_ref(base)), std::ptr::null_mut());
        assert_eq!(unsafe { jj_fixedbase_table_create(gpu.0, b.as_ptr() as _, 0, &mut t) }, 0);   // 0: LDS table, constant-time select
        FixedBase { gpu, t }
    }
    pub fn mul_batch(&self, scalars: &[Fr]) -> Vec<AffinePoint> {
        let (n, s) = (scalars.len(), put_scalars(scalars));
        let mut out = vec![0u8; 64 * n];
        assert_eq!(unsafe { jj_fixedbase_mul(self.gpu.0, self.t, n, s.as_ptr() as _, out.as_mut_ptr() as _) }, 0);
        out.chunks_exact(64).map(get_point).collect()
    }
}
impl Drop for FixedBase<'_> { fn drop(&mut self) { unsafe { jj_fixedbase_table_destroy(self.gpu.0, self.t); } } }

/// Windowed Pedersen hashes (`jj_pedersen_*`; the function and its arguments: include/jubjub_hip.h).  VARIABLE-TIME: public inputs.
pub struct PedersenTable<'a> { gpu: &'a Gpu, t: *mut JjTable, nseg: c_int, seg_chunks: c_int }
impl<'a> PedersenTable<'a> {
    /// `gens`: 1..=8 generators, each on the curve and torsion-free; `window_chunks` 0 = the default
    pub fn new(gpu: &'a Gpu, gens: &[AffinePoint], seg_chunks: c_int, window_chunks: c_int) -> Option<Self> {
        let (g, mut t) = (put_points(gens), std::ptr::null_mut());
        if unsafe { jj_pedersen_table_create(gpu.0, gens.len() as c_int, g.as_ptr() as _, seg_chunks, window_chunks, &mut t) } != 0 { return None; }
        Some(PedersenTable { gpu, t, nseg: gens.len() as c_int, seg_chunks })
    }
    /// One message per `row_stride` bytes of `rows`: `prefix_bits` bits of `prefix`, then the `fields` (byte_offset, nbits) -> canonical u-coordinates.
    /// A Merkle layer over node u-coordinates: `hash(nodes, 64, &[[0, 255], [32, 255]], layer, 6)`.
    pub fn hash(&self, rows: &[u8], row_stride: usize, fields: &[[u32; 2]], prefix: u32, prefix_bits: c_int) -> Vec<[u8; 32]> {
        let n = if row_stride == 0 { 0 } else { rows.len() / row_stride };
        let mut out = vec![[0u8; 32]; n];
        assert_eq!(unsafe { jj_pedersen_hash_vartime(self.gpu.0, self.t, n, prefix, prefix_bits, rows.as_ptr() as _, row_stride, fields.len() as c_int, fields.as_ptr() as *const u32, 0, out.as_mut_ptr() as _) }, 0);
        out
    }
    /// `<M_j> mod r`, segment-major (nseg x n): what `jj_fixedbase_multi_mul` reads -- the route for secret inputs, over the constant-time LDS tables
    pub fn scalars(&self, rows: &[u8], row_stride: usize, fields: &[[u32; 2]], prefix: u32, prefix_bits: c_int) -> Vec<[u8; 32]> {
        let n = if row_stride == 0 { 0 } else { rows.len() / row_stride };
        let mut out = vec![[0u8; 32]; n * self.nseg as usize];
        assert_eq!(unsafe { jj_pedersen_scalars(self.gpu.0, self.nseg, self.seg_chunks, n, prefix, prefix_bits, rows.as_ptr() as _, row_stride, fields.len() as c_int, fields.as_ptr() as *const u32, out.as_mut_ptr() as _) }, 0);
        out
    }
    /// `H(M) + [r] R` per unit (`jj_pedersen_commit_vartime`): the message's `fields` (src, byte_offset, nbits) lie in up to four row arrays,
    /// `sources[s]` holding n rows of `strides[s]` bytes; R is the base of `rbase`, `r` one 32-byte scalar per unit (n = r.len()).  `rbase` None
    /// with an empty `r`: the plain multi-source hash of `n` units.  -> canonical u-coordinates.  VARIABLE-TIME in the message; r is
    /// constant-time with an LDS table (`FixedBase`'s default).
    pub fn commit(&self, rbase: Option<&FixedBase>, sources: &[&[u8]], strides: &[usize], fields: &[[u32; 3]], r: &[[u8; 32]], n: usize, prefix: u32, prefix_bits: c_int) -> Vec<[u8; 32]> {
        let n = if rbase.is_some() { r.len() } else { n };
        assert!(sources.len() == strides.len() && sources.len() <= 4 && (rbase.is_some() || r.is_empty()));
        assert!(sources.iter().zip(strides).all(|(s, st)| s.len() >= n * st));
        let ptrs: Vec<*const c_void> = sources.iter().map(|s| s.as_ptr() as *const c_void).collect();
        let mut out = vec![[0u8; 32]; n];
        let (tab, rp) = match rbase { Some(b) => (b.t as *const JjTable, r.as_ptr() as *const c_void), None => (std::ptr::null(), std::ptr::null()) };
        assert_eq!(unsafe { jj_pedersen_commit_vartime(self.gpu.0, self.t, tab, n, prefix, prefix_bits, sources.len() as c_int, ptrs.as_ptr(), strides.as_ptr(), fields.len() as c_int,
                                                       fields.as_ptr() as *const u32, rp, 0, out.as_mut_ptr() as _) }, 0);
        out
    }
}
impl Drop for PedersenTable<'_> { fn drop(&mut self) { unsafe { jj_fixedbase_table_destroy(self.gpu.0, self.t); } } }

/// Many scalar vectors against ONE set of points (`jj_msm_basis_*`): the points go to the device once, every call brings scalars only.
pub struct MsmBasis<'a> { gpu: &'a Gpu, b: *mut JjMsmBasis, n: usize }
impl<'a> MsmBasis<'a> {
    /// mode 0 = auto, 1 = points, 2 = windows; windows 0 = auto or 16..=36 (include/jubjub_hip.h)
    pub fn new(gpu: &'a Gpu, points: &[AffinePoint], mode: c_int, windows: c_int) -> Self {
        let (p, mut b) = (put_points(points), std::ptr::null_mut());
        assert_eq!(unsafe { jj_msm_basis_create(gpu.0, points.len(), p.as_ptr() as _, mode, windows, &mut b) }, 0);
        MsmBasis { gpu, b, n: points.len() }
    }
    pub fn len(&self) -> usize { self.n }
    pub fn is_empty(&self) -> bool { self.n == 0 }
    /// `sum_i points[i] * scalars[i]` over the first `scalars.len()` points of the basis
    pub fn msm(&self, scalars: &[Fr]) -> ExtendedPoint {
        assert!(scalars.len() <= self.n);
        let s = put_scalars(scalars);
        let mut out = [0u8; 64];
        assert_eq!(unsafe { jj_msm_basis_mul(self.gpu.0, self.b, 1, scalars.len(), s.as_ptr() as _, out.as_mut_ptr() as _) }, 0);
        get_point(&out).into()
    }
    /// one sum per row; every row has the same length `m <= len()`
    pub fn msm_rows(&self, rows: &[Vec<Fr>]) -> Vec<ExtendedPoint> {
        let m = rows.first().map_or(0, |r| r.len());
        assert!(m <= self.n && rows.iter().all(|r| r.len() == m));
        let flat: Vec<Fr> = rows.iter().flatten().copied().collect();
        let s = put_scalars(&flat);
        let mut out = vec![0u8; 64 * rows.len()];
        assert_eq!(unsafe { jj_msm_basis_mul(self.gpu.0, self.b, rows.len(), m, s.as_ptr() as _, out.as_mut_ptr() as _) }, 0);
        out.chunks_exact(64).map(|c| get_point(c).into()).collect()
    }
}
impl Drop for MsmBasis<'_> { fn drop(&mut self) { unsafe { jj_msm_basis_destroy(self.gpu.0, self.b); } } }

/// All GPUs of the node from one process: contiguous shards, one host thread and stream per device.
pub struct Node(*mut JjMulti);
impl Node {
    pub fn new(devices: &[i32]) -> Option<Self> {
        let mut p = std::ptr::null_mut();
        if unsafe { jj_multi_create(devices.as_ptr(), devices.len() as c_int, &mut p) } == 0 { Some(Node(p)) } else { None }
    }
    pub fn mul_batch(&self, points: &[AffinePoint], scalars: &[Fr]) -> Vec<AffinePoint> {
        let (n, s, p) = (points.len(), put_scalars(scalars), put_points(points));
        let mut out = vec![0u8; 64 * n];
        assert_eq!(unsafe { jj_multi_varbase_mul(self.0, n, s.as_ptr() as _, p.as_ptr() as _, out.as_mut_ptr() as _) }, 0);
        out.chunks_exact(64).map(get_point).collect()
    }
    pub fn msm(&self, points: &[AffinePoint], scalars: &[Fr]) -> ExtendedPoint {
        let (n, s, p) = (points.len(), put_scalars(scalars), put_points(points));
        let mut out = [0u8; 64];
        assert_eq!(unsafe { jj_multi_msm(self.0, n, s.as_ptr() as _, p.as_ptr() as _, out.as_mut_ptr() as _) }, 0);
        get_point(&out).into()
    }
}
impl Drop for Node { fn drop(&mut self) { unsafe { jj_multi_destroy(self.0); } } }

/// One process per GPU (the layout `north_star` names): this rank's terms stay resident on its GPU, the records of window sums
/// (8256 bytes per rank) are all-gathered over RCCL / xGMI and every rank runs one host tail.  The application owns the communicator:
/// `comm` is an `ncclComm_t` it made with `ncclCommInitRank` (e.g. through an `rccl-sys` binding; the ncclUniqueId travels over
/// whatever rendezvous the application has -- examples/msm_rccl.cpp uses a file), `all_gather` the address of that library's
/// `ncclAllGather` (or null: looked up in the process, then in librccl.so.1).  examples/msm_rccl.cpp is this sequence in C++, built and
/// run by tests/test_gpu_host_path.py.
impl Gpu {
    pub fn set_comm(&self, comm: *mut c_void, rank: i32, nranks: i32, all_gather: *mut c_void) {
        assert_eq!(unsafe { jj_ctx_set_comm(self.0, comm, rank, nranks, all_gather) }, 0);
    }
    /// every rank passes ITS terms (partition 0) and gets the same sum; a collective: all ranks call it, in the same order
    pub fn msm_all_ranks(&self, my_points: &[AffinePoint], my_scalars: &[Fr]) -> ExtendedPoint {
        let (n, s, p) = (my_points.len(), put_scalars(my_scalars), put_points(my_points));
        let mut out = [0u8; 64];
        assert_eq!(unsafe { jj_msm_allgather(self.0, n, s.as_ptr() as _, p.as_ptr() as _, 0, out.as_mut_ptr() as _) }, 0);
        get_point(&out).into()
    }
    /// the same in two halves for a stream of sums (`msm_finish` above takes the job): with 2-4 jobs in flight the gather, the fold
    /// and the host tail of one sum run beside the kernels of the next; every rank begins the same jobs in the same order
    pub fn msm_all_ranks_begin(&self, my_points: &[AffinePoint], my_scalars: &[Fr]) -> MsmJob {
        let (n, s, p) = (my_points.len(), put_scalars(my_scalars), put_points(my_points));
        let mut job: *mut JjMsmJob = std::ptr::null_mut();
        assert_eq!(unsafe { jj_msm_allgather_begin(self.0, n, s.as_ptr() as _, p.as_ptr() as _, 0, &mut job) }, 0);
        MsmJob { job, _keep: (s, p) }
    }
}
