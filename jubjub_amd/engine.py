"""
Batched Jubjub engine: thin, typed Python front-end over the C ABI (include/jubjub_hip.h).

Arguments are arrays of wire-format bytes — numpy uint8 arrays (host; staged by the library) or torch uint8 CUDA
tensors (device; zero-copy, asynchronous on torch's current stream).  Results come back as the same kind.
Shapes: scalars / field elements (n, 32); affine points (n, 64); compressed points (n, 32).
"""
import ctypes as C
import functools
import threading

import numpy as np

from . import _lib

FLAG_ZIP216 = 1
FLAG_TORSION_FREE = 2
FLAG_NOT_SMALL_ORDER = 4
FLAG_CLEAR_COFACTOR = 8
FLAG_SIG_COFACTORLESS = 16     # jj_sigverify_each only
FLAG_PEDERSEN_POINT = 1        # jj_pedersen_hash_vartime only: 64 affine bytes per unit instead of the u-coordinate
SIG_REJECT, SIG_OK, SIG_MALFORMED = 0, 1, 2      # verdict bytes of jj_sigverify_each
REDJUBJUB_PERSONAL = b"Zcash_RedJubjubH"         # the personalisation of RedJubjub's challenge hash: the documented example of sig_challenge's `personal` (the C library does not contain it)
SAPLING_KDF_PERSONAL = b"Zcash_SaplingKDF"       # the personalisation of the Sapling KDF: the documented example of ka_kdf's `personal` (the C library does not contain it)
SAPLING_OCK_PERSONAL = b"Zcash_Derive_ock"       # the personalisation of Sapling's outgoing cipher key: the documented example of blake2b's `personal` in note_encrypt and ovk_open (the C library does not contain it)
FLAG_KA_COFACTOR = 32          # jj_ka_kdf only: share = [8]([sk]P)
FLAG_KA_HASH_INPUT = 64        # jj_ka_kdf only: hash share || encoding
KA_SAPLING_FLAGS = FLAG_ZIP216 | FLAG_KA_COFACTOR | FLAG_KA_HASH_INPUT      # the Sapling recipient's ka_kdf flags
SAPLING_GD_PERSONAL = b"Zcash_gd"                # the personalisation of Sapling's diversified base g_d: a documented example of group_hash's `personal` (the C library does not contain it)
SAPLING_PH_PERSONAL = b"Zcash_PH"                # the personalisation of Sapling's Pedersen-hash generators: the other example (the protocol's prefix, its URS, is the caller's to supply)
SAPLING_EXPAND_PERSONAL = b"Zcash_ExpandSeed"    # the personalisation of Sapling's PRF^expand: the documented example of note_check's `expand_personal` (the C library does not contain it)
SAPLING_NOTE_PREFIX, SAPLING_NOTE_PREFIX_BITS = 0b111111, 6      # the six one bits in front of a note commitment's message (note_commit)
GROUP_HASH_FLAGS = FLAG_ZIP216 | FLAG_NOT_SMALL_ORDER | FLAG_CLEAR_COFACTOR  # the group hash of the Zcash specification: decode, refuse small order, multiply by 8


class JubjubError(RuntimeError):
    pass


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _host_bytes(x):
    """A host argument as a contiguous uint8 array, never by a cast of its values: an array of another dtype is a TypeError (as for a torch
    tensor), bytes-like objects are taken as they are, a sequence of integers must hold byte values."""
    if isinstance(x, np.ndarray):
        if x.dtype != np.uint8:
            raise TypeError("numpy arguments must be uint8, got %s" % x.dtype)
        return np.ascontiguousarray(x)
    if isinstance(x, memoryview) and (x.itemsize != 1 or not x.c_contiguous):
        raise TypeError("a memoryview argument must be contiguous bytes, got format %r" % x.format)
    if isinstance(x, (bytes, bytearray, memoryview)):
        return np.frombuffer(x, dtype=np.uint8)
    a = np.asarray(x)
    if a.size == 0:
        return np.zeros(0, np.uint8)
    if a.dtype.kind not in "iu":
        raise TypeError("byte values (integers 0 ... 255) expected, got %s" % a.dtype)
    if (a < 0).any() or (a > 255).any():
        raise ValueError("byte values (integers 0 ... 255) expected")
    return np.ascontiguousarray(a, dtype=np.uint8)


class _Arg:
    """Normalises one array argument to (pointer, keepalive)."""

    def __init__(self, x, width):
        if _is_torch(x):
            import torch

            if x.dtype != torch.uint8:
                raise TypeError("torch arguments must be uint8")
            x = x.contiguous()
            if width is not None and x.numel() % width:
                raise ValueError("byte length %d is not a multiple of %d" % (x.numel(), width))
            self.n = x.numel() // width if width else x.numel()
            self.ptr = x.data_ptr()
            self.keep = x
            self.torch = True
            self.device = x.device
        else:
            a = _host_bytes(x)
            if width is not None and a.size % width:
                raise ValueError("byte length %d is not a multiple of %d" % (a.size, width))
            self.n = a.size // width if width else a.size
            self.ptr = a.ctypes.data if a.size else None
            self.keep = a
            self.torch = False
            self.device = None


def _msm_batch_shapes(scalars, points):
    """(B, n, points_shared) of jj_msm_batch's arguments: scalars (B, n, 32); points (n, 64) shared by every row or (B, n, 64)"""
    ss, ps = tuple(scalars.shape), tuple(points.shape)
    if len(ss) != 3 or ss[2] != 32:
        raise ValueError("scalars: shape (B, n, 32) expected, got %r" % (ss,))
    B, n = ss[0], ss[1]
    if ps == (n, 64):
        return B, n, 1
    if ps == (B, n, 64):
        return B, n, 0
    raise ValueError("points: shape (%d, 64) (shared) or (%d, %d, 64) expected, got %r" % (n, B, n, ps))


def _ragged_offsets(offsets):
    """offsets of jj_msm_ragged as a contiguous host uint64 array"""
    if _is_torch(offsets):
        offsets = offsets.cpu().numpy()
    o = np.asarray(offsets)
    if o.ndim != 1 or o.size == 0:
        raise ValueError("offsets: a sequence of S + 1 >= 1 integers expected")
    if o.dtype.kind not in "iu":
        raise ValueError("offsets: integers expected, got %s" % o.dtype)
    if o.dtype.kind == "i" and (o < 0).any():
        raise ValueError("offsets: negative value")
    o = np.ascontiguousarray(o, dtype=np.uint64)
    if o[0] != 0:
        raise ValueError("offsets[0] must be 0, got %d" % int(o[0]))
    if (o[1:] < o[:-1]).any():
        raise ValueError("offsets must be non-decreasing")
    return o


def _msm_ragged_shapes(scalars, points, offsets):
    """(S, N) of jj_msm_ragged's arguments: scalars (N, 32); points (N, 64); offsets: S + 1 integers, offsets[0] = 0, non-decreasing,
    offsets[-1] = N"""
    ss, ps = tuple(scalars.shape), tuple(points.shape)
    if len(ss) != 2 or ss[1] != 32:
        raise ValueError("scalars: shape (N, 32) expected, got %r" % (ss,))
    if ps != (ss[0], 64):
        raise ValueError("points: shape (%d, 64) expected, got %r" % (ss[0], ps))
    o = _ragged_offsets(offsets)
    if int(o[-1]) != ss[0]:
        raise ValueError("offsets[-1] = %d, but there are %d terms" % (int(o[-1]), ss[0]))
    return o.size - 1, ss[0]


def _sigbatch_z(n):
    """n x 16 bytes from the operating system's generator (secrets), every z_i non-zero"""
    import secrets

    z = np.frombuffer(secrets.token_bytes(16 * n), dtype=np.uint8).reshape(n, 16).copy()
    for i in np.nonzero(~z.any(axis=1))[0]:
        while not z[i].any():
            z[i] = np.frombuffer(secrets.token_bytes(16), dtype=np.uint8)
    return z


def _sigbatch_args(base, R, A, s, c, z):
    """jj_sigbatch_begin's arguments, checked before any C call: base 64 bytes; R, A, s, c of shape (n, 32); z of shape (n, 16) or None.
    -> (n, [_Arg of base, R, A, s, c, z])"""
    shapes = [tuple(x.shape) if hasattr(x, "shape") else None for x in (base, R, A, s, c)]
    if shapes[0] not in ((64,), (1, 64)):
        raise ValueError("base: one affine point of shape (64,) expected, got %r" % (shapes[0],))
    if shapes[1] is None or len(shapes[1]) != 2 or shapes[1][1] != 32:
        raise ValueError("R: shape (n, 32) expected, got %r" % (shapes[1],))
    n = shapes[1][0]
    for name, sh in zip(("A", "s", "c"), shapes[2:]):
        if sh != (n, 32):
            raise ValueError("%s: shape (%d, 32) expected, got %r" % (name, n, sh))
    if 2 * n + 1 > 1 << 24:
        raise ValueError("at most %d signatures per job (2n + 1 terms of one MSM pass), got %d" % (((1 << 24) - 1) // 2, n))
    if z is None:
        z = _sigbatch_z(n)
    elif not hasattr(z, "shape") or tuple(z.shape) != (n, 16):
        raise ValueError("z: shape (%d, 16) expected, got %r" % (n, tuple(z.shape) if hasattr(z, "shape") else None))
    return n, [_Arg(x, w) for x, w in zip((base, R, A, s, c, z), (64, 32, 32, 32, 32, 16))]


def _sigbatch_keyed_args(base, keys, offsets, R, s, c, z):
    """jj_sigbatch_keyed_begin's arguments, checked before any C call: base 64 bytes; keys (K, 32); offsets K + 1 integers (CSR, offsets[-1] = n);
    R, s, c of shape (n, 32); z of shape (n, 16) or None.  -> (K, n, offsets as a host uint64 array, [_Arg of base, keys, R, s, c, z])"""
    shapes = [tuple(x.shape) if hasattr(x, "shape") else None for x in (base, keys, R, s, c)]
    if shapes[0] not in ((64,), (1, 64)):
        raise ValueError("base: one affine point of shape (64,) expected, got %r" % (shapes[0],))
    if shapes[1] is None or len(shapes[1]) != 2 or shapes[1][1] != 32:
        raise ValueError("keys: shape (K, 32) expected, got %r" % (shapes[1],))
    K = shapes[1][0]
    o = _ragged_offsets(offsets)
    if o.size != K + 1:
        raise ValueError("offsets: %d values expected for %d keys, got %d" % (K + 1, K, o.size))
    n = int(o[-1])
    for name, sh in zip(("R", "s", "c"), shapes[2:]):
        if sh != (n, 32):
            raise ValueError("%s: shape (%d, 32) expected (offsets[-1] signatures), got %r" % (name, n, sh))
    if n + K + 1 > 1 << 24:
        raise ValueError("at most 2^24 terms per job (n + K + 1 of one MSM pass), got %d" % (n + K + 1))
    if z is None:
        z = _sigbatch_z(n)
    elif not hasattr(z, "shape") or tuple(z.shape) != (n, 16):
        raise ValueError("z: shape (%d, 16) expected, got %r" % (n, tuple(z.shape) if hasattr(z, "shape") else None))
    return K, n, o, [_Arg(x, w) for x, w in zip((base, keys, R, s, c, z), (64, 32, 32, 32, 32, 16))]


def _group_by_key(A):
    """Per-signature keys (n, 32) (numpy, or a torch tensor, which is copied to the host) -> (keys, offsets, order) for sigbatch_keyed_begin:
    keys (K, 32) the distinct encodings in lexicographic order of their bytes, offsets (K + 1,) uint64, order (n,) a STABLE permutation
    (signatures of one key keep their order): the caller passes R[order], s[order], c[order], z[order].  Pure numpy."""
    if _is_torch(A):
        A = A.cpu().numpy()
    A = np.ascontiguousarray(A, dtype=np.uint8)
    if A.ndim != 2 or A.shape[1] != 32:
        raise ValueError("A: shape (n, 32) expected, got %r" % (A.shape,))
    n = A.shape[0]
    if n == 0:
        return np.zeros((0, 32), np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.int64)
    rows = A.view(np.dtype((np.void, 32))).reshape(n)
    order = np.argsort(rows, kind="stable")
    srt = A[order]
    first = np.concatenate([[True], (srt[1:] != srt[:-1]).any(axis=1)])
    starts = np.nonzero(first)[0]
    return srt[starts], np.concatenate([starts, [n]]).astype(np.uint64), order.astype(np.int64)


def _sigbatch_ragged_args(base, offsets, R, A, s, c, z):
    """jj_sigbatch_ragged's arguments, checked before any C call: base 64 bytes; offsets S + 1 integers (CSR, offsets[-1] = n); R, A, s, c of shape
    (n, 32); z of shape (n, 16) or None.  -> (S, n, offsets as a host uint64 array, [_Arg of base, R, A, s, c, z])"""
    shapes = [tuple(x.shape) if hasattr(x, "shape") else None for x in (base, R, A, s, c)]
    if shapes[0] not in ((64,), (1, 64)):
        raise ValueError("base: one affine point of shape (64,) expected, got %r" % (shapes[0],))
    o = _ragged_offsets(offsets)
    S, n = o.size - 1, int(o[-1])
    for name, sh in zip(("R", "A", "s", "c"), shapes[1:]):
        if sh != (n, 32):
            raise ValueError("%s: shape (%d, 32) expected (offsets[-1] signatures), got %r" % (name, n, sh))
    if 2 * n + S > 1 << 24:
        raise ValueError("at most 2^24 terms per call (2n + S), got %d" % (2 * n + S))
    if z is None:
        z = _sigbatch_z(n)
    elif not hasattr(z, "shape") or tuple(z.shape) != (n, 16):
        raise ValueError("z: shape (%d, 16) expected, got %r" % (n, tuple(z.shape) if hasattr(z, "shape") else None))
    return S, n, o, [_Arg(x, w) for x, w in zip((base, R, A, s, c, z), (64, 32, 32, 32, 32, 16))]


def _sigbatch_verdicts(rows):
    """(S, 64) verdict points (numpy or torch) -> a list of "ok" | "reject" | "malformed" """
    if _is_torch(rows):
        rows = rows.cpu().numpy()
    out = []
    for row in np.asarray(rows, np.uint8).reshape(-1, 64):
        b = row.tobytes()
        out.append("ok" if b == SIGBATCH_IDENTITY else "malformed" if b == SIGBATCH_MALFORMED else "reject")
    return out


def _locate_cut(lo, hi, fanout):
    """[lo, hi) cut into min(fanout, hi - lo) consecutive non-empty parts whose lengths differ by at most one: the list of their bounds"""
    k = min(fanout, hi - lo)
    base, rem = divmod(hi - lo, k)
    bounds = [lo]
    for j in range(k):
        bounds.append(bounds[-1] + base + (1 if j < rem else 0))
    return bounds


def _sigbatch_locate(n, fanout, verdicts_of):
    """The bisection of Engine.sigbatch_locate over a verdict function: verdicts_of(index, offsets) -> one verdict string per segment of the gathered
    units (index None: all n units in their order; else the list of units to gather).  Pure Python; tests/test_sig_seg_cases_cpu.py runs it over
    the oracle."""
    fanout = int(fanout)
    if fanout < 2:
        raise ValueError("fanout: at least 2 expected, got %r" % (fanout,))
    if n == 0:
        return []
    found = []
    segs = [(0, n)]                                      # the failing segments of the round before, as ranges of the caller's indices
    first = True
    while segs:
        index, offsets, parts = [], [0], []
        for lo, hi in segs:
            b = _locate_cut(lo, hi, fanout)
            for p0, p1 in zip(b[:-1], b[1:]):
                parts.append((p0, p1))
                offsets.append(offsets[-1] + p1 - p0)
                if not first:
                    index.extend(range(p0, p1))
        verdicts = verdicts_of(None if first else index, offsets)
        first = False
        segs = []
        for (p0, p1), v in zip(parts, verdicts):
            if v == "ok":
                continue
            if p1 - p0 == 1:
                found.append((p0, v))
            else:
                segs.append((p0, p1))
    return sorted(found)


SIGBATCH_IDENTITY = bytes(32) + bytes([1]) + bytes(31)
SIGBATCH_MALFORMED = bytes(32) + (0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001 - 1).to_bytes(32, "little")

_MSM_BASIS_MODES = {"auto": 0, "points": 1, "windows": 2, 0: 0, 1: 1, 2: 2}


def _msm_basis_shapes(basis_n, scalars):
    """(B, m, single) of jj_msm_basis_mul's scalars: (m, 32) -> one row, result (64,); (B, m, 32) -> result (B, 64); m <= the basis's points"""
    ss = tuple(scalars.shape)
    if len(ss) not in (2, 3) or ss[-1] != 32:
        raise ValueError("scalars: shape (m, 32) or (B, m, 32) expected, got %r" % (ss,))
    B, m = (1, ss[0]) if len(ss) == 2 else (ss[0], ss[1])
    if m > basis_n:
        raise ValueError("scalars: %d terms per row, the basis has %d points" % (m, basis_n))
    return B, m, len(ss) == 2


def _pedersen_layout(rows, fields):
    """(n, row_stride, the C array of (byte_offset, nbits) pairs, nfields) of a pedersen call"""
    shape = tuple(rows.shape) if hasattr(rows, "shape") else None
    if shape is None or len(shape) != 2:
        raise ValueError("rows: shape (n, row_stride) expected, got %r" % (shape,))
    flat = [int(v) for f in fields for v in (f if isinstance(f, (tuple, list)) else (f,))]
    if len(flat) % 2 or len(flat) > 8:
        raise ValueError("fields: up to four (byte_offset, nbits) pairs expected")
    if any(v < 0 or v >= 1 << 32 for v in flat):
        raise ValueError("fields: values of 32 bits expected")
    return shape[0], shape[1], (C.c_uint32 * max(len(flat), 1))(*flat), len(flat) // 2


def _fixed_bytes(x, size, name):
    """a short host-side argument (personalisation, nonce) as bytes of exactly `size`, or None"""
    if x is None:
        return None
    x = bytes(x)
    if len(x) != size:
        raise ValueError("%s: %d bytes expected, got %d" % (name, size, len(x)))
    return x


class _Rows:
    """An (n, L) uint8 array or CUDA tensor as (pointer, n, L, row stride in bytes) WITHOUT a copy where its rows are contiguous and a fixed
    number of bytes apart -- a slice buf[:, :L] of a wider array --; any other layout, and a device view whose first byte is not 16-byte
    aligned, is copied into a contiguous array first (stride = L).  That holds for a single row too: only the row stride, which one row does
    not have, goes unasked there."""

    def __init__(self, x, name="msgs"):
        shape = tuple(x.shape) if hasattr(x, "shape") else None
        if shape is None or len(shape) != 2:
            raise ValueError("%s: shape (n, L) expected, got %r" % (name, shape))
        self.n, self.len = int(shape[0]), int(shape[1])
        empty = self.n == 0 or self.len == 0
        self.torch = _is_torch(x)
        if self.torch:
            import torch

            if x.dtype != torch.uint8:
                raise TypeError("torch arguments must be uint8")
            st = tuple(x.stride())
            # one row has no row stride to ask about; its bytes must still be adjacent and, on the device, its first byte aligned
            if not (empty or ((self.len == 1 or st[1] == 1) and (self.n == 1 or st[0] >= self.len) and x.data_ptr() % 16 == 0)):
                x, st = x.clone(memory_format=torch.contiguous_format), (self.len, 1)      # (contiguous() hands a one-row slice back as it is)
            self.device, self.ptr = x.device, (x.data_ptr() if x.numel() else None)
        else:
            if not isinstance(x, np.ndarray):
                x = _host_bytes(x).reshape(shape)
            if x.dtype != np.uint8:
                raise TypeError("numpy arguments must be uint8, got %s" % x.dtype)
            st = x.strides
            if not (empty or ((self.len == 1 or st[1] == 1) and (self.n == 1 or st[0] >= self.len))):
                x, st = np.ascontiguousarray(x), (self.len, 1)
            self.device, self.ptr = None, (x.ctypes.data if x.size else None)
        self.stride = self.len if (self.n <= 1 or empty) else int(st[0])
        self.keep = x


class _HostBlock:
    """owner of one jj_host_alloc block"""

    def __init__(self, lib, ptr):
        self._lib, self._ptr = lib, ptr

    def __del__(self):
        try:
            if self._ptr:
                self._lib.jj_host_free(C.c_void_p(self._ptr))
                self._ptr = None
        except Exception:
            pass


class FixedBaseTable:
    def __init__(self, engine, handle):
        self._engine = engine
        self._h = handle

    def close(self):
        if self._h is not None and self._engine._ctx is not None:
            self._engine._lib.jj_fixedbase_table_destroy(self._engine._ctx, self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MsmBasis:
    """A fixed set of points resident on the device (Engine.msm_basis); Engine.msm_basis_mul sums scalar vectors against it."""

    def __init__(self, engine, handle, n):
        self._engine = engine
        self._h = handle
        self.n = n

    @property
    def info(self):
        """{"n", "mode" ("points" | "windows"), "windows", "bytes"} of jj_msm_basis_info"""
        out = (C.c_int64 * 4)()
        self._engine._check(self._engine._lib.jj_msm_basis_info(self._h, out))
        return {"n": out[0], "mode": "windows" if out[1] == 2 else "points", "windows": out[2], "bytes": out[3]}

    def close(self):
        if self._h is not None and self._engine._ctx is not None:
            self._engine._lib.jj_msm_basis_destroy(self._engine._ctx, self._h)
        self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MsmJob:
    """Handle of an MSM in flight (Engine.msm_begin); finished exactly once by Engine.msm_finish."""

    def __init__(self, handle, keep):
        self._h = handle
        self._keep = keep


class Engine:
    def __init__(self, device=0, options=None):
        """options: {key: int} for jj_ctx_set_option (include/jubjub_hip.h lists the keys), applied before the first call.  Neither this class nor
        the library reads JJ_* environment variables."""
        self._mu = threading.RLock()      # stream selection + call form one critical section per Engine (see _locked below)
        self._lib = _lib.load()
        ctx = C.c_void_p()
        rc = self._lib.jj_ctx_create(int(device), C.byref(ctx))
        if rc != 0:
            self._ctx = None
            raise JubjubError("jj_ctx_create(device=%d) failed with %d (%s)" % (
                device, rc, "no gfx950 GPU visible; there is no CPU fallback" if rc == _lib.JJ_ERR_NODEVICE else "HIP error"))
        self._ctx = ctx
        self.device = int(device)
        for key, value in (options or {}).items():
            self.set_option(key, value)

    # -------------------------------------------------------------- plumbing
    def close(self):
        if self._ctx is not None:
            self._lib.jj_ctx_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise JubjubError("libjubjub_hip error %d: %s" % (rc, self._lib.jj_last_error(self._ctx).decode()))

    def sync(self):
        self._check(self._lib.jj_ctx_sync(self._ctx))

    def set_option(self, key, value):
        """jj_ctx_set_option: per-context tuning by key ("msm_lanes", "msm_fold_min", ...); "host_tail_scalar" is process-wide."""
        if key == "host_tail_scalar":
            rc = self._lib.jj_ctx_set_option(None, key.encode(), int(value))
            if rc:
                raise JubjubError("jj_ctx_set_option(%s=%r) failed with %d" % (key, value, rc))
            return
        self._check(self._lib.jj_ctx_set_option(self._ctx, key.encode(), int(value)))

    def get_option(self, key):
        v = C.c_longlong()
        rc = self._lib.jj_ctx_get_option(None if key == "host_tail_scalar" else self._ctx, key.encode(), C.byref(v))
        if rc:
            raise JubjubError("jj_ctx_get_option(%s) failed with %d" % (key, rc))
        return v.value

    def device_info(self):
        out = (C.c_int64 * 4)()
        self._check(self._lib.jj_device_info(self._ctx, out))
        return {"cus": out[0], "clock_khz": out[1], "wavefront": out[2]}

    # -------------------------------------------------------------- page-locked host arrays (jj_host_alloc / jj_host_register)
    def host_alloc(self, shape):
        """numpy uint8 array in page-locked host memory (jj_host_alloc): host batches in such arrays are pipelined over the copy
        streams without any per-call registration.  Freed when the array (and every view of it) is gone."""
        shape = tuple(shape) if isinstance(shape, (tuple, list)) else (int(shape),)
        nbytes = int(np.prod(shape, dtype=np.int64))
        if nbytes == 0:
            return np.empty(shape, np.uint8)
        p = C.c_void_p()
        rc = self._lib.jj_host_alloc(C.c_size_t(nbytes), C.byref(p))
        if rc:
            raise JubjubError("jj_host_alloc(%d bytes) failed with %d" % (nbytes, rc))
        buf = (C.c_uint8 * nbytes).from_address(p.value)
        buf._jj_owner = _HostBlock(self._lib, p.value)   # numpy keeps `buf` alive through .base; the block is freed with it
        return np.frombuffer(buf, dtype=np.uint8).reshape(shape)

    def result_acquire(self, shape):
        """numpy uint8 array over a page-locked result buffer from the context's pool (jj_result_acquire): pass it as `out=`; give it back with
        result_release(array) when the result has been consumed.  Several may be out at a time: every call can return a different result object."""
        shape = tuple(shape) if isinstance(shape, (tuple, list)) else (int(shape),)
        nbytes = int(np.prod(shape, dtype=np.int64))
        if nbytes == 0:
            return np.empty(shape, np.uint8)
        p = C.c_void_p()
        self._check(self._lib.jj_result_acquire(self._ctx, C.c_size_t(nbytes), C.byref(p)))
        buf = (C.c_uint8 * nbytes).from_address(p.value)
        return np.frombuffer(buf, dtype=np.uint8).reshape(shape)

    def result_release(self, array):
        if array is not None and array.size:
            self._check(self._lib.jj_result_release(self._ctx, C.c_void_p(array.ctypes.data)))

    def result_pool_stats(self):
        nb, by, iu = C.c_size_t(), C.c_size_t(), C.c_size_t()
        self._check(self._lib.jj_result_pool_stats(self._ctx, C.byref(nb), C.byref(by), C.byref(iu)))
        return {"buffers": nb.value, "bytes": by.value, "in_use": iu.value}

    def host_register(self, array, nbytes=None):
        """page-locks an existing numpy array once (jj_host_register); pair with host_unregister(array).  The array must consist of whole pages
        (page-aligned start AND a whole number of pages: np.frombuffer over an anonymous mmap; or host_alloc instead): anything else is refused."""
        a = np.ascontiguousarray(array)
        if a is not array and a.ctypes.data != array.ctypes.data:
            raise ValueError("a contiguous array is required")
        # nbytes: the length of the mapping the array lies at the start of, when that is longer than the array (a mapping is whole pages, an array of
        # n x 64 bytes usually is not: the caller vouches that [data, data + nbytes) is mapped and its own)
        rc = self._lib.jj_host_register(C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes if nbytes is None else int(nbytes)))
        if rc:
            raise JubjubError("jj_host_register failed with %d" % rc)

    def host_unregister(self, array):
        rc = self._lib.jj_host_unregister(C.c_void_p(array.ctypes.data))
        if rc:
            raise JubjubError("jj_host_unregister failed with %d" % rc)

    def profile(self, enable=True):
        self._check(self._lib.jj_ctx_profile(self._ctx, 1 if enable else 0))

    def profile_read(self, max_records=4096):
        a = (C.c_float * max_records)()
        b = (C.c_float * max_records)()
        k = C.c_int(0)
        self._check(self._lib.jj_ctx_profile_read(self._ctx, max_records, a, b, C.byref(k)))
        return [a[i] for i in range(k.value)], [b[i] for i in range(k.value)]

    def peak_imad32(self):
        out = C.c_double(0)
        self._check(self._lib.jj_peak_imad32(self._ctx, C.byref(out)))
        return out.value

    def peak_imad32_samples(self, count=7):
        """`count` single measurements of the integer multiply-add peak (jj_peak_imad32_samples), in launch order"""
        out = (C.c_double * count)()
        self._check(self._lib.jj_peak_imad32_samples(self._ctx, count, out))
        return [out[i] for i in range(count)]

    def _bind_stream(self, args):
        """When any argument is a torch CUDA tensor, run on torch's current stream."""
        if any(a.torch for a in args):
            import torch

            s = torch.cuda.current_stream(args[[a.torch for a in args].index(True)].device).cuda_stream
            self._lib.jj_ctx_set_stream(self._ctx, C.c_void_p(s))   # s == 0 is torch's default (null) stream
        else:
            self._lib.jj_ctx_use_own_stream(self._ctx)

    def _alloc(self, like, n, width):
        if like.torch:
            import torch

            t = torch.empty((n, width) if width > 1 else (n,), dtype=torch.uint8, device=like.device)
            return t, t.data_ptr()
        a = np.empty((n, width) if width > 1 else (n,), dtype=np.uint8)
        return a, (a.ctypes.data if a.size else None)

    def _call(self, name, ins, in_widths, out_widths, extra_before=(), extra_mid=(), n_override=None, out=None):
        """`out`: caller-owned result array(s) (one per output, same kind as the inputs, exact byte size) instead of fresh ones —
        e.g. page-locked buffers from host_alloc() that are reused across calls."""
        args = [_Arg(x, w) for x, w in zip(ins, in_widths)]
        n = args[0].n if n_override is None else n_override
        for a in args[1:]:
            if a.n != n and n_override is None:
                raise ValueError("length mismatch: %d vs %d" % (a.n, n))  # cf. the assert at reference src/lib.rs:841
        self._bind_stream(args)
        outs, optrs = [], []
        if out is not None:
            given = list(out) if isinstance(out, (tuple, list)) else [out]
            if len(given) != len(out_widths):
                raise ValueError("%d output arrays expected" % len(out_widths))
            for o, w in zip(given, out_widths):
                oa = _Arg(o, w)
                if oa.n != (n if n_override is None else 1) or oa.torch != args[0].torch or oa.keep is not o:
                    raise ValueError("out: a contiguous uint8 array of %d x %d bytes of the inputs' kind expected" % (n, w))
                outs.append(o)
                optrs.append(oa.ptr)
        for w in out_widths[len(outs):]:
            o, p = self._alloc(args[0], n if n_override is None else 1, w)
            outs.append(o)
            optrs.append(p)
        fn = getattr(self._lib, name)
        rc = fn(self._ctx, *extra_before, C.c_size_t(n), *[a.ptr for a in args], *extra_mid, *optrs)
        self._check(rc)
        return outs[0] if len(outs) == 1 else tuple(outs)

    # -------------------------------------------------------------- fields (reference src/fr.rs; Fq = bls12_381::Scalar)
    def field_binary(self, field, op, a, b):
        return self._call("jj_%s_%s" % (field, op), [a, b], [32, 32], [32])

    def field_unary(self, field, op, a):
        return self._call("jj_%s_%s" % (field, op), [a], [32], [32])

    def field_unary_ok(self, field, op, a):
        return self._call("jj_%s_%s" % (field, op), [a], [32], [32, 1])

    def from_bytes_wide(self, field, a):
        return self._call("jj_%s_from_bytes_wide" % field, [a], [64], [32])

    # -------------------------------------------------------------- points
    def point_double(self, p):
        return self._call("jj_point_double", [p], [64], [64])

    def point_add(self, p, q):
        return self._call("jj_point_add", [p, q], [64, 64], [64])

    def point_sub(self, p, q):
        return self._call("jj_point_sub", [p, q], [64, 64], [64])

    def point_neg(self, p):
        return self._call("jj_point_neg", [p], [64], [64])

    def mul_by_cofactor(self, p):
        return self._call("jj_point_mul_by_cofactor", [p], [64], [64])

    def to_niels(self, p):
        return self._call("jj_point_to_niels", [p], [64], [96])

    def predicate(self, name, p):
        return self._call("jj_" + name, [p], [64], [1])

    def point_sum(self, p):
        return self._sum_like("jj_point_sum", [p], [64])

    def fold_partials(self, parts):
        """Last step of an MSM cut across devices / processes: the sum of a few partial points (count x 64 bytes, numpy or a torch
        tensor on any device) on the calling host thread (jj_msm_fold_partials: the MSM's own host tail; ~5 us where the GPU
        launches of point_sum take ~180 us).  Returns the same kind of array as it was given, in host memory."""
        is_torch = type(parts).__module__.startswith("torch")
        host = np.ascontiguousarray((parts.detach().cpu().numpy() if is_torch else np.asarray(parts)).reshape(-1, 64), dtype=np.uint8)
        out = np.empty((64,), np.uint8)
        rc = self._lib.jj_msm_fold_partials(C.c_size_t(host.shape[0]), host.ctypes.data if host.shape[0] else None, out.ctypes.data)
        if rc:
            raise RuntimeError("jj_msm_fold_partials failed (%d): host pointers to 64-byte affine points expected" % rc)
        if is_torch:
            import torch

            return torch.from_numpy(out)
        return out

    def _sum_like(self, name, ins, widths):
        args = [_Arg(x, w) for x, w in zip(ins, widths)]
        n = args[0].n
        for a in args[1:]:
            if a.n != n:
                raise ValueError("length mismatch")
        self._bind_stream(args)
        out, optr = self._alloc(args[0], 1, 64)
        # zero-length numpy arrays have no data pointer; the library ignores inputs when n == 0
        rc = getattr(self._lib, name)(self._ctx, C.c_size_t(n), *[a.ptr for a in args], optr)
        self._check(rc)
        return out.reshape(64)

    # -------------------------------------------------------------- scalar multiplication
    def varbase_mul(self, scalars, points, out=None):
        return self._call("jj_varbase_mul", [scalars, points], [32, 64], [64], out=out)

    def varbase_mul_ct(self, scalars, points):
        """the constant-time ladder under the name rounds 3-4 gave it (jj_varbase_mul_ct): what varbase_mul runs by default since round 5"""
        return self._call("jj_varbase_mul_ct", [scalars, points], [32, 64], [64])

    def varbase_mul_vartime(self, scalars, points, out=None):
        """variable-time ladder for PUBLIC scalars (jj_varbase_mul_vartime): per-lane window table in memory, digit-dependent addresses"""
        return self._call("jj_varbase_mul_vartime", [scalars, points], [32, 64], [64], out=out)

    def varbase_mul_vartime_compressed(self, scalars, points, out=None):
        return self._call("jj_varbase_mul_vartime_compressed", [scalars, points], [32, 64], [32], out=out)

    def varbase_mul_scalar(self, scalar, points):
        """points[i] * scalar for one 32-byte scalar (numpy or torch), every point of the batch."""
        a, p = _Arg(scalar, 32), _Arg(points, 64)
        if a.n != 1:
            raise ValueError("scalar must be 32 bytes")
        self._bind_stream([a, p])
        out, optr = self._alloc(p, p.n, 64)
        self._check(self._lib.jj_varbase_mul_scalar(self._ctx, C.c_size_t(p.n), a.ptr, p.ptr, optr))
        return out

    def varbase_mul2_vartime(self, a, p, b, q, out=None):
        """p[i] * a[i] + q[i] * b[i] for PUBLIC scalars in one interleaved ladder per unit (jj_varbase_mul2_vartime): byte for byte
        point_add(varbase_mul(a, p), varbase_mul(b, q)); two per-lane window tables in memory, digit-dependent addresses"""
        return self._call("jj_varbase_mul2_vartime", [a, p, b, q], [32, 64, 32, 64], [64], out=out)

    def varbase_mul2_vartime_compressed(self, a, p, b, q, out=None):
        return self._call("jj_varbase_mul2_vartime_compressed", [a, p, b, q], [32, 64, 32, 64], [32], out=out)

    def varbase_mul2_scalars(self, ab, p, q):
        """p[i] * a + q[i] * b for ONE pair of 32-byte scalars (ab = a then b: 64 bytes or 2 x 32, numpy or torch), every pair of points of the batch."""
        s, pp, qq = _Arg(ab, 64), _Arg(p, 64), _Arg(q, 64)
        if s.n != 1:
            raise ValueError("ab must be 64 bytes: a then b")
        if pp.n != qq.n:
            raise ValueError("length mismatch: %d vs %d" % (pp.n, qq.n))
        self._bind_stream([s, pp, qq])
        out, optr = self._alloc(pp, pp.n, 64)
        self._check(self._lib.jj_varbase_mul2_scalars(self._ctx, C.c_size_t(pp.n), s.ptr, pp.ptr, qq.ptr, optr))
        return out

    def varbase_mul_compressed(self, scalars, points, out=None):
        return self._call("jj_varbase_mul_compressed", [scalars, points], [32, 64], [32], out=out)

    def fixedbase_mul_compressed(self, table, scalars, out=None):
        return self._call("jj_fixedbase_mul_compressed", [scalars], [32], [32], extra_before=(table._h,), out=out)

    def varbase_mul_exact(self, scalars, points):
        return self._call("jj_varbase_mul_exact", [scalars, points], [32, 64], [160])

    def fixedbase_table(self, base, window_bits=0):
        a = _Arg(base, 64)
        if a.n != 1:
            raise ValueError("base must be one affine point (64 bytes)")
        self._bind_stream([a])
        h = C.c_void_p()
        self._check(self._lib.jj_fixedbase_table_create(self._ctx, a.ptr, int(window_bits), C.byref(h)))
        return FixedBaseTable(self, h)

    def fixedbase_mul(self, table, scalars, out=None):
        return self._call("jj_fixedbase_mul", [scalars], [32], [64], extra_before=(table._h,), out=out)

    def fixedvar_mul_vartime(self, table, a, b, q, out=None):
        """G * a[i] + q[i] * b[i] for PUBLIC scalars, G the base of `table` (fixedbase_table, every window_bits): byte for byte
        point_add(fixedbase_mul(table, a), varbase_mul(b, q)).  A gathered table (window_bits 8..16) runs both terms in one kernel
        (jj_fixedvar_mul_vartime); digit-dependent addresses in both terms"""
        return self._call("jj_fixedvar_mul_vartime", [a, b, q], [32, 32, 64], [64], extra_before=(table._h,), out=out)

    def fixedvar_mul_vartime_compressed(self, table, a, b, q, out=None):
        return self._call("jj_fixedvar_mul_vartime_compressed", [a, b, q], [32, 32, 64], [32], extra_before=(table._h,), out=out)

    def fixedbase_multi_mul(self, tables, scalars):
        """out[i] = sum_j tables[j] * scalars[j][i]; scalars: (len(tables), n, 32) bytes, base-major."""
        nb = len(tables)
        a = _Arg(scalars, 32)
        if nb < 1 or a.n % nb:
            raise ValueError("scalars must hold len(tables) x n x 32 bytes")
        n = a.n // nb
        self._bind_stream([a])
        out, optr = self._alloc(a, n, 64)
        handles = (C.c_void_p * nb)(*[t._h for t in tables])
        self._check(self._lib.jj_fixedbase_multi_mul(self._ctx, handles, C.c_int(nb), C.c_size_t(n), a.ptr, optr))
        return out

    def fixedbase_composite_table(self, bases, scalar_bits):
        """One LDS table set for several bases with short scalars (jj_fixedbase_composite_create): bases (nb, 64) bytes, scalar_bits a
        list of nb bit lengths with sum(ceil((bits + 2) / 6)) <= 42."""
        a = _Arg(bases, 64)
        if a.n != len(scalar_bits) or a.n < 1:
            raise ValueError("one bit length per base")
        self._bind_stream([a])
        bits = (C.c_int * a.n)(*[int(b) for b in scalar_bits])
        h = C.c_void_p()
        self._check(self._lib.jj_fixedbase_composite_create(self._ctx, C.c_int(a.n), a.ptr, bits, C.byref(h)))
        t = FixedBaseTable(self, h)
        t.nbases = a.n
        return t

    def fixedbase_composite_mul(self, table, scalars):
        """out[i] = sum_b bases[b] * (scalars[b][i] mod 2^bits[b]) in ONE pass (43 additions per unit); scalars: (nb, n, 32) bytes."""
        a = _Arg(scalars, 32)
        nb = table.nbases
        if a.n % nb:
            raise ValueError("scalars must hold nbases x n x 32 bytes")
        n = a.n // nb
        self._bind_stream([a])
        out, optr = self._alloc(a, n, 64)
        self._check(self._lib.jj_fixedbase_composite_mul(self._ctx, table._h, C.c_size_t(n), a.ptr, optr))
        return out

    # -------------------------------------------------------------- windowed Pedersen hashes (jj_pedersen_*; the function: include/jubjub_hip.h)
    def pedersen_table(self, gens, seg_chunks=63, window_chunks=0):
        """The table of jj_pedersen_hash_vartime: gens (nseg, 64) affine generators, nseg 1..8, each on the curve and torsion-free;
        seg_chunks 1..63 chunks of three bits per generator; window_chunks 1..4 chunks per table window, 0 = the default."""
        a = _Arg(gens, 64)
        if a.n < 1:
            raise ValueError("gens: at least one affine point (64 bytes) expected")
        self._bind_stream([a])
        h = C.c_void_p()
        self._check(self._lib.jj_pedersen_table_create(self._ctx, C.c_int(a.n), a.ptr, C.c_int(int(seg_chunks)), C.c_int(int(window_chunks)), C.byref(h)))
        t = FixedBaseTable(self, h)
        t.nseg, t.seg_chunks = a.n, int(seg_chunks)
        return t

    def pedersen_hash(self, table, rows, fields, prefix=0, prefix_bits=0, point=False, out=None):
        """Windowed Pedersen hashes of n messages in one launch (jj_pedersen_hash_vartime, VARIABLE-TIME: public inputs).  Message i is
        prefix_bits bits of `prefix` (low bits first) followed by the fields of rows[i]: rows is an (n, row_stride) uint8 array or CUDA
        tensor, fields up to four (byte_offset, nbits) pairs, bits LSB-first within a byte.  -> (n, 32) canonical u-coordinates, or (n, 64)
        affine points with point=True, of rows' kind, or `out`."""
        n, stride, cf, nf = _pedersen_layout(rows, fields)
        ra = _Arg(rows, None)
        width = 64 if point else 32
        if out is None:
            out, optr = self._alloc(ra, n, width)
        else:
            oa = _Arg(out, width)
            if oa.n != n or oa.torch != ra.torch or oa.keep is not out:
                raise ValueError("out: a contiguous uint8 array of %d x %d bytes of rows' kind expected" % (n, width))
            optr = oa.ptr
        self._bind_stream([ra])
        self._check(self._lib.jj_pedersen_hash_vartime(self._ctx, table._h, C.c_size_t(n), C.c_uint(int(prefix) & 0xFFFFFFFF), C.c_int(int(prefix_bits)), ra.ptr, C.c_size_t(stride),
                                                        C.c_int(nf), cf, C.c_uint(FLAG_PEDERSEN_POINT if point else 0), optr))
        return out

    def pedersen_scalars(self, nseg, seg_chunks, rows, fields, prefix=0, prefix_bits=0):
        """<M_j> mod r of the same messages as canonical Fr bytes, (nseg, n, 32): what fixedbase_multi_mul reads (jj_pedersen_scalars).  With
        tables of the same generators, fixedbase_multi_mul over these scalars gives the bytes of pedersen_hash(point=True); a caller with
        secret inputs feeds them to the constant-time LDS tables."""
        n, stride, cf, nf = _pedersen_layout(rows, fields)
        ra = _Arg(rows, None)
        out, optr = self._alloc(ra, int(nseg) * n, 32)
        self._bind_stream([ra])
        self._check(self._lib.jj_pedersen_scalars(self._ctx, C.c_int(int(nseg)), C.c_int(int(seg_chunks)), C.c_size_t(n), C.c_uint(int(prefix) & 0xFFFFFFFF), C.c_int(int(prefix_bits)),
                                                   ra.ptr, C.c_size_t(stride), C.c_int(nf), cf, optr))
        return out.reshape(int(nseg), n, 32)

    def pedersen_merkle(self, table, leaves, first_layer=0):
        """The layers above n = 2^k leaves (an (n, 32) array of node u-coordinates), the root last: k calls of pedersen_hash, each over the
        buffer of the layer below read as rows of 64 bytes -- fields (0, 255), (32, 255), the 6-bit prefix first_layer, first_layer + 1, ...
        With a CUDA tensor nothing visits the host.  Padding a tree with empty roots is protocol and stays with the caller."""
        shape = tuple(leaves.shape) if hasattr(leaves, "shape") else None
        if shape is None or len(shape) != 2 or shape[1] != 32 or shape[0] < 1 or shape[0] & (shape[0] - 1):
            raise ValueError("leaves: shape (n, 32) with n a power of two expected, got %r" % (shape,))
        if first_layer < 0 or first_layer + shape[0].bit_length() - 1 > 64:
            raise ValueError("layer numbers are six bits")
        layers, cur, layer = [], leaves, int(first_layer)
        while cur.shape[0] > 1:
            cur = self.pedersen_hash(table, cur.reshape(cur.shape[0] // 2, 64), ((0, 255), (32, 255)), prefix=layer, prefix_bits=6)
            layers.append(cur)
            layer += 1
        return layers

    def pedersen_commit(self, ped, rtab, sources, fields, r, prefix=0, prefix_bits=0, point=False, out=None):
        """Windowed Pedersen commitments H(M_i) + [r_i] R in one call (jj_pedersen_commit_vartime).  H is pedersen_hash over `ped`; R is the
        base of `rtab`, a fixedbase_table of any window_bits; r is (n, 32) raw bytes read as fixedbase_mul reads its scalars.  Message i is
        prefix_bits bits of `prefix`, then the fields in the order given: `sources` is a list of up to four (n, L_s) uint8 arrays -- numpy
        arrays, or CUDA tensors of one kind; a view whose rows lie a fixed number of bytes apart is read where it is, as group_hash reads
        one -- and `fields` up to four (src, byte_offset, nbits) triples.  rtab = None with r = None is the plain multi-source hash.
        -> (n, 32) canonical u-coordinates, or (n, 64) affine points with point=True, of the sources' kind, or `out`.
        VARIABLE-TIME in the message (the decoder of the fields and the table addresses).  The blinding term is CONSTANT-TIME in r with an
        LDS rtab (window_bits 0, 6, 7) and variable-time with a gathered one (8..16)."""
        if (rtab is None) != (r is None):
            raise ValueError("rtab and r: both or neither (the hash-only form)")
        srcs = [_Rows(s, "sources[%d]" % k) for k, s in enumerate(sources)]
        if len(srcs) > 4:
            raise ValueError("sources: at most four arrays")
        flat = [tuple(int(v) for v in f) for f in fields]
        if len(flat) > 4 or any(len(f) != 3 or min(f) < 0 or max(f) >= 1 << 32 for f in flat):
            raise ValueError("fields: up to four (src, byte_offset, nbits) triples of 32-bit values expected")
        for s, off, nb in flat:
            if s >= len(srcs) or nb < 1 or off + (nb + 7) // 8 > srcs[s].len:
                raise ValueError("field (%d, %d, %d): no such source, empty, or past the %s bytes of its rows" % (s, off, nb, srcs[s].len if s < len(srcs) else "-"))
        ra = None if r is None else _Arg(r, 32)
        if not srcs and ra is None:
            raise ValueError("sources or r: something must say how many units there are")
        n = srcs[0].n if srcs else ra.n
        if any(s.n != n for s in srcs) or (ra is not None and ra.n != n):
            raise ValueError("length mismatch: %d units expected in every source and in r" % n)
        if any(s.torch != srcs[0].torch for s in srcs):
            raise ValueError("sources: numpy arrays or CUDA tensors, of one kind")
        like = srcs[0] if srcs else ra
        width = 64 if point else 32
        if out is None:
            out, optr = self._alloc(like, n, width)
        else:
            oa = _Arg(out, width)
            if oa.n != n or oa.torch != like.torch or oa.keep is not out:
                raise ValueError("out: a contiguous uint8 array of %d x %d bytes of the sources' kind expected" % (n, width))
            optr = oa.ptr
        self._bind_stream(srcs + ([ra] if ra is not None else []))
        cs = (C.c_void_p * 4)(*[s.ptr for s in srcs])
        cst = (C.c_size_t * 4)(*[s.stride for s in srcs])
        cf = (C.c_uint32 * 12)(*[v for f in flat for v in f])
        self._check(self._lib.jj_pedersen_commit_vartime(self._ctx, ped._h, rtab._h if rtab is not None else None, C.c_size_t(n), C.c_uint(int(prefix) & 0xFFFFFFFF),
                                                          C.c_int(int(prefix_bits)), C.c_int(len(srcs)), cs, cst, C.c_int(len(flat)), cf, ra.ptr if ra is not None else None,
                                                          C.c_uint(FLAG_PEDERSEN_POINT if point else 0), optr))
        return out

    def note_commit(self, ped, rtab, value_rows, value_offset, gd32, pkd32, rcm32):
        """The u-coordinate of a note commitment -> cm_u (n, 32): pedersen_commit over the prefix 0b111111 (6 bits), the 64 value bits at
        byte value_offset of value_rows, repr(g_d) and repr(pk_d) (256 bits each), blinded by rcm32 over rtab's base.  582 bits, 194 chunks:
        `ped` is the caller's four-segment table of 63 chunks (the last segment holds 5).  The generators are the caller's: the library
        knows no protocol.  Variable-time in the note's contents; rcm is constant-time with an LDS rtab."""
        return self.pedersen_commit(ped, rtab, [value_rows, gd32, pkd32], ((0, int(value_offset), 64), (1, 0, 256), (2, 0, 256)), rcm32,
                                    prefix=SAPLING_NOTE_PREFIX, prefix_bits=SAPLING_NOTE_PREFIX_BITS)

    def note_check(self, ivk32, plaintexts, cmu, ped, rtab, gd_personal, gd_prefix, expand_personal, epk=None, leads=(2,)):
        """The check that follows a trial-decryption hit -> verdict (n,) uint8, the codes of sigverify_each: 1 the row is a note, 0 the
        commitment or epk differs, 2 malformed (a lead byte not in `leads`, a diversifier with no point, or for lead 1 an rseed that is not a
        canonical Fr).  plaintexts: (n, L >= 52) rows as ka_open_aead returns them -- lead = row[0], d = row[1:12], v = row[12:20], rseed =
        row[20:52]; cmu, epk: (n, 32); ivk32: 32 bytes.  Steps, all on the arrays' device (nothing visits the host with CUDA tensors):
        g_d = group_hash(d, gd_personal, gd_prefix); pk_d = varbase_mul(ivk, g_d), the CONSTANT-TIME ladder; both compressed; lead 2:
        rcm = sig_challenge(None, None, rseed || 0x04, expand_personal) and, with epk given, esk likewise with 0x05 and
        varbase_mul_compressed(esk, g_d) == epk; lead 1: rcm = rseed, no epk check; note_commit(..) == cmu.
        SAPLING_GD_PERSONAL and SAPLING_EXPAND_PERSONAL are the documented examples; ped, rtab and gd_prefix are the caller's.
        VARIABLE-TIME in the note's contents (the decoder of the group hash, the Pedersen table addresses); CONSTANT-TIME in ivk and esk,
        and in rcm with an LDS rtab.  Real hits are rare: this serves rescans and callers who check every output they created."""
        shape = tuple(plaintexts.shape) if hasattr(plaintexts, "shape") else None
        if shape is None or len(shape) != 2 or shape[1] < 52:
            raise ValueError("plaintexts: shape (n, L) with L >= 52 expected, got %r" % (shape,))
        n, on_dev = shape[0], _is_torch(plaintexts)
        if on_dev:
            import torch as xp

            def like(x):
                return x if _is_torch(x) else xp.from_numpy(_host_bytes(x)).to(plaintexts.device)

            def cat(a, b):
                return xp.cat([a, b], dim=1)

            def every(m):
                return m.all(dim=1)

            rows, u8 = plaintexts, xp.uint8
            const = lambda v: xp.full((n, 1), v, dtype=xp.uint8, device=rows.device)      # noqa: E731
        else:
            xp = np

            def like(x):
                return x.cpu().numpy() if _is_torch(x) else _host_bytes(x)

            def cat(a, b):
                return np.concatenate([a, b], axis=1)

            def every(m):
                return m.all(axis=1)

            rows, u8 = _host_bytes(plaintexts).reshape(shape), np.uint8
            const = lambda v: np.full((n, 1), v, np.uint8)      # noqa: E731
        cmu, ivk = like(cmu).reshape(n, 32), like(ivk32).reshape(1, 32)
        lead, rseed = rows[:, 0], rows[:, 20:52]
        gd, gd_ok = self.group_hash(rows[:, 1:12], gd_personal, gd_prefix)
        gd[:, 32] |= 1 - gd_ok                                  # a row without a point carries (0, 0): the identity (0, 1) goes through the ladders instead
        ivk_n = ivk.repeat(n, 1) if on_dev else np.repeat(ivk, n, axis=0)
        gd32, pkd32 = self.compress(gd), self.compress(self.varbase_mul(ivk_n, gd))
        rcm = self.sig_challenge(None, None, cat(rseed, const(4)), expand_personal)
        is1 = lead == 1
        _, fr_ok = self.field_unary_ok("fr", "from_bytes", rseed)
        rcm = xp.where(is1[:, None], rseed, rcm)
        good = every(self.note_commit(ped, rtab, rows, 12, gd32, pkd32, rcm) == cmu)
        if epk is not None:
            esk = self.sig_challenge(None, None, cat(rseed, const(5)), expand_personal)
            good = good & (is1 | every(self.varbase_mul_compressed(esk, gd) == like(epk).reshape(n, 32)))
        known = lead != lead
        for v in leads:
            known = known | (lead == int(v))
        malformed = ~known | (gd_ok == 0) | (is1 & (fr_ok.reshape(n) == 0))
        good, bad = (good.to(u8), malformed.to(u8)) if on_dev else (good.astype(u8), malformed.astype(u8))
        return good * (1 - bad) + SIG_MALFORMED * bad              # arithmetic on bytes: no masked store, so no wait for the device

    def msm(self, scalars, points):
        return self._sum_like("jj_msm", [scalars, points], [32, 64])

    def msm_batch(self, scalars, points, out=None):
        """B independent MSMs in one call (jj_msm_batch): row b = msm(scalars[b], points or points[b]).  scalars (B, n, 32); points (n, 64)
        shared by every row or (B, n, 64); returns (B, 64).  numpy arrays or torch CUDA tensors (then on torch's current stream; up to 8192
        terms per row the call only queues the work); `out`: a caller-owned (B, 64) array of the inputs' kind."""
        B, n, shared = _msm_batch_shapes(scalars, points)
        a, p = _Arg(scalars, 32), _Arg(points, 64)
        if out is None:
            out, optr = self._alloc(a, B, 64)
        else:
            oa = _Arg(out, 64)
            if oa.n != B or oa.torch != a.torch or oa.keep is not out:
                raise ValueError("out: a contiguous uint8 array of %d x 64 bytes of the inputs' kind expected" % B)
            optr = oa.ptr
        self._bind_stream([a, p])
        self._check(self._lib.jj_msm_batch(self._ctx, C.c_size_t(B), C.c_size_t(n), a.ptr, p.ptr, C.c_int(shared), optr))
        return out

    def msm_ragged(self, scalars, points, offsets, out=None):
        """S independent MSMs of different lengths in one call (jj_msm_ragged): row s = msm(scalars[offsets[s]:offsets[s + 1]], points[the same]).
        scalars (N, 32), points (N, 64): numpy arrays or torch CUDA tensors; offsets: S + 1 integers (any sequence or array; kept on the host),
        offsets[0] = 0, non-decreasing, offsets[-1] = N; returns (S, 64) of the scalars' kind, an empty segment giving the identity.  With torch
        tensors and segments of up to 8192 terms the call only queues the work.  `out`: a caller-owned (S, 64) array of the scalars' kind."""
        S, N = _msm_ragged_shapes(scalars, points, offsets)
        o = _ragged_offsets(offsets)
        a, p = _Arg(scalars, 32), _Arg(points, 64)
        if out is None:
            out, optr = self._alloc(a, S, 64)
        else:
            oa = _Arg(out, 64)
            if oa.n != S or oa.torch != a.torch or oa.keep is not out:
                raise ValueError("out: a contiguous uint8 array of %d x 64 bytes of the scalars' kind expected" % S)
            optr = oa.ptr
        self._bind_stream([a, p])
        self._check(self._lib.jj_msm_ragged(self._ctx, C.c_size_t(S), o.ctypes.data, a.ptr, p.ptr, optr))
        return out

    def plan_msm_ragged(self, offsets, slice_min=0, waves=0, round_terms=0, items=False):
        """What msm_ragged does with these offsets (jj_plan_msm_ragged; no device work): {"short", "long", "items", "rounds"}; 0 = the default
        of slice_min / waves / round_terms (16 / 2048 / 2^18; this context's options are NOT read).  items=True adds "list": an (items, 4)
        uint64 array of (round, segment, first term, end term)."""
        o = _ragged_offsets(offsets)
        lib = _lib.load()
        out4 = (C.c_int64 * 4)()
        if lib.jj_plan_msm_ragged(C.c_size_t(o.size - 1), o.ctypes.data, int(slice_min), int(waves), C.c_uint64(int(round_terms)), out4):
            raise ValueError("jj_plan_msm_ragged refused its arguments")
        plan = {"short": out4[0], "long": out4[1], "items": out4[2], "rounds": out4[3]}
        if items:
            arr = np.zeros((max(1, out4[2]), 4), dtype=np.uint64)
            count = C.c_size_t()
            if lib.jj_plan_msm_ragged_items(C.c_size_t(o.size - 1), o.ctypes.data, int(slice_min), int(waves), C.c_uint64(int(round_terms)),
                                            arr.ctypes.data, C.c_size_t(arr.shape[0]), C.byref(count)):
                raise ValueError("jj_plan_msm_ragged_items refused its arguments")
            plan["list"] = arr[:count.value]
        return plan

    def msm_basis(self, points, mode="auto", windows=0):
        """Hands a fixed set of points over once (jj_msm_basis_create): points (n, 64), numpy or torch CUDA; the array may be reused
        afterwards.  mode "auto" | "points" | "windows"; windows 0 or 16..36 (include/jubjub_hip.h)."""
        ps = tuple(points.shape)
        if len(ps) != 2 or ps[1] != 64:
            raise ValueError("points: shape (n, 64) expected, got %r" % (ps,))
        if mode not in _MSM_BASIS_MODES:
            raise ValueError("mode: 'auto', 'points' or 'windows' expected, got %r" % (mode,))
        if int(windows) != 0 and not 16 <= int(windows) <= 36:
            raise ValueError("windows: 0 or 16..36 expected, got %r" % (windows,))
        p = _Arg(points, 64)
        self._bind_stream([p])
        h = C.c_void_p()
        self._check(self._lib.jj_msm_basis_create(self._ctx, C.c_size_t(p.n), p.ptr, C.c_int(_MSM_BASIS_MODES[mode]), C.c_int(int(windows)), C.byref(h)))
        return MsmBasis(self, h, p.n)

    def msm_basis_mul(self, basis, scalars, out=None):
        """Sums of scalar vectors against the first m points of a basis (jj_msm_basis_mul): scalars (m, 32) -> (64,), (B, m, 32) -> (B, 64);
        numpy arrays or torch CUDA tensors; `out`: a caller-owned array of that shape and of the scalars' kind."""
        B, m, single = _msm_basis_shapes(basis.n, scalars)
        a = _Arg(scalars, 32)
        if out is None:
            out, optr = self._alloc(a, B, 64)
            if single:
                out = out.reshape(64)
        else:
            oa = _Arg(out, 64)
            if oa.n != B or oa.torch != a.torch or oa.keep is not out or tuple(out.shape) != ((64,) if single else (B, 64)):
                raise ValueError("out: a contiguous uint8 array of shape %r of the scalars' kind expected" % (((64,) if single else (B, 64)),))
            optr = oa.ptr
        self._bind_stream([a])
        self._check(self._lib.jj_msm_basis_mul(self._ctx, basis._h, C.c_size_t(B), C.c_size_t(m), a.ptr, optr))
        return out

    def msm_dev(self, scalars, points, out=None):
        """The same sum finished ON THE DEVICE (jj_msm_dev): no host hop, nothing waits; returns a torch uint8 tensor of 64 bytes on
        the inputs' device (torch inputs), queued on torch's current stream."""
        import torch

        a, p = _Arg(scalars, 32), _Arg(points, 64)
        if a.n != p.n:
            raise ValueError("length mismatch: %d vs %d" % (a.n, p.n))
        if out is None:
            out = torch.empty(64, dtype=torch.uint8, device=a.device if a.torch else torch.device("cuda", self.device))
        self._bind_stream([a, p, _Arg(out, 64)])
        self._check(self._lib.jj_msm_dev(self._ctx, C.c_size_t(a.n), a.ptr, p.ptr, out.data_ptr()))
        return out

    def msm_begin(self, scalars, points):
        """Queues one MSM (jj_msm_begin) and returns a job; msm_finish(job) waits for it and runs the host tail.  Several jobs
        may be in flight: the host tail of one overlaps the kernels of the next.  The inputs are kept alive by the job."""
        a, p = _Arg(scalars, 32), _Arg(points, 64)
        if a.n != p.n:
            raise ValueError("length mismatch: %d vs %d" % (a.n, p.n))
        self._bind_stream([a, p])
        h = C.c_void_p()
        self._check(self._lib.jj_msm_begin(self._ctx, C.c_size_t(a.n), a.ptr, p.ptr, C.byref(h)))
        return MsmJob(h, (a.keep, p.keep))

    def sigbatch_begin(self, base, R, A, s, c, z=None, zip216=False):
        """Queues the batch check of n Schnorr signatures as ONE MSM job (jj_sigbatch_begin): R, A compressed points (n, 32), s responses and
        c challenges (n, 32; c is reduced mod r), base the affine point B (64,), z the (n, 16) random weights -- drawn from `secrets`, every
        z_i non-zero, when None.  numpy arrays or torch CUDA tensors, mixed freely.  msm_finish(job) returns
        [8] (sum [z_i] R_i + sum [z_i c_i] A_i - [sum z_i s_i] B): (0, 1) when every signature passes the cofactored check, (0, -1) for
        malformed input, any other point when a signature fails.  VARIABLE-TIME; everything here is public."""
        n, args = _sigbatch_args(base, R, A, s, c, z)
        self._bind_stream(args)
        h = C.c_void_p()
        self._check(self._lib.jj_sigbatch_begin(self._ctx, args[0].ptr, C.c_size_t(n), *[a.ptr for a in args[1:]], C.c_uint(FLAG_ZIP216 if zip216 else 0), C.byref(h)))
        return MsmJob(h, tuple(a.keep for a in args))

    def sigbatch_verify(self, base, R, A, s, c, z=None, zip216=False):
        """sigbatch_begin + msm_finish -> "ok" | "reject" | "malformed" """
        out = self.msm_finish(self.sigbatch_begin(base, R, A, s, c, z, zip216)).tobytes()
        return "ok" if out == SIGBATCH_IDENTITY else "malformed" if out == SIGBATCH_MALFORMED else "reject"

    def sigbatch_keyed_begin(self, base, keys, offsets, R, s, c, z=None, zip216=False):
        """sigbatch_begin for signatures grouped by key (jj_sigbatch_keyed_begin): keys (K, 32) compressed verification keys, offsets K + 1
        integers (CSR, host): signatures offsets[k] .. offsets[k+1] of R, s, c, z are checked under keys[k].  The terms of equal keys are folded:
        n + K + 1 MSM terms and n + K decodes.  msm_finish(job) returns the same 64 bytes as sigbatch_begin on the expanded arrays whenever every
        key has a signature; a key with none contributes nothing, but must decode.  group_by_key builds keys, offsets and the order from
        per-signature keys.  VARIABLE-TIME; everything here is public."""
        K, n, o, args = _sigbatch_keyed_args(base, keys, offsets, R, s, c, z)
        self._bind_stream(args)
        h = C.c_void_p()
        self._check(self._lib.jj_sigbatch_keyed_begin(self._ctx, args[0].ptr, C.c_size_t(K), args[1].ptr, o.ctypes.data, *[a.ptr for a in args[2:]],
                                                      C.c_uint(FLAG_ZIP216 if zip216 else 0), C.byref(h)))
        return MsmJob(h, tuple(a.keep for a in args))

    def sigbatch_keyed_verify(self, base, keys, offsets, R, s, c, z=None, zip216=False):
        """sigbatch_keyed_begin + msm_finish -> "ok" | "reject" | "malformed" """
        out = self.msm_finish(self.sigbatch_keyed_begin(base, keys, offsets, R, s, c, z, zip216)).tobytes()
        return "ok" if out == SIGBATCH_IDENTITY else "malformed" if out == SIGBATCH_MALFORMED else "reject"

    def sigbatch_ragged(self, base, offsets, R, A, s, c, z=None, zip216=False, out=None):
        """S batch checks over consecutive runs of one signature array in one call (jj_sigbatch_ragged): segment g holds signatures
        offsets[g] .. offsets[g+1] (offsets: S + 1 integers, kept on the host, offsets[0] = 0, non-decreasing, offsets[-1] = n).  R, A, s, c (n, 32),
        z (n, 16) -- drawn from `secrets`, every z_i non-zero, when None -- and base (64,): numpy arrays or torch CUDA tensors, mixed freely.
        Returns (S, 64) of R's kind: row g is byte for byte what sigbatch_begin + msm_finish give for segment g alone -- (0, 1) accept (also an empty
        segment), (0, -1) a malformed unit in that segment, any other point a failing signature.  A segment of one signature is an exact cofactored
        check of it.  `out`: a caller-owned (S, 64) array of R's kind.  VARIABLE-TIME; everything here is public."""
        S, n, o, args = _sigbatch_ragged_args(base, offsets, R, A, s, c, z)
        like = args[1]
        if out is None:
            out, optr = self._alloc(like, S, 64)
        else:
            oa = _Arg(out, 64)
            if oa.n != S or oa.torch != like.torch or oa.keep is not out:
                raise ValueError("out: a contiguous uint8 array of %d x 64 bytes of R's kind expected" % S)
            optr = oa.ptr
        self._bind_stream(args)
        self._check(self._lib.jj_sigbatch_ragged(self._ctx, args[0].ptr, C.c_size_t(S), o.ctypes.data, *[a.ptr for a in args[1:]], C.c_uint(FLAG_ZIP216 if zip216 else 0), optr))
        return out

    def sigbatch_ragged_verify(self, base, offsets, R, A, s, c, z=None, zip216=False):
        """sigbatch_ragged -> a list of "ok" | "reject" | "malformed", one per segment"""
        return _sigbatch_verdicts(self.sigbatch_ragged(base, offsets, R, A, s, c, z, zip216))

    def sigbatch_locate(self, base, R, A, s, c, z=None, zip216=False, fanout=16):
        """The signatures of a batch that fail on their own: the sorted list of (index, "reject" | "malformed").  Bisection with sigbatch_ragged: the
        whole batch as `fanout` segments first; each following round gathers only the units of the segments that are not "ok", cuts each such
        segment into up to `fanout` parts and repeats until the failing segments hold one signature (an exact check of it).  A valid batch costs
        one call, a batch with failures at most 1 + ceil(log_fanout(n)) calls.  Two failing signatures in one segment hide each other -- their terms
        cancel in the weighted sum -- with chance 2^-128 per round; a malformed unit never hides.  z: (n, 16) weights, drawn once when None and
        gathered with their signatures.  sig_locate answers the same question with one batch job and, for a rejected batch, one sigverify_each."""
        n = int(R.shape[0])
        arrays = [R, A, s, c, _sigbatch_z(n) if z is None else z]

        def gather(x, index):
            if _is_torch(x):
                import torch

                return x[torch.as_tensor(index, dtype=torch.long, device=x.device)]
            return np.asarray(x)[np.asarray(index, dtype=np.int64)]

        def verdicts_of(index, offsets):
            sub = arrays if index is None else [gather(x, index) for x in arrays]
            return self.sigbatch_ragged_verify(base, offsets, *sub, zip216=zip216)

        return _sigbatch_locate(n, fanout, verdicts_of)

    def sigverify_each(self, table, R, A, s, c, zip216=False, cofactored=True, out=None):
        """One verdict per signature in one call (jj_sigverify_each): table a fixedbase_table of the base B (any window_bits, not a composite
        one); R, A compressed points, s responses, c challenges (n, 32; c is reduced mod r): numpy arrays or torch CUDA tensors, mixed freely.
        Returns n bytes of R's kind: SIG_OK (1) iff [8]([s]B - [c]A - R) = O -- the cofactored equation of every sigbatch_* call; with
        cofactored=False iff [s]B - [c]A - R = O, what comparing encodings checks --, SIG_MALFORMED (2) for an R or A that does not decode
        (zip216: the decoder's rule) or s >= r, else SIG_REJECT (0).  `out`: a caller-owned array of n bytes of R's kind.  VARIABLE-TIME;
        everything here is public."""
        shapes = [tuple(x.shape) if hasattr(x, "shape") else None for x in (R, A, s, c)]
        if shapes[0] is None or len(shapes[0]) != 2 or shapes[0][1] != 32:
            raise ValueError("R: shape (n, 32) expected, got %r" % (shapes[0],))
        n = shapes[0][0]
        for name, sh in zip(("A", "s", "c"), shapes[1:]):
            if sh != (n, 32):
                raise ValueError("%s: shape (%d, 32) expected, got %r" % (name, n, sh))
        args = [_Arg(x, 32) for x in (R, A, s, c)]
        like = args[0]
        if out is None:
            out, optr = self._alloc(like, n, 1)
        else:
            oa = _Arg(out, 1)
            if oa.n != n or oa.torch != like.torch or oa.keep is not out:
                raise ValueError("out: a contiguous uint8 array of %d bytes of R's kind expected" % n)
            optr = oa.ptr
        self._bind_stream(args)
        flags = (FLAG_ZIP216 if zip216 else 0) | (0 if cofactored else FLAG_SIG_COFACTORLESS)
        self._check(self._lib.jj_sigverify_each(self._ctx, table._h, C.c_size_t(n), *[a.ptr for a in args], C.c_uint(flags), optr))
        return out

    def sig_locate(self, base, table, R, A, s, c, z=None, zip216=False):
        """The signatures of a batch that fail on their own, in sigbatch_locate's list format: one sigbatch_begin + msm_finish over the whole
        batch first; "ok" returns []; otherwise ONE sigverify_each (cofactored, the batch's own equation) gives every signature its verdict and
        the sorted list of (index, "reject" | "malformed") is returned.  table: a fixedbase_table of `base`.  Two calls at most, whatever
        the number of failures; a rejected batch whose signatures all pass on their own (chance 2^-128 of the opposite kind) gives []."""
        if self.sigbatch_verify(base, R, A, s, c, z, zip216) == "ok":
            return []
        v = self.sigverify_each(table, R, A, s, c, zip216=zip216, cofactored=True)
        v = v.cpu().numpy() if _is_torch(v) else np.asarray(v)
        return [(int(i), "malformed" if v[i] == SIG_MALFORMED else "reject") for i in np.nonzero(v != SIG_OK)[0]]

    def sig_challenge(self, R, A, msgs, personal=None, offsets=None, out=None):
        """The challenges of the signature family, hashed on the device (jj_sig_challenge):
        c_i = Fr::from_bytes_wide(BLAKE2b-512(personal; R_i || A_i || M_i)) as (n, 32) canonical bytes.  R, A: (n, 32) arrays, hashed as given;
        either may be None and is then left out of the hash (both None: hash-to-scalar of the messages alone).  msgs: an (n, L) uint8 array or
        CUDA tensor (every message L bytes), a flat uint8 array or tensor with `offsets` (n + 1 integers, CSR: message i is bytes
        offsets[i] .. offsets[i + 1]), or a list of bytes objects, which is packed here.  personal: 16 bytes (REDJUBJUB_PERSONAL is RedJubjub's)
        or None for sixteen zero bytes.  numpy arrays or torch CUDA tensors, mixed freely; the result is of R's kind when R is given, else of
        msgs' kind, or `out`.  A device result may be handed straight to sigbatch_begin, sigbatch_verify or sigverify_each: they read it on
        the same stream.  Meant for SHORT messages (one lane hashes one message)."""
        if personal is not None:
            personal = bytes(personal)
            if len(personal) != 16:
                raise ValueError("personal: 16 bytes expected, got %d" % len(personal))
        if isinstance(msgs, (list, tuple)) and all(isinstance(m, (bytes, bytearray, memoryview)) for m in msgs):
            if offsets is not None:
                raise ValueError("offsets: not with a list of messages (it is packed here)")
            offsets = np.zeros(len(msgs) + 1, np.uint64)
            offsets[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
            msgs = np.frombuffer(b"".join(bytes(m) for m in msgs), dtype=np.uint8)
        shape = tuple(msgs.shape) if hasattr(msgs, "shape") else None
        if offsets is None:
            if shape is None or len(shape) != 2:
                raise ValueError("msgs: shape (n, L), a flat array with offsets, or a list of bytes expected, got %r" % (shape,))
            n, msg_len, optr_off = shape[0], shape[1], None
        else:
            if shape is None or len(shape) != 1:
                raise ValueError("msgs: a flat uint8 array expected beside offsets, got %r" % (shape,))
            offsets = _ragged_offsets(offsets)
            if int(offsets[-1]) != shape[0]:
                raise ValueError("offsets[-1] = %d, but msgs holds %d bytes" % (int(offsets[-1]), shape[0]))
            n, msg_len, optr_off = offsets.size - 1, 0, offsets.ctypes.data
        if n > 1 << 24:
            raise ValueError("at most 2^24 challenges per call, got %d" % n)
        if n * msg_len > 1 << 32 or (offsets is not None and int(offsets[-1]) > 1 << 32):
            raise ValueError("at most 2^32 message bytes per call")
        for name, x in (("R", R), ("A", A)):
            if x is not None and (not hasattr(x, "shape") or tuple(x.shape) != (n, 32)):
                raise ValueError("%s: shape (%d, 32) or None expected, got %r" % (name, n, tuple(x.shape) if hasattr(x, "shape") else None))
        ra, aa, ma = (None if R is None else _Arg(R, 32)), (None if A is None else _Arg(A, 32)), _Arg(msgs, None)
        like = ra if ra is not None else ma
        if out is None:
            out, optr = self._alloc(like, n, 32)
        else:
            oa = _Arg(out, 32)
            if oa.n != n or oa.torch != like.torch or oa.keep is not out:
                raise ValueError("out: a contiguous uint8 array of %d x 32 bytes of %s kind expected" % (n, "R's" if ra is not None else "msgs'"))
            optr = oa.ptr
        self._bind_stream([a for a in (ra, aa, ma) if a is not None] + [like])
        self._check(self._lib.jj_sig_challenge(self._ctx, C.c_size_t(n), personal, ra.ptr if ra else None, aa.ptr if aa else None, ma.ptr, C.c_size_t(msg_len), optr_off, optr))
        return out

    def sigverify_each_msgs(self, table, R, A, s, msgs, personal, offsets=None, zip216=False, cofactored=True, out=None):
        """sig_challenge(R, A, msgs, personal, offsets), then sigverify_each with those challenges: one verdict byte per signature from the
        messages themselves.  With R on the device the challenges never visit the host."""
        return self.sigverify_each(table, R, A, s, self.sig_challenge(R, A, msgs, personal, offsets), zip216=zip216, cofactored=cofactored, out=out)

    def sigbatch_verify_msgs(self, base, R, A, s, msgs, personal, offsets=None, z=None, zip216=False):
        """sig_challenge(R, A, msgs, personal, offsets), then sigbatch_verify with those challenges -> "ok" | "reject" | "malformed".  With R on
        the device the challenges never visit the host."""
        return self.sigbatch_verify(base, R, A, s, self.sig_challenge(R, A, msgs, personal, offsets), z, zip216)

    def ka_kdf(self, sk, P, personal=None, flags=KA_SAPLING_FLAGS, out=None):
        """Key agreement with ONE secret scalar and its KDF (jj_ka_kdf) -> (keys (n, 32), ok (n,)):
        keys[i] = BLAKE2b-256(personal; to_bytes(share_i) [|| P[i] with FLAG_KA_HASH_INPUT]), share_i = [sk]P_i, or [8]([sk]P_i) with
        FLAG_KA_COFACTOR, P_i decoded under the FLAG_ZIP216 | FLAG_TORSION_FREE | FLAG_NOT_SMALL_ORDER bits of `flags` (the default is the
        Sapling recipient's set; SAPLING_KDF_PERSONAL its personalisation).  sk: 32 bytes (bytes, a uint8 array or a CUDA tensor), an integer
        of which the low 252 bits are used, never reduced mod r.  P: (n, 32) encodings, a numpy array or a torch CUDA tensor; the results are
        of P's kind, or `out` = (keys, ok).  Where P[i] fails the decoder, ok[i] = 0 and keys[i] is zero.  CONSTANT-TIME in sk and in the
        shares; the points are public.  A device result may be handed straight to chacha20_xor: it reads the keys on the same stream."""
        personal = _fixed_bytes(personal, 16, "personal")
        if not hasattr(P, "shape") or len(P.shape) != 2 or P.shape[1] != 32:
            raise ValueError("P: shape (n, 32) expected, got %r" % (tuple(P.shape) if hasattr(P, "shape") else None,))
        n = P.shape[0]
        ska, pa = _Arg(sk, 32), _Arg(P, 32)
        if ska.n != 1:
            raise ValueError("sk: ONE scalar of 32 bytes expected, got %d" % ska.n)
        if out is None:
            (keys, kptr), (ok, okptr) = self._alloc(pa, n, 32), self._alloc(pa, n, 1)
        else:
            keys, ok = out
            ka, oa = _Arg(keys, 32), _Arg(ok, 1)
            if ka.n != n or oa.n != n or ka.torch != pa.torch or oa.torch != pa.torch or ka.keep is not keys or oa.keep is not ok:
                raise ValueError("out: (keys, ok), contiguous uint8 arrays of %d x 32 and %d bytes of P's kind expected" % (n, n))
            kptr, okptr = ka.ptr, oa.ptr
        self._bind_stream([pa, ska])
        self._check(self._lib.jj_ka_kdf(self._ctx, C.c_size_t(n), ska.ptr, pa.ptr, C.c_uint(flags), personal, kptr, okptr))
        return keys, ok

    def chacha20_xor(self, keys, data, nonce=None, counter=0, length=None, out=None):
        """One RFC 8439 ChaCha20 key per row (jj_chacha20_xor): out[i] = data[i, :length] xor the keystream of keys[i] under `nonce` (12 bytes,
        None = zeros; one nonce for all rows) from block `counter` on (wrapping mod 2^32).  keys (n, 32), data (n, stride): numpy arrays or torch
        CUDA tensors, mixed freely; length (default: stride) a multiple of 4 in 4..1024, stride a multiple of 4.  Returns (n, length) of data's
        kind, or `out`; data and out must not overlap."""
        nonce = _fixed_bytes(nonce, 12, "nonce")
        for name, x in (("keys", keys), ("data", data)):
            if not hasattr(x, "shape") or len(x.shape) != 2:
                raise ValueError("%s: a two-dimensional uint8 array expected" % name)
        n, stride = data.shape
        length = stride if length is None else int(length)
        if tuple(keys.shape) != (n, 32):
            raise ValueError("keys: shape (%d, 32) expected, got %r" % (n, tuple(keys.shape)))
        if length < 4 or length > 1024 or length % 4 or stride % 4 or stride < length:
            raise ValueError("length must be a multiple of 4 in 4..1024 and the row stride a multiple of 4 and at least the length, got %d in %d" % (length, stride))
        if n * stride > 1 << 32:
            raise ValueError("at most 2^32 bytes of rows per call")
        if not 0 <= counter < 1 << 32:
            raise ValueError("counter: a 32-bit block counter expected")
        ka, da = _Arg(keys, 32), _Arg(data, None)
        if out is None:
            out, optr = self._alloc(da, n, length)
        else:
            oa = _Arg(out, None)
            if oa.n != n * length or oa.torch != da.torch or oa.keep is not out:
                raise ValueError("out: a contiguous uint8 array of %d x %d bytes of data's kind expected" % (n, length))
            optr = oa.ptr
        self._bind_stream([ka, da])
        self._check(self._lib.jj_chacha20_xor(self._ctx, C.c_size_t(n), ka.ptr, nonce, C.c_uint(counter), da.ptr, C.c_size_t(length), C.c_size_t(stride), optr))
        return out

    def ka_open(self, sk, P, ct, personal, flags=KA_SAPLING_FLAGS, nonce=None, counter=1, length=None):
        """Trial decryption: ka_kdf(sk, P, personal, flags), then chacha20_xor of the rows of `ct` with those keys -> (plaintext, ok).  The
        plaintext of a row whose ok byte is 0 is the row under the all-zero key: ok says which rows mean anything.  With P on the device the
        keys never visit the host (the cipher reads them on the stream the KDF wrote them on)."""
        keys, ok = self.ka_kdf(sk, P, personal, flags)
        return self.chacha20_xor(keys, ct, nonce, counter, length), ok

    def _mac_rows(self, keys, data, length, tail):
        """the shape checks of poly1305, aead_open (tail = 16: the tag behind the row) and aead_seal -> (n, stride, length)"""
        for name, x in (("keys", keys), ("data", data)):
            if not hasattr(x, "shape") or len(x.shape) != 2:
                raise ValueError("%s: a two-dimensional uint8 array expected" % name)
        n, stride = data.shape
        length = stride - tail if length is None else int(length)
        if tuple(keys.shape) != (n, 32):
            raise ValueError("keys: shape (%d, 32) expected, got %r" % (n, tuple(keys.shape)))
        if length < 4 or length > 1024 or length % 4 or stride % 4 or stride < length + tail:
            raise ValueError("length must be a multiple of 4 in 4..1024 and the row stride a multiple of 4 and at least the length%s, got %d in %d"
                             % (" plus the 16 tag bytes" if tail else "", length, stride))
        if n * stride > 1 << 32:
            raise ValueError("at most 2^32 bytes of rows per call")
        return n, stride, length

    def _mac_out(self, like, out, n, width, name):
        if out is None:
            return self._alloc(like, n, width)
        oa = _Arg(out, None)
        if oa.n != n * width or oa.torch != like.torch or oa.keep is not out:
            raise ValueError("%s: a contiguous uint8 array of %d x %d bytes of data's kind expected" % (name, n, width))
        return out, oa.ptr

    def _aad_bytes(self, aad):
        aad = bytes(aad or b"")
        if len(aad) > 64:
            raise ValueError("aad: at most 64 bytes, got %d" % len(aad))
        return aad

    def poly1305(self, keys, data, length=None, out=None):
        """One Poly1305 one-time key per row (jj_poly1305): tags[i] = Poly1305(keys[i]; data[i, :length]), r in key bytes 0..15 and s in bytes
        16..31 (RFC 8439 section 2.5).  keys (n, 32), data (n, stride): numpy arrays or torch CUDA tensors, mixed freely; length (default:
        stride) a multiple of 4 in 4..1024, stride a multiple of 4.  Returns (n, 16) of data's kind, or `out`."""
        n, stride, length = self._mac_rows(keys, data, length, 0)
        ka, da = _Arg(keys, 32), _Arg(data, None)
        out, optr = self._mac_out(da, out, n, 16, "out")
        self._bind_stream([ka, da])
        self._check(self._lib.jj_poly1305(self._ctx, C.c_size_t(n), ka.ptr, da.ptr, C.c_size_t(length), C.c_size_t(stride), optr))
        return out

    def aead_open(self, keys, data, nonce=None, aad=b"", length=None, out=None):
        """RFC 8439 ChaCha20-Poly1305, one key per row, the tag checked on the device (jj_aead_open) -> (plain (n, length), ok (n,)).  A row of
        data (n, stride) is `length` ciphertext bytes (default: stride - 16) followed by the 16 tag bytes; `nonce` (12 bytes, None = zeros) and
        `aad` (at most 64 bytes) are the same for all rows.  Where the tag does not verify, ok[i] = 0 and plain[i] is zero: a failed row never
        holds plaintext.  length a multiple of 4 in 4..1024, stride a multiple of 4 and at least length + 16.  Results of data's kind, or `out`
        = (plain, ok); data and out must not overlap.  A device result of ka_kdf may be handed over as keys: it is read on the same stream."""
        nonce, aad = _fixed_bytes(nonce, 12, "nonce"), self._aad_bytes(aad)
        n, stride, length = self._mac_rows(keys, data, length, 16)
        ka, da = _Arg(keys, 32), _Arg(data, None)
        if out is not None and (not isinstance(out, (tuple, list)) or len(out) != 2):
            raise ValueError("out: (plain, ok) expected")
        (plain, pptr), (ok, okptr) = self._mac_out(da, out[0] if out else None, n, length, "out[0]"), self._mac_out(da, out[1] if out else None, n, 1, "out[1]")
        self._bind_stream([ka, da])
        self._check(self._lib.jj_aead_open(self._ctx, C.c_size_t(n), ka.ptr, nonce, aad or None, C.c_size_t(len(aad)), da.ptr, C.c_size_t(length), C.c_size_t(stride), pptr, okptr))
        return plain, ok

    def aead_seal(self, keys, data, nonce=None, aad=b"", length=None, out=None):
        """RFC 8439 ChaCha20-Poly1305, one key per row (jj_aead_seal): out[i] = the ciphertext of data[i, :length] under keys[i], `nonce` and `aad`
        followed by its 16-byte tag -> (n, length + 16) of data's kind, or `out`.  length (default: stride) a multiple of 4 in 4..1024, stride a
        multiple of 4; data and out must not overlap."""
        nonce, aad = _fixed_bytes(nonce, 12, "nonce"), self._aad_bytes(aad)
        n, stride, length = self._mac_rows(keys, data, length, 0)
        ka, da = _Arg(keys, 32), _Arg(data, None)
        out, optr = self._mac_out(da, out, n, length + 16, "out")
        self._bind_stream([ka, da])
        self._check(self._lib.jj_aead_seal(self._ctx, C.c_size_t(n), ka.ptr, nonce, aad or None, C.c_size_t(len(aad)), da.ptr, C.c_size_t(length), C.c_size_t(stride), optr))
        return out

    def ka_open_aead(self, sk, P, ct, personal, flags=KA_SAPLING_FLAGS, nonce=None, aad=b"", length=None):
        """Tag-checked trial decryption: ka_kdf(sk, P, personal, flags), then aead_open of the rows of `ct` with those keys -> (plaintext, ok),
        ok the AND of the two ok arrays.  A row whose P did not decode, or whose tag does not verify, is a zero row with ok = 0.  With P on the
        device the keys never visit the host.  (A row that did not decode is opened under the all-zero key, which a forged row could satisfy,
        so the plaintext is multiplied by the combined verdict: no host round trip and no branch on the data.)"""
        keys, ok = self.ka_kdf(sk, P, personal, flags)
        plain, tag_ok = self.aead_open(keys, ct, nonce, aad, length)
        if _is_torch(ok) != _is_torch(tag_ok):                  # P and ct of different kinds: the verdicts are of ct's kind
            if _is_torch(ok):
                ok = ok.cpu().numpy()
            else:
                import torch

                ok = torch.from_numpy(ok).to(tag_ok.device)
        both = ok & tag_ok
        plain *= both[:, None]
        return plain, both

    # -------------------------------------------------------------- the sender's side of a note (jj_blake2b, jj_ka_kdf_each)
    def blake2b(self, sources, personal=None, prefix=b"", digest_len=32, out=None):
        """Raw BLAKE2b digests over rows gathered from several arrays (jj_blake2b) -> (n, digest_len):
        out[i] = BLAKE2b-digest_len(personal; prefix || sources[0][i] || sources[1][i] || ..), digest_len 32 or 64 (BLAKE2b-256 is its own
        hash, not a truncation).  sources: a list of up to four (n, L) uint8 arrays -- numpy arrays or CUDA tensors, mixed freely; L a multiple
        of 4 in 4..65536 --; a strided view (buf[:, 16:48]) keeps its stride where that is a multiple of 4 and is read where it is, any other
        layout is copied first.  One array may serve several sources.  personal: 16 bytes or None for sixteen zero bytes; prefix: up to 4096
        bytes of HOST memory, a multiple of 4, the same for every row (it may be a viewing key: nothing in the instruction stream or in an
        address depends on the data).  With no source every row is the digest of the prefix alone, and n is out's row count (1 without out).
        The result is of the first source's kind, or `out`; a device result may be handed straight to aead_open or aead_seal as keys: they
        read it on the same stream.  The library knows no protocol: SAPLING_OCK_PERSONAL with prefix = ovk and sources cv, cmu, epk is the
        documented example."""
        personal = _fixed_bytes(personal, 16, "personal")
        prefix = bytes(prefix)
        digest_len = int(digest_len)
        if digest_len not in (32, 64):
            raise ValueError("digest_len: 32 or 64 expected, got %d" % digest_len)
        if len(prefix) > 4096 or len(prefix) % 4:
            raise ValueError("prefix: at most 4096 bytes and a multiple of 4, got %d" % len(prefix))
        sources = list(sources)
        if len(sources) > 4:
            raise ValueError("sources: at most four arrays")
        srcs = []
        for k, s in enumerate(sources):
            r = _Rows(s, "sources[%d]" % k)
            if r.n > 1 and r.stride % 4:                  # a row stride the kernel cannot read as dwords: a contiguous copy
                r = _Rows(r.keep.contiguous() if r.torch else np.ascontiguousarray(r.keep), "sources[%d]" % k)
            if r.len < 4 or r.len > 65536 or r.len % 4:
                raise ValueError("sources[%d]: rows of a multiple of 4 in 4..65536 bytes expected, got %d" % (k, r.len))
            srcs.append(r)
        if srcs:
            n = srcs[0].n
        elif out is not None:
            n = _Arg(out, digest_len).n
        else:
            n = 1
        if any(s.n != n for s in srcs):
            raise ValueError("length mismatch: %d rows expected in every source" % n)
        if n > 1 << 24 or any(n * s.stride > 1 << 32 for s in srcs):
            raise ValueError("at most 2^24 rows and 2^32 bytes of rows per source and call")
        oa = None
        if out is None and srcs:
            out, optr = self._alloc(srcs[0], n, digest_len)
        elif out is None:
            out = np.empty((n, digest_len), np.uint8)
            optr = out.ctypes.data
        else:
            oa = _Arg(out, digest_len)
            if oa.n != n or oa.keep is not out:
                raise ValueError("out: a contiguous uint8 array of %d x %d bytes expected" % (n, digest_len))
            optr = oa.ptr
        self._bind_stream(srcs + ([oa] if oa is not None else []))
        cs = (C.c_void_p * 4)(*[s.ptr for s in srcs])
        cl = (C.c_size_t * 4)(*[s.len for s in srcs])
        cst = (C.c_size_t * 4)(*[max(s.stride, s.len) for s in srcs])
        self._check(self._lib.jj_blake2b(self._ctx, C.c_size_t(n), C.c_int(digest_len), personal, prefix or None, C.c_size_t(len(prefix)), C.c_int(len(srcs)),
                                         cs, cl, cst, optr))
        return out

    def ka_kdf_each(self, sk, P, personal=None, flags=KA_SAPLING_FLAGS, hash_input=None, out=None):
        """Key agreement with one secret scalar PER ROW and its KDF (jj_ka_kdf_each) -> (keys (n, 32), ok (n,)): exactly ka_kdf, but sk is
        (n, 32) -- each row read as varbase_mul reads a scalar: the low 252 bits, an integer never reduced mod r -- and, with
        FLAG_KA_HASH_INPUT, the second hashed part is hash_input[i] when hash_input (n, 32) is given and P[i] when it is None (the sender
        hashes share || epk, and epk is not the point that was multiplied).  hash_input without that flag is refused.  sk, P, hash_input:
        numpy arrays or CUDA tensors, mixed freely; the results are of P's kind, or `out` = (keys, ok).  CONSTANT-TIME in the scalars and the
        shares; the points are public."""
        personal = _fixed_bytes(personal, 16, "personal")
        if not hasattr(P, "shape") or len(P.shape) != 2 or P.shape[1] != 32:
            raise ValueError("P: shape (n, 32) expected, got %r" % (tuple(P.shape) if hasattr(P, "shape") else None,))
        n = P.shape[0]
        ska, pa = _Arg(sk, 32), _Arg(P, 32)
        ha = None if hash_input is None else _Arg(hash_input, 32)
        if ska.n != n or (ha is not None and ha.n != n):
            raise ValueError("sk and hash_input: %d rows of 32 bytes expected, one per row of P" % n)
        if ha is not None and not flags & FLAG_KA_HASH_INPUT:
            raise ValueError("hash_input needs FLAG_KA_HASH_INPUT")
        if out is None:
            (keys, kptr), (ok, okptr) = self._alloc(pa, n, 32), self._alloc(pa, n, 1)
        else:
            keys, ok = out
            ka, oa = _Arg(keys, 32), _Arg(ok, 1)
            if ka.n != n or oa.n != n or ka.torch != pa.torch or oa.torch != pa.torch or ka.keep is not keys or oa.keep is not ok:
                raise ValueError("out: (keys, ok), contiguous uint8 arrays of %d x 32 and %d bytes of P's kind expected" % (n, n))
            kptr, okptr = ka.ptr, oa.ptr
        self._bind_stream([pa, ska] + ([ha] if ha is not None else []))
        self._check(self._lib.jj_ka_kdf_each(self._ctx, C.c_size_t(n), ska.ptr, pa.ptr, ha.ptr if ha is not None else None, C.c_uint(flags), personal, kptr, okptr))
        return keys, ok

    def _same_kind(self, like, arrays):
        """`arrays` as (n, w) arrays of `like`'s kind (numpy, or CUDA tensors on its device)"""
        if _is_torch(like):
            import torch

            return [x if _is_torch(x) else torch.from_numpy(_host_bytes(x).reshape(tuple(x.shape))).to(like.device) for x in arrays]
        return [x.cpu().numpy() if _is_torch(x) else _host_bytes(x).reshape(tuple(np.shape(x))) for x in arrays]

    def note_encrypt(self, esk, gd, pkd, plain, ovk32, cv, cmu, kdf_personal, ock_personal, flags=KA_SAPLING_FLAGS):
        """The ciphertexts of n outputs -> (epk (n, 32), c_enc (n, L + 16), c_out (n, 80)), of plain's kind.  esk (n, 32): one fresh secret
        scalar per output; gd (n, 64): the diversified bases as affine points; pkd, cv, cmu (n, 32); plain (n, L), L a multiple of 4 in
        4..1024; ovk32: 32 bytes of host memory.  Steps, all on plain's device (with CUDA tensors neither a key nor a share visits the host):
        epk = varbase_mul_compressed(esk, gd), the CONSTANT-TIME ladder; keys = ka_kdf_each(esk, pkd, kdf_personal, flags, hash_input=epk);
        c_enc = aead_seal(keys, plain); ock = blake2b([cv, cmu, epk], ock_personal, prefix=ovk32); c_out = aead_seal(ock, pkd || esk) --
        zero nonce, empty aad.  SAPLING_KDF_PERSONAL and SAPLING_OCK_PERSONAL are the documented examples; the library knows no protocol.
        A pkd that the decoder refuses gives that row the all-zero note key (ka_kdf_each's rule): check pkd where it is not the caller's own."""
        ovk32 = _fixed_bytes(bytes(_host_bytes(ovk32)), 32, "ovk32")
        esk, gd, pkd, cv, cmu = self._same_kind(plain, [esk, gd, pkd, cv, cmu])
        epk = self.varbase_mul_compressed(esk, gd)
        keys, _ = self.ka_kdf_each(esk, pkd, kdf_personal, flags, hash_input=epk)
        c_enc = self.aead_seal(keys, plain)
        ock = self.blake2b([cv, cmu, epk], ock_personal, prefix=ovk32)
        if _is_torch(plain):
            import torch

            op = torch.cat([pkd, esk], dim=1)
        else:
            op = np.concatenate([pkd, esk], axis=1)
        return epk, c_enc, self.aead_seal(ock, op)

    def ovk_open(self, ovk32, cv, cmu, epk, c_out, c_enc, kdf_personal, ock_personal, flags=KA_SAPLING_FLAGS):
        """Recover sent notes with an outgoing viewing key -> (plain (n, L), op (n, 64), ok (n,)), of c_enc's kind.  cv, cmu, epk (n, 32);
        c_out (n, 80); c_enc (n, L + 16).  First stage, over all n rows -- one BLAKE2b block and one 80-byte AEAD open per output, no scalar
        multiplication: ock = blake2b([cv, cmu, epk], ock_personal, prefix=ovk32); op = pk_d || esk from aead_open(ock, c_out).  Second
        stage, over the rows that HIT only: esk canonical (fr from_bytes' ok), ka_kdf_each(esk, pk_d, kdf_personal, flags, hash_input=epk),
        aead_open of c_enc.  The hit rows are gathered with index operations of numpy or torch: the ONE place where this call
        waits for the device (the number of hits sizes the second stage).  The results are scattered back into full-size zero arrays: ok is the AND of
        the four verdicts, and every row that is not ok is zeros in plain and in op.  CONSTANT-TIME in esk and the shares like
        ka_kdf_each; which rows hit is the public outcome of the scan."""
        ovk32 = _fixed_bytes(bytes(_host_bytes(ovk32)), 32, "ovk32")
        shape = tuple(c_enc.shape) if hasattr(c_enc, "shape") else None
        if shape is None or len(shape) != 2 or shape[1] < 20:
            raise ValueError("c_enc: shape (n, L + 16) expected, got %r" % (shape,))
        n, L = shape[0], shape[1] - 16
        cv, cmu, epk, c_out = self._same_kind(c_enc, [cv, cmu, epk, c_out])
        ock = self.blake2b([cv, cmu, epk], ock_personal, prefix=ovk32)
        op, hit = self.aead_open(ock, c_out)
        if _is_torch(c_enc):
            import torch

            idx = torch.nonzero(hit).reshape(-1)                         # waits for the device
            plain = torch.zeros((n, L), dtype=torch.uint8, device=c_enc.device)
            op_out, ok = torch.zeros_like(op), torch.zeros_like(hit)
        else:
            idx = np.nonzero(hit)[0]
            plain, op_out, ok = np.zeros((n, L), np.uint8), np.zeros_like(op), np.zeros_like(hit)
        if len(idx) == 0:
            return plain, op_out, ok
        op_h = op[idx]
        pkd, esk = op_h[:, :32], op_h[:, 32:]
        if _is_torch(c_enc):
            pkd, esk = pkd.contiguous(), esk.contiguous()
        else:
            pkd, esk = np.ascontiguousarray(pkd), np.ascontiguousarray(esk)
        _, fr_ok = self.field_unary_ok("fr", "from_bytes", esk)
        keys, ka_ok = self.ka_kdf_each(esk, pkd, kdf_personal, flags, hash_input=epk[idx])
        plain_h, tag_ok = self.aead_open(keys, c_enc[idx])
        good = fr_ok.reshape(-1) & ka_ok & tag_ok
        plain[idx] = plain_h * good[:, None]
        op_out[idx] = op_h * good[:, None]
        ok[idx] = good
        return plain, op_out, ok

    def _b2s_args(self, msgs, personal, prefix):
        personal = _fixed_bytes(personal, 8, "personal")
        prefix = bytes(prefix)
        if len(prefix) > 4096:
            raise ValueError("prefix: at most 4096 bytes, got %d" % len(prefix))
        ma = _Rows(msgs)
        if ma.len > 65536:
            raise ValueError("msgs: at most 65536 bytes per message, got %d" % ma.len)
        if ma.n > 1 << 24 or ma.n * ma.stride > 1 << 32:
            raise ValueError("at most 2^24 messages and 2^32 bytes of rows per call")
        return ma, personal, (prefix or None), len(prefix)

    def blake2s(self, msgs, personal=None, prefix=b"", out=None):
        """BLAKE2s-256(personal; prefix || msgs[i]) for every row (jj_blake2s) -> (n, 32) digests of msgs' kind, or `out`.  msgs: an (n, L)
        uint8 numpy array or CUDA tensor, L in 0..65536; a view whose rows lie a fixed number of bytes apart (buf[:, :L]) is read where it is,
        at any byte offset of its rows.  personal: 8 bytes or None for eight zero bytes; prefix: up to 4096 bytes of host memory, the same
        for every row (its whole blocks are compressed once, on the host).  A device result may be handed straight to any other call: it is
        written on the stream they read on.  Variable-time over public inputs."""
        ma, personal, prefix, plen = self._b2s_args(msgs, personal, prefix)
        if out is None:
            out, optr = self._alloc(ma, ma.n, 32)
        else:
            oa = _Arg(out, 32)
            if oa.n != ma.n or oa.torch != ma.torch or oa.keep is not out:
                raise ValueError("out: a contiguous uint8 array of %d x 32 bytes of msgs' kind expected" % ma.n)
            optr = oa.ptr
        self._bind_stream([ma])
        self._check(self._lib.jj_blake2s(self._ctx, C.c_size_t(ma.n), personal, prefix, C.c_size_t(plen), ma.ptr, C.c_size_t(ma.len), C.c_size_t(ma.stride), optr))
        return out

    def group_hash(self, msgs, personal, prefix=b"", flags=GROUP_HASH_FLAGS, out=None):
        """Hash to the curve (jj_group_hash) -> (points (n, 64), ok (n,)): the digest of blake2s(msgs, personal, prefix) decoded exactly as
        decompress(digests, flags) decodes it -- the four FLAG_* decoder bits; the default is the group hash of the Zcash specification,
        [8] * decode(digest) with small-order results refused --, in one call and without the digests leaving the device.  A refused row
        gets the point (0, 0) and ok = 0.  The results are of msgs' kind, or `out` = (points, ok).  The library knows no protocol:
        personalisation, prefix and message layout are the caller's (SAPLING_GD_PERSONAL, SAPLING_PH_PERSONAL are examples)."""
        ma, personal, prefix, plen = self._b2s_args(msgs, personal, prefix)
        n = ma.n
        if out is None:
            (pts, pptr), (ok, okptr) = self._alloc(ma, n, 64), self._alloc(ma, n, 1)
        else:
            pts, ok = out
            pa, oa = _Arg(pts, 64), _Arg(ok, 1)
            if pa.n != n or oa.n != n or pa.torch != ma.torch or oa.torch != ma.torch or pa.keep is not pts or oa.keep is not ok:
                raise ValueError("out: (points, ok), contiguous uint8 arrays of %d x 64 and %d bytes of msgs' kind expected" % (n, n))
            pptr, okptr = pa.ptr, oa.ptr
        self._bind_stream([ma])
        self._check(self._lib.jj_group_hash(self._ctx, C.c_size_t(n), personal, prefix, C.c_size_t(plen), ma.ptr, C.c_size_t(ma.len), C.c_size_t(ma.stride), C.c_uint(flags), pptr, okptr))
        return pts, ok

    def find_group_hash(self, msgs, personal, prefix=b"", flags=GROUP_HASH_FLAGS):
        """The first counter at which the group hash exists, for every message -> (points (m, 64), counters (m,) uint8): ONE group_hash call
        over the 256 m rows msgs[j] || byte(i), i = 0..255, and per message the point of the smallest i with ok = 1 and that i.  msgs: (m, L)
        uint8, a numpy array or a CUDA tensor; the results are of its kind (device points can go straight into pedersen_table).  Raises
        JubjubError if a message has no counter with a point: about 47 % of digests decode, so the chance is about 0.53^256 = 2^-234 per message;
        with FLAG_TORSION_FREE an eighth of those remain and it is about 0.94^256 = 2 * 10^-7, which a caller of many messages may meet."""
        shape = tuple(msgs.shape) if hasattr(msgs, "shape") else None
        if shape is None or len(shape) != 2:
            raise ValueError("msgs: shape (m, L) expected, got %r" % (shape,))
        m, L = shape
        if _is_torch(msgs):
            import torch

            rows = torch.empty((m, 256, L + 1), dtype=torch.uint8, device=msgs.device)
            rows[:, :, :L] = msgs[:, None, :]
            rows[:, :, L] = torch.arange(256, dtype=torch.uint8, device=msgs.device)[None, :]
            pts, ok = self.group_hash(rows.view(m * 256, L + 1), personal, prefix, flags)
            ok = ok.view(m, 256) != 0
            first = ok.to(torch.uint8).argmax(dim=1)
            found = bool(ok.any(dim=1).all().item()) if m else True
            sel = pts.view(m, 256, 64)[torch.arange(m, device=msgs.device), first] if m else pts.view(0, 64)
            first = first.to(torch.uint8)
        else:
            msgs = _host_bytes(msgs).reshape(m, L)
            rows = np.empty((m, 256, L + 1), np.uint8)
            rows[:, :, :L] = msgs[:, None, :]
            rows[:, :, L] = np.arange(256, dtype=np.uint8)[None, :]
            pts, ok = self.group_hash(rows.reshape(m * 256, L + 1), personal, prefix, flags)
            ok = ok.reshape(m, 256) != 0
            first = ok.argmax(axis=1)
            found = bool(ok.any(axis=1).all())
            sel = pts.reshape(m, 256, 64)[np.arange(m), first]
            first = first.astype(np.uint8)
        if not found:
            raise JubjubError("find_group_hash: a message has no counter 0..255 with a point")
        return sel, first

    def msm_finish(self, job):
        """-> the 64-byte affine sum as a numpy array (host memory)."""
        if job._h is None:
            raise JubjubError("MSM job already finished")
        out = np.empty((64,), np.uint8)
        h, job._h = job._h, None
        try:
            self._check(self._lib.jj_msm_finish(h, out.ctypes.data))      # waits for the job's kernels: they run on a lane no other stream is ordered with ...
        finally:
            job._keep = None                                              # ... so the inputs are released only now (a caching allocator could hand the block on at once)
        return out

    def msm_partial(self, scalars, points, part_index=0, part_count=1):
        """First half of an MSM cut across devices / ranks (jj_msm_partial): the record of partial window sums
        (MSM_PARTIAL_BYTES bytes, same kind of array as the inputs: a CUDA tensor is ready for all_gather over RCCL).
        part_index = g, part_count = G: windows g, g + G, ... of ALL the terms given (window partition); 0 / 1: all windows
        of the terms given (term partition)."""
        a, p = _Arg(scalars, 32), _Arg(points, 64)
        if a.n != p.n:
            raise ValueError("length mismatch: %d vs %d" % (a.n, p.n))
        self._bind_stream([a, p])
        out, optr = self._alloc(a, _lib.MSM_PARTIAL_BYTES, 1)
        self._check(self._lib.jj_msm_partial(self._ctx, C.c_size_t(a.n), a.ptr, p.ptr, C.c_int(part_index), C.c_int(part_count), optr))
        return out

    def set_comm(self, comm):
        """Lends the context an RCCL communicator (jj_ctx_set_comm): `comm` is a jubjub_amd.dist.RcclComm (or None to detach)."""
        if comm is None:
            self._check(self._lib.jj_ctx_set_comm(self._ctx, None, 0, 1, None))
            self._comm = None
            return
        self._check(self._lib.jj_ctx_set_comm(self._ctx, C.c_void_p(comm.handle), C.c_int(comm.rank), C.c_int(comm.world), C.c_void_p(comm.all_gather_addr)))
        self._comm = comm                                          # keep the communicator (and its library) alive

    def msm_allgather(self, scalars, points, partition="terms"):
        """One MSM over all ranks of the communicator lent with set_comm, entirely behind the C ABI (jj_msm_allgather): record of
        window sums -> ncclAllGather over xGMI -> the gathered records folded into one on the device (from 8 ranks; below that one copy of all of them) -> one host tail.  partition "terms": the arrays are THIS
        rank's terms; "window": ALL terms on every rank.  Returns the 64-byte affine sum as a numpy array (host) on every rank."""
        a, p = _Arg(scalars, 32), _Arg(points, 64)
        if a.n != p.n:
            raise ValueError("length mismatch: %d vs %d" % (a.n, p.n))
        self._bind_stream([a, p])
        out = np.empty((64,), np.uint8)
        self._check(self._lib.jj_msm_allgather(self._ctx, C.c_size_t(a.n), a.ptr, p.ptr, C.c_int({"terms": 0, "window": 1}[partition]), out.ctypes.data))
        return out

    def msm_allgather_begin(self, scalars, points, partition="terms"):
        """msm_allgather in two halves (jj_msm_allgather_begin): queues this rank's window sums, the ncclAllGather and the fold of the
        gathered records, returns a job; msm_finish(job) waits for it and runs the host tail.  With several jobs in flight the exchange
        and the host tail of one MSM overlap the kernels of the next.  A collective: every rank begins the same jobs in the same order."""
        a, p = _Arg(scalars, 32), _Arg(points, 64)
        if a.n != p.n:
            raise ValueError("length mismatch: %d vs %d" % (a.n, p.n))
        self._bind_stream([a, p])
        h = C.c_void_p()
        self._check(self._lib.jj_msm_allgather_begin(self._ctx, C.c_size_t(a.n), a.ptr, p.ptr, C.c_int({"terms": 0, "window": 1}[partition]), C.byref(h)))
        return MsmJob(h, (a.keep, p.keep))

    def msm_combine(self, records):
        """Second half: any number of records (count x MSM_PARTIAL_BYTES bytes) -> the 64-byte affine sum as a numpy array.  A CUDA
        tensor takes jj_msm_combine_dev (the records are added on the device, ONE record is copied to the host tail); numpy / CPU
        tensors take jj_msm_combine (host only)."""
        is_torch = type(records).__module__.startswith("torch")
        if is_torch and records.is_cuda:
            # device-resident records (what all_gather delivered): folded window by window on the device, one record goes to the host tail
            t = records.detach().contiguous().view(-1, _lib.MSM_PARTIAL_BYTES)
            self._bind_stream([_Arg(t, _lib.MSM_PARTIAL_BYTES)] if t.shape[0] else [])
            out = np.empty((64,), np.uint8)
            self._check(self._lib.jj_msm_combine_dev(self._ctx, C.c_size_t(t.shape[0]), C.c_void_p(t.data_ptr()) if t.shape[0] else None, out.ctypes.data))
            return out
        host = np.ascontiguousarray((records.detach().cpu().numpy() if is_torch else np.asarray(records)).reshape(-1, _lib.MSM_PARTIAL_BYTES), dtype=np.uint8)
        out = np.empty((64,), np.uint8)
        rc = self._lib.jj_msm_combine(C.c_size_t(host.shape[0]), host.ctypes.data if host.shape[0] else None, out.ctypes.data)
        if rc:
            raise JubjubError("jj_msm_combine failed (%d): damaged or mismatched MSM records" % rc)
        return out

    # -------------------------------------------------------------- encodings
    def decompress(self, enc, flags=FLAG_ZIP216, out=None):
        return self._call("jj_decompress", [enc], [32], [64, 1], extra_mid=(C.c_uint(flags),), out=out)

    def compress(self, points):
        return self._call("jj_compress", [points], [64], [32])

    def batch_normalize(self, ext160):
        return self._call("jj_batch_normalize", [ext160], [160], [64])

    # -------------------------------------------------------------- bit decomposition (reference src/fr.rs:746-785)
    def to_le_bits(self, field, a):
        return self._call("jj_%s_to_le_bits" % field, [a], [32], [256])

    def char_le_bits(self):
        out = (C.c_uint8 * 256)()
        self._check(self._lib.jj_fr_char_le_bits(out))
        return np.frombuffer(bytes(out), dtype=np.uint8)

    # -------------------------------------------------------------- synthetic inputs (reference Group::random, src/lib.rs:1244-1298)
    def _generate(self, name, n, width, device, extra):
        """device: None -> numpy result, else a torch device -> CUDA tensor on torch's current stream"""
        if device is None:
            out = np.empty((n, width), dtype=np.uint8)
            ptr = out.ctypes.data if n else None
            self._lib.jj_ctx_use_own_stream(self._ctx)
        else:
            import torch

            out = torch.empty((n, width), dtype=torch.uint8, device=device)
            ptr = out.data_ptr()
            self._lib.jj_ctx_set_stream(self._ctx, C.c_void_p(torch.cuda.current_stream(device).cuda_stream))
        self._check(getattr(self._lib, name)(self._ctx, C.c_size_t(n), *extra(ptr)))
        return out

    def synth_scalars(self, n, seed, first_index=0, device=None):
        return self._generate("jj_synth_scalars", n, 32, device, lambda p: (C.c_uint64(seed), C.c_uint64(first_index), p))

    def synth_bytes32(self, n, seed, first_index=0, device=None):
        return self._generate("jj_synth_bytes32", n, 32, device, lambda p: (C.c_uint64(seed), C.c_uint64(first_index), p))

    def random_points(self, n, seed, first_index=0, subgroup=False, device=None):
        return self._generate("jj_random_points", n, 64, device,
                              lambda p: (C.c_uint64(seed), C.c_uint64(first_index), C.c_int(1 if subgroup else 0), p, None))



def _locked(fn):
    @functools.wraps(fn)
    def wrapper(self, *a, **k):
        with self._mu:
            return fn(self, *a, **k)
    return wrapper


# Engine methods select the launch stream and then call the library: two host threads sharing an Engine must not
# interleave those two steps (the C entry points themselves serialise on the context lock).
for _name, _fn in list(vars(Engine).items()):
    if callable(_fn) and not _name.startswith("__"):
        setattr(Engine, _name, _locked(_fn))
Engine.group_by_key = staticmethod(_group_by_key)      # no context, no lock: Engine.group_by_key(A) or eng.group_by_key(A)


class MultiEngine:
    """Several devices of one node driven from one process (include/jubjub_hip.h jj_multi_*): one context, host thread and
    stream per listed device, contiguous shards, host (numpy) arrays in and out; the MSM's per-device partial points are
    added on the host.  A device may be listed more than once."""

    def __init__(self, devices):
        self._lib = _lib.load()
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        h = C.c_void_p()
        rc = self._lib.jj_multi_create(devs, C.c_int(len(devices)), C.byref(h))
        self._h = None
        if rc != 0:
            raise JubjubError("jj_multi_create(%r) failed with %d" % (list(devices), rc))
        self._h = h
        self._tables = []

    def close(self):
        if self._h is not None:
            for t in self._tables:
                self._lib.jj_multi_fixedbase_table_destroy(self._h, t)
            self._tables = []
            self._lib.jj_multi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise JubjubError("rc=%d: %s" % (rc, (self._lib.jj_multi_last_error(self._h) or b"").decode()))

    @property
    def device_count(self):
        return self._lib.jj_multi_device_count(self._h)

    @staticmethod
    def _np(x, width):
        a = np.ascontiguousarray(x, dtype=np.uint8).reshape(-1, width)
        return a, (a.ctypes.data if a.size else None)

    @staticmethod
    def _out(out, shape):
        """a caller-owned result array (e.g. page-locked, reused across calls) or a fresh one"""
        if out is None:
            return np.empty(shape, np.uint8)
        if out.dtype != np.uint8 or not out.flags["C_CONTIGUOUS"] or out.size != int(np.prod(shape)):
            raise ValueError("out: a contiguous uint8 array of shape %r expected" % (shape,))
        return out

    def varbase_mul(self, scalars, points, out=None):
        s, sp = self._np(scalars, 32)
        p, pp = self._np(points, 64)
        if len(s) != len(p):
            raise ValueError("length mismatch")
        out = self._out(out, (len(s), 64))
        self._check(self._lib.jj_multi_varbase_mul(self._h, C.c_size_t(len(s)), sp, pp, out.ctypes.data if len(s) else None))
        return out

    def fixedbase_table(self, base, window_bits=0):
        b, bp = self._np(base, 64)
        t = C.c_void_p()
        self._check(self._lib.jj_multi_fixedbase_table_create(self._h, bp, C.c_int(window_bits), C.byref(t)))
        self._tables.append(t)
        return t

    def fixedbase_mul(self, table, scalars, out=None):
        s, sp = self._np(scalars, 32)
        out = self._out(out, (len(s), 64))
        self._check(self._lib.jj_multi_fixedbase_mul(self._h, table, C.c_size_t(len(s)), sp, out.ctypes.data if len(s) else None))
        return out

    def decompress(self, enc, flags=FLAG_ZIP216, out=None):
        e, ep = self._np(enc, 32)
        out, ok = (self._out(out[0], (len(e), 64)), self._out(out[1], (len(e),))) if out is not None else (np.empty((len(e), 64), np.uint8), np.empty((len(e),), np.uint8))
        self._check(self._lib.jj_multi_decompress(self._h, C.c_size_t(len(e)), ep, C.c_uint(flags), out.ctypes.data if len(e) else None,
                                                  ok.ctypes.data if len(e) else None))
        return out, ok

    def msm(self, scalars, points):
        s, sp = self._np(scalars, 32)
        p, pp = self._np(points, 64)
        if len(s) != len(p):
            raise ValueError("length mismatch")
        out = np.empty((64,), np.uint8)
        self._check(self._lib.jj_multi_msm(self._h, C.c_size_t(len(s)), sp, pp, out.ctypes.data))
        return out

    def msm_batch(self, scalars, points, out=None):
        """jj_multi_msm_batch: Engine.msm_batch's shapes, rows cut into one contiguous block per device; host (numpy) arrays in and out"""
        B, n, shared = _msm_batch_shapes(scalars, points)
        s, sp = self._np(scalars, 32)
        p, pp = self._np(points, 64)
        out = self._out(out, (B, 64))
        self._check(self._lib.jj_multi_msm_batch(self._h, C.c_size_t(B), C.c_size_t(n), sp, pp, C.c_int(shared), out.ctypes.data if B else None))
        return out
