"""The 32-bit row offsets of k_sig_challenge, k_blake2s and k_pedersen_*, and the 64-bit products i * in_stride of k_chacha20_xor, k_poly1305 and
k_aead, on the GPU at the layouts of tests/high_offset_cases.py: rows that end at 2^31, lie across it, start at it, and a last row that ends
exactly at 2^32 -- the largest calls the ABI accepts.

One input buffer of 2^32 bytes is filled on the device from a seeded generator (in chunks, so that it can be made again chunk by chunk for a
comparison) and one output buffer of 2^32 + 2^26 bytes lies beside it; nothing large crosses PCIe.  PEAK DEVICE MEMORY: 8.1 GiB of these two
buffers and, with the 2^22 keys, tags and ok bytes and the comparison's chunk beside them, 8.8 GiB in all (measured: 8.82 GiB of tensors); an
allocation that fails fails the test.

Every layout is held three ways:
 1. the oracle on NAMED rows, byte for byte (rows 0 and 1, every row that touches [2^31 - 2 rowbytes, 2^31 + 2 rowbytes), the last three, 64
    seeded others; every row of a sparse layout), the rows copied back one by one, against tests/ka_cases.py, tests/aead_cases.py, hashlib,
    tests/sig_challenge_cases.py, tests/group_hash_cases.py and tests/pedersen_cases.py;
 2. for ALL rows of a dense layout, the same call in two halves that both run below 2^31 -- rows [0, k) from the base and rows [k, n) from
    base + k * stride (16-byte aligned) -- compared on the device with the whole call: the library at low offsets, which the rest of the suite
    holds to the oracle, is the reference for the rows not named.  Where the output is as large as the input (jj_chacha20_xor, jj_aead_seal)
    two outputs do not fit beside the input, and the halves run the INVERSE on the whole call's output instead: the halves of the cipher
    applied to the whole call's output must give the input buffer back (compared with the regenerated fill), and jj_aead_open in halves must
    accept every row jj_aead_seal wrote in one call and return the input;
 3. the digests or tags of a dense call are pairwise distinct: a row that aliases another through a lost high bit shows here.
Durations are printed, never asserted."""
import ctypes as C
import hashlib
import time

import numpy as np
import pytest

from oracle import jubjub_ref as J
from tests import aead_cases as AC
from tests import group_hash_cases as GH
from tests import high_offset_cases as HC
from tests import ka_cases as KC
from tests import pedersen_cases as PC
from tests import sig_challenge_cases as CC

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

T31, T32 = HC.T31, HC.T32
CHUNK_WORDS = 1 << 23                          # the buffer is filled, and made again, 2^26 bytes at a time
SEED = 0x4A4A4F4646
NONCE = AC.NONCE
AAD = b"high offsets"
COUNTER = 7
PREFIX = np.random.default_rng(4471).integers(0, 256, HC.B2S_PREFIX_LEN, dtype=np.uint8).tobytes()
GH_FLAGS = GH.SAPLING_SHAPED


class Env:
    def __init__(self):
        from jubjub_amd import Engine, _lib

        self.eng = Engine(0)
        self.lib, self.ctx, self.INVALID = self.eng._lib, self.eng._ctx, _lib.JJ_ERR_INVALID
        self.lib.jj_ctx_use_own_stream(self.ctx)
        self.dev = torch.device("cuda", 0)
        try:
            self.words = torch.empty(T32 // 8, dtype=torch.int64, device=self.dev)
            self.out = torch.empty(T32 + (1 << 26), dtype=torch.uint8, device=self.dev)
            self.tmp = torch.empty(CHUNK_WORDS, dtype=torch.int64, device=self.dev)
        except RuntimeError as e:                                      # torch.cuda.OutOfMemoryError is one
            pytest.fail("the high-offset tests need about 8.8 GiB of device memory: %s" % e)
        self.buf = self.words.view(torch.uint8)
        assert self.buf.data_ptr() % 16 == 0 and self.out.data_ptr() % 16 == 0
        self.fill()
        self._keys = {}
        self.g = torch.Generator(device=self.dev)
        self.g.manual_seed(SEED + 1)

    def _chunks(self, into=None):
        g = torch.Generator(device=self.dev)
        g.manual_seed(SEED)
        for c in range(0, T32 // 8, CHUNK_WORDS):
            dst = self.words[c:c + CHUNK_WORDS] if into is None else into
            torch.randint(-(1 << 63), (1 << 63) - 1, (CHUNK_WORDS,), dtype=torch.int64, device=self.dev, generator=g, out=dst)
            yield c * 8

    def fill(self):
        for _ in self._chunks():
            pass
        torch.cuda.synchronize()

    def changed_rows(self, rowlen):
        """the rows of `rowlen` bytes in which the buffer differs from its fill, compared on the device chunk by chunk"""
        rows = set()
        for lo in self._chunks(into=self.tmp):
            ne = self.tmp.view(torch.uint8) != self.buf[lo:lo + 8 * CHUNK_WORDS]
            count = int(ne.sum())
            assert count <= 1 << 16, "%d bytes of the chunk at %d differ from the fill" % (count, lo)
            if count:
                rows |= {int(x) for x in torch.unique((ne.nonzero().reshape(-1) + lo) // rowlen).cpu()}
        return rows

    def keys(self, n):
        if n not in self._keys:
            self._keys[n] = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=self.dev, generator=self.g)
        return self._keys[n]

    def rand(self, *shape):
        return torch.randint(0, 256, shape, dtype=torch.uint8, device=self.dev, generator=self.g)

    def call(self, name, *args, want=0):
        torch.cuda.synchronize()
        rc = getattr(self.lib, name)(self.ctx, *args)
        assert rc == want, (name, rc, self.lib.jj_last_error(self.ctx))
        assert self.lib.jj_ctx_sync(self.ctx) == 0
        return rc

    def read(self, t, lo, nbytes):
        return t[lo:lo + nbytes].cpu().numpy().tobytes()

    def close(self):
        del self.words, self.buf, self.out, self.tmp, self._keys
        self.eng.close()
        torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def env():
    torch.cuda.reset_peak_memory_stats()
    e = Env()
    yield e
    print("peak device memory of the module's tensors: %.2f GiB" % (torch.cuda.max_memory_allocated() / 2.0 ** 30))
    e.close()


@pytest.fixture(autouse=True)
def duration(request):
    t0 = time.perf_counter()
    yield
    print("%s: %.2f s" % (request.node.name, time.perf_counter() - t0))


def ptr(t, off=0):
    return C.c_void_p(t.data_ptr() + off)


def sz(x):
    return C.c_size_t(x)


def ids(layouts):
    return [L.id for L in layouts]


def distinct(t):
    """every row of a (n, 8 m) uint8 tensor differs from every other"""
    return torch.unique(t.contiguous().view(torch.int64).reshape(t.shape[0], -1), dim=0).shape[0] == t.shape[0]


# ---------------------------------------------------------------------------------------------------- jj_chacha20_xor
@pytest.mark.parametrize("L", HC.CHACHA20, ids=ids(HC.CHACHA20))
def test_chacha20_xor(env, L):
    keys = env.keys(L.n)
    args = lambda n, kofs, src, sofs, dst, dofs: (sz(n), ptr(keys, kofs), NONCE, C.c_uint(COUNTER), ptr(src, sofs), sz(L.length), sz(L.stride), ptr(dst, dofs))      # noqa: E731
    if L.dense:                                                        # one row more than 2^32 bytes is refused, the limit itself accepted
        env.call("jj_chacha20_xor", *args(L.n + 1, 0, env.buf, 0, env.out, 0), want=env.INVALID)
    env.call("jj_chacha20_xor", *args(L.n, 0, env.buf, 0, env.out, 0))
    for i in L.named_rows():
        row = np.frombuffer(env.read(env.buf, L.start(i), L.length), np.uint8)
        ks = np.frombuffer(KC.keystream(keys[i].cpu().numpy().tobytes(), COUNTER, NONCE, L.length), np.uint8)
        assert env.read(env.out, i * L.length, L.length) == (row ^ ks).tobytes(), "row %d at byte %d" % (i, L.start(i))
    if L.dense:
        k = L.split_row()
        try:                                                           # the halves undo the whole call: the buffer's fill comes back
            env.call("jj_chacha20_xor", *args(k, 0, env.out, 0, env.buf, 0))
            env.call("jj_chacha20_xor", *args(L.n - k, 32 * k, env.out, k * L.stride, env.buf, k * L.length))
            assert env.changed_rows(L.length) == set()
        except BaseException:
            env.fill()
            raise


# ---------------------------------------------------------------------------------------------------- jj_poly1305
@pytest.mark.parametrize("L", HC.POLY1305, ids=ids(HC.POLY1305))
def test_poly1305(env, L):
    keys = env.keys(L.n)
    tags = torch.zeros((L.n, 16), dtype=torch.uint8, device=env.dev)
    args = lambda n, kofs, sofs, dst, dofs: (sz(n), ptr(keys, kofs), ptr(env.buf, sofs), sz(L.length), sz(L.stride), ptr(dst, dofs))      # noqa: E731
    if L.dense:
        env.call("jj_poly1305", *args(L.n + 1, 0, 0, tags, 0), want=env.INVALID)
    env.call("jj_poly1305", *args(L.n, 0, 0, tags, 0))
    for i in L.named_rows():
        want = AC.poly1305(keys[i].cpu().numpy().tobytes(), env.read(env.buf, L.start(i), L.length))
        assert tags[i].cpu().numpy().tobytes() == want, "row %d at byte %d" % (i, L.start(i))
    if L.dense:
        k = L.split_row()
        halves = torch.zeros_like(tags)
        env.call("jj_poly1305", *args(k, 0, 0, halves, 0))
        env.call("jj_poly1305", *args(L.n - k, 32 * k, k * L.stride, halves, 16 * k))
        assert torch.equal(halves, tags)
        assert distinct(tags)


# ---------------------------------------------------------------------------------------------------- jj_aead_seal, jj_aead_open
def seal_args(L, keys, n, kofs, src, sofs, dst, dofs):
    return (sz(n), ptr(keys, kofs), NONCE, AAD, sz(len(AAD)), ptr(src, sofs), sz(L.length), sz(L.stride), ptr(dst, dofs))


def open_args(L, keys, n, kofs, src, sofs, dst, dofs, ok, okofs):
    return (sz(n), ptr(keys, kofs), NONCE, AAD, sz(len(AAD)), ptr(src, sofs), sz(L.length), sz(L.stride), ptr(dst, dofs), C.cast(ok.data_ptr() + okofs, C.POINTER(C.c_uint8)))


def test_aead_sparse(env):
    S, O = HC.AEAD_SEAL[0], HC.AEAD_OPEN[0]
    keys = env.keys(S.n)
    env.call("jj_aead_seal", *seal_args(S, keys, S.n, 0, env.buf, 0, env.out, 0))
    hk = keys.cpu().numpy()
    for i in range(S.n):
        want = AC.seal_one(hk[i].tobytes(), NONCE, AAD, env.read(env.buf, S.start(i), S.length))
        assert env.read(env.out, i * S.out_row, S.out_row) == want, "sealed row %d" % i
    # open: rows the restatement sealed, planted at the sparse offsets of the output buffer
    plain = np.random.default_rng(9911).integers(0, 256, (O.n, O.length), dtype=np.uint8)
    for i in range(O.n):
        row = np.frombuffer(AC.seal_one(hk[i].tobytes(), NONCE, AAD, plain[i].tobytes()), np.uint8)
        env.out[O.start(i):O.end(i)] = torch.from_numpy(row.copy()).to(env.dev)
    got, ok = torch.full((O.n, O.length), 0xEE, dtype=torch.uint8, device=env.dev), torch.full((16,), 0xEE, dtype=torch.uint8, device=env.dev)
    env.call("jj_aead_open", *open_args(O, keys, O.n, 0, env.out, 0, got, 0, ok, 0))
    assert ok[:O.n].tolist() == [1] * O.n and (got.cpu().numpy() == plain).all()
    env.out[O.start(3) + O.length + 15] ^= 0x80                        # the last byte of the last row's tag
    env.out[O.start(2) + 600] ^= 1                                     # a ciphertext byte behind 2^31 in the row across it
    env.call("jj_aead_open", *open_args(O, keys, O.n, 0, env.out, 0, got, 0, ok, 0))
    assert ok[:O.n].tolist() == [1, 1, 0, 0] and (got[:2].cpu().numpy() == plain[:2]).all() and not bool(got[2:].any())


def test_aead_round_trip_dense(env):
    S, O = HC.SEAL_DENSE, HC.OPEN_DENSE
    n = S.n
    keys = env.keys(n)
    env.call("jj_aead_seal", *seal_args(S, keys, n, 0, env.buf, 0, env.out, 0))                            # 2^22 x 1008 bytes in, 2^32 bytes out
    for i in sorted(set(S.named_rows()) | set(O.named_rows())):
        want = AC.seal_one(keys[i].cpu().numpy().tobytes(), NONCE, AAD, env.read(env.buf, S.start(i), S.length))
        assert env.read(env.out, O.start(i), O.rowbytes) == want, "sealed row %d, written at byte %d" % (i, O.start(i))
    sealed = env.out[:T32].view(n, O.stride)
    assert distinct(sealed[:, O.length:])                                                                  # the n tags
    ok = torch.zeros(n, dtype=torch.uint8, device=env.dev)
    try:
        env.call("jj_aead_open", *open_args(O, keys, n + 1, 0, env.out, 0, env.buf, 0, ok, 0), want=env.INVALID)
        env.call("jj_aead_open", *open_args(O, keys, n, 0, env.out, 0, env.buf, 0, ok, 0))               # the whole call: rows up to 2^32
        assert bool(ok.all()) and env.changed_rows(O.length) == set()
        k = O.split_row()
        ok.zero_()
        env.call("jj_aead_open", *open_args(O, keys, k, 0, env.out, 0, env.buf, 0, ok, 0))               # the halves: both below 2^31
        env.call("jj_aead_open", *open_args(O, keys, n - k, 32 * k, env.out, k * O.stride, env.buf, k * O.length, ok, k))
        assert bool(ok.all()) and env.changed_rows(O.length) == set()
        at31 = T31 // O.stride                                                                             # the row at 2^31; the row in front of it ends there
        env.out[O.start(at31) + O.length + 3] ^= 0x10                                                      # a tag bit
        env.out[T32 - 1] ^= 0x80                                                                           # the last bit of the last row's tag
        env.out[17] ^= 1                                                                                   # a ciphertext bit of row 0
        victims = {0, at31, n - 1}
        env.call("jj_aead_open", *open_args(O, keys, n, 0, env.out, 0, env.buf, 0, ok, 0))
        bad = torch.nonzero(ok == 0).reshape(-1).tolist()
        assert set(bad) == victims and len(bad) == 3
        assert env.changed_rows(O.length) == victims                                                       # the others are unchanged ...
        for i in victims:
            assert not bool(env.buf[i * O.length:(i + 1) * O.length].any())                                # ... and these are all zeros
    finally:
        env.fill()


# ---------------------------------------------------------------------------------------------------- jj_blake2s, jj_group_hash
def b2s_args(L, n, sofs, dst, dofs):
    return (sz(n), HC.B2S_PERSONAL, PREFIX, sz(len(PREFIX)), ptr_of(sofs), sz(L.length), sz(L.stride), ptr(dst, dofs))


def ptr_of(x):
    return x if isinstance(x, C.c_void_p) else C.c_void_p(x)


@pytest.fixture(scope="module")
def digests(env):
    """the whole call of every BLAKE2s layout, made once: test_blake2s holds it, test_group_hash builds on it"""
    made = {}

    def get(L):
        if L.id not in made:
            d = torch.zeros((L.n, 32), dtype=torch.uint8, device=env.dev)
            env.call("jj_blake2s", *b2s_args(L, L.n, env.buf.data_ptr(), d, 0))
            made[L.id] = d
        return made[L.id]

    return get


@pytest.mark.parametrize("L", HC.BLAKE2S, ids=ids(HC.BLAKE2S))
def test_blake2s(env, digests, L):
    base = env.buf.data_ptr()
    if L.span == T32:
        env.call("jj_blake2s", *b2s_args(L, L.n + 1, base, env.out, 0), want=env.INVALID)
    d = digests(L)
    for i in L.named_rows():
        want = hashlib.blake2s(PREFIX + env.read(env.buf, L.start(i), L.length), digest_size=32, person=HC.B2S_PERSONAL).digest()
        assert d[i].cpu().numpy().tobytes() == want, "row %d at byte %d" % (i, L.start(i))
    if L.dense:
        k = L.split_row()
        halves = torch.zeros_like(d)
        env.call("jj_blake2s", *b2s_args(L, k, base, halves, 0))
        env.call("jj_blake2s", *b2s_args(L, L.n - k, base + k * L.stride, halves, 32 * k))
        assert torch.equal(halves, d)
        assert distinct(d)


@pytest.mark.parametrize("L", HC.GROUP_HASH[:2], ids=ids(HC.GROUP_HASH[:2]))
def test_group_hash(env, digests, L):
    pts, ok = torch.zeros((L.n, 64), dtype=torch.uint8, device=env.dev), torch.zeros(L.n, dtype=torch.uint8, device=env.dev)
    okp = lambda t, o=0: C.cast(t.data_ptr() + o, C.POINTER(C.c_uint8))      # noqa: E731
    gh = lambda n, sofs, p, pofs, o, oofs: (sz(n), HC.B2S_PERSONAL, PREFIX, sz(len(PREFIX)), C.c_void_p(sofs), sz(L.length), sz(L.stride), C.c_uint(GH_FLAGS), ptr(p, pofs), okp(o, oofs))      # noqa: E731
    base = env.buf.data_ptr()
    env.call("jj_group_hash", *gh(L.n, base, pts, 0, ok, 0))
    # the decoder over the digests of jj_blake2s, under the same flags: points and ok bytes alike, on every row
    pts2, ok2 = torch.zeros_like(pts), torch.zeros_like(ok)
    env.call("jj_decompress", sz(L.n), ptr(digests(L)), C.c_uint(GH_FLAGS), ptr(pts2), okp(ok2))
    assert torch.equal(pts, pts2) and torch.equal(ok, ok2)
    named = L.named_rows()
    want_pts, want_ok = GH.expected(HC.B2S_PERSONAL, PREFIX, [env.read(env.buf, L.start(i), L.length) for i in named], GH_FLAGS)
    idx = torch.tensor(named, device=env.dev)
    assert (ok[idx].cpu().numpy() == want_ok).all() and (pts[idx].cpu().numpy() == want_pts).all()
    assert 0 < int(ok.sum()) < L.n or L.n <= 4
    if L.dense:
        k = L.split_row()
        env.call("jj_group_hash", *gh(k, base, pts2, 0, ok2, 0))
        env.call("jj_group_hash", *gh(L.n - k, base + k * L.stride, pts2, 64 * k, ok2, k))
        assert torch.equal(pts, pts2) and torch.equal(ok, ok2)
        good = ok.bool()
        assert distinct(pts[good])


def test_blake2s_sparse_from_a_pageable_host_array():
    """the bounce path: a pageable numpy array of 3 * stride + 150 bytes with only the four rows written, staged through a 3 GiB copy.  Its own
    context, closed afterwards: staging keeps its buffer."""
    from jubjub_amd import Engine

    L = HC.B2S_SPARSE
    msgs = np.zeros(L.span, np.uint8)
    rows = np.random.default_rng(6106).integers(0, 256, (L.n, L.length), dtype=np.uint8)
    for i in range(L.n):
        msgs[L.start(i):L.end(i)] = rows[i]
    view = np.lib.stride_tricks.as_strided(msgs, shape=(L.n, L.length), strides=(L.stride, 1), writeable=False)
    eng = Engine(0)
    try:
        t0 = time.perf_counter()
        got = eng.blake2s(view, HC.B2S_PERSONAL, PREFIX)
        print("jj_blake2s over a pageable host array of %d bytes: %.2f s" % (L.span, time.perf_counter() - t0))
    finally:
        eng.close()
    for i in range(L.n):
        assert got[i].tobytes() == hashlib.blake2s(PREFIX + rows[i].tobytes(), digest_size=32, person=HC.B2S_PERSONAL).digest(), i


# ---------------------------------------------------------------------------------------------------- jj_sig_challenge
def sig_args(n, R, A, rofs, msgs, msg_len, offsets, dst, dofs):
    return (sz(n), HC.SIG_PERSONAL, ptr(R, rofs) if R is not None else None, ptr(A, rofs) if A is not None else None, C.c_void_p(msgs), sz(msg_len),
            offsets.ctypes.data_as(C.c_void_p) if offsets is not None else None, ptr(dst, dofs))


def test_sig_challenge_fixed(env):
    L = HC.SIG_FIXED
    n, base = L.n, env.buf.data_ptr()
    R, A = env.rand(n + 1, 32), env.rand(n + 1, 32)
    c = torch.zeros((n, 32), dtype=torch.uint8, device=env.dev)
    env.call("jj_sig_challenge", *sig_args(n + 1, R, A, 0, base, L.length, None, env.out, 0), want=env.INVALID)
    env.call("jj_sig_challenge", *sig_args(n, R, A, 0, base, L.length, None, c, 0))
    for i in L.named_rows():
        want = CC.challenge(HC.SIG_PERSONAL, R[i].cpu().numpy().tobytes() + A[i].cpu().numpy().tobytes() + env.read(env.buf, L.start(i), L.length))
        assert (c[i].cpu().numpy() == want).all(), "message %d at byte %d" % (i, L.start(i))
    k = L.split_row()
    halves = torch.zeros_like(c)
    env.call("jj_sig_challenge", *sig_args(k, R, A, 0, base, L.length, None, halves, 0))
    env.call("jj_sig_challenge", *sig_args(n - k, R, A, 32 * k, base + k * L.stride, L.length, None, halves, 32 * k))
    assert torch.equal(halves, c)
    assert distinct(c)


@pytest.mark.parametrize("parts", [2, 0])
def test_sig_challenge_ragged(env, parts):
    off = HC.sig_ragged_offsets()
    n, base = len(off) - 1, env.buf.data_ptr()
    R, A = (env.rand(n, 32), env.rand(n, 32)) if parts else (None, None)
    c = torch.zeros((n, 32), dtype=torch.uint8, device=env.dev)
    over = off.copy()
    over[-1] += 1                                                     # one byte more than 2^32 in all
    env.call("jj_sig_challenge", *sig_args(n, R, A, 0, base, 0, over, env.out, 0), want=env.INVALID)
    env.call("jj_sig_challenge", *sig_args(n, R, A, 0, base, 0, off, c, 0))
    for i in HC.sig_ragged_named(off):
        lo, hi = int(off[i]), int(off[i + 1])
        head = R[i].cpu().numpy().tobytes() + A[i].cpu().numpy().tobytes() if parts else b""
        want = CC.challenge(HC.SIG_PERSONAL, head + env.read(env.buf, lo, hi - lo))
        assert (c[i].cpu().numpy() == want).all(), "message %d, bytes %d .. %d" % (i, lo, hi)
    # the three empty messages at offset 2^32: the hash of the parts alone
    for i in range(n - HC.SIG_RAGGED_EMPTY, n):
        head = R[i].cpu().numpy().tobytes() + A[i].cpu().numpy().tobytes() if parts else b""
        assert (c[i].cpu().numpy() == CC.challenge(HC.SIG_PERSONAL, head)).all(), i
    # two halves below 2^31: the second from a 16-byte aligned message start, its offsets counted from there
    k = next(j for d in range(n) for j in (n // 2 - d, n // 2 + d) if int(off[j]) % 16 == 0)
    assert abs(int(off[k]) - T31) < 1 << 24
    first, second = off[:k + 1].copy(), (off[k:] - off[k]).astype(np.uint64)
    halves = torch.zeros_like(c)
    env.call("jj_sig_challenge", *sig_args(k, R, A, 0, base, 0, first, halves, 0))
    env.call("jj_sig_challenge", *sig_args(n - k, R, A, 32 * k, base + int(off[k]), 0, second, halves, 32 * k))
    assert torch.equal(halves, c)
    if parts:
        assert distinct(c)
    else:
        assert distinct(c[:n - HC.SIG_RAGGED_EMPTY + 1]) and bool((c[n - HC.SIG_RAGGED_EMPTY:] == c[n - 1]).all())      # the empty ones alone coincide


# ---------------------------------------------------------------------------------------------------- jj_pedersen_hash_vartime, jj_pedersen_scalars
@pytest.mark.parametrize("P", HC.PEDERSEN, ids=[P.id for P in HC.PEDERSEN])
def test_pedersen(env, P):
    """every row of every layout against the restatement: the u-coordinate and the point under two table widths, and the scalars.  Layout d has
    cover = row_stride = 2^32: it is accepted and works (jj_pedersen.h: the 32-bit cover wraps to 0 and last_dword(0, 0) is the last dword)."""
    gs = PC.generators(P.gens)
    nseg, n, base = len(gs), P.n, env.buf.data_ptr()
    flat = [v for f in P.fields for v in f]
    fields = (C.c_uint32 * len(flat))(*flat)
    read = lambda lo, nbytes: env.read(env.buf, lo, nbytes)      # noqa: E731
    bits = [P.bits(i, read) for i in range(n)]
    want = np.stack([PC.point_bytes(PC.expected(gs, P.seg_chunks, b)) for b in bits])
    args = lambda nn: (sz(nn), C.c_uint(P.prefix), C.c_int(P.prefix_bits), C.c_void_p(base), sz(P.row_stride), C.c_int(len(P.fields)), fields)      # noqa: E731
    out = torch.zeros((n + 1, 64), dtype=torch.uint8, device=env.dev)
    for w in HC.PED_WINDOWS:
        t = env.eng.pedersen_table(PC.gens_bytes(P.gens), P.seg_chunks, w)
        env.lib.jj_ctx_use_own_stream(env.ctx)
        try:
            env.call("jj_pedersen_hash_vartime", t._h, *args(n + 1), C.c_uint(1), ptr(out), want=env.INVALID)      # one row more than 2^32 bytes
            assert b"2^32" in env.lib.jj_last_error(env.ctx)
            out.fill_(0xEE)
            env.call("jj_pedersen_hash_vartime", t._h, *args(n), C.c_uint(1), ptr(out))
            got = out.cpu().numpy()
            assert (got[:n] == want).all() and (got[n] == 0xEE).all(), "layout %s, window_chunks %d, points: rows %s differ" % (P.id, w, np.nonzero((got[:n] != want).any(axis=1))[0])
            out.fill_(0xEE)
            env.call("jj_pedersen_hash_vartime", t._h, *args(n), C.c_uint(0), ptr(out))
            got = out.reshape(-1, 32).cpu().numpy()
            assert (got[:n] == want[:, :32]).all() and (got[n:] == 0xEE).all(), "layout %s, window_chunks %d, u" % (P.id, w)
        finally:
            t.close()
    sc = torch.zeros((nseg, n, 32), dtype=torch.uint8, device=env.dev)
    env.call("jj_pedersen_scalars", C.c_int(nseg), C.c_int(P.seg_chunks), *args(n + 1), ptr(sc), want=env.INVALID)
    env.call("jj_pedersen_scalars", C.c_int(nseg), C.c_int(P.seg_chunks), *args(n), ptr(sc))
    got = sc.cpu().numpy()
    for i in range(n):
        for j, m in enumerate(PC.segment_sums(P.seg_chunks, nseg, bits[i])):
            assert got[j, i].tobytes() == (m % J.R_MOD).to_bytes(32, "little"), "layout %s, unit %d, segment %d" % (P.id, i, j)
