"""
GPU tests of jj_blake2s and jj_group_hash (BLAKE2s-256 over prefix || message in k_blake2s, then the decoder chain of jj_decompress as it is;
Engine.blake2s, Engine.group_hash, Engine.find_group_hash).  Every check demands byte equality -- with hashlib.blake2s for the digests, with
the restatement of tests/group_hash_cases.py (hashlib, tests/ka_cases.decode, three ext_double of oracle.jubjub_ref) for the points and ok
bytes --; no row is sampled or tolerated where a restatement is computed.  The digests over the whole cross product of prefix and message
lengths at every stride, the points over the seeded shapes of tests/group_hash_cases.py (every length, the totals 0, 64 and 128) under every
flag set, on host arrays and on device tensors; views that cannot be read in place, one row and several; the wave and workgroup edges; the composition
identity jj_group_hash = jj_decompress(jj_blake2s) across the seam between two chunks of 2^20 units, where the decoder takes its large-n
instantiation; the two buffer-discipline rows through the guarded arenas; find_group_hash against the restatement's loop; generators that
never leave the device, from find_group_hash into pedersen_table; every refused call with the outputs watched; and a sequence of calls that
share the decoder's workspaces on one context.
"""
import hashlib

import numpy as np
import pytest

from tests import group_hash_buffer_row as BR
from tests import group_hash_cases as GC
from tests import ka_cases as KC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from jubjub_amd import Engine

    e = Engine(0)
    yield e
    e.close()


def cuda(x):
    import torch

    return torch.from_numpy(np.array(x)).cuda()


def host(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


def same(got, want, what):
    got = host(got)
    assert got.shape == want.shape and got.dtype == np.uint8, (what, got.shape, want.shape)
    if got.ndim == 1:
        got, want = got.reshape(-1, 1), want.reshape(-1, 1)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert not len(bad), "%s: %d of %d rows differ from the restatement, the first is row %d" % (what, len(bad), len(want), bad[0])


def placed(msgs, pad, where):
    """the rows at a stride of msg_len + pad, as a view into one flat buffer on the host or on the device -> (buffer, view)"""
    buf, view = GC.layout(msgs, pad)
    if where == "device":
        buf = cuda(buf)
        view = buf.view(len(msgs), msgs.shape[1] + pad)[:, :msgs.shape[1]]
    return buf, view


def test_blake2s_equals_hashlib_over_the_matrix(eng):
    calls = 0
    for k, shape in enumerate(GC.PAIRS):                     # the whole cross product of the two lists; the shapes of the group-hash test on both sides
        person, prefix, msgs = GC.personal_of(shape), GC.prefix_of(shape), GC.messages(shape)
        want = GC.digests(person, prefix, msgs)
        for j, pad in enumerate(GC.PAD):
            for where in (("host", "device") if shape in GC.SHAPES else ("device" if (j + k) % 2 else "host",)):
                buf, view = placed(msgs, pad, where)
                before = host(buf).copy()
                got = eng.blake2s(view, person, prefix)
                what = "prefix %d, message %d, stride %d, %s" % (shape[0], shape[1], shape[1] + pad, where)
                assert (hasattr(got, "is_cuda") and got.is_cuda) == (where == "device"), what
                same(got, want, what)
                assert np.array_equal(host(buf), before), what                       # the rows and the bytes between them as they were
                calls += 1
    assert calls == len(GC.SHAPES) * 6 + (len(GC.PAIRS) - len(GC.SHAPES)) * 3 and len(GC.PAIRS) == 104
    # the wave and workgroup edges at the shape of a diversifier behind a 64-byte prefix
    person, prefix = GC.personal_of(GC.MAIN), GC.prefix_of(GC.MAIN)
    for n in (1, 63, 64, 65, 257):
        msgs = GC.messages(GC.MAIN, n)
        want = GC.digests(person, prefix, msgs)
        for pad in (0, 1):
            for where in ("host", "device"):
                same(eng.blake2s(placed(msgs, pad, where)[1], person, prefix), want, "n %d, pad %d, %s" % (n, pad, where))
    # RFC 7693's own value through the device
    assert host(eng.blake2s(np.frombuffer(b"abc", dtype=np.uint8).reshape(1, 3)))[0].tobytes().hex() == "508c5e8c327c14e2e1a72ba34eeb452f37458b209ed63a294d999b4c86675982"
    assert host(eng.blake2s(np.zeros((1, 0), np.uint8)))[0].tobytes().hex() == "69217a3079908094e11121d042354a7c1f55b6482ca1a51e1b250dfd1ed0eef9"


def test_views_the_library_cannot_read_in_place_are_copied(eng):
    """rows whose bytes are not adjacent, and device rows whose first byte is not 16-byte aligned, with ONE row and with several: the result
    is the hash of the view's bytes"""
    person, prefix = b"JJ_gh_vw", GC.PREFIX_POOL[:64]
    wide = KC.rng_bytes(9700, 8, 52)                                                      # candidate rows of 52 bytes
    dwide = cuda(wide)
    views = [("host", wide[:1, ::2]), ("host", wide[3:4, 1:23:2]), ("host", wide[:, ::2]), ("host", wide[::-1, :11]), ("host", wide[5:6, 7:18])]
    views += [("device", dwide[i:i + 1, :11]) for i in range(4)]                          # one-row slices: misaligned for three values of i in four
    views += [("device", dwide[1:3, :11]), ("device", dwide[:1, ::2]), ("device", dwide[:, 1::2]), ("device", dwide[2:3, 3:14])]
    assert sum(1 for w, v in views if w == "device" and v.shape[0] == 1 and v.data_ptr() % 16) >= 4
    for where, v in views:
        rows = host(v)
        what = "%s view of shape %r" % (where, tuple(v.shape))
        got = eng.blake2s(v, person, prefix)
        assert (hasattr(got, "is_cuda") and got.is_cuda) == (where == "device"), what
        same(got, GC.digests(person, prefix, rows), what)
        pts, ok = eng.group_hash(v, person, prefix, GC.SAPLING_SHAPED)
        want_pts, want_ok = GC.expected(person, prefix, rows, GC.SAPLING_SHAPED)
        same(pts, want_pts, what + " (points)")
        same(ok, want_ok, what + " (ok)")
    pts, first = eng.find_group_hash(dwide[1:2, :11], person, prefix)                    # one candidate's diversifier, where it lies
    b, i = GC.find_group_hash(person, prefix, wide[1, :11].tobytes(), GC.SAPLING_SHAPED)
    assert host(pts)[0].tobytes() == b and int(host(first)[0]) == i
    assert np.array_equal(host(dwide), wide)


def test_group_hash_equals_the_restatement_over_the_matrix(eng):
    calls = 0
    for si, shape in enumerate(GC.SHAPES):
        person, prefix, msgs = GC.personal_of(shape), GC.prefix_of(shape), GC.messages(shape)
        for fi, flags in enumerate(GC.FLAG_SETS):
            want_pts, want_ok = GC.case_expected(shape, flags)
            for pi, pad in enumerate(GC.PAD):
                where = "device" if (si + fi + pi) % 2 else "host"
                buf, view = placed(msgs, pad, where)
                pts, ok = eng.group_hash(view, person, prefix, flags)
                what = "prefix %d, message %d, stride %d, flags %d, %s" % (shape[0], shape[1], shape[1] + pad, flags, where)
                assert (hasattr(pts, "is_cuda") and pts.is_cuda) == (where == "device") == (hasattr(ok, "is_cuda") and ok.is_cuda), what
                same(pts, want_pts, what + " (points)")
                same(ok, want_ok, what + " (ok)")
                calls += 1
    assert calls == len(GC.SHAPES) * len(GC.FLAG_SETS) * len(GC.PAD)


def test_group_hash_is_decompress_of_blake2s_across_the_chunk_seam(eng):
    """2^20 + 3 rows of 11 bytes behind a 64-byte prefix, on the device: the one call equals the two calls byte for byte (the decoder's
    large-n instantiation on the first chunk, three rows in the second), and a seeded sample of the digests, the rows on both sides of
    index 2^20 among them, equals hashlib"""
    import torch

    N = (1 << 20) + 3
    person, prefix = b"JJ_gh_t0", GC.PREFIX_POOL[:64]
    g = torch.Generator(device="cpu").manual_seed(20260)
    msgs = torch.randint(0, 256, (N, 11), dtype=torch.uint8, generator=g).cuda()
    pts, ok = eng.group_hash(msgs, person, prefix, GC.SAPLING_SHAPED)
    dig = eng.blake2s(msgs, person, prefix)
    pts2, ok2 = eng.decompress(dig, GC.SAPLING_SHAPED)
    assert pts.is_cuda and tuple(pts.shape) == (N, 64) and tuple(ok.shape) == (N,) and tuple(dig.shape) == (N, 32)
    bad = (pts != pts2).any(dim=1) | (ok != ok2)
    assert not bool(bad.any()), "%d rows differ, the first is row %d" % (int(bad.sum()), int(bad.nonzero()[0]))
    share = float(ok.float().mean())
    assert 0.4 < share < 0.55 and bool(((ok == 0) | (ok == 1)).all()), share              # about 47 % of digests decode
    idx = np.unique(np.concatenate([np.random.default_rng(20261).integers(0, N, 4096 - 8), [0, 1, (1 << 20) - 2, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, N - 2, N - 1]]))
    tidx = torch.from_numpy(idx).cuda()
    rows, got = msgs[tidx].cpu().numpy(), dig[tidx].cpu().numpy()
    same(got, GC.digests(person, prefix, rows), "sampled digests")


def test_buffer_discipline_rows():
    """the rows of tests/group_hash_buffer_row.py through the runner of tests/test_gpu_buffers.py (its Env, checked_call, placements and
    skews): every size of the table x every skew (0, 16, 496 and the mixed one) in one device arena, the host arenas and the mixed placements
    at the host sizes, n = 0: return code 0, the output bytes equal to the restatement, guards and inputs untouched -- the byte between two
    message rows and the byte behind the last among them"""
    import test_gpu_buffers as TB

    env = TB.Env()
    try:
        for case in (BR.ROW_HASH, BR.ROW_GROUP):
            for options in case.options:
                for n in TB.SIZES:
                    for skew in TB.SKEW_SETS:
                        TB.checked_call(env, case, options, n, TB.placement(case, "dev", "dev"), skew)
                for n in TB.HOST_SIZES:
                    for ins, outs in (("host", "host"), ("pinned", "pinned"), ("dev", "host"), ("host", "dev"), ("dev", "pinned")):
                        TB.checked_call(env, case, options, n, TB.placement(case, ins, outs), TB.MIXED_SKEW)
                for where in ("dev", "host"):
                    for skew in (TB.SKEW_SETS[1], TB.MIXED_SKEW):
                        TB.checked_call(env, case, options, 0, TB.placement(case, where, where), skew)
    finally:
        env.close()


def test_find_group_hash_equals_the_restatements_loop(eng):
    from jubjub_amd.engine import GROUP_HASH_FLAGS

    person, prefix = b"JJ_gh_fd", GC.PREFIX_POOL[:64]
    msgs = KC.rng_bytes(9400, 16, 11)
    want = [GC.find_group_hash(person, prefix, m.tobytes(), GROUP_HASH_FLAGS) for m in msgs]
    want_pts = np.stack([np.frombuffer(b, dtype=np.uint8) for b, _ in want])
    want_i = np.array([i for _, i in want], np.uint8)
    assert want_i.max() >= 1                                                             # some message's first counter is not 0
    for where in ("host", "device"):
        pts, first = eng.find_group_hash(cuda(msgs) if where == "device" else msgs, person, prefix)
        assert (hasattr(pts, "is_cuda") and pts.is_cuda) == (where == "device")
        same(pts, want_pts, "find_group_hash points, " + where)
        same(first, want_i, "find_group_hash counters, " + where)
    with pytest.raises(ValueError):
        eng.find_group_hash(msgs[0], person, prefix)


def test_generators_stay_on_the_device_from_the_hash_to_the_pedersen_table(eng):
    from tests import pedersen_cases as PC

    every = GC.ZIP216 | GC.NOT_SMALL_ORDER | GC.CLEAR_COFACTOR | GC.TORSION_FREE
    names = np.stack([np.frombuffer(b"segment%d" % k, dtype=np.uint8) for k in range(3)])
    gens, first = eng.find_group_hash(cuda(names), b"JJ_gh_ph", GC.PREFIX_POOL[:64], every)
    assert gens.is_cuda and tuple(gens.shape) == (3, 64)
    case = PC.BY_ID["merkle"]
    table = eng.pedersen_table(gens, seg_chunks=case.seg_chunks)
    try:
        got = eng.pedersen_hash(table, cuda(case.rows[:8]), case.fields, prefix=case.prefix, prefix_bits=case.prefix_bits, point=True)
    finally:
        table.close()
    g = host(gens)
    gs = tuple((int.from_bytes(r[:32].tobytes(), "little"), int.from_bytes(r[32:].tobytes(), "little")) for r in g)
    assert len(set(gs)) == 3
    want = np.stack([PC.point_bytes(PC.expected(gs, case.seg_chunks, case.bits(i))) for i in range(8)])
    same(got, want, "pedersen_hash over hashed generators")
    for k in range(3):                                                                   # and the generators are the restatement's
        b, i = GC.find_group_hash(b"JJ_gh_ph", GC.PREFIX_POOL[:64], names[k].tobytes(), every)
        assert g[k].tobytes() == b and int(host(first)[k]) == i


def test_refused_calls_leave_the_outputs_untouched(eng):
    import torch

    from jubjub_amd import _lib

    lib, ctx = eng._lib, eng._ctx
    lib.jj_ctx_use_own_stream(ctx)
    INVALID = _lib.JJ_ERR_INVALID
    n = 4
    msgs = KC.rng_bytes(9500, n, 12)
    prefix = GC.PREFIX_POOL[:64]
    out = np.full((n + 1, 32), 0xEE, np.uint8)
    pts = np.full((n + 1, 64), 0xEE, np.uint8)
    ok = np.full(n + 1, 0xEE, np.uint8)
    dout = torch.full((n + 1, 32), 0xEE, dtype=torch.uint8, device="cuda")
    dpts = torch.full((n + 1, 64), 0xEE, dtype=torch.uint8, device="cuda")
    dok = torch.full((64,), 0xEE, dtype=torch.uint8, device="cuda")
    dmsgs = cuda(np.concatenate([msgs.reshape(-1), np.zeros(64, np.uint8)]))
    torch.cuda.synchronize()
    m, o, p, k = msgs.ctypes.data, out.ctypes.data, pts.ctypes.data, ok.ctypes.data
    b2s, gh = lib.jj_blake2s, lib.jj_group_hash
    # n = 0 succeeds and touches nothing, with NULL arrays too
    assert b2s(ctx, 0, None, None, 0, None, 0, 0, None) == 0 and gh(ctx, 0, None, None, 0, None, 0, 0, 13, None, None) == 0
    assert b2s(ctx, 0, b"12345678", prefix, 64, m, 11, 12, o) == 0 and gh(ctx, 0, None, prefix, 64, m, 11, 12, 13, dpts.data_ptr(), dok.data_ptr()) == 0
    both = lambda *a, flags=13: (b2s(ctx, *a, o), gh(ctx, *a, flags, p, k))      # noqa: E731
    assert both(n, None, prefix, 64, dmsgs.data_ptr() + 8, 11, 12) == (INVALID, INVALID)                # a misaligned device pointer: the messages
    assert b"16-byte aligned" in lib.jj_last_error(ctx)
    assert b2s(ctx, n, None, prefix, 64, m, 11, 12, dout.data_ptr() + 4) == INVALID                       # ... the outputs
    assert gh(ctx, n, None, prefix, 64, m, 11, 12, 13, dpts.data_ptr() + 8, k) == INVALID and gh(ctx, n, None, prefix, 64, m, 11, 12, 13, p, dok.data_ptr() + 1) == INVALID
    assert both(n, None, prefix, 64, m, 11, 10) == (INVALID, INVALID)                                     # msg_stride < msg_len
    assert both(n, None, prefix, 64, m, 11, 0) == (INVALID, INVALID)
    assert both((1 << 24), None, prefix, 64, m, 11, 257) == (INVALID, INVALID)                            # n * msg_stride > 2^32, before anything is read
    assert both((1 << 16) + 1, None, prefix, 64, m, 65536, 65536) == (INVALID, INVALID)
    assert both((1 << 24) + 1, None, prefix, 64, m, 11, 12) == (INVALID, INVALID)                         # n > 2^24
    assert both(n, None, prefix, 64, m, 65537, 65537) == (INVALID, INVALID)                               # msg_len > 65536
    assert both(n, None, None, 64, m, 11, 12) == (INVALID, INVALID) and both(n, None, None, 1, m, 11, 12) == (INVALID, INVALID)     # a NULL prefix with prefix_len > 0
    assert both(n, None, prefix, 4097, m, 11, 12) == (INVALID, INVALID)                                   # prefix_len > 4096
    assert both(n, None, prefix, 64, None, 11, 12) == (INVALID, INVALID)                                  # NULL msgs with msg_len > 0
    for flags in (16, 32, 64, 128, 13 | 16, 1 << 31):                                                      # an unknown flag bit, with n = 0 too
        assert gh(ctx, n, None, prefix, 64, m, 11, 12, flags, p, k) == INVALID and gh(ctx, 0, None, prefix, 64, m, 11, 12, flags, p, k) == INVALID, flags
    assert b2s(ctx, n, None, prefix, 64, m, 11, 12, None) == INVALID                                      # a NULL output with n > 0
    assert gh(ctx, n, None, prefix, 64, m, 11, 12, 13, None, k) == INVALID and gh(ctx, n, None, prefix, 64, m, 11, 12, 13, p, None) == INVALID
    assert b2s(None, n, None, prefix, 64, m, 11, 12, o) == INVALID and gh(None, n, None, prefix, 64, m, 11, 12, 13, p, k) == INVALID
    assert lib.jj_ctx_sync(ctx) == 0
    assert (out == 0xEE).all() and (pts == 0xEE).all() and (ok == 0xEE).all()                            # the outputs untouched by every refused call
    assert bool((dout == 0xEE).all()) and bool((dpts == 0xEE).all()) and bool((dok == 0xEE).all())
    assert np.array_equal(msgs, KC.rng_bytes(9500, n, 12))
    # the context is as good as before
    assert b2s(ctx, n, None, prefix, 64, m, 11, 12, o) == 0 and gh(ctx, n, None, prefix, 64, m, 11, 12, 13, p, k) == 0
    same(out[:n], GC.digests(None, prefix, msgs[:, :11]), "after the refused calls")
    want_pts, want_ok = GC.expected(None, prefix, msgs[:, :11], 13)
    same(pts[:n], want_pts, "after the refused calls (points)")
    assert (ok[:n] == want_ok).all() and ok[n] == 0xEE and (pts[n] == 0xEE).all() and (out[n] == 0xEE).all()
    # msg_len = 0 with a NULL msgs and any stride; a 4096-byte prefix; a 65536-byte message
    assert b2s(ctx, 2, None, prefix, 64, None, 0, 0, o) == 0 and out[0].tobytes() == out[1].tobytes() == hashlib.blake2s(prefix).digest()
    assert b2s(ctx, 2, None, prefix, 64, None, 0, 7, o) == 0 and out[1].tobytes() == hashlib.blake2s(prefix).digest()
    long_prefix, long_msg = KC.rng_bytes(9501, 4096).tobytes(), KC.rng_bytes(9502, 1, 65536)
    assert host(eng.blake2s(long_msg, b"12345678", long_prefix))[0].tobytes() == hashlib.blake2s(long_prefix + long_msg.tobytes(), person=b"12345678").digest()
    with pytest.raises(ValueError):
        eng.blake2s(msgs, b"short")
    with pytest.raises(ValueError):
        eng.group_hash(msgs, None, bytes(4097))
    with pytest.raises(ValueError):
        eng.blake2s(msgs.reshape(-1))


def test_a_sequence_on_one_context_equals_the_single_calls(eng):
    """ka_kdf, group_hash, decompress, group_hash, blake2s on ONE context: the calls share the decoder's workspaces (and ka_kdf the staging
    buffers); every result equals what the same call gives on a context of its own"""
    from jubjub_amd import Engine

    encs = KC.tiled(1025)
    shape = GC.MAIN
    person, prefix = GC.personal_of(shape), GC.prefix_of(shape)
    small, large = GC.messages(shape), cuda(KC.rng_bytes(9600, 20000, 11))
    dig = GC.digests(person, prefix, small)
    calls = (lambda e: e.ka_kdf(KC.SCALARS[-1], encs, KC.SAPLING_PERSONAL, KC.SAPLING_FLAGS),
             lambda e: e.group_hash(large, person, prefix, GC.FLAG_SETS[-1]),
             lambda e: e.decompress(dig, GC.SAPLING_SHAPED),
             lambda e: e.group_hash(small, person, prefix, GC.SAPLING_SHAPED),
             lambda e: (e.blake2s(large, person, prefix),))
    alone = []
    for call in calls:
        e = Engine(0)
        try:
            alone.append([host(x).copy() for x in call(e)])
        finally:
            e.close()
    together = [[host(x).copy() for x in call(eng)] for call in calls]
    for k, (a, t) in enumerate(zip(alone, together)):
        assert len(a) == len(t) and all(np.array_equal(x, y) for x, y in zip(a, t)), "call %d of the sequence differs from the single call" % k
    want_keys, want_ok = KC.expected(KC.SCALARS[-1], encs, KC.SAPLING_FLAGS, KC.SAPLING_PERSONAL)
    same(together[0][0], want_keys, "ka_kdf in the sequence")
    want_pts, want_ok = GC.case_expected(shape, GC.SAPLING_SHAPED)
    same(together[3][0], want_pts, "group_hash in the sequence")
    same(together[3][1], want_ok, "group_hash in the sequence (ok)")
    assert np.array_equal(together[2][0], together[3][0]) and np.array_equal(together[2][1], together[3][1])      # decompress of hashlib's digests = group_hash
    sample = np.arange(0, 20000, 97)
    same(together[4][0][sample], GC.digests(person, prefix, host(large)[sample]), "blake2s in the sequence")
