"""jj_pedersen_table_create / jj_pedersen_hash_vartime / jj_pedersen_scalars on the GPU against the restatement of tests/pedersen_cases.py (the
formula on the oracle's point arithmetic), byte for byte.

Hash bytes: every case of the table (the Merkle shape, the twin shape with its planted identity and doubling, the one-field shape whose rows
start at every residue modulo 4, overlapping fields, five pieces in one window, prefix only, the empty message, every length 0 .. 27 of the
tiny shape) x every n around a wave and a workgroup x every window_chunks, both output forms, numpy arrays and CUDA tensors.  The composed
route: pedersen_scalars equals <M_j> mod r, and fixedbase_multi_mul over those scalars equals pedersen_hash(point=True).  A 16-leaf Merkle tree,
layer by layer.  The buffer-discipline rows through the guarded arenas.  Every refused call with the output watched."""
import ctypes as C

import numpy as np
import pytest

from oracle import jubjub_ref as J
from tests import pedersen_buffer_row as BR
from tests import pedersen_cases as PC

pytestmark = pytest.mark.gpu

GROUPS = {"merkle": ["merkle"], "twin": ["twin"], "one_field_stride9": ["one_field_stride9"], "overlap": ["overlap"], "five_pieces": ["five_pieces"],
          "prefix_only": ["prefix_only"], "empty": ["empty"], "tiny": [c.id for c in PC.TINY]}


@pytest.fixture(scope="module")
def eng():
    from jubjub_amd import Engine

    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def tables(eng):
    made = {}

    def get(gens, seg_chunks, w):
        key = (gens, seg_chunks, w)
        if key not in made:
            made[key] = eng.pedersen_table(PC.gens_bytes(gens), seg_chunks, w)
        return made[key]

    yield get
    for t in made.values():
        t.close()


def cuda(x):
    import torch

    return torch.from_numpy(np.array(x)).cuda()


def host(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


def same(got, want, what):
    got = host(got)
    assert got.shape == want.shape and got.dtype == np.uint8, (what, got.shape, want.shape)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert not len(bad), "%s: %d of %d units differ from the restatement, the first is unit %d" % (what, len(bad), len(want), bad[0])


def rows_of(case, n):
    return np.ascontiguousarray(case.rows[:n, :case.row_stride])


@pytest.mark.parametrize("w", PC.WINDOWS)
@pytest.mark.parametrize("group", list(GROUPS))
def test_hash_bytes_every_case_size_and_window(eng, tables, group, w):
    for cid in GROUPS[group]:
        c = PC.BY_ID[cid]
        t = tables(c.gens, c.seg_chunks, w)
        for n in PC.SIZES:
            want, rows = PC.expected_points(c, n), rows_of(c, n)
            what = "%s, n %d, window_chunks %d" % (cid, n, w)
            same(eng.pedersen_hash(t, rows, c.fields, c.prefix, c.prefix_bits), np.ascontiguousarray(want[:, :32]), what + ", host, u")
            same(eng.pedersen_hash(t, rows, c.fields, c.prefix, c.prefix_bits, point=True), want, what + ", host, point")
            drows = cuda(rows)
            same(eng.pedersen_hash(t, drows, c.fields, c.prefix, c.prefix_bits), np.ascontiguousarray(want[:, :32]), what + ", device, u")
            same(eng.pedersen_hash(t, drows, c.fields, c.prefix, c.prefix_bits, point=True), want, what + ", device, point")


def test_planted_rows_and_the_default_window(eng, tables):
    c = PC.BY_ID["twin"]
    got = eng.pedersen_hash(tables("twin", 63, 0), rows_of(c, 4), c.fields, point=True)
    assert not got[PC.TWIN_CANCEL_ROW][:32].any() and got[PC.TWIN_CANCEL_ROW][32] == 1 and not got[PC.TWIN_CANCEL_ROW][33:].any()      # the identity (0, 1)
    same(got, PC.expected_points(c, 4), "twin, default window")
    out = np.full((5, 32), 0xEE, np.uint8)
    res = eng.pedersen_hash(tables("twin", 63, 0), rows_of(c, 4), c.fields, out=out[:4])
    assert res.base is out or res is out[:4] or np.shares_memory(res, out)
    same(out[:4], np.ascontiguousarray(PC.expected_points(c, 4)[:, :32]), "out=")
    assert (out[4] == 0xEE).all()


@pytest.mark.parametrize("cid", ["merkle", "twin", "one_field_stride9", "overlap", "tiny_09", "tiny_27", "empty"])
def test_composed_route(eng, cid):
    c = PC.BY_ID[cid]
    n = 65
    rows = rows_of(c, n)
    want = PC.expected_scalars(c, n)
    got = eng.pedersen_scalars(c.nseg, c.seg_chunks, rows, c.fields, c.prefix, c.prefix_bits)
    assert got.shape == (c.nseg, n, 32)
    same(got.reshape(-1, 32), want.reshape(-1, 32), cid + ": scalars, host")
    dgot = eng.pedersen_scalars(c.nseg, c.seg_chunks, cuda(rows), c.fields, c.prefix, c.prefix_bits)
    same(dgot.reshape(-1, 32), want.reshape(-1, 32), cid + ": scalars, device")
    fb = [eng.fixedbase_table(g) for g in PC.gens_bytes(c.gens)]
    ped = eng.pedersen_table(PC.gens_bytes(c.gens), c.seg_chunks, 0)
    try:
        composed = eng.fixedbase_multi_mul(fb, dgot.reshape(-1, 32))
        fused = eng.pedersen_hash(ped, cuda(rows), c.fields, c.prefix, c.prefix_bits, point=True)
        same(fused, host(composed), cid + ": fused against composed")
        same(fused, PC.expected_points(c, n), cid + ": fused against the restatement")
    finally:
        ped.close()
        for t in fb:
            t.close()


def merkle_layer(prev, layer):
    """(m, 32) node bytes -> (m / 2, 32): the restatement over the 6-bit layer number and 255 bits of each child"""
    gs = PC.generators("three")
    out = np.zeros((len(prev) // 2, 32), np.uint8)
    for k in range(len(prev) // 2):
        bits = [(layer >> b) & 1 for b in range(6)]
        for child in (prev[2 * k], prev[2 * k + 1]):
            bits += [(int(child[b >> 3]) >> (b & 7)) & 1 for b in range(255)]
        out[k] = np.frombuffer(PC.expected(gs, 63, bits)[0].to_bytes(32, "little"), dtype=np.uint8)
    return out


def test_merkle_tree_of_sixteen_leaves(eng, tables):
    leaves = np.random.default_rng(4242).integers(0, 256, size=(16, 32), dtype=np.uint8)
    t = tables("three", 63, 0)
    first = 3
    layers = eng.pedersen_merkle(t, cuda(leaves), first_layer=first)
    assert [tuple(x.shape) for x in layers] == [(8, 32), (4, 32), (2, 32), (1, 32)] and all(hasattr(x, "cpu") for x in layers)
    prev, chained = leaves, leaves
    for k, layer in enumerate(layers):
        same(layer, merkle_layer(host(prev), first + k), "layer %d from the device's previous layer" % k)
        chained = merkle_layer(chained, first + k)
        prev = layer
    same(layers[-1], chained, "the root against four chained layers")
    hl = eng.pedersen_merkle(t, leaves, first_layer=first)
    assert all(isinstance(x, np.ndarray) for x in hl)
    same(hl[-1], chained, "the root from host arrays")
    with pytest.raises(ValueError):
        eng.pedersen_merkle(t, leaves[:12])


def test_buffer_discipline_rows():
    """the rows of tests/pedersen_buffer_row.py through the runner of tests/test_gpu_buffers.py (its Env, checked_call, placements and skews):
    every size of the table x every skew in one device arena, the host arenas and the mixed placements at the host sizes, n = 0"""
    import test_gpu_buffers as TB

    env = TB.Env()
    try:
        for case in (BR.ROW_HASH, BR.ROW_SCALARS):
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


def pt64(p):
    return np.frombuffer(p[0].to_bytes(32, "little") + p[1].to_bytes(32, "little"), dtype=np.uint8).copy()


def test_refused_calls_leave_the_output_untouched(eng, tables):
    import torch

    from jubjub_amd import _lib

    lib, ctx = eng._lib, eng._ctx
    lib.jj_ctx_use_own_stream(ctx)
    INVALID = _lib.JJ_ERR_INVALID
    c = PC.BY_ID["tiny_27"]                                                       # exactly at capacity: 27 bits in three segments of 3
    t = tables(c.gens, c.seg_chunks, 0)
    n = 4
    rows = rows_of(c, n)
    out = np.full((n + 1, 64), 0xEE, np.uint8)
    dout = torch.full((n + 1, 64), 0xEE, dtype=torch.uint8, device="cuda")
    dany = torch.zeros(256, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r, o = rows.ctypes.data, out.ctypes.data
    H, S = lib.jj_pedersen_hash_vartime, lib.jj_pedersen_scalars

    def f(*v):
        return (C.c_uint32 * max(len(v), 1))(*v)

    good = f(PC.TINY_OFFSET, 27)
    assert H(ctx, t._h, 0, 0, 0, None, 0, 0, None, 0, None) == 0 and S(ctx, 3, 3, 0, 0, 0, None, 0, 0, None, None) == 0       # n = 0 succeeds with NULL arrays
    assert H(ctx, t._h, 0, 0, 0, r, c.row_stride, 1, good, 0, o) == 0                                                        # ... and touches nothing
    for outp in (o, dout.data_ptr()):
        assert H(None, t._h, n, 0, 0, r, c.row_stride, 1, good, 0, outp) == INVALID                     # a NULL context
        assert H(ctx, None, n, 0, 0, r, c.row_stride, 1, good, 0, outp) == INVALID                      # a NULL table
        assert H(ctx, t._h, n, 0, 0, r, c.row_stride, 1, f(PC.TINY_OFFSET, 28), 0, outp) == INVALID     # one bit over capacity
        assert b"longer" in lib.jj_last_error(ctx)
        assert H(ctx, t._h, n, 1, 1, r, c.row_stride, 1, good, 0, outp) == INVALID                      # ... by the prefix
        assert H(ctx, t._h, n, 0, 0, r, c.row_stride, 1, f(2, 25), 0, outp) == INVALID                  # a field past row_stride: 2 + 4 bytes of 5
        assert b"row_stride" in lib.jj_last_error(ctx)
        assert H(ctx, t._h, n, 0, 0, r, c.row_stride, 1, f(0, 0), 0, outp) == INVALID                   # an empty field
        assert H(ctx, t._h, n, 0, 0, r, c.row_stride, 5, f(0, 1, 0, 1, 0, 1, 0, 1, 0, 1), 0, outp) == INVALID      # nfields = 5
        assert H(ctx, t._h, n, 0, 33, r, c.row_stride, 0, None, 0, outp) == INVALID                     # prefix_bits = 33
        assert H(ctx, t._h, n, 0, -1, r, c.row_stride, 0, None, 0, outp) == INVALID
        assert H(ctx, t._h, n, 0, 0, r, c.row_stride, 1, good, 2, outp) == INVALID                      # an unknown flag
        assert H(ctx, t._h, n, 0, 0, None, c.row_stride, 1, good, 0, outp) == INVALID                   # NULL rows with a field
        assert H(ctx, t._h, n, 0, 0, r, c.row_stride, 1, None, 0, outp) == INVALID                      # NULL fields
        assert H(ctx, t._h, n, 0, 0, dany.data_ptr() + 8, c.row_stride, 1, good, 0, outp) == INVALID    # a misaligned device pointer
        assert S(None, 3, 3, n, 0, 0, r, c.row_stride, 1, good, outp) == INVALID
        assert S(ctx, 3, 3, n, 0, 0, r, c.row_stride, 1, f(PC.TINY_OFFSET, 28), outp) == INVALID
        assert S(ctx, 9, 3, n, 0, 0, r, c.row_stride, 1, good, outp) == INVALID and S(ctx, 3, 64, n, 0, 0, r, c.row_stride, 1, good, outp) == INVALID
        assert S(ctx, 3, 3, n, 0, 33, r, c.row_stride, 0, None, outp) == INVALID
    assert H(ctx, t._h, n, 0, 0, r, c.row_stride, 1, good, 0, dout.data_ptr() + 4) == INVALID
    assert H(ctx, t._h, n, 0, 0, r, c.row_stride, 1, good, 0, None) == INVALID
    assert H(ctx, t._h, 1 << 30, 0, 0, r, 5, 1, good, 0, o) == INVALID and b"2^32" in lib.jj_last_error(ctx)       # more than 2^32 bytes of rows
    # a fixed-base table handed to the Pedersen call; a Pedersen table handed to the fixed-base calls
    fb = eng.fixedbase_table(pt64(J.GENERATOR), 8)
    scal = np.zeros((n, 32), np.uint8)
    verdict = np.full(n, 0xEE, np.uint8)
    try:
        assert H(ctx, fb._h, n, 0, 0, r, c.row_stride, 1, good, 0, o) == INVALID
        for outp in (o, dout.data_ptr()):
            assert lib.jj_fixedbase_mul(ctx, t._h, n, scal.ctypes.data, outp) == INVALID and b"Pedersen" in lib.jj_last_error(ctx)
            assert lib.jj_fixedbase_mul_compressed(ctx, t._h, n, scal.ctypes.data, outp) == INVALID
            assert lib.jj_fixedvar_mul_vartime(ctx, t._h, n, scal.ctypes.data, scal.ctypes.data, out.ctypes.data, outp) == INVALID
            handles = (C.c_void_p * 2)(fb._h, t._h)
            assert lib.jj_fixedbase_multi_mul(ctx, handles, 2, n // 2, scal.ctypes.data, outp) == INVALID
            assert lib.jj_fixedbase_composite_mul(ctx, t._h, n, scal.ctypes.data, outp) == INVALID
        assert lib.jj_sigverify_each(ctx, t._h, n, scal.ctypes.data, scal.ctypes.data, scal.ctypes.data, scal.ctypes.data, 0, verdict.ctypes.data) == INVALID
        assert b"Pedersen" in lib.jj_last_error(ctx)
    finally:
        fb.close()
    # generators: a torsion component, off the curve
    full = next(p for p in (J.synth_point(k)[0] for k in range(40, 80)) if not J.ext_is_torsion_free(J.affine_to_extended(p)))
    off = (2, 3)
    assert J.affine_is_on_curve(full) and not J.affine_is_on_curve(off)
    g = PC.gens_bytes("three")
    handle = C.c_void_p(0x5678)
    for k, bad in ((0, full), (2, full), (1, off)):
        gb = g.copy()
        gb[k] = pt64(bad)
        for ptr in (gb.ctypes.data, cuda(gb).data_ptr()):
            assert lib.jj_pedersen_table_create(ctx, 3, ptr, 63, 0, C.byref(handle)) == INVALID and handle.value == 0x5678
    assert b"curve" in lib.jj_last_error(ctx)
    for nseg, chunks, w in ((0, 63, 0), (9, 63, 0), (3, 0, 0), (3, 64, 0), (3, 63, 5), (3, 63, -1)):
        assert lib.jj_pedersen_table_create(ctx, nseg, g.ctypes.data, chunks, w, C.byref(handle)) == INVALID and handle.value == 0x5678
    assert lib.jj_ctx_sync(ctx) == 0
    assert (out == 0xEE).all() and bool((dout == 0xEE).all()) and (verdict == 0xEE).all()             # untouched by every refused call
    assert np.array_equal(rows, rows_of(c, n))
    assert H(ctx, t._h, n, 0, 0, r, c.row_stride, 1, good, 1, o) == 0                                  # the context is as good as before
    same(out[:n], PC.expected_points(c, n), "after the refused calls")
    assert (out[n] == 0xEE).all()
    with pytest.raises(ValueError):
        eng.pedersen_hash(t, rows.reshape(-1), c.fields)
    with pytest.raises(ValueError):
        eng.pedersen_hash(t, rows, ((0, 1),) * 5)
