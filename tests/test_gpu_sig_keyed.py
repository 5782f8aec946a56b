"""
GPU tests of jj_sigbatch_keyed_begin (batch Schnorr verification with the terms of equal keys folded, finished by jj_msm_finish): every case of
tests/sig_keyed_cases.py byte for byte -- every planted variant of tests/sig_batch_cases.py regrouped by key, keys without signatures, a key listed
twice, and group sizes whose boundaries fall on the wave and workgroup edges of k_sig_keyed_terms and k_sig_keyed_close
(tests/test_sig_keyed_cases_cpu.py holds the expected bytes to the oracle).  Host arrays and device tensors; a mix of pointer kinds; the base as a
host and as a device pointer; jobs in flight finished in reverse order; jj_sigbatch_begin on the expanded arrays gives the same bytes; the argument
checks on a live context; the empty batch; unaligned device pointers.
"""
import ctypes as C

import numpy as np
import pytest

from tests import sig_batch_cases as SC
from tests import sig_keyed_cases as KC

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


def run(eng, c, keys=None, arrays=None, base=None):
    r, s, ch, z = arrays if arrays is not None else c.arrays()
    job = eng.sigbatch_keyed_begin(c.base if base is None else base, c.keys if keys is None else keys, c.offsets, r, s, ch, z, zip216=bool(c.flags))
    return bytes(eng.msm_finish(job))


def test_every_case_on_host_arrays(eng):
    for c in KC.all_cases():
        got = run(eng, c)
        assert got == bytes(c.expected), "%s: got %s, want %s" % (c.name, got.hex(), bytes(c.expected).hex())


def test_every_case_on_device_tensors(eng):
    import torch

    for c in KC.all_cases():
        got = run(eng, c, cuda(c.keys), [cuda(x) for x in c.arrays()], cuda(c.base))
        assert got == bytes(c.expected), "%s: got %s, want %s" % (c.name, got.hex(), bytes(c.expected).hex())
    torch.cuda.synchronize()


def test_sigbatch_begin_on_the_expanded_arrays_gives_the_same_bytes(eng):
    """on the device, for every case in which each listed key has a signature: the two sums differ by multiples of [r]A_k only"""
    import torch

    ran = 0
    for c in KC.all_cases():
        if c.has_empty_group():
            continue
        b = c.expanded()
        base = cuda(c.base)
        r, s, ch, z = [cuda(x) for x in c.arrays()]
        keyed = bytes(eng.msm_finish(eng.sigbatch_keyed_begin(base, cuda(c.keys), c.offsets, r, s, ch, z, zip216=bool(c.flags))))
        plain = bytes(eng.msm_finish(eng.sigbatch_begin(base, r, cuda(b.a), s, ch, z, zip216=bool(c.flags))))
        assert keyed == plain == bytes(c.expected), c.name
        ran += 1
    torch.cuda.synchronize()
    assert ran >= len(KC.regrouped_cases()) + 15


def test_pointer_kinds(eng):
    """the five arrays in mixes of device, pageable host and page-locked host memory; the base as a host and as a device pointer"""
    import torch

    by_name = {c.name: c for c in KC.all_cases()}
    picks = [by_name["sizes 1, 2, 3, ..., 23, bad s in the last group"], by_name["off-curve key without signatures"], by_name["sizes [0, 5, 0, 0, 300, 0]"],
             KC.regrouped(257, "noncanonical_a_zip216", 64), KC.regrouped(257, "bad_r", 256)]
    for c in picks:
        r, s, ch, z = c.arrays()
        dk, dr, ds, dc, dz = [cuda(x) for x in (c.keys, r, s, ch, z)]
        pinned_c = eng.host_alloc(ch.shape)
        pinned_c[...] = ch
        pinned_k = eng.host_alloc(c.keys.shape)
        pinned_k[...] = c.keys
        mixes = [(dk, (r, ds, pinned_c, dz)), (c.keys, (dr, s, dc, z)), (pinned_k, (dr, ds, ch, dz)), (dk, (r, s, ch, z)), (c.keys, (dr, ds, dc, dz))]
        for i, (keys, arrays) in enumerate(mixes):
            for base in (c.base, cuda(c.base)):
                assert run(eng, c, keys, arrays, base) == bytes(c.expected), "%s, mix %d" % (c.name, i)
        torch.cuda.synchronize()


def test_three_jobs_in_flight_finished_in_reverse_order(eng):
    """device-resident inputs: each job owns its workspace and its flag; one fails, one is malformed; the second round takes pooled jobs, whose
    workspaces hold the other layout's stale heads"""
    import torch

    by_name = {c.name: c for c in KC.all_cases()}
    plan = [by_name["one group of %d, bad s in its last wave" % KC.LARGE], by_name["off-curve key without signatures"], by_name["every group of one"]]
    for rounds in range(2):
        keep, jobs = [], []
        for c in plan:
            dev = [cuda(c.base), cuda(c.keys)] + [cuda(x) for x in c.arrays()]
            keep.append(dev)
            jobs.append(eng.sigbatch_keyed_begin(dev[0], dev[1], c.offsets, *dev[2:], zip216=bool(c.flags)))
        for c, job in reversed(list(zip(plan, jobs))):
            assert bytes(eng.msm_finish(job)) == bytes(c.expected), c.name
        plan = plan[::-1]
    torch.cuda.synchronize()
    # between a plain signature job and a plain MSM job
    from oracle import c_oracle as O
    from tests.util import rand_points, rand_scalars

    s, p = rand_scalars(5, 200), rand_points(5, 200)
    bad, good = by_name["off-curve key with signatures"], by_name["90 groups of three"]
    plain = SC.batch(100, "bad_s", 3)
    j1 = eng.sigbatch_keyed_begin(bad.base, bad.keys, bad.offsets, *bad.arrays())
    j2 = eng.msm_begin(s, p)
    j3 = eng.sigbatch_begin(plain.base, *plain.arrays())
    j4 = eng.sigbatch_keyed_begin(good.base, good.keys, good.offsets, *good.arrays())
    assert bytes(eng.msm_finish(j4)) == bytes(SC.IDENTITY) and bytes(eng.msm_finish(j3)) == bytes(plain.expected)
    assert bytes(eng.msm_finish(j2)) == bytes(O.msm(s, p)) and bytes(eng.msm_finish(j1)) == bytes(SC.MALFORMED)


def test_no_signatures_with_null_arrays(eng):
    """offsets[K] = 0: the identity whatever K is; the arrays are not read"""
    lib, ctx = eng._lib, eng._ctx
    base = (C.c_uint8 * 64).from_buffer_copy(bytes(SC.bases()["prime"]))
    for K in (0, 1, 5):
        offsets = np.zeros(K + 1, np.uint64)
        for op in ([C.c_void_p(offsets.ctypes.data)] + ([None] if K == 0 else [])):
            for flags in (0, 1):
                job = C.c_void_p()
                assert lib.jj_sigbatch_keyed_begin(ctx, base, K, None, op, None, None, None, None, flags, C.byref(job)) == 0 and job.value
                out = (C.c_uint8 * 64)()
                assert lib.jj_msm_finish(job, out) == 0 and bytes(out) == bytes(SC.IDENTITY)
    none = [c for c in KC.all_cases() if c.n == 0]
    assert len(none) == 3 and all(run(eng, c) == bytes(SC.IDENTITY) for c in none)


def test_argument_checks_on_a_live_context(eng):
    """every JJ_ERR_INVALID row: *job = NULL, nothing queued, and the context works right after"""
    import torch

    from jubjub_amd import _lib

    lib, ctx = eng._lib, eng._ctx
    c = KC.layout("checks", [3, 4])
    good = np.array([0, 3, 7], np.uint64)
    host = [np.ascontiguousarray(x) for x in (c.base, c.keys, *c.arrays())]
    P = [C.c_void_p(x.ctypes.data) for x in host]
    base, keys, r, s, ch, z = P

    def po(a):
        return C.c_void_p(a.ctypes.data)

    def call(ctx_, base_, K, keys_, offs, r_, s_, c_, z_, flags, slot=True):
        job = C.c_void_p(0xDEAD)
        rc = lib.jj_sigbatch_keyed_begin(ctx_, base_, K, keys_, offs, r_, s_, c_, z_, flags, C.byref(job) if slot else None)
        return rc, job.value

    def works():
        rc, job = call(ctx, base, 2, keys, po(good), r, s, ch, z, 0)
        out = (C.c_uint8 * 64)()
        return rc == 0 and job and lib.jj_msm_finish(C.c_void_p(job), out) == 0 and bytes(out) == bytes(SC.IDENTITY)

    assert works()
    dev_offsets = torch.from_numpy(good.view(np.uint8).copy()).cuda()
    rows = {
        "NULL context": (None, base, 2, keys, po(good), r, s, ch, z, 0),
        "NULL base": (ctx, None, 2, keys, po(good), r, s, ch, z, 0),
        "NULL offsets, K > 0": (ctx, base, 2, keys, None, r, s, ch, z, 0),
        "NULL keys": (ctx, base, 2, None, po(good), r, s, ch, z, 0),
        "NULL r": (ctx, base, 2, keys, po(good), None, s, ch, z, 0),
        "NULL s": (ctx, base, 2, keys, po(good), r, None, ch, z, 0),
        "NULL c": (ctx, base, 2, keys, po(good), r, s, None, z, 0),
        "NULL z": (ctx, base, 2, keys, po(good), r, s, ch, None, 0),
        "offsets[0] != 0": (ctx, base, 2, keys, po(np.array([1, 3, 7], np.uint64)), r, s, ch, z, 0),
        "a decreasing pair": (ctx, base, 2, keys, po(np.array([0, 8, 7], np.uint64)), r, s, ch, z, 0),
        "offsets in device memory": (ctx, base, 2, keys, C.c_void_p(dev_offsets.data_ptr()), r, s, ch, z, 0),
        "flags 2": (ctx, base, 2, keys, po(good), r, s, ch, z, 2),
        "flags 0x80000001": (ctx, base, 2, keys, po(good), r, s, ch, z, 0x80000001),
        "n + K + 1 = 2^24 + 1": (ctx, base, 2, keys, po(np.array([0, 3, (1 << 24) - 2], np.uint64)), r, s, ch, z, 0),
        "K = 2^24": (ctx, base, 1 << 24, keys, po(good), r, s, ch, z, 0),
    }
    for name, args in rows.items():
        rc, job = call(*args)
        assert rc == _lib.JJ_ERR_INVALID and not job, name
        assert works(), "after " + name
    assert call(ctx, base, 2, keys, po(good), r, s, ch, z, 0, slot=False)[0] == _lib.JJ_ERR_INVALID and works()
    with pytest.raises(ValueError):
        eng.sigbatch_keyed_begin(c.base, c.keys, [0, 3, 6], *c.arrays())
    with pytest.raises(ValueError):
        eng.sigbatch_keyed_begin(c.base, c.keys, [0, 7], *c.arrays())


def test_unaligned_device_pointers_are_refused(eng):
    import torch

    from jubjub_amd import _lib

    lib, ctx = eng._lib, eng._ctx
    c = KC.layout("unaligned", [40, 30])
    offs = np.ascontiguousarray(c.offsets)
    host = [np.ascontiguousarray(x) for x in (c.keys, *c.arrays())]
    base = np.ascontiguousarray(c.base)
    for which in range(5):
        keep, ptrs = [], []
        for i, x in enumerate(host):
            if i == which:
                t = torch.zeros(x.size + 16, dtype=torch.uint8, device="cuda")
                t[8:8 + x.size] = torch.from_numpy(x.reshape(-1).copy()).cuda()
                keep.append(t)
                ptrs.append(C.c_void_p(t.data_ptr() + 8))
            else:
                ptrs.append(C.c_void_p(x.ctypes.data))
        torch.cuda.synchronize()
        job = C.c_void_p(0xDEAD)
        rc = lib.jj_sigbatch_keyed_begin(ctx, C.c_void_p(base.ctypes.data), 2, ptrs[0], C.c_void_p(offs.ctypes.data), *ptrs[1:], 0, C.byref(job))
        assert rc == _lib.JJ_ERR_INVALID and not job.value, which
        assert "device pointers must be 16-byte aligned" in lib.jj_last_error(ctx).decode(), which
    assert run(eng, c) == bytes(SC.IDENTITY)


def test_engine_verdicts_and_group_by_key(eng):
    """a caller holding per-signature keys: group_by_key, permute by its order, verify -- the three strings, with the caller's z and with z drawn"""
    n = 500
    for variant, k, want in (("valid", None, "ok"), ("order8r", None, "ok"), ("torsion_r", 63, "ok"), ("bad_s", 499, "reject"), ("bad_r", 0, "reject"),
                             ("s_plus_r", 250, "malformed"), ("off_curve_r", 64, "malformed"), ("noncanonical_a_zip216", 1, "malformed"), ("noncanonical_a", 1, "ok")):
        b = SC.batch(n, variant, k)
        keys, offsets, order = eng.group_by_key(b.a)
        r, s, c, z = b.r[order], b.s[order], b.c[order], b.z[order]
        assert eng.sigbatch_keyed_verify(b.base, keys, offsets, r, s, c, z, zip216=bool(b.flags)) == want, b.name
        assert eng.sigbatch_keyed_verify(b.base, keys, offsets, r, s, c, zip216=bool(b.flags)) == want, b.name + " (z drawn)"
        assert eng.sigbatch_verify(b.base, b.r, b.a, b.s, b.c, b.z, zip216=bool(b.flags)) == want, b.name + " (not grouped)"
