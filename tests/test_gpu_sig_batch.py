"""
GPU tests of jj_sigbatch_begin (batch Schnorr verification as one MSM job, finished by jj_msm_finish): every planted case of
tests/sig_batch_cases.py at every size, byte for byte -- the identity for batches that pass the cofactored check, the closed forms
-[8 z_k delta] B and [8 z_k] D for a tampered signature (tests/test_sig_batch_cpu.py holds them to the oracle's evaluation of the whole sum),
(0, -1) for malformed input.  Sizes: the wave and workgroup edges of k_sig_terms, both sides of msm_small_max (2n + 1 terms: the small route
and Pippenger), and one batch with more workgroup partials than one pass of k_sig_close covers.  Every kind of pointer; jobs in flight finished
in reverse order; the empty batch; the argument checks on a live context; Engine.sigbatch_verify.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import sig_batch_cases as SC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def close_pass():
    """signatures one pass of k_sig_close covers: its threads times the signatures behind one partial, read from the kernels' source"""
    src = open(os.path.join(ROOT, "jubjub_amd", "csrc", "jj_sig_kernels.h")).read()
    t = re.search(r"constexpr int SIG_THREADS = (\d+);", src)
    c = re.search(r"constexpr int SIG_CLOSE_THREADS = (\d+);", src)
    assert t and c, "SIG_THREADS / SIG_CLOSE_THREADS not found in jj_sig_kernels.h"
    return int(t.group(1)) * int(c.group(1))


SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 8191, 8192, close_pass() + 1]


@pytest.fixture(scope="module")
def eng():
    from jubjub_amd import Engine

    e = Engine(0)
    yield e
    e.close()


def run(eng, b, arrays=None, base=None):
    r, a, s, c, z = arrays if arrays is not None else b.arrays()
    job = eng.sigbatch_begin(b.base if base is None else base, r, a, s, c, z, zip216=bool(b.flags))
    return eng.msm_finish(job)


def test_sizes_straddle_what_they_must(eng):
    assert close_pass() == 65536
    small_max = eng.get_option("msm_small_max")
    assert 2 * 8191 + 1 <= small_max < 2 * 8192 + 1


@pytest.mark.parametrize("n", SIZES)
def test_every_planted_case(eng, n):
    for variant, k in SC.variants(n):
        b = SC.batch(n, variant, k)
        got = run(eng, b)
        assert bytes(got) == bytes(b.expected), "%s: got %s, want %s" % (b.name, bytes(got).hex(), bytes(b.expected).hex())


def test_pointer_kinds(eng):
    """all-host (above), all-device, and one mixed set: device R, host A, device s, page-locked c, device z, host base"""
    import torch

    n = 300
    for variant, k in (("valid", None), ("bad_r", 64), ("off_curve_r", 299), ("noncanonical_a_zip216", 0)):
        b = SC.batch(n, variant, k)
        dev = [torch.from_numpy(np.array(x)).cuda() for x in b.arrays()]
        base_dev = torch.from_numpy(np.array(b.base)).cuda()
        assert bytes(run(eng, b, dev, base_dev)) == bytes(b.expected), b.name
        pinned = eng.host_alloc(b.c.shape)
        pinned[...] = b.c
        mixed = [dev[0], b.a, dev[2], pinned, dev[4]]
        assert bytes(run(eng, b, mixed)) == bytes(b.expected), b.name
        torch.cuda.synchronize()


def test_device_result_pointer(eng):
    """jj_msm_finish writes the verdict of such a job to device memory like any other sum: the identity, a point, the sentinel"""
    import torch

    lib, ctx = eng._lib, eng._ctx
    for variant, k in (("valid", None), ("bad_s", 10), ("s_plus_r", 10)):
        b = SC.batch(100, variant, k)
        job = eng.sigbatch_begin(b.base, *b.arrays(), zip216=bool(b.flags))
        out = torch.full((64,), 0xEE, dtype=torch.uint8, device="cuda")
        h, job._h = job._h, None
        assert lib.jj_msm_finish(h, C.c_void_p(out.data_ptr())) == 0
        eng.sync()
        torch.cuda.synchronize()
        assert bytes(out.cpu().numpy()) == bytes(b.expected), b.name


def test_four_jobs_finished_in_reverse_order(eng):
    """device-resident inputs: the jobs run on the context's lanes, each with its own workspace and flag; one fails, one is malformed"""
    import torch

    plan = [(257, "valid", None), (8192, "bad_s", 64), (65, "s_plus_r", 64), (8191, "valid", None)]
    for rounds in range(2):                                                 # the second round takes its jobs (and their workspaces) from the pool
        batches = [SC.batch(*p) for p in plan]
        keep, jobs = [], []
        for b in batches:
            dev = [torch.from_numpy(np.array(x)).cuda() for x in b.arrays()]
            keep.append(dev)
            jobs.append(eng.sigbatch_begin(torch.from_numpy(np.array(b.base)).cuda(), *dev, zip216=bool(b.flags)))
        for b, job in reversed(list(zip(batches, jobs))):
            assert bytes(eng.msm_finish(job)) == bytes(b.expected), b.name
        plan = plan[::-1]
    # a plain MSM job between two signature jobs keeps its own verdict-free finish
    from oracle import c_oracle as O
    from tests.util import rand_points, rand_scalars

    s, p = rand_scalars(5, 200), rand_points(5, 200)
    bad = SC.batch(100, "off_curve_r", 0)
    j1 = eng.sigbatch_begin(bad.base, *bad.arrays())
    j2 = eng.msm_begin(s, p)
    j3 = eng.sigbatch_begin(bad.base, *SC.batch(100, "valid").arrays())
    assert bytes(eng.msm_finish(j2)) == bytes(O.msm(s, p))
    assert bytes(eng.msm_finish(j3)) == bytes(SC.IDENTITY) and bytes(eng.msm_finish(j1)) == bytes(SC.MALFORMED)


def test_empty_batch(eng):
    b = SC.batch(0, "valid")
    assert bytes(run(eng, b)) == bytes(SC.IDENTITY)
    lib, ctx = eng._lib, eng._ctx
    base = (C.c_uint8 * 64).from_buffer_copy(bytes(SC.bases()["prime"]))
    for flags in (0, 1):
        job = C.c_void_p()
        assert lib.jj_sigbatch_begin(ctx, base, 0, None, None, None, None, None, flags, C.byref(job)) == 0 and job.value
        out = (C.c_uint8 * 64)()
        assert lib.jj_msm_finish(job, out) == 0 and bytes(out) == bytes(SC.IDENTITY)


def test_argument_checks_on_a_live_context(eng):
    """JJ_ERR_INVALID and *job = NULL; 2n + 1 > 2^24 is refused before anything is read: the arrays behind these pointers are 64 bytes long"""
    from jubjub_amd import _lib

    lib, ctx = eng._lib, eng._ctx
    buf = (C.c_uint8 * 64)()
    p = C.cast(buf, C.c_void_p)

    def refused(*args):
        job = C.c_void_p(0xDEAD)
        return lib.jj_sigbatch_begin(*args, C.byref(job)) == _lib.JJ_ERR_INVALID and not job.value

    assert refused(ctx, p, 1 << 23, p, p, p, p, p, 0)
    assert refused(ctx, p, (1 << 24) - 1, p, p, p, p, p, 1)
    assert refused(ctx, None, 1, p, p, p, p, p, 0)
    assert refused(ctx, p, 1, p, p, None, p, p, 0)
    assert refused(ctx, p, 1, p, p, p, p, p, 2) and refused(ctx, p, 0, None, None, None, None, None, 0x80000001)
    assert lib.jj_sigbatch_begin(ctx, p, 1, p, p, p, p, p, 0, None) == _lib.JJ_ERR_INVALID
    with pytest.raises(ValueError):
        eng.sigbatch_begin(buf, np.zeros((2, 32), np.uint8), np.zeros((3, 32), np.uint8), np.zeros((2, 32), np.uint8), np.zeros((2, 32), np.uint8))
    b = SC.batch(64, "valid")                                                 # the context still works
    assert bytes(run(eng, b)) == bytes(SC.IDENTITY)


def test_engine_verdicts(eng):
    """the three strings, with the caller's z and with z drawn by the Engine (a tampered batch is rejected whatever z is, short of a 2^-128 event)"""
    n = 500
    for variant, k, want in (("valid", None, "ok"), ("order8r", None, "ok"), ("torsion_r", 63, "ok"), ("bad_s", 499, "reject"), ("bad_r", 0, "reject"),
                             ("s_plus_r", 250, "malformed"), ("off_curve_r", 64, "malformed"), ("noncanonical_a_zip216", 1, "malformed"), ("noncanonical_a", 1, "ok")):
        b = SC.batch(n, variant, k)
        r, a, s, c, z = b.arrays()
        assert eng.sigbatch_verify(b.base, r, a, s, c, z, zip216=bool(b.flags)) == want, b.name
        assert eng.sigbatch_verify(b.base, r, a, s, c, zip216=bool(b.flags)) == want, b.name + " (z drawn)"
