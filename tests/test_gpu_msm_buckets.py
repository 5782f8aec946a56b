"""
The bucket lists of the Pippenger MSM held to the oracle at planted bucket layouts (tests/msm_bucket_cases.py; shown to be what they
say, from the generated scalars alone, by tests/test_msm_bucket_cases_cpu.py).

Chunked accumulation (k_msm_accumulate<lds> + k_msm_fixup): buckets with exactly 0 .. 129 heads on both sides of the 32 / 33 boundary
between the pair and the wave, starting and ending on chunk boundaries and one entry off, several wave-folded buckets in one wave (the
first and the last pair among them), non-empty buckets hundreds of empty ones apart.  Segment accumulation (k_seg_* +
k_msm_accumulate_seg + k_msm_fixup_big): buckets of P - 1 .. 34 P entries (merge items with k = 32, the first listed bucket), and more
listed buckets than the big-bucket list holds: the overflowed ones fall back to the merge list with k = 33.  Both, and the default
context on either side of its switch: the last bucket of every window, all-zero scalars, one non-zero term, one populated window.

Every (configuration, layout) runs bit-exact through jj_msm on host arrays, jj_msm_begin / jj_msm_finish on device tensors,
jj_msm_partial(g, 3) + jj_msm_combine and, for one configuration per scheme, jj_msm_basis_mul in both modes -- each twice back to back
on one context per configuration: the counters are cleared by the pass itself and the sort's bins alternate.
"""
import numpy as np
import pytest

import msm_bucket_cases as M
from oracle import c_oracle as O

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PAIRS = M.pairs()


@pytest.fixture(scope="module")
def oracle():
    """key -> (layout, points, oracle sum, bucket sizes from the scalars): built on first use, once per layout, never changed"""
    cache = {}

    def get(key):
        if key not in cache:
            lay = M.build(key)
            P = M.points(lay.n)
            want = O.msm_pippenger(lay.S, P).reshape(64)
            for a in (lay.S, P, want):
                a.setflags(write=False)
            cache[key] = (lay, P, want, M.bucket_sizes(lay.S, lay.W))
        return cache[key]

    return get


@pytest.fixture(scope="module")
def engines():
    """one context per configuration, kept for all its layouts"""
    from jubjub_amd import Engine

    made = {}

    def get(cfg):
        if cfg.id not in made:
            made[cfg.id] = Engine(0, options=cfg.options)
        return made[cfg.id]

    yield get
    for eng in made.values():
        eng.close()


def _carries(cfg, lay, sizes, windows):
    """what the layout puts on the lists of the pass that owns `windows`, for the failure message"""
    scheme, unit = M.pass_unit(cfg, lay.n)
    return "%s unit %d: %s" % (scheme, unit, M.describe(M.model(sizes[windows], scheme, unit, lay.n)))


@pytest.mark.parametrize("cfg,key", PAIRS, ids=["%s-%s" % (cfg.id, M.layout_id(key)) for cfg, key in PAIRS])
def test_bucket_layout(oracle, engines, cfg, key):
    lay, P, want, sizes = oracle(key)
    eng = engines(cfg)
    W = lay.W
    assert eng.get_option("msm_windows") == (W if cfg.scheme else 0) and (cfg.scheme or M.default_windows(lay.n) == W)   # the model's windows are the kernel's
    where ="configuration %s %r, layout %s" % (cfg.id, cfg.options, M.layout_id(key))
    whole = _carries(cfg, lay, sizes, list(range(W)))
    S = lay.S
    for rep in (0, 1):
        got = eng.msm(S, P)
        assert (got == want).all(), "%s: msm on host arrays, run %d [%s]" % (where, rep, whole)
    dev = torch.device("cuda", 0)
    Sd, Pd = torch.from_numpy(S.copy()).to(dev), torch.from_numpy(P.copy()).to(dev)
    jobs = [eng.msm_begin(Sd, Pd) for rep in (0, 1)]                          # two passes queued back to back
    for rep, job in enumerate(jobs):
        assert (eng.msm_finish(job) == want).all(), "%s: msm_begin / msm_finish on device tensors, job %d [%s]" % (where, rep, whole)
    for rep in (0, 1):
        recs = np.stack([eng.msm_partial(S, P, g, 3) for g in range(3)])
        thirds = "; ".join("part %d: %s" % (g, _carries(cfg, lay, sizes, list(range(g, W, 3)))) for g in range(3))
        assert (eng.msm_combine(recs) == want).all(), "%s: msm_partial(g, 3) + msm_combine, run %d [%s]" % (where, rep, thirds)
    if cfg.basis:
        for mode in ("points", "windows"):
            basis = eng.msm_basis(P, mode=mode, windows=W)
            try:
                info = basis.info
                assert info["mode"] == mode and info["windows"] == W, (where, info)        # the model's windows are the basis's
                for rep in (0, 1):
                    got = eng.msm_basis_mul(basis, S)
                    assert (got == want).all(), "%s: msm_basis(%s) + msm_basis_mul, run %d, basis %r [%s]" % (where, mode, rep, info, whole)
            finally:
                basis.close()
