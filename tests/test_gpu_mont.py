"""
The default constant-time ladder above vb_quad_max, k_varbase_mont (the x-only ladder on the Montgomery form, jubjub_amd/csrc/jj_mont.h),
against the Edwards ladder it replaced (vb_ct_window=3: k_varbase_ct3) and the oracle: byte for byte on 2^20 random units, on every
edge scalar x torsion / identity / generator / mixed-order points, and on ragged batches around the batch-inversion groups of
k_varbase_mont_x1 (16 units per lane, 1024 per wave) with identity bases inside them.
"""
import numpy as np
import pytest

from oracle import c_oracle as O
from oracle import jubjub_ref as J
from util import EDGE_SCALARS, Q, R, arr32, arr64, b32, rand_points, rand_scalars, torsion_points

pytestmark = pytest.mark.gpu


def _edge_set(golden):
    tors = torsion_points(golden)
    mixed = O.point_op("add", np.repeat(rand_points(31, 1, subgroup=True), len(tors), 0), tors)
    pts = np.concatenate([rand_points(32, 6), tors, mixed, arr64([J.GENERATOR, J.AFFINE_IDENTITY, (0, Q - 1)])])
    ks = [k & ((1 << 256) - 1) for k in EDGE_SCALARS] + [R - 2, 2 * R - 1, 3, 4, 5, 6, 8 * R % (1 << 252), 4 * R % (1 << 252)]
    S = np.repeat(arr32(ks), len(pts), 0)
    P = np.tile(pts, (len(ks), 1))
    return S, P


def test_default_is_the_montgomery_ladder_and_matches_ct3_on_2_20_units(golden):
    import torch

    from jubjub_amd import Engine

    n = 1 << 20
    e_new, e_old = Engine(0), Engine(0, options={"vb_ct_window": 3})
    assert e_new.get_option("vb_ct_window") == 0 and e_old.get_option("vb_ct_window") == 3
    dev = torch.device("cuda:0")
    S = e_new.synth_scalars(n, 0x5CA1AB1E, 0, device=dev)
    P = e_new.random_points(n, 0x90127, 0, subgroup=False, device=dev)
    got, old = e_new.varbase_mul(S, P), e_old.varbase_mul(S, P)
    assert torch.equal(got, old), "%d of %d rows differ" % (int((got != old).any(dim=1).sum()), n)
    idx = np.random.default_rng(3).choice(n, 512, replace=False)
    Sh, Ph, Gh = S.cpu().numpy(), P.cpu().numpy(), got.cpu().numpy()
    assert (Gh[idx] == O.varbase_mul(Sh[idx], Ph[idx])).all()
    # the same through host arrays (the pipelined path runs the ladder chunk by chunk) and the compressed output
    assert (e_new.varbase_mul(Sh[: 1 << 18], Ph[: 1 << 18]) == Gh[: 1 << 18]).all()
    assert (e_new.varbase_mul_compressed(Sh[:65536], Ph[:65536]) == e_old.varbase_mul_compressed(Sh[:65536], Ph[:65536])).all()
    e_new.close(); e_old.close()


@pytest.mark.parametrize("quad_max", [0, 32768])
def test_edge_set_matches_ct3_and_the_oracle(golden, quad_max):
    from jubjub_amd import Engine

    e_new, e_old = Engine(0, options={"vb_quad_max": quad_max}), Engine(0, options={"vb_ct_window": 3, "vb_quad_max": 0})
    S, P = _edge_set(golden)
    # pad past vb_quad_max so the Montgomery ladder runs in both parametrisations
    S = np.concatenate([S, rand_scalars(33, 40000 - len(S), full_width=True)])
    P = np.concatenate([P, rand_points(34, 40000 - len(P))])
    want = O.varbase_mul(S, P)
    got = e_new.varbase_mul(S, P)
    assert (got == want).all(), "%d rows differ from the oracle" % int((got != want).any(axis=1).sum())
    assert (got == e_old.varbase_mul(S, P)).all()
    assert (e_new.varbase_mul_ct(S, P) == want).all()
    e_new.close(); e_old.close()


def test_ragged_batches_and_identities_inside_inversion_groups():
    from jubjub_amd import Engine

    eng = Engine(0, options={"vb_quad_max": 0})
    n = 3100
    S = rand_scalars(41, n, full_width=True)
    P = rand_points(42, n)
    ident = [0, 1, 15, 16, 63, 64, 1023, 1024, 1040, 2047, 3099]            # lanes' first / last units, wave boundaries, the batch's end
    P[ident] = arr64([J.AFFINE_IDENTITY] * len(ident))
    P[[2, 1025]] = arr64([(0, Q - 1)] * 2)
    want = O.varbase_mul(S, P)
    for m in (1, 2, 17, 63, 64, 65, 1023, 1024, 1025, 1041, 2048, 3100):
        assert (eng.varbase_mul(S[:m], P[:m]) == want[:m]).all(), m
    eng.close()
