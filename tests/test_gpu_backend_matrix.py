"""
The shared normaliser, the sum tree and the Fq root held to the oracle, bit for bit (cases: tests/backend_cases.py, shown to be what
they say by tests/test_backend_cases_cpu.py).

k_normalize<4|16|32|64>: every threshold of normalize_launch, the size below it and a size with a short last lane, taken from the
device's lane count; rows with Z = 0, Z = q, non-canonical and off-curve coordinates planted at the first, a middle and the last position
of a lane's group, on whole groups (one of them all zero: the empty product; one with a single non-zero Z) and on the ragged last lane.
The rows of one lane share one inversion, so a zero that is not skipped shows up in the valid neighbours: every unplanted row is
compared on the device, none is sampled away.  Compressed output (mode 1) at one ragged size per variant; zero Z through the
decoder's cofactor clearing.
sum_reduce / k_sum_pass<32>: the sizes on both sides of every pass boundary up to five passes, ragged at every level.
fq_sqrt_fast: elements with a prescribed log in the 2^32-torsion (every digit value alone in every digit, the borrows of e >> 1), alone
and through the decoder.
"""
import numpy as np
import pytest

import backend_cases as B
from oracle import c_oracle as O
from oracle import jubjub_ref as J
from test_gpu_planner import dec_chunk
from util import b32, pt64

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def env():
    from jubjub_amd import Engine

    eng = Engine(0)
    dev = torch.device("cuda", 0)
    base = torch.from_numpy(pt64(J.GENERATOR).copy()).to(dev)
    table = eng.fixedbase_table(base)
    lanes = eng.device_info()["cus"] * B.LANES_PER_CU
    yield eng, dev, table, lanes
    table.close()
    eng.close()


def _gen(dev, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return g


def _scalars(dev, g, n):
    s = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev, generator=g)
    s[:, 31] &= 0x0F
    return s


def _where(rows, T):
    return [(int(i) % T, int(i) // T) for i in rows]


def _sample(n, planted, count=2048):
    """about `count` strided rows that are not planted"""
    s = np.arange(0, n, max(1, n // count))
    return s[~np.isin(s, planted)]


# ------------------------------------------------------------------------------------------------------------- normaliser
@pytest.mark.parametrize("spec", B.NORM_SPECS, ids=[B.norm_spec_id(s) for s in B.NORM_SPECS])
def test_normalize_affine(env, spec):
    eng, dev, table, lanes = env
    chunk, mult, off = spec
    n = mult * lanes + off
    assert B.norm_chunk(n, lanes) == chunk, (n, lanes)
    if spec in B.NORM_RAGGED:
        assert n % chunk, (n, chunk)                                                  # a short last lane
    T = (n + chunk - 1) // chunk
    where = "k_normalize<%d>, n=%d, T=%d, lanes=%d" % (chunk, n, T, lanes)
    g = _gen(dev, 0x4E4F524D + n)
    P = eng.fixedbase_mul(table, _scalars(dev, g, n))
    z = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev, generator=g)
    ext = torch.empty((n, 160), dtype=torch.uint8, device=dev)
    ext[:, 0:32] = eng.field_binary("fq", "mul", P[:, :32].contiguous(), z)
    ext[:, 32:64] = eng.field_binary("fq", "mul", P[:, 32:].contiguous(), z)
    ext[:, 64:96] = z
    del z
    ext[:, 96:] = torch.randint(0, 256, (n, 64), dtype=torch.uint8, device=dev, generator=g)      # T1, T2: not read
    idx, kind, rows, groups = B.norm_plant(n, T, chunk, n)
    it = torch.from_numpy(idx).to(dev)
    ext[it] = torch.from_numpy(rows).to(dev)
    out = eng.batch_normalize(ext)
    assert out.shape == (n, 64)
    wrong = (out != P).any(dim=1)
    wrong[it] = False
    if bool(wrong.any()):
        first = torch.nonzero(wrong).flatten()[:8].cpu().tolist()
        pytest.fail("%s: %d unplanted rows differ from the points they were scaled from, first at %s (lane i %% T, position i // T: %s); "
                    "planted lanes: %s" % (where, int(wrong.sum()), first, _where(first, T), groups))
    del wrong
    want = O.batch_normalize(rows)
    got = out[it].cpu().numpy()
    bad = np.nonzero((got != want).any(axis=1))[0]
    if len(bad):
        pytest.fail("%s: %d planted rows differ from the oracle, first at %s (lane, position: %s), kinds %s"
                    % (where, len(bad), idx[bad[:8]].tolist(), _where(idx[bad[:8]], T), [B.norm_kinds[k][0] for k in kind[bad[:8]]]))
    zero = np.array([B.norm_kinds[k][1] for k in kind])
    assert (got[zero] == 0).all() and (zero.any() or not groups), where                 # Z = 0 mod q: (0, 0)
    st = torch.from_numpy(_sample(n, idx)).to(dev)
    assert (out[st].cpu().numpy() == O.batch_normalize(ext[st].cpu().numpy())).all(), "%s: strided sample vs the oracle" % where


@pytest.mark.parametrize("spec", B.NORM_RAGGED, ids=[B.norm_spec_id(s) for s in B.NORM_RAGGED])
def test_normalize_compressed(env, spec):
    eng, dev, table, lanes = env
    chunk, mult, off = spec
    n = mult * lanes + off
    assert B.norm_chunk(n, lanes) == chunk and n % chunk, (n, lanes)
    T = (n + chunk - 1) // chunk
    where = "k_normalize<%d> mode 1, n=%d, T=%d, lanes=%d" % (chunk, n, T, lanes)
    g = _gen(dev, 0x434F4D50 + n)
    s = _scalars(dev, g, n)
    st = torch.from_numpy(_sample(n, np.zeros(0, np.int64), 512)).to(dev)             # the oracle's ladder: 50 us a row
    sh = s[st].cpu().numpy()
    runs = [("fixedbase_mul", lambda: eng.fixedbase_mul_compressed(table, s), lambda: eng.fixedbase_mul(table, s),
             lambda: O.fixedbase_mul(sh, pt64(J.GENERATOR)))]
    if chunk == 16:
        P = eng.fixedbase_mul(table, _scalars(dev, g, n))
        ph = P[st].cpu().numpy()
        runs.append(("varbase_mul", lambda: eng.varbase_mul_compressed(s, P), lambda: eng.varbase_mul(s, P), lambda: O.varbase_mul(sh, ph)))
    for name, compressed, affine, oracle in runs:
        got = compressed()
        assert got.shape == (n, 32)
        wrong = (got != eng.compress(affine())).any(dim=1)
        if bool(wrong.any()):
            first = torch.nonzero(wrong).flatten()[:8].cpu().tolist()
            pytest.fail("%s: %s_compressed differs from compress(%s) in %d rows, first at %s (lane, position: %s)"
                        % (where, name, name, int(wrong.sum()), first, _where(first, T)))
        assert (got[st].cpu().numpy() == O.compress(oracle())).all(), "%s: %s_compressed, strided sample vs the oracle" % (where, name)


def test_zero_z_through_the_decoder(env):
    """decompress(enc, 1 | 8): an invalid encoding leaves the decoder as (0, 0), k_small_order_cofactor doubles that to Z = 0, and the
    normaliser meets it among the valid rows of its lane"""
    eng, dev, table, lanes = env
    n, chunk = 70001, 4
    assert dec_chunk(n, lanes, 8) == chunk and B.norm_chunk(n, lanes) == chunk and n % chunk, (n, lanes)
    T = (n + chunk - 1) // chunk
    g = _gen(dev, 0x5A45524F)
    enc = eng.compress(eng.fixedbase_mul(table, _scalars(dev, g, n)))
    idx = B.plant_positions(n, T, chunk)
    enc[torch.from_numpy(idx).to(dev)] = torch.from_numpy(B.bad_encodings(len(idx), n)).to(dev)
    out, ok = eng.decompress(enc, 1 | 8)
    eo, ek = O.decompress(enc.cpu().numpy(), 1 | 8)
    assert not ek[idx].any() and ek.sum() == n - len(idx) and (eo[idx] == 0).all()
    out, ok = out.cpu().numpy(), ok.cpu().numpy()
    bad = np.nonzero((ok != ek) | (out != eo).any(axis=1))[0]
    assert not len(bad), ("k_decompress<4> + k_small_order_cofactor + k_normalize<4>, n=%d, T=%d: %d rows differ from the oracle, first at %s "
                          "(lane, position: %s), planted: %s" % (n, T, len(bad), bad[:8].tolist(), _where(bad[:8], T), np.isin(bad[:8], idx).tolist()))


# --------------------------------------------------------------------------------------------------------------- sum tree
@pytest.mark.parametrize("layout", B.SUM_LAYOUTS)
@pytest.mark.parametrize("n", B.sum_sizes)
def test_point_sum(env, n, layout):
    eng, dev, table, lanes = env
    P = B.sum_layout(n, layout)
    want = O.point_sum(P)
    passes = B.sum_passes(n)
    got = eng.point_sum(P)
    assert (got == want).all(), "point_sum (host array), n=%d, layout %s, passes %s" % (n, layout, passes)
    got = eng.point_sum(torch.from_numpy(P).to(dev))
    assert (got.cpu().numpy() == want).all(), "point_sum (device tensor), n=%d, layout %s, passes %s" % (n, layout, passes)


# ---------------------------------------------------------------------------------------------------------------- Fq root
def test_fq_sqrt_patterns(env):
    """the patterns between random elements (a log with four random digits) and elements of odd order (e = 0), so that a wave holds
    e == 0 and e != 0 lanes"""
    eng, dev, table, lanes = env
    A, _ = B.sqrt_inputs()
    m = len(A)
    rng = np.random.default_rng(0x46515351)
    X = np.empty((3 * m, 32), np.uint8)
    X[0::3] = A
    X[1::3] = rng.integers(0, 256, size=(m, 32), dtype=np.uint8)
    odd = [B.fq_with_log(0, 1000 + k) for k in range(64)]
    X[2::3] = np.stack([b32(odd[k % 64]) for k in range(m)])
    eo, ek = O.field_op(O.FQ, "sqrt", X)
    assert ek[2::3].all() and 0 < ek[1::3].sum() < m
    for name, arg in (("host array", X), ("device tensor", torch.from_numpy(X).to(dev))):
        out, ok = eng.field_unary_ok("fq", "sqrt", arg)
        if name == "device tensor":
            out, ok = out.cpu().numpy(), ok.cpu().numpy()
        bad = np.nonzero((ok != ek) | (out != eo).any(axis=1))[0]
        pats = B.sqrt_patterns()
        assert not len(bad), ("fq sqrt (%s): %d of %d rows differ from the oracle; first logs: %s"
                              % (name, len(bad), len(X), [hex(pats[i // 3]) if i % 3 == 0 else "row %d" % i for i in bad[:8]]))


@pytest.mark.parametrize("variant", (1, 4))
def test_fq_sqrt_patterns_through_the_decoder(env, variant):
    """every pattern as the u^2 of an encoding, at a k_decompress<1> size and padded past 16 384 rows with valid encodings, where
    k_decompress<4> shares the inversion of four rows"""
    eng, dev, table, lanes = env
    _, E = B.sqrt_inputs()
    pats = B.sqrt_patterns()
    assert len(E) == len(pats)
    pool = O.compress(B.sum_pool()[0])
    n = 2 * len(E) + 1 if variant == 1 else 20011
    assert dec_chunk(n, lanes, 8) == variant, (n, lanes)
    T = (n + variant - 1) // variant
    at = (np.arange(len(E)) * n) // len(E)                                            # spread over every position of the lanes
    assert len(set((at // T).tolist())) == variant
    fill = np.arange(n) % len(pool)
    enc = pool[fill]
    enc[at] = E
    denc = torch.from_numpy(enc).to(dev)
    for flags in (0, 1, 1 | 2 | 4 | 8):
        po, pk = O.decompress(pool, flags)
        eo, ek = po[fill], pk[fill]
        eo[at], ek[at] = O.decompress(E, flags)
        out, ok = eng.decompress(denc, flags)
        out, ok = out.cpu().numpy(), ok.cpu().numpy()
        bad = np.nonzero((ok != ek) | (out != eo).any(axis=1))[0]
        hit = {int(r): hex(pats[k]) for k, r in enumerate(at)}
        assert not len(bad), ("k_decompress<%d>, n=%d, flags %d: %d rows differ from the oracle, first at %s (lane, position: %s), logs %s"
                              % (variant, n, flags, len(bad), bad[:8].tolist(), _where(bad[:8], T), [hit.get(int(i), "-") for i in bad[:8]]))
