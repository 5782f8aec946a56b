"""
Every wrapper of include/jubjub_hip.hpp that tests/cpp/test_reference_suite.cpp does not reach, executed on the GPU by
tests/cpp/test_mirror_calls.cpp and held to the project's Python restatements byte for byte, the size of each returned container included.
This module writes the vectors file (inputs and expected bytes: oracle.c_oracle, oracle.jubjub_ref and the tests/*_cases.py modules, never the
library) and runs one group per test, one child process each.  tests/test_cpp_mirror_stub_cpu.py is the CPU half: the same wrappers against a
recording stub of the C ABI under the host sanitizers.
"""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "test_mirror_calls.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "test_mirror_calls")

# The wrappers no other program executes, by the group that runs them.  Both programs print one `wrapper <name>` line for each; both tests hold
# the set of those lines to this table, so a wrapper dropped from a C++ file fails its test.
WRAPPERS = {
    "mul": ["multiply_vartime", "multiply2_vartime", "multiply2_scalars", "multiply_fixed_add_vartime", "batch_normalize", "HostBuffer", "multiply_raw"],
    "msm": ["msm_batch(shared)", "msm_batch(own)", "msm_ragged", "MsmBasis", "msm(basis,rows)", "MsmBasis::info"],
    "pedersen": ["PedersenTable::hash", "PedersenTable::hash_points", "PedersenTable::scalars"],
    "sig": ["MsmJob(sig)", "MsmJob(keyed)", "sigbatch_begin", "sigbatch_keyed_begin", "sigbatch_verify", "sigbatch_keyed_verify", "sigbatch_verdict",
            "sigbatch_ragged", "sigbatch_ragged_verify", "sigverify_each", "sig_challenge"],
    "ka": ["ka_kdf", "chacha20_xor"],
    "aead": ["poly1305", "aead_open", "aead_seal"],
    "hash": ["blake2s", "group_hash"],
}
ALL_WRAPPERS = sorted(w for ws in WRAPPERS.values() for w in ws)
N = 67                                             # one wave and three units


def printed_wrappers(stdout):
    return sorted(line.split(" ", 1)[1].strip() for line in stdout.splitlines() if line.startswith("wrapper "))


# ---------------------------------------------------------------------------------------------------- the vectors file
class Vectors:
    """`key hex` lines: one array per key, `-` for an empty one"""

    def __init__(self):
        self.lines = {}

    def put(self, key, value):
        b = value if isinstance(value, (bytes, bytearray)) else np.ascontiguousarray(value, dtype=np.uint8).tobytes()
        assert key not in self.lines, key
        self.lines[key] = bytes(b).hex() or "-"

    def nums(self, key, values):
        self.put(key, np.asarray([int(v) for v in values], dtype="<u8").view(np.uint8) if len(values) else b"")

    def num(self, key, value):
        self.nums(key, [value])

    def write(self, path):
        with open(path, "w") as f:
            for k, v in self.lines.items():
                f.write(k + " " + v + "\n")


def _spread(total, count):
    """`count` indices spread evenly over range(total), the first and the last among them"""
    return np.unique(np.linspace(0, total - 1, count).astype(np.int64))


def _pick_units(arrays, needs, count):
    """`count` units of an edge matrix, spread evenly over it; where the spread holds no unit that meets one of `needs` (predicates of a unit's
    index), the first unit of the matrix that does takes a slot"""
    n = len(arrays[0])
    idx = [int(i) for i in _spread(n, count)]
    assert len(idx) == count
    slot = 1
    for need in needs:
        if not any(need(i) for i in idx):
            idx[slot] = next(i for i in range(n) if need(i))
            slot += 2
    assert all(any(need(i) for i in idx) for need in needs)
    return [np.ascontiguousarray(x[np.array(idx)]) for x in arrays]


def vectors_mul(v, golden):
    from oracle import c_oracle as O
    from tests import buffer_cases as BC
    from tests import fixedvar_cases as FV
    from tests import sig_batch_cases as SC
    from tests import straus_cases as ST
    from tests.util import R, arr32, to_int, torsion_points

    tors = {bytes(t) for t in torsion_points(golden)} - {bytes(SC.IDENTITY)}

    def needs(scalars, points):
        """the identity, a torsion point, and the scalars 0, 1, r - 1, r"""
        out = [lambda i: any(bytes(p[i]) == bytes(SC.IDENTITY) for p in points), lambda i: any(bytes(p[i]) in tors for p in points)]
        return out + [(lambda i, k=k: any(to_int(s[i]) == k for s in scalars)) for k in (0, 1, R - 1, R)]

    a, p, b, q = ST.edge_matrix(golden)
    a, p, b, q = _pick_units((a, p, b, q), needs((a, b), (p, q)), N)
    v.put("mul.a", a), v.put("mul.p", p), v.put("mul.b", b), v.put("mul.q", q)
    v.put("mul.vartime", O.varbase_mul(a, p))
    v.put("mul.raw", O.varbase_mul(a, p))
    v.put("mul.mul2", ST.want(a, p, b, q))
    sa, sb = arr32([R - 1]), arr32([ST.EDGE_KS[20]])
    v.put("mul.sa", sa), v.put("mul.sb", sb)
    v.put("mul.mul2s", ST.want(np.repeat(sa, N, 0), p, np.repeat(sb, N, 0), q))
    g, fa, fb, fq = FV.edge_matrix(golden)["P+T8"]                                     # a base with a component of order 8
    fa, fb, fq = _pick_units((fa, fb, fq), needs((fa, fb), (fq,)), N)
    v.put("mul.fv.g", g), v.put("mul.fv.a", fa), v.put("mul.fv.b", fb), v.put("mul.fv.q", fq)
    v.put("mul.fv.want", FV.want(g, fa, fb, fq))
    ext = BC.ext_points(N, 605)                                                        # Z != 1, some rows with Z = 0
    v.put("mul.ext", ext)
    v.put("mul.norm", O.batch_normalize(ext))


def vectors_msm(v, golden):
    from oracle import c_oracle as O
    from tests import sig_batch_cases as SC
    from tests.util import rand_points, rand_scalars

    n, B = 40, 3
    p = rand_points(4101, n)
    p[0], p[1] = SC.IDENTITY, SC.T8                                                   # the identity and a point of order 8 among the terms
    s = rand_scalars(4102, B * n, full_width=True).reshape(B, n, 32)
    s[0, 2], s[1, 3] = 0, 0xFF
    v.put("msm.p", p), v.put("msm.s", s)
    v.put("msm.shared", np.stack([O.msm(s[b], p) for b in range(B)]))
    op = rand_points(4103, B * n).reshape(B, n, 64)
    os_ = rand_scalars(4104, B * n, full_width=True).reshape(B, n, 32)
    v.put("msm.op", op), v.put("msm.os", os_)
    v.put("msm.own", np.stack([O.msm(os_[b], op[b]) for b in range(B)]))
    off = [0, 0, 5, 40]
    v.nums("msm.offsets", off)
    rows = [O.msm(s[0][lo:hi], p[lo:hi]) if hi > lo else SC.IDENTITY for lo, hi in zip(off[:-1], off[1:])]
    assert bytes(rows[0]) == bytes(SC.IDENTITY)
    v.put("msm.ragged", np.stack(rows))
    v.put("msm.ragged_empty", np.stack([SC.IDENTITY, SC.IDENTITY]))
    bp = rand_points(4105, 64)
    bs = rand_scalars(4106, 2 * n, full_width=True).reshape(2, n, 32)
    v.put("msm.bp", bp), v.put("msm.bs", bs)
    v.put("msm.basis", np.stack([O.msm(bs[b], bp[:n]) for b in range(2)]))


def vectors_pedersen(v, golden):
    from tests import pedersen_cases as PC

    def put_case(key, case, n):
        rows = np.ascontiguousarray(case.rows[:n, :case.row_stride])
        gens = PC.generators(case.gens)
        pts = np.stack([PC.point_bytes(PC.expected(gens, case.seg_chunks, case.bits(i))) for i in range(n)])
        v.nums(key + ".params", [case.row_stride, case.prefix, case.prefix_bits, n])
        v.nums(key + ".fields", [x for f in case.fields for x in f])
        v.put(key + ".rows", rows)
        v.put(key + ".points", pts)
        v.put(key + ".hash", pts[:, :32])
        v.put(key + ".scalars", PC.expected_scalars(case, n))                          # (nseg, n, 32): segment-major
        return PC.expected_scalars(case, n)

    v.put("ped.gens2", PC.gens_bytes("two"))
    v.put("ped.gens3", PC.gens_bytes("three"))
    one = PC.Case("mirror_one_segment", "two", 3, 2, ((0, 7),), prefix=0b01, prefix_bits=2, seed=31)           # 9 bits: three chunks, segment 0 only
    both = PC.Case("mirror_both_segments", "two", 3, 3, ((0, 7), (1, 9)), prefix=0b1, prefix_bits=1, seed=32)  # 17 bits: six chunks, both segments
    s1 = put_case("ped.one_segment", one, N)
    s2 = put_case("ped.both_segments", both, N)
    assert not s1[1].any() and s1[0].any(axis=1).all() and s2[1].any(axis=1).all(), "segment 1 is reached by the second case only"
    merkle = PC.BY_ID["merkle"]
    assert merkle.fields == PC.MERKLE_FIELDS and merkle.row_stride == 64 and merkle.prefix_bits == 6
    put_case("ped.merkle", merkle, 5)


def vectors_sig(v, golden):
    from tests import sig_batch_cases as SC
    from tests import sig_challenge_cases as CH
    from tests import sig_each_cases as SE
    from tests import sig_keyed_cases as SK
    from tests import sig_seg_cases as SG

    code = {"ok": 0, "reject": 1, "malformed": 2}

    def put_arrays(key, base, r, a, s, c, z, zip216):
        v.put(key + ".base", base), v.put(key + ".r", r), v.put(key + ".s", s), v.put(key + ".c", c)
        if a is not None:
            v.put(key + ".a", a)
        if z is not None:
            v.put(key + ".z", z)
        v.num(key + ".zip216", 1 if zip216 else 0)

    # a valid, a rejecting and a malformed batch of 9; the non-canonical key is malformed under the ZIP-216 rule and accepted without it
    batches = [SC.batch(9), SC.batch(9, "bad_s", 4), SC.batch(9, "off_curve_r", 8), SC.batch(9, "noncanonical_a_zip216", 3), SC.batch(9, "noncanonical_a", 3)]
    wants = ["ok", "reject", "malformed", "malformed", "ok"]
    v.num("sig.batches", len(batches))
    for i, (b, want) in enumerate(zip(batches, wants)):
        out = SC.full_evaluation(b)
        assert SG.verdict(out) == want and bytes(out) == bytes(b.expected), b.name
        put_arrays("sig.b%d" % i, b.base, b.r, b.a, b.s, b.c, b.z, b.flags & SC.ZIP216)
        v.put("sig.b%d.out" % i, out)
        v.num("sig.b%d.verdict" % i, code[want])
    assert [b.flags for b in batches] == [0, 0, 0, 1, 0]

    keyed = [SK.layout("valid", [4, 0, 5]), SK.layout("reject", [4, 0, 5], "bad_s", 4), SK.layout("malformed", [4, 0, 5], bad_key=1),
             SK.regrouped(9, "noncanonical_a_zip216", 3), SK.regrouped(9, "noncanonical_a", 3)]
    v.num("sig.keyed", len(keyed))
    for i, (k, want) in enumerate(zip(keyed, wants)):
        out = SK.keyed_evaluation(k)
        assert SG.verdict(out) == want and k.n == 9, k.name
        put_arrays("sig.k%d" % i, k.base, k.r, None, k.s, k.c, k.z, k.flags & SC.ZIP216)
        v.put("sig.k%d.keys" % i, k.keys)
        v.nums("sig.k%d.offsets" % i, k.offsets)
        v.put("sig.k%d.out" % i, out)
        v.num("sig.k%d.verdict" % i, code[want])
    assert [k.flags for k in keyed] == [0, 0, 0, 1, 0]

    reject_point = SC.batch(9, "bad_s", 4).expected
    off_curve = SC.pt64((0, 2))
    u_only = SC.pt64((5, 1))
    points = [SC.IDENTITY, SC.MALFORMED, reject_point, SC.bases()["prime"], off_curve, u_only]
    v.put("sig.verdict.points", np.stack(points))
    v.put("sig.verdict.want", bytes([0, 2, 1, 1, 1, 1]))
    assert [SG.verdict(p) for p in points] == ["ok", "malformed", "reject", "reject", "reject", "reject"]

    # segments: valid, empty, rejecting, malformed; then one under the ZIP-216 rule, whose arrays are also checked without it
    seg = SG.layout("mirror", [3, 0, 4, 2], {2: ("bad_s", 1), 3: ("off_curve_r", 0)})
    zseg = SG.layout("mirror zip216", [2, 3], {1: ("noncanonical_a_zip216", 1)})
    assert seg.flags == 0 and zseg.flags == SC.ZIP216
    ragged = []
    for case, flags in ((seg, 0), (zseg, SC.ZIP216), (zseg, 0)):
        rows = []
        for g in range(case.S):
            sl = case.slice(g)
            rows.append(SC.full_evaluation(SC.Batch(sl.name, sl.base, sl.r, sl.a, sl.s, sl.c, sl.z, flags, None)))
        if flags == case.flags:
            assert (np.stack(rows) == case.expected).all(), case.name
        ragged.append((case, flags, np.stack(rows)))
    assert [SG.verdict(r) for r in ragged[0][2]] == ["ok", "ok", "reject", "malformed"]
    assert [SG.verdict(r) for r in ragged[1][2]] == ["ok", "malformed"] and [SG.verdict(r) for r in ragged[2][2]] == ["ok", "ok"]
    v.num("sig.ragged", len(ragged))
    for i, (case, flags, rows) in enumerate(ragged):
        put_arrays("sig.r%d" % i, case.base, case.r, case.a, case.s, case.c, case.z, flags)
        v.nums("sig.r%d.offsets" % i, case.offsets)
        v.put("sig.r%d.out" % i, rows)
        v.put("sig.r%d.verdicts" % i, bytes(code[SG.verdict(r)] for r in rows))

    each = [SE.planted_batch(N, ["torsion_r", "bad_s", "off_curve_r", "r_order2", "noncanonical_a"]),
            SE.planted_batch(N, ["noncanonical_a_zip216", "torsion_a_odd_c", "s_plus_r", "c_all_ones", "bad_r"])]
    v.num("sig.each", len(each))
    for i, b in enumerate(each):
        cof, less = SE.full_evaluation(b, True), SE.full_evaluation(b, False)
        assert (cof == b.expect[True]).all() and (less == b.expect[False]).all() and (cof != less).any(), b.name
        assert {SE.OK, SE.REJECT, SE.MALFORMED} <= set(cof.tolist())
        put_arrays("sig.e%d" % i, b.base, b.r, b.a, b.s, b.c, None, b.flags & SE.ZIP216)
        v.put("sig.e%d.cofactored" % i, cof)
        v.put("sig.e%d.cofactorless" % i, less)
    assert [b.flags for b in each] == [0, SE.ZIP216]

    lens = (0, 1, 127, 128, 129)
    msgs = [CH.rng_bytes(5100 + L, L).tobytes() for L in lens]
    R, A = CH.parts(len(lens), "both", seed=3)
    v.put("sig.ch.r", R), v.put("sig.ch.a", A)
    v.nums("sig.ch.lens", lens)
    v.put("sig.ch.msgs", b"".join(msgs))
    v.put("sig.ch.personal", CH.REDJUBJUB)
    v.put("sig.ch.both", CH.expected(CH.REDJUBJUB, R, A, msgs))
    v.put("sig.ch.no_r", CH.expected(CH.REDJUBJUB, None, A, msgs))
    v.put("sig.ch.no_a", CH.expected(CH.REDJUBJUB, R, None, msgs))
    v.put("sig.ch.null_personal", CH.expected(None, R, A, msgs))


def vectors_ka(v, golden):
    from tests import aead_cases as AE
    from tests import ka_cases as KC

    encs = KC.tiled(N)
    sk = KC.SCALARS[10]
    v.put("ka.p", encs), v.put("ka.sk", sk)
    cases = [(KC.SAPLING_FLAGS, KC.SAPLING_PERSONAL), (KC.ZIP216, None), (KC.SAPLING_FLAGS, None), (KC.ZIP216, KC.PERSONALS["ones"])]
    v.num("ka.cases", len(cases))
    for i, (flags, personal) in enumerate(cases):
        keys, ok = KC.expected(sk, encs, flags, personal)
        assert ok.any() and not ok.all()
        v.num("ka.k%d.flags" % i, flags)
        if personal is not None:
            v.put("ka.k%d.personal" % i, personal)
        v.put("ka.k%d.keys" % i, keys), v.put("ka.k%d.ok" % i, ok)
    ciphers = [(52, 60, 1, None), (68, 68, 0xFFFFFFFF, KC.NONCE)]                        # the compact-note shape in a wider stride; the counter's wrap
    v.num("ka.ciphers", len(ciphers))
    for i, (length, stride, counter, nonce) in enumerate(ciphers):
        keys = AE.pool_keys(N, 8, 8100 + i)
        data = KC.rng_bytes(8200 + i, N, stride)
        k = "ka.c%d" % i
        v.put(k + ".keys", keys)
        v.put(k + ".in", data.reshape(-1)[:(N - 1) * stride + length])
        v.num(k + ".len", length), v.num(k + ".stride", stride), v.num(k + ".counter", counter)
        if nonce is not None:
            v.put(k + ".nonce", nonce)
        v.put(k + ".out", KC.chacha20_xor(keys, data, length, nonce, counter))


def vectors_aead(v, golden):
    from tests import aead_cases as AE
    from tests import ka_cases as KC

    aad17 = KC.rng_bytes(8300, 17).tobytes()
    cases = [(length, length + pad, aad, nonce) for length in (4, 64, 68) for pad in (16, 28) for aad in (b"", aad17) for nonce in (None, AE.NONCE)]
    v.num("aead.cases", len(cases))
    for i, (length, stride, aad, nonce) in enumerate(cases):
        k = "aead.c%d" % i
        keys = AE.pool_keys(N, 8, 8400 + i)
        data = KC.rng_bytes(8500 + i, N, stride)
        v.num(k + ".len", length), v.num(k + ".stride", stride)
        v.put(k + ".keys", keys)
        v.put(k + ".plain", data.reshape(-1)[:(N - 1) * stride + length])
        v.put(k + ".aad", aad)
        if nonce is not None:
            v.put(k + ".nonce", nonce)
        if not aad and nonce is None:                                                 # the MAC alone knows neither: once per length and stride
            v.put(k + ".tags", AE.mac_rows(keys, data, length))
        sealed = AE.seal_rows(keys, data, length, nonce, aad)
        v.put(k + ".sealed", sealed)
        rows = KC.rng_bytes(8600 + i, N, stride)
        rows[:, :length + 16] = sealed
        victims = list(range(0, N, 3))
        okeys, rows, _ = AE.tamper(keys, rows, length, victims)
        plain, ok = AE.open_rows(okeys, rows, length, nonce, aad)
        assert ok.sum() == N - len(victims) and not plain[victims].any() and (plain[ok == 1] == data[ok == 1, :length]).all()
        v.put(k + ".open_keys", okeys)
        v.put(k + ".open_in", rows.reshape(-1)[:(N - 1) * stride + length + 16])
        v.put(k + ".opened", plain), v.put(k + ".ok", ok)


def vectors_hash(v, golden):
    from tests import group_hash_cases as GH

    cases = [(N, p, m, pad) for m in (0, 11, 64) for pad in (0, 5) for p in (0, 64)] + [(0, 64, 11, 0)]
    v.num("hash.cases", len(cases))
    for i, (n, prefix_len, msg_len, pad) in enumerate(cases):
        k = "hash.c%d" % i
        shape = (prefix_len, msg_len)
        personal = GH.PERSONALS[i % len(GH.PERSONALS)] if i % 3 else None             # null and given under every length
        flags = GH.FLAG_SETS[i % len(GH.FLAG_SETS)]
        prefix = GH.prefix_of(shape)
        msgs = GH.messages(shape, n)
        buf, _ = GH.layout(msgs, pad)
        stride = msg_len + pad
        v.num(k + ".n", n), v.num(k + ".len", msg_len), v.num(k + ".stride", stride), v.num(k + ".flags", flags)
        v.put(k + ".msgs", buf[:(n - 1) * stride + msg_len] if n and msg_len else b"")
        v.put(k + ".prefix", prefix)
        if personal is not None:
            v.put(k + ".personal", personal)
        pts, ok = GH.expected(personal, prefix, msgs, flags)
        v.put(k + ".digests", GH.digests(personal, prefix, msgs))
        v.put(k + ".points", pts), v.put(k + ".ok", ok)
    assert {GH.FLAG_SETS[i % len(GH.FLAG_SETS)] for i in range(len(cases))} == set(GH.FLAG_SETS)


WRITERS = {"mul": vectors_mul, "msm": vectors_msm, "pedersen": vectors_pedersen, "sig": vectors_sig, "ka": vectors_ka, "aead": vectors_aead, "hash": vectors_hash}


def write_vectors(group, path, golden):
    v = Vectors()
    WRITERS[group](v, golden)
    v.write(path)


# ---------------------------------------------------------------------------------------------------- the binary and its children
def build_binary():
    """g++ only, against the C-ABI library; rebuilt when the source, either header or the library is newer"""
    libdir = os.path.join(ROOT, "jubjub_amd", "lib")
    deps = [SRC, os.path.join(ROOT, "include", "jubjub_hip.hpp"), os.path.join(ROOT, "include", "jubjub_hip.h"), os.path.join(libdir, "libjubjub_hip.so")]
    if os.path.exists(BIN) and all(os.path.getmtime(d) <= os.path.getmtime(BIN) for d in deps):
        return BIN
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", BIN, "-L", libdir, "-ljubjub_hip",
                           "-Wl,-rpath,$ORIGIN/../../jubjub_amd/lib", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"])
    return BIN


_CHILD_DIED = None      # set when a child ended by a signal or at its time limit: no later group starts another process on the GPU


def run_group(group, tmp_path, golden):
    global _CHILD_DIED
    if _CHILD_DIED:
        pytest.fail("not started: " + _CHILD_DIED, pytrace=False)
    build_binary()
    vec = tmp_path / ("vectors_%s.txt" % group)
    write_vectors(group, str(vec), golden)
    try:
        r = subprocess.run([BIN, str(vec), group], capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        _CHILD_DIED = "the child of group %r did not end within its time limit" % group
        pytest.fail(_CHILD_DIED, pytrace=False)
    print(r.stdout)
    print(r.stderr)
    if r.returncode < 0 or r.returncode in (134, 139):
        _CHILD_DIED = "the child of group %r ended by a signal (return code %d)" % (group, r.returncode)
        pytest.fail(_CHILD_DIED + "\n" + r.stdout[-2000:] + r.stderr[-2000:], pytrace=False)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "ALL PASSED" in r.stdout
    assert printed_wrappers(r.stdout) == sorted(WRAPPERS[group])


def test_wrapper_table_is_the_list_of_unreached_wrappers():
    """CPU-side: every name of the table once, and each wrapper's C entry point is in the header the programs compile"""
    assert len(ALL_WRAPPERS) == len(set(ALL_WRAPPERS)) == 34
    hpp = open(os.path.join(ROOT, "include", "jubjub_hip.hpp")).read()
    for name in ALL_WRAPPERS:
        plain = name.split("(")[0].split("::")[-1]
        assert plain + "(" in hpp or "class " + plain in hpp, name


def test_mirror_calls_compiles():
    """CPU-side: the program compiles against the mirror and the C ABI"""
    assert os.path.exists(build_binary())


@pytest.mark.gpu
def test_mirror_mul(tmp_path, golden):
    run_group("mul", tmp_path, golden)


@pytest.mark.gpu
def test_mirror_msm(tmp_path, golden):
    run_group("msm", tmp_path, golden)


@pytest.mark.gpu
def test_mirror_pedersen(tmp_path, golden):
    run_group("pedersen", tmp_path, golden)


@pytest.mark.gpu
def test_mirror_sig(tmp_path, golden):
    run_group("sig", tmp_path, golden)


@pytest.mark.gpu
def test_mirror_ka(tmp_path, golden):
    run_group("ka", tmp_path, golden)


@pytest.mark.gpu
def test_mirror_aead(tmp_path, golden):
    run_group("aead", tmp_path, golden)


@pytest.mark.gpu
def test_mirror_hash(tmp_path, golden):
    run_group("hash", tmp_path, golden)
