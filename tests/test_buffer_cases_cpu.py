"""tests/buffer_cases.py, pinned without a GPU: the table covers the header, its sizes and its guard come from the constants in the kernels'
source, the checker sees what it is there to see, every row can be built, and the host-only entry points already run through a guarded arena."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import buffer_cases as BC  # noqa: E402
from buffer_cases import ALIGN, CASES, EXEMPT, GUARD, SIZES, SKEWS, Arena, K, Run  # noqa: E402

ROOT = BC.ROOT
HANDLES = ("jj_ctx", "jj_table", "jj_msm_basis", "jj_msm_job", "jj_multi", "jj_mtable")


def _prototypes():
    """{entry point: [(const?, base type, pointer depth)]} of include/jubjub_hip.h (the parsing of tests/test_rust_shim_signatures.py, with the type names kept)"""
    text = open(os.path.join(ROOT, "include", "jubjub_hip.h")).read()
    text = re.sub(r"//.*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    out = {}
    for name, args in re.findall(r"^\s*(?:const\s+)?[A-Za-z_][\w\s\*]*?\b(jj_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.M):
        params = []
        for p in [a.strip() for a in args.split(",")] if args.strip() not in ("", "void") else []:
            depth = p.count("*") + p.count("[")
            words = re.sub(r"\[\d*\]|\*", " ", p).split()
            const = "const" in words
            words = [w for w in words if w != "const"]
            params.append((const, words[0], depth))
        assert name not in out
        out[name] = params
    return out


def _needs_a_row(params):
    """a pointer the entry point may write through that is neither a handle nor a handle out-parameter"""
    return any(depth and not const and base not in HANDLES for const, base, depth in params)


def test_every_entry_point_that_writes_through_a_pointer_has_a_row():
    protos = _prototypes()
    assert len(protos) >= 100, "header parser lost prototypes (%d)" % len(protos)
    assert _needs_a_row(protos["jj_fq_add"]) and _needs_a_row(protos["jj_fr_char_le_bits"]) and _needs_a_row(protos["jj_device_info"])
    assert not _needs_a_row(protos["jj_ctx_create"]) and not _needs_a_row(protos["jj_msm_begin"]) and not _needs_a_row(protos["jj_fixedbase_table_destroy"])
    covered = {fn for c in CASES for fn in c.covers}
    missing = sorted(fn for fn, params in protos.items() if _needs_a_row(params) and fn not in covered and fn not in EXEMPT)
    assert missing == [], "entry points that write through a pointer and have neither a row in buffer_cases.CASES nor a reason in EXEMPT: %s" % missing
    assert sorted(covered - set(protos)) == [] and sorted(set(EXEMPT) - set(protos)) == [], "rows or exemptions for entry points the header lacks"
    assert sorted(covered & set(EXEMPT)) == []
    assert all(isinstance(r, str) and r for r in EXEMPT.values())
    for c in CASES:                                         # a row names every pointer parameter of its prototype, in order
        if c.call is None:
            ptrs = [a for a in c.args if isinstance(a, str) and a not in ("ctx", "n")] + [a for a in c.args if isinstance(a, tuple) and a[0] in ("handle", "handles")]
            want = [p for p in protos[c.fn] if p[2] and p[1] not in ("jj_ctx", "jj_multi")]
            assert len(ptrs) == len(want) and len(c.args) == len(protos[c.fn]), c.id
            assert set(a for a in c.args if isinstance(a, str)) - {"ctx", "n"} == {k for k, _ in c.ins + c.outs}, c.id


def pipelined_entry_points():
    """the entry points whose body, or the shared body they forward to, asks pipe_chunk_for for a chunk length and hands it to the front end
    (run_batch in jj_abi.hip, the one caller of run_pipelined)"""
    abi = open(os.path.join(BC.CSRC, "jj_abi.hip")).read()
    bodies, current = set(), None
    for line in abi.split("\n"):
        m = re.match(r"^(?:static int|JJ_API int) (\w+)\(", line)
        if m:
            current = m.group(1)
        if "pipe_chunk_for(" in line:
            bodies.add(current)
    assert len(bodies) == 6 == abi.count("pipe_chunk_for("), bodies
    assert abi.count("run_pipelined(") == 1
    forwards = dict(re.findall(r"^JJ_API int (jj_\w+)\(.*?\) \{ return (\w+)\(", abi, flags=re.M))
    return {fn for fn in bodies if fn.startswith("jj_")} | {fn for fn, body in forwards.items() if body in bodies}


def test_shared_pieces_are_written_once():
    """in jj_abi.hip every refusal of a table an entry point cannot use, the loop over the chunks of a call and the grid of k_varbase_mont_x1
    stand in one helper each (table_check, for_chunks, mont_x1_launch)"""
    abi = open(os.path.join(BC.CSRC, "jj_abi.hip")).read()
    for refusal in ("fixed-base table belongs to another device", "Pedersen table (jj_pedersen_table_create): only jj_pedersen_hash_vartime takes it",
                    "needs the table of one base (jj_fixedbase_table_create)"):
        assert abi.count(refusal) == 1, refusal
    assert len(re.findall(r"for \(size_t lo = 0; lo < n; lo \+= ", abi)) == 1
    assert abi.count("hipLaunchKernelGGL(k_varbase_mont_x1,") == 1


def test_the_table_holds_what_it_must():
    ids = {c.id for c in CASES}
    fns = {c.fn for c in CASES}
    for f in ("fq", "fr"):
        for op in ("add", "sub", "mul", "neg", "square", "double", "invert", "sqrt", "pow", "from_bytes", "from_bytes_wide", "to_le_bits"):
            assert "jj_%s_%s" % (f, op) in fns
    opts = lambda fn: [c.options for c in CASES if c.fn == fn][0]      # noqa: E731
    for fn in ("jj_varbase_mul", "jj_varbase_mul_compressed", "jj_varbase_mul_ct", "jj_varbase_mul_vartime", "jj_varbase_mul_vartime_compressed",
               "jj_varbase_mul_scalar", "jj_varbase_mul_exact"):
        assert opts(fn) == [{}, {"vb_quad_max": 1}, {"vb_ct_window": 3, "vb_quad_max": 1}, {"vb_ct_window": 2, "vb_quad_max": 1}]
    for fn in ("jj_varbase_mul2_vartime", "jj_varbase_mul2_vartime_compressed", "jj_varbase_mul2_scalars"):
        assert opts(fn) == [{"vb_mul2_window": 4}, {"vb_mul2_window": 5}]
    for w in (7, 6, 8, 13):
        assert {"jj_fixedbase_mul[w%d]" % w, "jj_fixedbase_mul_compressed[w%d]" % w} <= ids
    for w in (7, 8):
        assert {"jj_fixedvar_mul_vartime[w%d]" % w, "jj_fixedvar_mul_vartime_compressed[w%d]" % w} <= ids and opts("jj_fixedvar_mul_vartime") == [{}, {"vb_quad_max": 1}]
    assert {"jj_decompress[flags%d]" % f for f in (0, 1, 3, 13)} <= ids
    assert opts("jj_msm") == [{}, {"msm_small_max": 0}]
    assert {"jj_msm_batch[shared]", "jj_msm_batch[distinct]", "jj_msm_basis_mul[mode1]", "jj_msm_basis_mul[mode2]", "jj_msm_ragged", "jj_msm_partial",
            "jj_msm_combine_dev", "jj_msm_dev", "jj_msm_begin", "jj_random_points[subgroup0]"} <= ids
    assert {c.fn for c in CASES if c.pipelined} == pipelined_entry_points()
    for S in SIZES:                                         # the ragged rows: empty segments at the front, in the middle and at the end
        lens = BC.ragged_lengths(S)
        assert lens[0] == 0 and lens[S // 2] == 0 and lens[-1] == 0 and (S < 4 or any(lens))
    assert any(S % K["finish_rows"] for S in SIZES)


def test_sizes_and_guard_come_from_the_source():
    """the constants the sizes bracket, each where the kernels' source has it"""
    abi = open(os.path.join(BC.CSRC, "jj_abi.hip")).read()
    assert K["block"] == 256 and set(re.findall(r"hipLaunchKernelGGL\(\(?k_field_\w+(?:<[^>]*>)?\)?, dim3\(blocks_for\(n\)\), dim3\((\d+)\)", abi)) == {"256"}
    msmk, msm = open(os.path.join(BC.CSRC, "jj_msm_kernels.h")).read(), open(os.path.join(BC.CSRC, "jj_msm.hip")).read()
    assert (K["wave"], K["quad"], K["mont_x1_units"], K["finish_rows"]) == (64, 4, 16, 16)
    assert re.search(r"blocks_for\(64 \* \(\(n \+ 64 \* MONT_X1_UNITS - 1\) / \(64 \* MONT_X1_UNITS\)\)\)", abi)       # a wave of k_varbase_mont_x1 takes 64 x MONT_X1_UNITS units
    # the finish kernels: one quad per row, MSM_BATCH_FINISH_ROWS rows per wave, in both launches
    assert msmk.count("row = blockIdx.x * MSM_BATCH_FINISH_ROWS + (threadIdx.x >> 2)") == 2 and K["finish_rows"] * K["quad"] == K["wave"]
    for kern in ("k_msm_batch_finish", "k_msm_ragged_finish"):
        assert re.search(r"hipLaunchKernelGGL\(%s, dim3\(blocks_for\(gn, MSM_BATCH_FINISH_ROWS\)\), dim3\(%d\)" % (kern, K["wave"]), msm), kern
    assert K["bounce_threshold"] == 1 << 20
    assert SIZES == BC.derive_sizes(K) == (1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
    assert BC.MAX_ROW_BYTES == 256                                               # to_le_bits
    widths = {w for c in CASES for _, w in c.outs}
    assert widths <= {1, 4, 8, 32, 64, 96, 160, 256, K["msm_partial_bytes"]} and {1, 4, 32, 64, 96, 160, 256} <= widths
    bound = 2 * max(K["block"] * BC.MAX_ROW_BYTES, K["wave"] * K["mont_x1_units"] * 64)
    assert GUARD >= bound and GUARD % ALIGN == 0 and GUARD < bound + ALIGN
    assert SKEWS == (0, 16, 496)


def test_the_patterns_differ_everywhere():
    g, f = BC._images(np, 1 << 16)
    assert (g != f).all() and not np.isin(f, (0, 1)).any()
    assert len(set(g[:256].tolist())) == 256                                     # position-dependent: every value within 256 bytes
    assert (g[1:] != g[:-1]).all() and (f[1:] != f[:-1]).all()                   # no two neighbours alike: a shifted copy is seen


# ---- the checker checks: a Python stand-in for an entry point writes into the arena
def _stand_in(skew, n=65):
    a = Arena()
    a.carve(n * 32, skew, "in", "a")
    a.carve(n * 32, (skew + 16) % ALIGN if skew else 0, "out", "out")
    a.carve(n, skew, "out", "ok")
    src = np.arange(n * 32, dtype=np.uint32).astype(np.uint8)
    a.commit(None, {"a": src})
    assert a.ptr("a") % ALIGN == skew and a.ptr("ok") % ALIGN == skew and a.base % ALIGN == 0
    return a, src


def _write(a, name, data, at=0):
    r = a.region(name)
    a.view[r.off + at:r.off + at + len(data)] = data


@pytest.mark.parametrize("skew", SKEWS)
def test_checker_sees_each_kind_of_stray_write(skew):
    n = 65
    want_out, want_ok = np.full(n * 32, 7, np.uint8), np.ones(n, np.uint8)
    a, src = _stand_in(skew)
    assert a.violations() == [] and a.untouched("out") and a.untouched("ok")
    # regions end at exactly their length: the guard behind an `ok` array of 65 bytes begins at its 66th byte
    assert a.region("ok").nbytes == n and a.region("out").off - (a.region("a").off + a.region("a").nbytes) >= GUARD
    _write(a, "out", want_out)
    _write(a, "ok", want_ok)
    assert a.violations() == [] and (a.read("out") == want_out).all() and (a.read("ok") == want_ok).all() and not a.untouched("out")   # a clean call
    assert (a.read("a") == src).all()

    def one(name, at, value=None):
        b, _ = _stand_in(skew)
        _write(b, "out", want_out)
        _write(b, "ok", want_ok)
        r = b.region(name)
        pos = r.off + at
        b.view[pos] = (int(b.view[pos]) ^ 0x40) if value is None else value(int(b.view[pos]))
        return b.violations()

    assert one("ok", n) == [{"kind": "guard", "region": "ok", "side": "behind", "distance": 0, "count": 1}]             # directly behind an output
    assert one("out", n * 32) == [{"kind": "guard", "region": "out", "side": "behind", "distance": 0, "count": 1}]
    assert one("out", -1) == [{"kind": "guard", "region": "out", "side": "front", "distance": 1, "count": 1}]           # directly in front of it
    assert one("ok", n + GUARD - 1) == [{"kind": "guard", "region": "ok", "side": "behind", "distance": GUARD - 1, "count": 1}]   # the far end of the last guard
    first = -a.region("a").off
    assert one("a", first) == [{"kind": "guard", "region": "a", "side": "front", "distance": a.region("a").off, "count": 1}]      # the far end of the first
    assert one("a", 5 * 32 + 3) == [{"kind": "input", "region": "a", "side": "inside", "distance": 5 * 32 + 3, "count": 1}]       # a byte flipped inside an input
    # A write that leaves the guard's own value in place is reported as nothing -- it cannot be told from no write.  That is why the pattern
    # depends on the position (a constant or a shifted copy agrees with it at one offset in 256 at most) and differs from the outputs' fill.
    assert one("out", n * 32, value=lambda v: v) == []
    b, _ = _stand_in(skew)
    r = b.region("out")
    b.view[r.off + n * 32:r.off + n * 32 + 40] = 0                                # a constant over 40 guard bytes: one run, or two around a byte that is 0 anyway
    v = b.violations()
    assert sum(x["count"] for x in v) >= 39 and v[0]["side"] == "behind" and v[0]["region"] == "out"


@pytest.mark.parametrize("skew", SKEWS)
def test_an_unwritten_output_row_cannot_pass(skew):
    """the fill of an output never equals what an entry point would write there: field elements, points, 0 / 1 bytes"""
    a, _ = _stand_in(skew)
    want_out, want_ok = np.full(65 * 32, 7, np.uint8), np.ones(65, np.uint8)
    _write(a, "out", want_out[:64 * 32])                                           # row 64 of `out`, byte 64 of `ok` never written
    _write(a, "ok", want_ok[:64])
    assert a.violations() == []
    assert (a.read("out") != want_out).any() and (a.read("ok") != want_ok).any() and (a.read("ok")[64] not in (0, 1))
    for bit in (0, 1):                                                             # whatever the oracle's byte is
        assert (a.read("ok") != np.full(65, bit, np.uint8))[64]
    assert not np.isin(a.fill("ok"), (0, 1)).any()


# ---- every row of the table can be built
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_row_builds_at_three_units(case):
    ins, outs = case.data(3)
    assert sorted(ins) == sorted(k for k, _ in case.ins) and sorted(outs) == sorted(k for k, _ in case.outs)
    for name, w in case.ins:
        assert ins[name].dtype == np.uint8 and ins[name].shape == (case.nrows(name, 3), w), (name, ins[name].shape)
    for name, w in case.outs:
        if outs[name] is not None:
            assert outs[name].dtype == np.uint8 and outs[name].ndim == 2 and outs[name].shape[1] == w, (name, outs[name].shape)
            assert outs[name].shape[0] <= case.nrows(name, 3) and (outs[name].shape[0] == case.nrows(name, 3) or case.host_only)
    assert case.options and all(isinstance(o, dict) for o in case.options)


# ---- the host-only entry points, through a pageable arena, here and now
HOST_ONLY = [c for c in CASES if c.host_only]


@pytest.fixture(scope="module")
def lib():
    from jubjub_amd import _lib

    return _lib.load()


@pytest.mark.parametrize("case", HOST_ONLY, ids=[c.id for c in HOST_ONLY])
def test_host_only_entry_points_keep_to_their_buffers(lib, case):
    assert {c.fn for c in HOST_ONLY} == {"jj_msm_combine", "jj_msm_fold_partials", "jj_fr_char_le_bits", "jj_plan_host_chunks", "jj_plan_msm_ragged_items",
                                         "jj_plan_msm_host_passes", "jj_plan_msm_ragged", "jj_plan_msm_basis"}
    sizes = (1, 3, 4, 5, 15, 16, 17, 63, 64, 65) if case.sized else (1,)           # records of 8 KB and Python window sums: the small sizes
    for n in sizes:
        for skew in SKEWS:
            run = Run(case, n, lambda name, role: "host", lambda name, role, skew=skew: skew, {})
            rc = run.call(lib)
            assert rc == (case.rc(n) if case.rc else 0), (case.id, n, skew, rc)
            assert run.problems(lib) == [], (case.id, n, skew)


def test_capped_writers_stop_at_cap(lib):
    """too little room: JJ_ERR_INVALID, the count set all the same, not one entry written; room to spare: the entries past the count untouched"""
    for fn in ("jj_plan_host_chunks", "jj_plan_msm_ragged_items"):
        small, exact, large = [next(c for c in CASES if c.id == "%s[cap_%s]" % (fn, v)) for v in ("small", "exact", "large")]
        out = small.outs[0][0]
        for n in (5, 64, 65):
            assert small.rc(n) == BC.INVALID and exact.rc(n) == 0 and large.rc(n) == 0
            assert small.out_bytes(n)[out] < exact.out_bytes(n)[out] < large.out_bytes(n)[out] and small.out_bytes(n)[out] > 0
            assert small.data(n)[1][out] is None and small.data(n)[1]["count"] is not None
            assert exact.data(n)[1][out].nbytes == exact.out_bytes(n)[out] < large.out_bytes(n)[out]
