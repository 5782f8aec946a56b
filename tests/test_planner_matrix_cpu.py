"""
CPU guard of the planner parity matrix (tests/planner_matrix.py): every planner override of jj_ctx_set_option has a row, both ends
of its range are run (or UNCOVERED_ENDS says why not), and the header lists every key.  A new option cannot ship without a row.
"""
import os
import re

import planner_matrix as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jubjub_amd", "csrc")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _constants():
    """integer constexpr / #define values of the library's sources (MSM_WINDOWS_MAX, MSM_SMALL_BLK_MAX, ...)"""
    out = {}
    for name in sorted(os.listdir(CSRC)):
        text = _read("jubjub_amd", "csrc", name)
        for m in re.finditer(r"constexpr\s+(?:int|u32|size_t|unsigned)\s+([^;]+);", text):
            for decl in m.group(1).split(","):
                k, _, v = decl.partition("=")
                if re.fullmatch(r"\s*[\d\s<()u+*-]+\s*", v or "x"):
                    out[k.strip()] = v.strip()
        for m in re.finditer(r"^#define\s+(\w+)\s+([\d\s<()u+*-]+)$", text, re.M):
            out[m.group(1)] = m.group(2).strip()
    return out


def _eval(expr, consts):
    expr = expr.strip()
    for _ in range(4):
        expr = re.sub(r"[A-Z_][A-Z0-9_]*", lambda m: "(%s)" % consts[m.group(0)], expr)
    assert re.fullmatch(r"[\d\s<()+*-]+", expr), expr
    return int(eval(expr))


def planner_options():
    """{key: (lo, hi)} of the planner-override section of ctx_options() in jj_pipeline.hip"""
    src = _read("jubjub_amd", "csrc", "jj_pipeline.hip")
    start = src.index("static const CtxOption* ctx_options()")
    body = src[start:src.index("{nullptr", start)]
    section = body[body.index("// planner overrides"):]
    consts = _constants()
    opts = {}
    for m in re.finditer(r'JJ_OPT\("(\w+)",\s*([^,]+),\s*([^,]+),', section):
        opts[m.group(1)] = (_eval(m.group(2), consts), _eval(m.group(3), consts))
    assert len(opts) >= 18, sorted(opts)
    return opts


def header_planner_keys():
    """the keys of the 'Planner overrides' sentence of include/jubjub_hip.h"""
    h = _read("include", "jubjub_hip.h")
    m = re.search(r"Planner overrides[^:]*:(.*?)\(ranges:", h, re.S)
    assert m, "the header has lost its list of planner overrides"
    return set(re.findall(r"\b[a-z][a-z0-9]*(?:_[a-z0-9]+)+\b", m.group(1)))


# The rows the matrix must keep, by the paths they select (a row may carry more options than these; rows may be added, none dropped).
P0 = {"msm_small_max": 0}
REQUIRED = (
    [dict(msm_front1=0, msm_windows=20, msm_sort_two_pass=0, **P0)]
    + [dict(msm_front1=0, msm_windows=w, **P0) for w in (23, 28, 36)]
    + [dict(msm_front1=0, msm_accum=1, **P0), dict(msm_front1=1, msm_windows=20, msm_sort_two_pass=0, **P0)]
    + [dict(msm_sort_blocks_per_cu=b, msm_windows=20, msm_sort_two_pass=0, msm_accum=0, **P0) for b in (1, 3, 4)]
    + [dict(msm_sort_blocks_per_cu=b, msm_windows=23, msm_accum=0, **P0) for b in (1, 3, 4)]
    + [dict(msm_chunk=c, msm_acc_lds=lds, msm_accum=0, **P0) for c in (8, 13, 1000, 1024) for lds in (0, 1)]
    + [dict(msm_chunk_waves=cw, msm_accum=0, **P0) for cw in (1, 8)]
    + [dict(msm_windows=w, msm_reduce_l1=0, msm_reduce_chunk=L, **P0) for w in (16, 23) for L in (2, 4, 256)]
    + [dict(msm_windows=36, msm_reduce_l1=0, msm_reduce_chunk=256, **P0)]
    + [dict(msm_windows=16, msm_reduce_l1=64, **P0), dict(msm_windows=16, msm_reduce_l1=2, msm_reduce_l2_chunk=64, **P0),
       dict(msm_windows=16, msm_reduce_l1=8, msm_reduce_l2_chunk=2, **P0)]
    + [dict(msm_small_blk=b, msm_small_max=65536) for b in (1, 2)] + [dict(msm_small_blk=64, msm_small_max=1 << 20)]
    + [dict(msm_accum=1, msm_seg_len=p, **P0) for p in (8, 33, 1024)]
    + [dict(msm_windows=w, **P0) for w in (33, 36)]
    + [dict(msm_windows=20, msm_sort_two_pass=1, **P0)] + [dict(msm_windows=18, msm_sort_hist_fused=f, **P0) for f in (0, 1)]
    + [dict(msm_windows=0, msm_accum=-1, msm_seg_len=0, msm_chunk=0, msm_reduce_chunk=0, msm_reduce_l1=-1, msm_reduce_l2_chunk=0, msm_sort_two_pass=-1)]
    + [dict(vb_ct_window=2, vb_quad_max=0), dict(vb_ct_window=3, vb_quad_max=1 << 20), dict(dec_c_mid=8), dict(dec_c_mid=16)]
)


def test_required_rows_are_present():
    """one row per required entry (matched in order of the rows: a row serves one entry), and no row that serves none"""
    free = list(range(len(M.ROWS)))
    for req in REQUIRED:
        k = next((k for k in free if all(M.ROWS[k][0].get(key, None) == v for key, v in req.items())), None)
        assert k is not None, "tests/planner_matrix.py has no row for %s" % (req,)
        free.remove(k)
    assert not free, "rows that no required entry names (add them to REQUIRED): %s" % [M.row_id(k) for k in free]


def test_every_planner_key_has_a_row():
    keys = set(planner_options())
    covered = {k for opts, _ in M.ROWS for k in opts}
    assert not keys - covered, "planner overrides without a parity row in tests/planner_matrix.py: %s" % sorted(keys - covered)
    unknown = covered - keys
    assert not unknown, "rows name keys that are not planner overrides: %s" % sorted(unknown)


def test_header_lists_every_planner_key():
    missing = set(planner_options()) - header_planner_keys()
    assert not missing, "include/jubjub_hip.h does not list these planner overrides: %s" % sorted(missing)


def test_both_ends_of_every_range_are_run():
    values = {}
    for opts, _ in M.ROWS:
        for k, v in opts.items():
            values.setdefault(k, set()).add(v)
    for key, (lo, hi) in planner_options().items():
        for end, v in (("lo", lo), ("hi", hi)):
            if v in values.get(key, ()):
                continue
            reason = M.UNCOVERED_ENDS.get((key, end), "")
            assert reason.strip(), "%s = %d (%s end of %d .. %d) is in no row and UNCOVERED_ENDS gives no reason" % (key, v, end, lo, hi)


def test_rows_are_in_range_and_explained():
    opts = planner_options()
    for k, (row, reason) in enumerate(M.ROWS):
        assert row and reason.strip(), k
        for key, v in row.items():
            lo, hi = opts[key]
            assert lo <= v <= hi, (M.row_id(k), key, v)
            assert (key, v) not in M.REJECTED, (M.row_id(k), key, v)
    ids = [M.row_id(k) for k in range(len(M.ROWS))]
    assert len(set(ids)) == len(ids)
    for key, v in M.REJECTED:
        lo, hi = opts[key]
        assert lo <= v <= hi, (key, v)          # refused by the checks of ctx_option_apply, not by the table's range
