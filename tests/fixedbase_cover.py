"""
Plain models of the three fixed-base recodings (jubjub_amd/csrc/jj_kernels.h) and scalar sets that, taken together, make every kernel
read every table entry it can ever read.  Test infrastructure only: Python integers, no GPU, no import of the native library.

  gather  k_fixedbase_gather, window_bits w = 8..16: k' = (k mod 2^252) + sum_{i<W-1} 2^(w i + w - 1), W = ceil(253 / w); window i < W - 1
          gives the signed digit d_i = window_i - E (E = 2^(w-1)), the top window an unsigned digit.  Entry (i, |d_i|, sign).
  lds6    k_fixedbase, window_bits 6: k' = (k mod 2^252) + sum_{i<42} 32 * 64^i; 42 signed digits in [-32, 31] and the carry d_42 at
          bit 252.  Entry (i, |d_i|, sign), the carry as (42, d_42, +).
  comb    k_fixedbase_comb, window_bits 7: kk = (k mod 2^252) | 1 written with signs +-1; column j (0..31) gives (table j >> 2, index,
          sign); an even k takes the entry of column 0 from T_0 - B (table 8, sign +) or T_0 + B (table 9, sign -).
          Entry (j, table, index, sign).

The reachable entries are computed from the constraints alone (k < 2^252; the top 4 bits of a 32-byte scalar are ignored), window by
window; cover_scalars(kind, w) is built constructively (raw windows or comb column bytes first, then k) and tests/test_fixedbase_cover_cpu.py
checks that it hits every reachable entry.  tests/test_gpu_fixedbase_matrix.py runs the sets on the GPU against the oracle.

    python -c "import tests.fixedbase_cover as c; print(c.coverage_report())"
"""
import functools
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jubjub_amd", "csrc")
SCALAR_BITS = 252                 # the kernels keep k mod 2^252 (k[7] &= 0x0fffffff)
GATHER_WIDTHS = tuple(range(8, 17))
ACCEPTED_WINDOW_BITS = (0, 6, 7) + GATHER_WIDTHS
REFUSED_WINDOW_BITS = (-1, 1, 2, 3, 4, 5, 17)


def _read(*parts):
    with open(os.path.join(CSRC, *parts)) as f:
        return f.read()


def kernel_constants():
    """FB_*, FBC_*, FBX_MAX_BASES and the thread counts of jj_kernels.h, and the gathered kernel's blocks per CU (jj_engine.h)."""
    text = _read("jj_kernels.h")
    out = {d.group(1): int(d.group(2)) for d in re.finditer(r"^#define\s+(JJ_FBC?_THREADS)\s+(\d+)\s*$", text, re.M)}
    for m in re.finditer(r"constexpr\s+int\s+([^;]+);", text):
        for decl in m.group(1).split(","):
            name, _, expr = decl.partition("=")
            name, expr = name.strip(), expr.strip()
            if re.fullmatch(r"\w+", name) and re.fullmatch(r"[\w\s()+*-]+", expr):
                try:
                    out[name] = int(eval(expr, {"__builtins__": {}}, dict(out)))
                except NameError:
                    pass
    m = re.search(r"int\s+fb_gather_blocks_per_cu\s*=\s*(\d+)\s*;", _read("jj_engine.h"))
    out["fb_gather_blocks_per_cu"] = int(m.group(1))
    for key in ("FB_W", "FB_NWIN", "FB_ENT", "FBC_TEETH", "FBC_SPACING", "FBC_BLOCKS", "FBC_COLS", "FBC_TENT", "FBC_TABLES",
                "FBX_MAX_BASES", "JJ_FB_THREADS", "JJ_FBC_THREADS"):
        assert key in out, key
    return out


K = kernel_constants()


def recode6_words():
    """RECODE6 of jj_constants.h as one integer (the 6-bit kernel's recoding constant)"""
    m = re.search(r"RECODE6\[8\]\s*=\s*\{([^}]*)\}", _read("jj_constants.h"))
    words = [int(x.strip().rstrip("uU"), 16) for x in m.group(1).split(",")]
    return sum(w << (32 * i) for i, w in enumerate(words))


def grid_lanes(kind, cus):
    """lanes of one grid round of a kernel kind (fixedbase_launch, fb_lanes in jj_abi.hip): one workgroup per CU for the LDS tables"""
    return cus * {"comb": K["JJ_FBC_THREADS"], "lds6": K["JJ_FB_THREADS"], "gather": K["fb_gather_blocks_per_cu"] * 256}[kind]


# ------------------------------------------------------------------------------------------------ the window recodings
def gather_layout(w):
    """(W, E, recode) of a gathered table of width w (FbParams in jj_kernels.h)"""
    W = -(-253 // w)
    return W, 1 << (w - 1), sum(1 << (w * i + w - 1) for i in range(W - 1))


def lds6_layout():
    """(windows, E, recode, carry bit) of the 6-bit LDS table"""
    w, nwin = K["FB_W"], K["FB_NWIN"]
    return nwin, K["FB_ENT"] - 1, sum((K["FB_ENT"] - 1) << (w * i) for i in range(nwin)), w * nwin


def _windows(kp, w, nlow, E, top_shift):
    out = []
    for i in range(nlow):
        d = ((kp >> (w * i)) & ((1 << w) - 1)) - E
        out.append((i, abs(d), -1 if d < 0 else 1))
    out.append((nlow, kp >> top_shift, 1))
    return out


def gather_digits(k, w):
    """k_fixedbase_gather: [(window, index, sign)] for windows 0 .. W - 1 (the last one unsigned)"""
    W, E, recode = gather_layout(w)
    kp = (k % (1 << SCALAR_BITS)) + recode
    return _windows(kp, w, W - 1, E, w * (W - 1))


def lds6_digits(k):
    """k_fixedbase: [(window, index, sign)] for the 42 signed windows and the carry (window 42)"""
    nwin, E, recode, top = lds6_layout()
    kp = (k % (1 << SCALAR_BITS)) + recode
    return _windows(kp, K["FB_W"], nwin, E, top)


def window_value(entries, w):
    """sum of sign * index * 2^(w * window): the multiple of B the selected entries add up to"""
    return sum(s * j << (w * i) for i, j, s in entries)


def comb_entry_value(table, idx):
    """the multiple of B held by entry idx of comb table `table` (build_comb_table in jj_abi.hip)"""
    t0 = (1 << 224) + sum((1 if (idx >> i) & 1 else -1) << (32 * i) for i in range(K["FBC_TEETH"] - 1))
    if table < K["FBC_BLOCKS"]:
        return t0 << (K["FBC_COLS"] * table)
    return t0 - 1 if table == K["FBC_BLOCKS"] else t0 + 1


def comb_digits(k):
    """k_fixedbase_comb: [(column, table, index, sign)] for the 32 columns"""
    k %= 1 << SCALAR_BITS
    kk = k | 1
    sw = (kk >> 1) | (1 << 255)                    # bit p of sw: s_p = +1
    teeth, spacing = K["FBC_TEETH"], K["FBC_SPACING"]
    out = []
    for j in range(spacing):
        bits = [(sw >> (j + spacing * i)) & 1 for i in range(teeth)]
        top = bits[teeth - 1]
        idx = sum((1 if bits[i] == top else 0) << i for i in range(teeth - 1))
        sign = 1 if top else -1
        table = j // K["FBC_COLS"]
        if j == 0 and k % 2 == 0:
            table = K["FBC_BLOCKS"] if sign > 0 else K["FBC_BLOCKS"] + 1
        out.append((j, table, idx, sign))
    return out


def comb_value(entries):
    return sum(s * comb_entry_value(t, i) << (j % K["FBC_COLS"]) for j, t, i, s in entries)


def entries_of(kind, k, w=None):
    if kind == "gather":
        return gather_digits(k, w)
    if kind == "lds6":
        return lds6_digits(k)
    return comb_digits(k)


# ------------------------------------------------------------------------------------------------ reachable entries
def _window_params(kind, w):
    if kind == "gather":
        W, E, recode = gather_layout(w)
        return w, W - 1, E, recode, w * (W - 1)
    nwin, E, recode, top = lds6_layout()
    return K["FB_W"], nwin, E, recode, top


@functools.lru_cache(maxsize=None)
def reachable(kind, w=None):
    """every entry a scalar below 2^252 can select, window by window, from the constraints alone: k' runs over the interval
    [recode, 2^252 - 1 + recode]; a signed window takes value v iff some k' of the interval has v there; the top window takes
    every value between the top of the interval's ends.  Comb: the bits 251..254 of sw are 0 and bit 255 is 1, every other bit
    and the parity of k are free."""
    out = set()
    if kind == "comb":
        teeth, spacing, blocks = K["FBC_TEETH"], K["FBC_SPACING"], K["FBC_BLOCKS"]
        for j in range(spacing):
            for pattern in range(1 << teeth):
                pos = [j + spacing * i for i in range(teeth)]
                bit = [(pattern >> i) & 1 for i in range(teeth)]
                if any((p == 255 and b != 1) or (SCALAR_BITS - 1 <= p < 255 and b != 0) for p, b in zip(pos, bit)):
                    continue
                top = bit[teeth - 1]
                idx = sum((1 if bit[i] == top else 0) << i for i in range(teeth - 1))
                sign = 1 if top else -1
                for even in (False, True):
                    table = j // K["FBC_COLS"] if not (j == 0 and even) else (blocks if sign > 0 else blocks + 1)
                    out.add((j, table, idx, sign))
        return frozenset(out)
    w, nlow, E, recode, top_shift = _window_params(kind, w)
    lo, hi = recode, (1 << SCALAR_BITS) - 1 + recode
    for i in range(nlow):
        block = 1 << (w * (i + 1))
        for v in range(1 << w):
            x = (lo // block) * block + (v << (w * i))
            if x < lo:
                x += block
            if x <= hi:
                d = v - E
                out.add((i, abs(d), -1 if d < 0 else 1))
    for t in range(lo >> top_shift, (hi >> top_shift) + 1):
        out.add((nlow, t, 1))
    return frozenset(out)


def top_digit_max(kind, w=None):
    return max(j for i, j, s in reachable(kind, w) if i == (_window_params(kind, w)[1]))


# ------------------------------------------------------------------------------------------------ scalar generators
def _window_cover(w, nlow, E, recode, top_shift):
    """2^w scalars whose signed windows run through every value (window i of scalar m holds (m + i * step) mod 2^w), the top
    window cycled through its range where the low windows allow it, then one scalar for each top value still missing"""
    mask = (1 << w) - 1
    step = (0x9E3779B9 & mask) | 1
    top_max = ((1 << SCALAR_BITS) - 1 + recode) >> top_shift
    out, tops = [], set()
    for m in range(1 << w):
        low = sum(((m + i * step) & mask) << (w * i) for i in range(nlow))
        t_min = 0 if low >= recode else 1
        t_hi = ((1 << SCALAR_BITS) - 1 + recode - low) >> top_shift
        t = min(max(m % (top_max + 1), t_min), t_hi)
        out.append((t << top_shift) + low - recode)
        tops.add(t)
    for t in range(top_max + 1):
        if t not in tops:
            out.append(0 if t == 0 else (t << top_shift) - recode)       # t = 0: every digit 0; t > 0: every low digit -E
    assert all(0 <= k < (1 << SCALAR_BITS) for k in out)
    return out


def _comb_cover():
    """512 scalars: column j of scalar m carries the byte (m + 37 j) mod 256 (top bit: the sign, low 7 bits: the entry), odd k for
    m < 256 and even k from 256 on, so that column 0 reads every entry of T_0, T_0 - B and T_0 + B; columns 27..30 are forced to -
    and column 31 to + (bits 251..255 of sw)"""
    teeth, spacing = K["FBC_TEETH"], K["FBC_SPACING"]
    out = []
    for m in range(2 << teeth):
        sw = 0
        for j in range(spacing):
            c = (m + 37 * j) & 0xFF
            if j + spacing * (teeth - 1) == 255:
                c |= 0x80
            elif j + spacing * (teeth - 1) >= SCALAR_BITS - 1:
                c &= 0x7F
            top = c >> 7
            for i in range(teeth):
                b = top if i == teeth - 1 else (top if (c >> i) & 1 else 1 - top)
                sw |= b << (j + spacing * i)
        kk = ((sw & ((1 << 255) - 1)) << 1) | 1
        out.append(kk if m < (1 << teeth) else kk - 1)
    assert all(0 <= k < (1 << SCALAR_BITS) for k in out)
    return out


_COVER = {}


def cover_scalars(kind, w=None):
    """integers below 2^252 that together select every reachable entry of every window (column) of a kernel kind"""
    key = (kind, w if kind == "gather" else None)
    if key not in _COVER:
        _COVER[key] = _comb_cover() if kind == "comb" else _window_cover(*_window_params(kind, w))
    return list(_COVER[key])


def covered(kind, w=None, scalars=None):
    out = set()
    for k in cover_scalars(kind, w) if scalars is None else scalars:
        out.update(entries_of(kind, k, w))
    return out


def kind_of_window_bits(wb, default=7):
    wb = default if wb == 0 else wb
    return ("comb", None) if wb == 7 else ("lds6", None) if wb == K["FB_W"] else ("gather", wb)


def coverage_report():
    lines = ["kind    w   scalars  reachable  covered"]
    for kind, w in [("comb", None), ("lds6", None)] + [("gather", w) for w in GATHER_WIDTHS]:
        r, c = reachable(kind, w), covered(kind, w)
        lines.append("%-6s %3s %9d %10d %8d%s" % (kind, w or "-", len(cover_scalars(kind, w)), len(r), len(c & r),
                                                  "" if r <= c else "   MISSING %d" % len(r - c)))
    return "\n".join(lines)


# ------------------------------------------------------------------------------------------------ composite tables
def composite_slots(bits):
    """window offsets of jj_fixedbase_composite_create, or None where it refuses the partition"""
    if not 1 <= len(bits) <= K["FBX_MAX_BASES"] or any(not 1 <= b <= 250 for b in bits):
        return None
    off, slots = [], 0
    for b in bits:
        off.append(slots)
        slots += -(-(b + 2) // K["FB_W"])
    return off if slots <= K["FB_NWIN"] else None


def pack_composite(values, bits):
    """k_pack_composite: field b holds (value mod 2^bits_b) at bit 6 * off_b"""
    off = composite_slots(bits)
    return sum((v % (1 << b)) << (K["FB_W"] * o) for v, b, o in zip(values, bits, off))


def composite_field_values(bits):
    """field values that put digit -32, digit 31 and 0 into every window of the field, and its top bit (all below 2^bits)"""
    w, E = K["FB_W"], K["FB_ENT"] - 1
    W = -(-(bits + 2) // w)
    vals = {0, 1, (1 << bits) - 1, 1 << (bits - 1), (1 << (bits - 1)) - 1}
    scale = 1 << (w * (W - 1))
    for pattern in ((-E, -E), (E - 1, E - 1), (0, 0), (-E, E - 1), (E - 1, -E)):
        low = sum(pattern[i % 2] << (w * i) for i in range(W - 1))
        t_lo, t_hi = -(low // scale), ((1 << bits) - 1 - low) // scale
        for t in (t_lo, t_hi):
            if t_lo <= t_hi and -E <= t < E:
                vals.add(low + t * scale)
    return sorted(v for v in vals if 0 <= v < (1 << bits))


def composite_cases():
    """[(bits, accepted, why)]: partitions at the slot and base limits, bits + 2 = 0 (mod 6) next to bits + 2 != 0, and refusals"""
    nmax, nwin = K["FBX_MAX_BASES"], K["FB_NWIN"]
    return [
        ([250], True, "one base, the widest field: 42 slots"),
        ([10] * nmax, True, "the base limit at two slots each: 42 slots"),
        ([1] * nmax, True, "the base limit at one slot each"),
        ([4, 5, 10, 11, 16, 17, 22, 23], True, "bits + 2 = 0 (mod 6) next to bits + 2 = 1 (mod 6)"),
        ([34, 33, 40, 39, 46, 45], True, "bits + 2 = 0 (mod 6) next to bits + 2 = 5 (mod 6)"),
        ([244, 4], True, "41 + 1 slots"),
        ([1] * (nmax + 1), False, "one base more than FBX_MAX_BASES"),
        ([250, 1], False, "43 slots"),
        ([64] * 4, False, "44 slots"),
        ([0], False, "scalar_bits 0"),
        ([251], False, "scalar_bits 251"),
        ([10, 0, 10], False, "scalar_bits 0 between valid fields"),
    ] + [([6 * nwin - 2 - 6 * (nmax - 2)] + [4] * (nmax - 2), True, "a wide field and 19 one-slot fields: 42 slots")]
