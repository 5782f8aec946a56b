#!/usr/bin/env python3
"""A/B of the windowed Pedersen hash (jj_pedersen_hash_vartime) against the routes without the fused kernel, on the GPU box:
    python tools/pedersen_ab.py --parent-lib PATH [--log2n 10 16 20] [--rounds 3]
    python tools/pedersen_ab.py --worker trace      (nothing is timed: one call of every route at the largest size after a warm-up, for rocprofv3 --kernel-trace)
    python tools/pedersen_ab.py --read-trace DIR    (the library's dispatches of that trace, in order)

A process loads ONE library (JJ_LIB_PATH is read when jubjub_amd is imported), so this driver opens no GPU itself: it starts one worker process
per route and round, one at a time, each under a time limit, and stops at the first worker that does not end well.  Rounds ALTERNATE:
  a   what a user had before, on a build of the PARENT commit: the rows copied from the device, the segment sums <M_j> mod r encoded on the
      host in numpy (vectorised: unpackbits, nibbles, one multi-limb subtraction; the time is counted), jj_fixedbase_multi_mul over 16-bit
      gathered tables, the points copied to the host and their u-coordinates taken there
  b   this commit's composed device route: jj_pedersen_scalars + jj_fixedbase_multi_mul, over 16-bit gathered tables and over the default
      LDS tables; rows and result stay on the device
  c   jj_pedersen_hash_vartime at window_chunks 2, 3 and 4 (u-coordinates; rows and result on the device)
Shapes: the Merkle shape (three segments of 63, fields (0, 255), (32, 255) of rows of 64 bytes, a 6-bit prefix) and the one-field shape of a note
commitment's hash (576 bits of rows of 72 bytes behind the prefix 0b111111: four segments).  Also a 2^20-leaf Engine.pedersen_merkle end to
end.  Every worker warms every shape up, holds one unit of every shape to the restatement of tests/pedersen_cases.py and reports host-clock
seconds per call over a window of --seconds of work per shape (one pass where a pass is longer).  Median [min .. max] of the rounds.
The output is profiles/pedersen_ab.txt."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
SHAPES = {"merkle": dict(nseg=3, stride=64, fields=((0, 255), (32, 255)), prefix=0b000101, prefix_bits=6),
          "note": dict(nseg=4, stride=72, fields=((0, 576),), prefix=0b111111, prefix_bits=6)}
SEG_CHUNKS = 63
WINDOWS = (2, 3, 4)
R_MOD = 0x0E7DB4EA6533AFA906673B0101343B00A6682093CCC81082D0970E5ED6F72CB7


def numpy_scalars(rows, shape):
    """the host encoding of route a: (n, stride) uint8 rows -> (nseg, n, 32) canonical bytes of <M_j> mod r, 2^16 rows at a time"""
    import numpy as np

    return np.concatenate([_numpy_scalars_block(rows[lo:lo + (1 << 16)], shape) for lo in range(0, rows.shape[0], 1 << 16)], axis=1)


def _numpy_scalars_block(rows, shape):
    import numpy as np

    n, nseg = rows.shape[0], shape["nseg"]
    parts = [np.tile(np.array([(shape["prefix"] >> k) & 1 for k in range(shape["prefix_bits"])], np.uint8), (n, 1))]
    for off, nb in shape["fields"]:
        parts.append(np.unpackbits(rows[:, off:off + (nb + 7) // 8], axis=1, bitorder="little")[:, :nb])
    bits = np.concatenate(parts, axis=1)
    cap = 3 * SEG_CHUNKS * nseg
    present = np.zeros(cap // 3, np.uint8)
    present[:(bits.shape[1] + 2) // 3] = 1                              # a chunk that is not there contributes nothing
    bits = np.concatenate([bits, np.zeros((n, cap - bits.shape[1]), np.uint8)], axis=1).reshape(n, nseg, SEG_CHUNKS, 3)
    mag = (1 + bits[..., 0] + 2 * bits[..., 1]) * present.reshape(1, nseg, SEG_CHUNKS)
    limbs = []
    for sel in (bits[..., 2] == 0, bits[..., 2] == 1):
        nib = np.concatenate([np.where(sel, mag, 0).astype(np.uint8), np.zeros((n, nseg, 1), np.uint8)], axis=2)      # 64 nibbles
        limbs.append(np.ascontiguousarray(nib[..., 0::2] | (nib[..., 1::2] << 4)).view("<u4").astype(np.int64))     # (n, nseg, 8)
    P, N = limbs
    d, borrow = np.zeros_like(P), np.zeros(P.shape[:2], np.int64)
    for k in range(8):
        t = P[..., k] - N[..., k] - borrow
        borrow = (t < 0).astype(np.int64)
        d[..., k] = t + (borrow << 32)
    carry = np.zeros_like(borrow)
    for k in range(8):                                                   # P < N: add r
        t = d[..., k] + borrow * ((R_MOD >> (32 * k)) & 0xFFFFFFFF) + carry
        carry = t >> 32
        d[..., k] = t & 0xFFFFFFFF
    return np.ascontiguousarray(d.astype("<u4").view(np.uint8).reshape(n, nseg, 32).transpose(1, 0, 2))


def generators(nseg):
    import numpy as np

    from tests import pedersen_cases as PC

    pts = PC.synth_generators(nseg)
    return pts, np.stack([PC.point_bytes(p) for p in pts])


# ---- worker: one library, one route, every shape once ---------------------------------------------------------------------------------------
def worker(args):
    import numpy as np
    import torch

    from jubjub_amd import Engine, _lib
    from tests import pedersen_cases as PC

    route = args.worker
    if route == "a":
        for name in [k for k in _lib._SIGS if k.startswith("jj_pedersen")]:
            if name.encode() not in open(_lib.LIB_PATH, "rb").read():
                _lib._SIGS.pop(name)                                     # the parent's build: the binding must not ask for the symbols
    eng = Engine(0)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0x9ED5)

    def timed(fn, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / k

    def window(fn):
        per = timed(fn, 1)
        if per > 2.0:                                             # seconds of host work per pass (route a at 2^20): that pass is the figure
            return per
        if per > args.seconds:
            return timed(fn, 1)
        timed(fn, 2)
        return timed(fn, max(2, min(4096, int(args.seconds / per) + 1)))

    def check(name, shape, pts, rows, got, unit):
        want = PC.expected(tuple(pts), SEG_CHUNKS, _bits(rows[unit].cpu().numpy(), shape))
        assert bytes(np.asarray(got[unit].cpu() if hasattr(got, "cpu") else got[unit])[:32]) == want[0].to_bytes(32, "little"), (route, name, unit)

    out, order = {}, []
    for name, shape in SHAPES.items():
        pts, gens = generators(shape["nseg"])
        a16 = [eng.fixedbase_table(g, 16) for g in gens] if route in ("a", "b", "trace") else []
        lds = [eng.fixedbase_table(g, 0) for g in gens] if route in ("b", "trace") else []
        ped = {w: eng.pedersen_table(gens, SEG_CHUNKS, w) for w in WINDOWS} if route in ("c", "trace", "merkle") else {}
        largest = None
        for lg in ([max(args.log2n)] if route == "trace" else args.log2n):
            n = 1 << lg
            rows = torch.randint(0, 256, (n, shape["stride"]), dtype=torch.uint8, device=dev, generator=gen)
            lay = (rows, shape["fields"], shape["prefix"], shape["prefix_bits"])

            def route_a():
                s = numpy_scalars(rows.cpu().numpy(), shape)
                return eng.fixedbase_multi_mul(a16, torch.from_numpy(s.reshape(-1, 32)).to(dev)).cpu().numpy()[:, :32]

            def route_b(tabs):
                return eng.fixedbase_multi_mul(tabs, eng.pedersen_scalars(shape["nseg"], SEG_CHUNKS, *lay).reshape(-1, 32))

            unit = int(np.random.default_rng(lg).integers(0, n))
            if route == "a":
                out["%s %d a: numpy scalars + multi_mul (16-bit tables) + u on the host" % (name, lg)] = window(route_a)
                s = numpy_scalars(rows[unit:unit + 1].cpu().numpy(), shape)
                assert [int.from_bytes(bytes(s[j, 0]), "little") for j in range(shape["nseg"])] == [v % R_MOD for v in PC.segment_sums(SEG_CHUNKS, shape["nseg"], _bits(rows[unit].cpu().numpy(), shape))]
                if lg <= 16:                                           # (a pass at 2^20 is seconds of host work: the smaller sizes hold the route to the restatement)
                    check(name, shape, pts, rows, route_a(), unit)
            elif route == "b":
                out["%s %d b: pedersen_scalars + multi_mul (16-bit tables)" % (name, lg)] = window(lambda: route_b(a16))
                out["%s %d b: pedersen_scalars + multi_mul (default LDS tables)" % (name, lg)] = window(lambda: route_b(lds))
                check(name, shape, pts, rows, route_b(a16), unit)
                check(name, shape, pts, rows, route_b(lds), unit)
            elif route == "c":
                res = torch.empty((n, 32), dtype=torch.uint8, device=dev)
                for w in WINDOWS:
                    out["%s %d c: pedersen_hash, window_chunks %d" % (name, lg, w)] = window(lambda: eng.pedersen_hash(ped[w], *lay, out=res))
                    check(name, shape, pts, rows, res, unit)
                largest = (n, lay)
            elif route == "trace":
                for label, fn in [("b16", lambda: route_b(a16)), ("blds", lambda: route_b(lds))] + [("c%d" % w, lambda w=w: eng.pedersen_hash(ped[w], *lay)) for w in WINDOWS]:
                    for _ in range(2):
                        fn()
                        torch.cuda.synchronize()
                    order.append("%s 2^%d %s (twice)" % (name, lg, label))
        if route == "c" and largest is not None:                           # the routes give the same bytes at the largest size
            n, lay = largest
            pt = eng.pedersen_hash(ped[4], *lay, point=True)
            for w in (2, 3):
                assert torch.equal(pt, eng.pedersen_hash(ped[w], *lay, point=True)), (name, w)
        if route == "merkle" and name == "merkle":
            lg = max(args.log2n)
            leaves = torch.randint(0, 256, (1 << lg, 32), dtype=torch.uint8, device=dev, generator=gen)
            out["merkle %d tree: pedersen_merkle end to end (%d layers)" % (lg, lg)] = window(lambda: eng.pedersen_merkle(ped[args.default_window], leaves))
            out["merkle %d tree: table bytes" % lg] = {w: 128 * _entries(3, w) for w in WINDOWS}
        for t in a16 + lds + list(ped.values()):
            t.close()
    eng.close()
    print(("TRACED " if route == "trace" else "RESULT ") + json.dumps(order if route == "trace" else out))


def _bits(row, shape):
    out = [(shape["prefix"] >> k) & 1 for k in range(shape["prefix_bits"])]
    for off, nb in shape["fields"]:
        out += [(int(row[off + (k >> 3)]) >> (k & 7)) & 1 for k in range(nb)]
    return out


def _entries(nseg, w):
    sub = lambda T: sum(1 << (3 * t - 1) for t in range(1, T + 1))      # noqa: E731
    nw = -(-SEG_CHUNKS // w)
    return nseg * ((nw - 1) * sub(w) + sub(SEG_CHUNKS - (nw - 1) * w))


# ---- driver: no GPU in this process ---------------------------------------------------------------------------------------------------------
def run_worker(route, lib, args, limit=560):
    env = dict(os.environ)
    env.pop("JJ_LIB_PATH", None)
    if lib:
        env["JJ_LIB_PATH"] = os.path.abspath(lib)
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--worker", route, "--seconds", str(args.seconds), "--default-window", str(args.default_window),
           "--log2n"] + [str(x) for x in args.log2n]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True)
    if p.returncode:
        sys.stdout.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit("worker %s ended with %d; nothing more is started on the GPU" % (route, p.returncode))
    line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")]
    return json.loads(line[-1][7:]) if line else {}


def read_trace(dirname):
    import csv
    import glob

    rows = []
    for path in sorted(glob.glob(os.path.join(dirname, "**", "*kernel_trace.csv"), recursive=True)):
        for r in csv.DictReader(open(path)):
            if "jj::" in r["Kernel_Name"] or "_ZN2jj" in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), r["Kernel_Name"].split("(")[0][:60], int(r["Grid_Size_X"] if "Grid_Size_X" in r else r["Grid_Size"])))
    rows.sort()
    rows = [r for r in rows if any(k in r[2] for k in ("k_pedersen", "k_fixedbase", "k_affine_u")) or ("k_normalize" in r[2] and r[3] >= 1 << 16)]
    print("# the hashing dispatches of --worker trace in order (the table builders' ladders and small launches left out): microseconds, kernel, grid")
    for k, (_, dur, name, grid) in enumerate(rows):
        print("%4d  %10.2f us  %-60s grid %d" % (k, dur / 1e3, name, grid))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="*", default=[10, 16, 20])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=0.2, help="work per timed window, at least")
    ap.add_argument("--default-window", type=int, default=4, help="window_chunks of the pedersen_merkle run")
    ap.add_argument("--parent-lib", default="", help="libjubjub_hip.so built from the parent commit: route a runs on it")
    ap.add_argument("--worker", default="")
    ap.add_argument("--read-trace", default="", metavar="DIR")
    args = ap.parse_args()
    if args.read_trace:
        return read_trace(args.read_trace)
    if args.worker:
        return worker(args)
    assert args.parent_lib and os.path.exists(args.parent_lib), "--parent-lib: route a must run on a build of the parent commit"
    res, sizes = {}, {}
    for _ in range(args.rounds):
        for route, lib in (("c", ""), ("b", ""), ("a", args.parent_lib), ("merkle", "")):
            for k, v in run_worker(route, lib, args).items():
                if isinstance(v, dict):
                    sizes = v
                else:
                    res.setdefault(k, []).append(v)
    res = {k: sorted(v) for k, v in res.items()}
    med = lambda v: v[len(v) // 2]      # noqa: E731
    print("# windowed Pedersen hashes: %d alternating rounds of one process per route; median [min .. max] of the rounds, ms per call; rows and results on the device" % args.rounds)
    print("# a: the PARENT commit's library, scalars encoded on the host in numpy; b: jj_pedersen_scalars + jj_fixedbase_multi_mul; c: jj_pedersen_hash_vartime")
    for name in SHAPES:
        for lg in args.log2n:
            print("%s shape, n = 2^%d" % (name, lg))
            for k in sorted(res):
                if k.startswith("%s %d " % (name, lg)) and "tree" not in k:
                    v = res[k]
                    print("  %-72s %12.4f ms  [%.4f .. %.4f]   %8.2f M hashes/s" % (k.split(" ", 2)[2], med(v) * 1e3, v[0] * 1e3, v[-1] * 1e3, (1 << lg) / med(v) / 1e6))
    for k in sorted(res):
        if "tree" in k:
            v = res[k]
            print("%s   %12.4f ms  [%.4f .. %.4f]" % (k, med(v) * 1e3, v[0] * 1e3, v[-1] * 1e3))
    print("table bytes of the Merkle shape by window_chunks: %s (three 16-bit gathered tables: %d)" % (json.dumps(sizes), 3 * 16 * 32769 * 128))


if __name__ == "__main__":
    main()
