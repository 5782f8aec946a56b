#!/usr/bin/env python3
"""A/B of the key agreement with its KDF on the device (jj_ka_kdf, jj_chacha20_xor) against what a caller had before, on the GPU box:
    python tools/ka_kdf_ab.py --parent-lib PATH [--log2n 10 16 20] [--rounds 3]
    python tools/ka_kdf_ab.py --worker trace      (nothing is timed: one jj_ka_kdf and one ka_open call at the largest size after a warm-up, for rocprofv3 --kernel-trace)
    python tools/ka_kdf_ab.py --read-trace DIR    (the library's dispatches of that trace, in order)

A process loads ONE library (JJ_LIB_PATH is read when jubjub_amd is imported), so this driver opens no GPU itself: it starts one worker process
per route and round, one at a time, each under a time limit, and stops at the first worker that does not end well.  Rounds ALTERNATE:
  new     this commit: jj_ka_kdf alone, and Engine.ka_open at len 52 (KDF, then one ChaCha20 block per row); inputs and results on the device
  parent  a build of the PARENT commit: the four-call composed device route -- jj_decompress, jj_varbase_mul with the scalar written n times
          (the array is made once, outside the timing), jj_point_mul_by_cofactor, jj_compress -- WITHOUT any hash: it cannot make the keys
  hash    the same route with the shares copied to the host and hashed by hashlib.blake2b(digest_size=32) in one thread and in 16 processes,
          the keys copied back; at 2^10 also the cipher in the Python of tests/ka_cases.py
The Sapling recipient's shape: ZIP 216 decoding, cofactor, the encoding hashed with the share.  Prime-order points made on the device.  Every
worker warms up, holds 64 units to the restatement of tests/ka_cases.py and reports host-clock seconds per call over a window of --seconds of
work (one pass where a pass is longer).  Median [min .. max] of the rounds.  The output is profiles/ka_kdf_ab.txt."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
PERSONAL = b"Zcash_SaplingKDF"
FLAGS = 1 | 32 | 64
LEN = 52


def _hash_block(args):
    shares, encs = args
    return b"".join(hashlib.blake2b(shares[i:i + 32] + encs[i:i + 32], digest_size=32, person=PERSONAL).digest() for i in range(0, len(shares), 32))


def worker(args):
    import numpy as np
    import torch

    from jubjub_amd import Engine, _lib
    from tests import ka_cases as KC

    route = args.worker
    blob = open(_lib.LIB_PATH, "rb").read()
    for name in ("jj_ka_kdf", "jj_chacha20_xor"):
        if name.encode() not in blob:
            assert route in ("parent", "hash"), "the library under test lacks %s" % name
            _lib._SIGS.pop(name)                                         # the parent's build: the binding must not ask for the symbols
    pool = None
    if route == "hash":
        import multiprocessing

        pool = multiprocessing.get_context("fork").Pool(16)              # forked BEFORE this process opens the GPU: the children never have it open
    eng = Engine(0)
    sk = KC.SCALARS[-1]

    def timed(fn, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / k

    def window(fn):
        per = timed(fn, 1)
        if per > args.seconds:
            return per if per > 2.0 else timed(fn, 1)
        timed(fn, 2)
        return timed(fn, max(2, min(4096, int(args.seconds / per) + 1)))

    out = {}
    for log2n in args.log2n:
        n = 1 << log2n
        pts = eng.random_points(n, 0xCAFE, 0, subgroup=True, device="cuda")
        encs = eng.compress(pts)
        ct = torch.randint(0, 256, (n, LEN), dtype=torch.uint8, device="cuda")
        scal = torch.from_numpy(np.frombuffer(sk, dtype=np.uint8).copy()).cuda().reshape(1, 32).repeat(n, 1).contiguous()
        want_keys, want_ok = KC.expected(sk, encs[:64].cpu().numpy(), FLAGS, PERSONAL)

        def composed():
            p, ok = eng.decompress(encs, 1)
            return eng.compress(eng.mul_by_cofactor(eng.varbase_mul(scal, p))), ok

        def hashed(procs):
            share, ok = composed()
            s, e = share.cpu().numpy().tobytes(), encs.cpu().numpy().tobytes()
            if procs == 1:
                keys = _hash_block((s, e))
            else:
                step = -(-n // procs) * 32
                keys = b"".join(pool.map(_hash_block, [(s[o:o + step], e[o:o + step]) for o in range(0, len(s), step)]))
            return torch.from_numpy(np.frombuffer(keys, dtype=np.uint8).reshape(n, 32).copy()).cuda(), ok

        if route in ("new", "trace"):
            keys, ok = eng.ka_kdf(sk, encs, PERSONAL, FLAGS)
            assert np.array_equal(keys[:64].cpu().numpy(), want_keys) and bool(ok.all())
            plain, _ = eng.ka_open(sk, encs, ct, PERSONAL, FLAGS, counter=1)
            assert np.array_equal(plain[:64].cpu().numpy(), KC.chacha20_xor(want_keys, ct[:64].cpu().numpy(), LEN, None, 1))
            if route == "trace":
                if log2n == max(args.log2n):
                    torch.cuda.synchronize()
                    eng.ka_kdf(sk, encs, PERSONAL, FLAGS)
                    eng.ka_open(sk, encs, ct, PERSONAL, FLAGS, counter=1)
                    torch.cuda.synchronize()
                continue
            out["ka_kdf %d" % log2n] = window(lambda: eng.ka_kdf(sk, encs, PERSONAL, FLAGS))
            out["ka_open %d" % log2n] = window(lambda: eng.ka_open(sk, encs, ct, PERSONAL, FLAGS, counter=1))
        elif route == "parent":
            share, ok = composed()
            got = _hash_block((share[:64].cpu().numpy().tobytes(), encs[:64].cpu().numpy().tobytes()))
            assert got == want_keys.tobytes() and bool(ok.all())
            out["composed, no hash %d" % log2n] = window(composed)
        else:
            keys, _ = hashed(16)
            assert np.array_equal(keys[:64].cpu().numpy(), want_keys)
            out["composed + hashlib x1 %d" % log2n] = window(lambda: hashed(1))
            out["composed + hashlib x16 %d" % log2n] = window(lambda: hashed(16))
            if log2n == 10:
                k, c = keys.cpu().numpy(), ct.cpu().numpy()
                t0 = time.perf_counter()
                KC.chacha20_xor(k, c, LEN, None, 1)
                out["cipher in Python %d" % log2n] = time.perf_counter() - t0
    if pool is not None:
        pool.close()
    eng.close()
    print("RESULT " + json.dumps(out), flush=True)


def read_trace(dirname):
    import glob
    import sqlite3

    for path in sorted(glob.glob(os.path.join(dirname, "**", "*.db"), recursive=True)):
        db = sqlite3.connect(path)
        tables = [r[0] for r in db.execute("select name from sqlite_master where type in ('table', 'view')")]
        if "kernels" not in tables:
            continue
        cols = [r[1] for r in db.execute("pragma table_info(kernels)")]
        rows = db.execute("select name, grid_x, workgroup_x, duration from kernels" + (" order by start" if "start" in cols else "")).fetchall()
        rows = [r for r in rows if "jj" in r[0]]
        tail = rows[-24:]                                                # the last two calls: one jj_ka_kdf, one ka_open
        print("# %s: %d dispatches of the library; the last %d (the two calls behind the warm-up):" % (os.path.basename(path), len(rows), len(tail)))
        for name, g, w, ns in tail:
            print("  %-64s grid %9d x %3d  %9.3f ms" % (name.split("(")[0][-64:], g, w, ns / 1e6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--worker", choices=["new", "parent", "hash", "trace"])
    ap.add_argument("--read-trace")
    ap.add_argument("--log2n", type=int, nargs="+", default=[10, 16, 20])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--limit", type=int, default=240, help="seconds allowed to one worker")
    args = ap.parse_args()
    if args.read_trace:
        return read_trace(args.read_trace)
    if args.worker:
        return worker(args)
    assert args.parent_lib and os.path.exists(args.parent_lib), "--parent-lib: a build of the parent commit"
    results = {}
    for rnd in range(args.rounds):
        order = ("new", "parent", "hash") if rnd % 2 == 0 else ("hash", "parent", "new")
        for route in order:
            env = dict(os.environ)
            if route != "new":
                env["JJ_LIB_PATH"] = os.path.abspath(args.parent_lib)
            else:
                env.pop("JJ_LIB_PATH", None)
            cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--worker", route, "--seconds", str(args.seconds), "--log2n"] + [str(x) for x in args.log2n]
            res = subprocess.run(cmd, env=env, capture_output=True, text=True, cwd=ROOT)
            line = [l for l in res.stdout.splitlines() if l.startswith("RESULT ")]
            if res.returncode != 0 or not line:
                print("STOP: worker %s of round %d ended with %d; nothing more is started\n%s" % (route, rnd, res.returncode, res.stderr[-2000:]))
                return 3
            for k, v in json.loads(line[0][7:]).items():
                results.setdefault(k, []).append(v)
            print("# round %d, %s: done" % (rnd, route), flush=True)
    print("# jj_ka_kdf / ka_open against the composed route on the parent's build; Sapling recipient's shape; seconds of host clock per call, device-resident data")
    print("# %d alternating rounds of one process per route; median [min .. max]" % args.rounds)
    print("%-34s %8s %12s %24s %14s" % ("route", "log2 n", "ms per call", "[min .. max]", "M units / s"))
    for key in sorted(results, key=lambda k: (int(k.rsplit(" ", 1)[1]), k)):
        v = sorted(results[key])
        name, log2n = key.rsplit(" ", 1)
        med = v[len(v) // 2]
        print("%-34s %8s %12.3f %24s %14.2f" % (name, log2n, med * 1e3, "[%.3f .. %.3f]" % (v[0] * 1e3, v[-1] * 1e3), (1 << int(log2n)) / med / 1e6))
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
