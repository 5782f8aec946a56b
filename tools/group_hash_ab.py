#!/usr/bin/env python3
"""A/B of the hash to the curve on the device (jj_group_hash) against what a caller had before, on the GPU box:
    python tools/group_hash_ab.py --parent-lib PATH [--log2n 10 16 20] [--rounds 3]
    python tools/group_hash_ab.py --worker trace      (nothing is timed: one jj_group_hash call at the largest size after a warm-up, for rocprofv3 --kernel-trace)
    python tools/group_hash_ab.py --read-trace DIR    (the library's dispatches of that trace, in order)

A process loads ONE library (JJ_LIB_PATH is read when jubjub_amd is imported), so this driver opens no GPU itself: it starts one worker process
per route and round, one at a time, each under a time limit, and stops at the first worker that does not end well.  Rounds ALTERNATE:
  new     this commit: (b) jj_group_hash; (c) jj_decompress alone on digests that are ready on the device -- the floor: what the decoder chain
          costs without any hash --; and jj_blake2s alone
  parent  (a) a build of the PARENT commit: the messages copied to the host, hashed by hashlib.blake2s in one thread and in 16 processes, the
          digests copied back, jj_decompress
A 64-byte prefix with 11-byte and with 32-byte messages (one block on the device after the host's midstate), the flags of the group hash of the
Zcash specification (ZIP216 | NOT_SMALL_ORDER | CLEAR_COFACTOR); messages and results on the device.  Every worker warms up, holds 64 rows to
the restatement of tests/group_hash_cases.py and reports host-clock seconds per call over a window of --seconds of work (one pass where a
pass is longer).  A window queues its calls on the stream and synchronises once at its end: with device-resident results that is time per call
in a full queue (back-to-back throughput), not the latency of one call.  Median [min .. max] of the rounds.  The output is profiles/group_hash_ab.txt.

EXPECTATION, written before the first run: (b) - (c) is near the traced time of k_blake2s and below the 0.084 ms per 2^20 units of
k_sig_challenge for one BLAKE2b block: one BLAKE2s block is 10 rounds of 32-bit operations against 12 rounds on register pairs,
reads 11 or 32 bytes per unit against 96 and writes 32 bytes as that kernel does."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
PERSONAL = b"JJ_gh_ab"
FLAGS = 1 | 4 | 8
MSG_LENS = (11, 32)
PREFIX = bytes((37 * i + 11) & 0xFF for i in range(64))


def _hash_block(args):
    rows, length = args
    return b"".join(hashlib.blake2s(PREFIX + rows[i:i + length], digest_size=32, person=PERSONAL).digest() for i in range(0, len(rows), length))


def worker(args):
    import numpy as np
    import torch

    from jubjub_amd import Engine, _lib
    from tests import group_hash_cases as GC

    route = args.worker
    blob = open(_lib.LIB_PATH, "rb").read()
    for name in ("jj_blake2s", "jj_group_hash"):
        if name.encode() not in blob:
            assert route == "parent", "the library under test lacks %s" % name
            _lib._SIGS.pop(name)                                         # the parent's build: the binding must not ask for the symbols
    pool = None
    if route == "parent":
        import multiprocessing

        pool = multiprocessing.get_context("fork").Pool(16)              # forked BEFORE this process opens the GPU: the children never have it open
    eng = Engine(0)

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
        for L in MSG_LENS:
            g = torch.Generator(device="cpu").manual_seed(1000 * log2n + L)
            msgs = torch.randint(0, 256, (n, L), dtype=torch.uint8, generator=g).cuda()
            want_pts, want_ok = GC.expected(PERSONAL, PREFIX, msgs[:64].cpu().numpy(), FLAGS)
            tag = "%d-byte messages %d" % (L, log2n)

            def hashed(procs):
                rows = msgs.cpu().numpy().tobytes()
                if procs == 1:
                    d = _hash_block((rows, L))
                else:
                    step = -(-n // procs) * L
                    d = b"".join(pool.map(_hash_block, [(rows[o:o + step], L) for o in range(0, len(rows), step)]))
                return eng.decompress(torch.from_numpy(np.frombuffer(d, dtype=np.uint8).reshape(n, 32).copy()).cuda(), FLAGS)

            if route in ("new", "trace"):
                pts, ok = eng.group_hash(msgs, PERSONAL, PREFIX, FLAGS)
                assert np.array_equal(pts[:64].cpu().numpy(), want_pts) and np.array_equal(ok[:64].cpu().numpy(), want_ok)
                if route == "trace":
                    if log2n == max(args.log2n):
                        torch.cuda.synchronize()
                        eng.group_hash(msgs, PERSONAL, PREFIX, FLAGS)
                        torch.cuda.synchronize()
                    continue
                dig = eng.blake2s(msgs, PERSONAL, PREFIX)
                out["(b) jj_group_hash, " + tag] = window(lambda: eng.group_hash(msgs, PERSONAL, PREFIX, FLAGS))
                out["(c) jj_decompress on ready digests, " + tag] = window(lambda: eng.decompress(dig, FLAGS))
                out["    jj_blake2s alone, " + tag] = window(lambda: eng.blake2s(msgs, PERSONAL, PREFIX))
            else:
                pts, ok = hashed(16)
                assert np.array_equal(pts[:64].cpu().numpy(), want_pts) and np.array_equal(ok[:64].cpu().numpy(), want_ok)
                out["(a) hashlib x1 + jj_decompress, " + tag] = window(lambda: hashed(1))
                out["(a) hashlib x16 + jj_decompress, " + tag] = window(lambda: hashed(16))
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
        first = max(k for k, r in enumerate(rows) if "k_blake2s" in r[0])         # the last call: one k_blake2s, then the decoder chain
        tail = rows[first:]
        print("# %s: %d dispatches of the library; the last jj_group_hash call (%d-byte messages, behind the warm-up):" % (os.path.basename(path), len(rows), MSG_LENS[-1]))
        for name, g, w, ns in tail:
            print("  %-64s grid %9d x %3d  %9.3f ms" % (name.split("(")[0][-64:], g, w, ns / 1e6))
        hs = sorted(ns for name, g, w, ns in rows if "k_blake2s" in name and g == max(r[1] for r in rows if "k_blake2s" in r[0]))
        print("# k_blake2s at the largest grid, every traced dispatch: %s ms" % ", ".join("%.3f" % (x / 1e6) for x in hs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--worker", choices=["new", "parent", "trace"])
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
        order = ("new", "parent") if rnd % 2 == 0 else ("parent", "new")
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
    print("# jj_group_hash against hashlib + jj_decompress on the parent's build; 64-byte prefix, flags ZIP216 | NOT_SMALL_ORDER | CLEAR_COFACTOR;")
    print("# seconds of host clock per call, device-resident messages and results; %d alternating rounds of one process per route; median [min .. max]" % args.rounds)
    print("%-58s %8s %12s %24s %14s" % ("route", "log2 n", "ms per call", "[min .. max]", "M units / s"))
    med = {}
    for key in sorted(results, key=lambda k: (int(k.rsplit(" ", 1)[1]), k.split(", ")[1], k)):
        v = sorted(results[key])
        name, log2n = key.rsplit(" ", 1)
        med[key] = v[len(v) // 2]
        print("%-58s %8s %12.3f %24s %14.2f" % (name, log2n, med[key] * 1e3, "[%.3f .. %.3f]" % (v[0] * 1e3, v[-1] * 1e3), (1 << int(log2n)) / med[key] / 1e6))
    print("# what the hash adds, (b) - (c) of the medians:")
    for key in sorted(med):
        if key.startswith("(b)"):
            tag = key.split(", ", 1)[1]
            print("#   %-32s %9.3f ms" % (tag, (med[key] - med["(c) jj_decompress on ready digests, " + tag]) * 1e3))
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
