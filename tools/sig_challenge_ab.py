#!/usr/bin/env python3
"""A/B of Schnorr challenges hashed on the device (jj_sig_challenge) against what a caller did before it, on the GPU box:
    python tools/sig_challenge_ab.py --parent-lib PATH [--log2n 10 16 20] [--rounds 3]
    python tools/sig_challenge_ab.py --worker trace      (nothing is timed: every shape once after a warm-up, for rocprofv3 --kernel-trace)
    python tools/sig_challenge_ab.py --read-trace DIR    (the k_sig_challenge dispatches of that trace, in order, beside the shapes of --worker trace)

A process loads ONE library (JJ_LIB_PATH is read when jubjub_amd is imported), so this driver opens no GPU itself: it starts one worker process
per route and round, one at a time, each under a time limit, and stops at the first worker that does not end well.  Rounds ALTERNATE:
  new   the shipped library: jj_sig_challenge on device-resident R, A and messages (fixed stride and ragged; 32-, 64- and 96-byte messages: one block, one block
        that ends exactly on its edge, two blocks; and one point at 1 KiB messages), a device result; then hash + sigbatch_verify and hash + sigverify_each through Engine.sigbatch_verify_msgs /
        Engine.sigverify_each_msgs at the largest size
  old   a build of the PARENT commit: hashlib.blake2b over R || A || M in (a) one thread and (b) 16 processes (hashlib holds the GIL below 2 KiB,
        so threads would not spread it; the processes are forked before the GPU is opened, never open it, and read the rows and write the
        digests through shared memory, so nothing is pickled), then jj_fr_from_bytes_wide.  "hash only" starts from host bytes; "from device
        arrays" adds what a verifier whose signature arrays are on the device pays: the copies of R, A and M to the host and of the digests
        back.  Then the same two checks end to end with route (b).
Every worker makes its own valid signatures (the challenges by its own route), warms every shape up, checks every verdict, and reports
host-clock seconds per call over a window of --seconds of work per shape (one pass where a pass is longer).  Median [min .. max] of the rounds.
The output is profiles/sig_challenge_ab.txt."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
PERSONAL = b"Zcash_RedJubjubH"
LENGTHS = (32, 64, 96)               # with R and A: 96 and 128 bytes are ONE block (128 ends exactly on it), 160 bytes are two
LONG = (16, 1024)                    # (log2 n, message bytes) of the one long-message point
PROCS = 16

# ---- the old route's hashing: rows in shared memory, set up before the fork -------------------------------------------------------------------
_SHM = {}


def _hash_rows(lo, hi, L):
    import numpy as np

    n = _SHM["n"]
    buf = _SHM["in"]
    R, A, M = buf[:32 * n].reshape(n, 32), buf[32 * n:64 * n].reshape(n, 32), buf[64 * n:64 * n + L * n].reshape(n, L)
    out = _SHM["out"][:64 * n].reshape(n, 64)
    for i in range(lo, hi):
        out[i] = np.frombuffer(hashlib.blake2b(R[i].tobytes() + A[i].tobytes() + M[i].tobytes(), digest_size=64, person=PERSONAL).digest(), np.uint8)
    return hi - lo


def _shm_setup(nmax, lmax):
    import multiprocessing as mp
    from multiprocessing import shared_memory

    import numpy as np

    a, b = shared_memory.SharedMemory(create=True, size=(64 + lmax) * nmax), shared_memory.SharedMemory(create=True, size=64 * nmax)
    _SHM.update({"in": np.ndarray(((64 + lmax) * nmax,), np.uint8, a.buf), "out": np.ndarray((64 * nmax,), np.uint8, b.buf), "blocks": (a, b)})
    return mp.get_context("fork").Pool(PROCS)


def _shm_close(pool):
    pool.close()
    pool.join()
    _SHM.pop("in"), _SHM.pop("out")
    for s in _SHM.pop("blocks"):
        s.close()
        s.unlink()


# ---- worker: one library, one route, every shape once ---------------------------------------------------------------------------------------
def worker(args):
    from jubjub_amd import _lib

    old = args.worker == "old"
    pool = None
    if old:
        if b"jj_sig_challenge" not in open(_lib.LIB_PATH, "rb").read():
            _lib._SIGS.pop("jj_sig_challenge", None)            # the parent's build: the binding must not ask for the symbol
        pool = _shm_setup(1 << max(args.log2n), max(LENGTHS))   # forked here: before torch and the library open the GPU
    import numpy as np
    import torch

    from jubjub_amd import Engine
    from tests import sig_batch_cases as SC

    eng = Engine(0)
    dev = torch.device("cuda", 0)
    base = SC.bases()["prime"]
    base_dev = torch.from_numpy(np.array(base)).to(dev)
    tab = eng.fixedbase_table(base, 13)
    gen = torch.Generator(device=dev).manual_seed(0x5C11)

    def rand(*shape):
        return torch.randint(0, 256, shape, dtype=torch.uint8, device=dev, generator=gen)

    def timed(fn, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / k

    def window(fn):
        per = timed(fn, 1)
        if per > args.seconds:                                  # a pass longer than the window (the host loops): the second pass is the figure
            return timed(fn, 1)
        timed(fn, 2)
        return timed(fn, max(2, min(4096, int(args.seconds / per) + 1)))

    def ragged_offsets(n, L):
        lens = np.random.default_rng(0x5C12 + L).integers(L // 2, 3 * L // 2 + 1, n)        # mean L
        off = np.zeros(n + 1, np.uint64)
        off[1:] = np.cumsum(lens, dtype=np.uint64)
        return off

    def host_hash(R, A, M, n, L, procs, from_device):
        """the old route -> (n, 32) challenges on the device"""
        _SHM["n"] = n
        buf = _SHM["in"]
        if from_device:
            buf[:32 * n] = R.cpu().numpy().reshape(-1)
            buf[32 * n:64 * n] = A.cpu().numpy().reshape(-1)
            buf[64 * n:64 * n + L * n] = M.cpu().numpy().reshape(-1)
        if procs == 1:
            _hash_rows(0, n, L)
        else:
            step = (n + procs - 1) // procs
            assert sum(pool.starmap(_hash_rows_n, [(n, lo, min(n, lo + step), L) for lo in range(0, n, step)])) == n
        wide = torch.from_numpy(_SHM["out"][:64 * n].reshape(n, 64)).to(dev) if from_device else _SHM["out"][:64 * n].reshape(n, 64)
        return eng.from_bytes_wide("fr", wide)

    out = {}
    shapes = [(lg, L) for lg in args.log2n for L in LENGTHS]
    if args.worker == "trace":
        order = []
        for lg, L in shapes + [LONG]:
            n = 1 << lg
            R, A, M = rand(n, 32), rand(n, 32), rand(n, L)
            off = ragged_offsets(n, L)
            F = rand(int(off[-1]))
            for kind in ("fixed", "ragged"):
                for _ in range(3):
                    eng.sig_challenge(R, A, M, PERSONAL) if kind == "fixed" else eng.sig_challenge(R, A, F, PERSONAL, offsets=off)
                    torch.cuda.synchronize()
                order.append("2^%d x %d bytes %s" % (lg, L, kind))
        print("TRACED " + json.dumps(order))
    elif not old:
        for lg, L in shapes + [LONG]:
            n = 1 << lg
            R, A, M = rand(n, 32), rand(n, 32), rand(n, L)
            off = ragged_offsets(n, L)
            F = rand(int(off[-1]))
            res = torch.empty((n, 32), dtype=torch.uint8, device=dev)
            out["%d %d fixed" % (lg, L)] = window(lambda: eng.sig_challenge(R, A, M, PERSONAL, out=res))
            out["%d %d ragged" % (lg, L)] = window(lambda: eng.sig_challenge(R, A, F, PERSONAL, offsets=off, out=res))
            row = np.random.default_rng(lg + L).integers(0, n)      # one unit of every shape held to hashlib
            want = hashlib.blake2b(bytes(R[row].cpu().numpy()) + bytes(A[row].cpu().numpy()) + bytes(F[int(off[row]):int(off[row + 1])].cpu().numpy()), digest_size=64, person=PERSONAL).digest()
            assert int.from_bytes(bytes(res[row].cpu().numpy()), "little") == int.from_bytes(want, "little") % SC.R
    else:
        for lg, L in shapes:
            n = 1 << lg
            R, A, M = rand(n, 32), rand(n, 32), rand(n, L)
            host_hash(R, A, M, n, L, PROCS, True)                # fills the shared rows
            out["%d %d one thread, hash only" % (lg, L)] = window(lambda: host_hash(R, A, M, n, L, 1, False))
            out["%d %d %d processes, hash only" % (lg, L, PROCS)] = window(lambda: host_hash(R, A, M, n, L, PROCS, False))
            out["%d %d %d processes, from device arrays" % (lg, L, PROCS)] = window(lambda: host_hash(R, A, M, n, L, PROCS, True))
    if args.worker in ("new", "old"):
        # end to end at the largest size: valid signatures whose challenges come from this worker's own route
        lg, L = max(args.log2n), 32
        n = 1 << lg
        sk, nonce = [eng.synth_scalars(n, seed, device=dev) for seed in (0x5C20, 0x5C21)]
        R, A, M = eng.compress(eng.fixedbase_mul(tab, nonce)), eng.compress(eng.fixedbase_mul(tab, sk)), rand(n, L)
        z = rand(n, 16)
        z[:, 0] |= 1
        hash_ = (lambda: host_hash(R, A, M, n, L, PROCS, True)) if old else (lambda: eng.sig_challenge(R, A, M, PERSONAL))
        s = eng.field_binary("fr", "add", nonce, eng.field_binary("fr", "mul", hash_(), sk))

        def batch():
            assert eng.sigbatch_verify(base_dev, R, A, s, hash_(), z) == "ok"

        def each():
            assert bool((eng.sigverify_each(tab, R, A, s, hash_()) == 1).all().item())
        out["%d %d end to end: hash + sigbatch_verify" % (lg, L)] = window(batch)
        out["%d %d end to end: hash + sigverify_each" % (lg, L)] = window(each)
    tab.close()
    eng.close()
    if pool is not None:
        _shm_close(pool)
    print("RESULT " + json.dumps(out))


def _hash_rows_n(n, lo, hi, L):
    _SHM["n"] = n
    return _hash_rows(lo, hi, L)


# ---- driver: no GPU in this process ---------------------------------------------------------------------------------------------------------
def run_worker(route, lib, args, limit=420):
    env = dict(os.environ)
    env.pop("JJ_LIB_PATH", None)
    if lib:
        env["JJ_LIB_PATH"] = os.path.abspath(lib)
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--worker", route, "--seconds", str(args.seconds), "--log2n"] + [str(x) for x in args.log2n]
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
            if "k_sig_challenge" in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), int(r["Grid_Size_X"] if "Grid_Size_X" in r else r["Grid_Size"]), r.get("VGPR_Count", "?")))
    rows.sort()
    print("# k_sig_challenge dispatches in order (three per shape of --worker trace: fixed, then ragged): microseconds, grid, VGPRs")
    for k, (_, dur, grid, vgpr) in enumerate(rows):
        print("%3d  %10.2f us  grid %-9d vgpr %s" % (k, dur / 1e3, grid, vgpr))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="*", default=[10, 16, 20])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=0.2, help="work per timed window, at least")
    ap.add_argument("--parent-lib", default="", help="libjubjub_hip.so built from the parent commit: the old route runs on it")
    ap.add_argument("--worker", default="")
    ap.add_argument("--read-trace", default="", metavar="DIR")
    args = ap.parse_args()
    if args.read_trace:
        return read_trace(args.read_trace)
    if args.worker:
        return worker(args)
    assert args.parent_lib and os.path.exists(args.parent_lib), "--parent-lib: the old route must run on a build of the parent commit"
    res = {}
    for _ in range(args.rounds):
        for route, lib in (("new", ""), ("old", args.parent_lib)):
            for k, v in run_worker(route, lib, args).items():
                res.setdefault((route, k), []).append(v)
    res = {k: sorted(v) for k, v in res.items()}
    med = lambda v: v[len(v) // 2]      # noqa: E731
    fmt = lambda v: "%12.4f ms  [%.4f .. %.4f]" % (med(v) * 1e3, v[0] * 1e3, v[-1] * 1e3)      # noqa: E731
    print("# Schnorr challenges: %d alternating rounds of one process per route; median [min .. max] of the rounds, ms per call" % args.rounds)
    print("# new: jj_sig_challenge on the shipped library, device-resident inputs and result; old: hashlib + jj_fr_from_bytes_wide on the PARENT commit's library")
    for lg in args.log2n:
        for L in LENGTHS:
            n = 1 << lg
            print("n = 2^%d, %d-byte messages (%d blocks with R and A)" % (lg, L, (64 + L + 127) // 128))
            new = res[("new", "%d %d fixed" % (lg, L))]
            print("  new  fixed stride                           %s   %.1f M challenges/s" % (fmt(new), n / med(new) / 1e6))
            print("  new  ragged (lengths %d .. %d)              %s" % (L // 2, 3 * L // 2, fmt(res[("new", "%d %d ragged" % (lg, L))])))
            for name in ("one thread, hash only", "%d processes, hash only" % PROCS, "%d processes, from device arrays" % PROCS):
                v = res[("old", "%d %d %s" % (lg, L, name))]
                print("  old  %-38s %s   %.0f x the new call" % (name, fmt(v), med(v) / med(new)))
    lg, L = LONG
    print("n = 2^%d, %d-byte messages (one lane per message is the wrong shape here)" % (lg, L))
    for kind in ("fixed", "ragged"):
        v = res[("new", "%d %d %s" % (lg, L, kind))]
        print("  new  %-38s %s   %.2f GB/s of message bytes" % (kind, fmt(v), (1 << lg) * L / med(v) / 1e9))
    lg = max(args.log2n)
    print("end to end, n = 2^%d, 32-byte messages, valid signatures, table 13" % lg)
    for name in ("hash + sigbatch_verify", "hash + sigverify_each"):
        a, b = res[("new", "%d 32 end to end: %s" % (lg, name))], res[("old", "%d 32 end to end: %s" % (lg, name))]
        print("  %-24s new %s   old (%d processes) %s   %.2f x" % (name, fmt(a), PROCS, fmt(b), med(b) / med(a)))


if __name__ == "__main__":
    main()
