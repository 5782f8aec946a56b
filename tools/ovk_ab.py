#!/usr/bin/env python3
"""A/B of jj_blake2b and jj_ka_kdf_each (the sender's side of a note), on the GPU box:
    python tools/ovk_ab.py --parent-lib PATH [--log2n 20 16 10] [--rounds 3]

A process loads ONE library (JJ_LIB_PATH is read when jubjub_amd is imported), so this driver opens no GPU itself: it starts one worker process
per route and round, one at a time, each under a time limit, and stops at the first worker that does not end well.  Rounds ALTERNATE:
  new     this commit's library: (a) jj_blake2b at the ock shape (a 32-byte prefix, three sources of 32 bytes, digest 32); (b) that call and
          jj_aead_open at len 64 in a stride of 80 behind it, the per-output cost of a rescan with an outgoing viewing key; (c) jj_ka_kdf_each
          with the Sapling flags and h32; (d) the composed five-call route on the same build: jj_decompress, jj_varbase_mul,
          jj_point_mul_by_cofactor, jj_compress, jj_blake2b over share || h
  parent  a build of the PARENT commit: (e) the four-call route without any hash -- jj_decompress, jj_varbase_mul with a scalar per row,
          jj_point_mul_by_cofactor, jj_compress --, the floor jj_ka_kdf was held to
  host    no GPU: hashlib.blake2b over the 128 bytes of an ock row, in one thread and in 16 processes
Inputs and results stay on the device.  Every GPU worker warms up, holds rows of every size to the restatement of tests/ovk_cases.py and reports
host-clock seconds per call over a window of --seconds of work.  Median [min .. max] of the rounds.  The expectation is printed BEFORE the
first worker starts.  The output is profiles/ovk_ab.txt."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

EXPECTATION = """# EXPECTATION, written before the run:
#   jj_blake2b at the ock shape: near the traced k_sig_challenge of one block, 0.084 ms per 2^20 (profiles/sig_challenge_ab.txt) -- one
#     compression, four times the loads; a call is that kernel and the launch, so the small sizes are launch-bound
#   jj_ka_kdf_each: level with the composed five-call route on the same build, and with the parent's four-call route without a hash
#     (14.39 ms per 2^20 in profiles/ka_kdf_ab.txt); BEHIND at 2^10, where jj_varbase_mul has a quad-of-lanes ladder and this call has none
#   the rule: the fused call stands where it is level or ahead within the larger run-to-run range of the two"""


def hash_rows(rows):
    return [hashlib.blake2b(r, digest_size=32, person=b"JJ_ovk_ab_ock___").digest() for r in rows]


def host_worker(args):
    import multiprocessing as mp

    import numpy as np

    out = {}
    for lg in args.log2n:
        n = 1 << lg
        data = np.random.default_rng(lg).integers(0, 256, (n, 128), dtype=np.uint8)
        rows = [r.tobytes() for r in data]
        t0 = time.perf_counter()
        hash_rows(rows)
        out["%d z: hashlib.blake2b, 128-byte rows, one thread" % lg] = time.perf_counter() - t0
        with mp.Pool(16) as pool:
            cut = [rows[k::16] for k in range(16)]
            pool.map(hash_rows, cut[:1])                                  # the workers exist
            t0 = time.perf_counter()
            pool.map(hash_rows, cut)
            out["%d z: hashlib.blake2b, 128-byte rows, 16 processes (rows already cut)" % lg] = time.perf_counter() - t0
    print("RESULT " + json.dumps(out))


def worker(args):
    import numpy as np
    import torch

    from jubjub_amd import Engine, _lib
    from tests import ka_cases as KC
    from tests import ovk_cases as OC

    route = args.worker
    if route == "parent":
        blob = open(_lib.LIB_PATH, "rb").read()
        for name in [k for k in _lib._SIGS if k.encode() + b"\0" not in blob]:
            _lib._SIGS.pop(name)                                       # the parent's build: the binding must not ask for the symbols it lacks
    eng = Engine(0)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0x0CC)
    personal, kdf = b"JJ_ovk_ab_ock___", KC.SAPLING_PERSONAL
    ovk = bytes(range(32))

    def timed(fn, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / k

    def window(fn):
        per = timed(fn, 1)
        timed(fn, 2)
        return timed(fn, max(2, min(4096, int(args.seconds / per) + 1)))

    out = {}
    for lg in args.log2n:
        n = 1 << lg
        sample = sorted({0, 1, n - 1} | {int(x) for x in np.random.default_rng(lg).integers(0, n, 5)})
        cv, cmu, epk = (torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev, generator=gen) for _ in range(3))
        # scalars and points: the planted grid of tests/ka_cases.py tiled, so that the restatement's ladders are shared
        sks, encs = OC.ka_grid(1025, shift=1)
        idx = torch.arange(n, device=dev) % 1025
        S, P = torch.from_numpy(sks).to(dev)[idx].contiguous(), torch.from_numpy(encs).to(dev)[idx].contiguous()
        keys, ok = torch.empty((n, 32), dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
        if route == "new":
            ock = torch.empty((n, 32), dtype=torch.uint8, device=dev)
            c_out = torch.randint(0, 256, (n, 80), dtype=torch.uint8, device=dev, generator=gen)
            op, hit = torch.empty((n, 64), dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
            out["%d a: jj_blake2b, the ock shape" % lg] = window(lambda: eng.blake2b([cv, cmu, epk], personal, ovk, out=ock))
            want = OC.digests([x[sample].cpu().numpy() for x in (cv, cmu, epk)], len(sample), 32, personal, ovk)
            assert np.array_equal(ock[sample].cpu().numpy(), want), (route, "a", lg)

            def scan():
                eng.blake2b([cv, cmu, epk], personal, ovk, out=ock)
                eng.aead_open(ock, c_out, out=(op, hit))

            out["%d b: jj_blake2b + jj_aead_open (len 64 in a stride of 80): an ovk rescan per output" % lg] = window(scan)
            out["%d c: jj_ka_kdf_each, Sapling flags, h32 given" % lg] = window(lambda: eng.ka_kdf_each(S, P, kdf, KC.SAPLING_FLAGS, hash_input=epk, out=(keys, ok)))
            wk, wo = OC.ka_each(sks[[i % 1025 for i in sample]], encs[[i % 1025 for i in sample]], KC.SAPLING_FLAGS, kdf, epk[sample].cpu().numpy())
            assert np.array_equal(keys[sample].cpu().numpy(), wk) and np.array_equal(ok[sample].cpu().numpy(), wo), (route, "c", lg)
            fused = keys.clone()

            def composed():
                pts, dec_ok = eng.decompress(P, KC.ZIP216)
                share = eng.compress(eng.mul_by_cofactor(eng.varbase_mul(S, pts)))
                eng.blake2b([share, epk], kdf, out=keys)
                return dec_ok

            out["%d d: composed, jj_decompress + jj_varbase_mul + jj_point_mul_by_cofactor + jj_compress + jj_blake2b" % lg] = window(composed)
            good = composed() != 0
            assert bool((keys[good] == fused[good]).all()), (route, "d", lg)
        if route == "parent":
            def four():
                pts, _ = eng.decompress(P, KC.ZIP216)
                return eng.compress(eng.mul_by_cofactor(eng.varbase_mul(S, pts)))

            out["%d e: parent commit, jj_decompress + jj_varbase_mul + jj_point_mul_by_cofactor + jj_compress, NO hash" % lg] = window(four)
    eng.close()
    print("RESULT " + json.dumps(out))


# ---- driver: no GPU in this process ---------------------------------------------------------------------------------------------------------
def run_worker(route, lib, args, limit=300):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="*", default=[20, 16, 10])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=0.2, help="work per timed window, at least")
    ap.add_argument("--parent-lib", default="", help="libjubjub_hip.so built from the parent commit: route e runs on it")
    ap.add_argument("--worker", default="")
    args = ap.parse_args()
    if args.worker == "host":
        return host_worker(args)
    if args.worker:
        return worker(args)
    assert args.parent_lib and os.path.exists(args.parent_lib), "--parent-lib: route e must run on a build of the parent commit"
    print("# jj_blake2b and jj_ka_kdf_each: %d alternating rounds of one process per route; median [min .. max] of the rounds, ms per call;" % args.rounds)
    print("# inputs and results on the device")
    print(EXPECTATION, flush=True)
    res = {}
    for rnd in range(args.rounds):
        for route, lib in (("new", ""), ("parent", args.parent_lib), ("host", "")):
            for k, v in run_worker(route, lib, args).items():
                res.setdefault(k, []).append(v)
            print("round %d, route %s: done" % (rnd, route), file=sys.stderr, flush=True)
    res = {k: sorted(v) for k, v in res.items()}
    med = lambda v: v[len(v) // 2]      # noqa: E731
    for lg in args.log2n:
        print("n = 2^%d" % lg)
        for k in sorted(res):
            if k.startswith("%d " % lg):
                v = res[k]
                print("  %-112s %10.4f ms  [%.4f .. %.4f]   %9.2f M rows/s" % (k.split(" ", 1)[1], med(v) * 1e3, v[0] * 1e3, v[-1] * 1e3, (1 << lg) / med(v) / 1e6))
        fused = next((res[k] for k in res if k.startswith("%d c:" % lg)), None)
        for tag, name in (("d", "the composed five-call route"), ("e", "the parent's four-call route without a hash")):
            other = next((res[k] for k in res if k.startswith("%d %s:" % (lg, tag))), None)
            if fused and other:
                gain, spread = med(other) - med(fused), max(fused[-1] - fused[0], other[-1] - other[0])
                print("  jj_ka_kdf_each against %s: %+.4f ms, the larger range %.4f ms -> %s" % (name, gain * 1e3, spread * 1e3, "AHEAD" if gain > spread else "BEHIND" if -gain > spread else "level within the ranges"))


if __name__ == "__main__":
    main()
