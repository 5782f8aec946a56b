#!/usr/bin/env python3
"""A/B of jj_msm_ragged against what a caller could do before it, on the GPU box:
python tools/msm_ragged_bench.py [--terms-log2 18] [--calls 20] [--rounds 5] [--only U G B] > profiles/msm_ragged_ab.txt

One process, device-resident inputs, three seeded length distributions at about 2^18 terms:
  U  uniform: 1024 segments of 256 terms
  G  geometric, mean 64, capped at 8192
  B  bimodal: 90 % segments of 4 terms, 10 % of 2000 terms
Per distribution every configuration is warmed up and compared byte for byte with `ragged` on the same inputs (tests/test_gpu_msm_ragged.py
holds jj_msm_ragged to the oracle), then the configurations ALTERNATE in `rounds` rounds of `calls` calls each (`jobs`: a tenth as many; host clock around calls
that end in a synchronise):
  ragged   jj_msm_ragged
  padded   jj_msm_batch on the rows zero-padded to the longest one (the padding is done once, outside the timed region)
  jobs     a stream of jj_msm_begin / jj_msm_finish jobs, one per non-empty segment, six in flight
  batch    (U only) jj_msm_batch on the same rectangle
Median and min .. max of the rounds' ms per call (spread = max - min), and the ratios padded / ragged, jobs / ragged, batch / ragged."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def lengths(kind, total, rng):
    if kind == "U":
        return np.full(total // 256, 256, dtype=np.int64)
    out, left = [], total
    while left > 0:
        if kind == "G":
            n = min(int(rng.geometric(1.0 / 64)), 8192)
        else:
            n = 2000 if rng.random() < 0.1 else 4
        n = min(n, left)
        out.append(n)
        left -= n
    return np.asarray(out, dtype=np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--terms-log2", type=int, default=18)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", nargs="*", default=["U", "G", "B"])
    ap.add_argument("--stamp", default="", help="what the build is (default: git describe of this checkout)")
    ap.add_argument("--no-jobs", action="store_true", help="leave the per-segment jobs stream out (e.g. under a kernel trace)")
    args = ap.parse_args()
    import torch

    from jubjub_amd import Engine

    eng = Engine(0)
    dev = torch.device("cuda", 0)
    stamp = args.stamp
    if not stamp:
        try:
            stamp = subprocess.check_output(["git", "-C", ROOT, "describe", "--always", "--dirty"], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            stamp = "unknown (not a git checkout; pass --stamp)"
    lib = os.path.join(ROOT, "jubjub_amd", "lib", "libjubjub_hip.so")
    print("# ragged MSM A/B: %d rounds x %d calls (jobs: %d), alternating, device-resident; ms per call: median [min .. max] of the rounds" % (args.rounds, args.calls, max(1, args.calls // 10)))
    print("# build: %s, libjubjub_hip.so of %d bytes; options: slice_min %d, waves %d, round_terms %d" % (
        stamp, os.path.getsize(lib), eng.get_option("msm_ragged_slice_min"), eng.get_option("msm_ragged_waves"), eng.get_option("msm_ragged_round_terms")))

    def timed(fn, calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / calls

    print("%-4s %-8s %10s %24s %8s %12s" % ("dist", "config", "median ms", "[min .. max]", "spread", "M terms/s"))
    for kind in args.only:
        rng = np.random.default_rng({"U": 1, "G": 2, "B": 3}[kind])
        lens = lengths(kind, 1 << args.terms_log2, rng)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        S, N, longest = len(lens), int(off[-1]), int(lens.max())
        plan = eng.plan_msm_ragged(off)
        print("# %s: %d segments, %d terms, longest %d, mean %.1f; plan: %d short, %d long, %d items, %d rounds; padded rectangle %d x %d = %.1f x the terms"
              % (kind, S, N, longest, N / S, plan["short"], plan["long"], plan["items"], plan["rounds"], S, longest, S * longest / N))
        s = eng.synth_bytes32(N, seed=700 + ord(kind), device=dev)
        p = eng.random_points(N, seed=800 + ord(kind), subgroup=False, device=dev)
        # the padded rectangle: zero scalars and the identity beyond a row's end
        idx = torch.from_numpy(np.repeat(np.arange(S), lens) * longest + (np.arange(N) - np.repeat(off[:-1].astype(np.int64), lens))).to(dev)
        sp = torch.zeros((S * longest, 32), dtype=torch.uint8, device=dev)
        pp = torch.zeros((S * longest, 64), dtype=torch.uint8, device=dev)
        pp[:, 32] = 1
        sp[idx] = s
        pp[idx] = p
        sp, pp = sp.reshape(S, longest, 32), pp.reshape(S, longest, 64)
        segs = [(s[int(off[k]):int(off[k + 1])], p[int(off[k]):int(off[k + 1])]) for k in range(S) if lens[k]]

        def jobs():
            q, res = [], []
            for a, b in segs:
                q.append(eng.msm_begin(a, b))
                if len(q) > 6:
                    res.append(eng.msm_finish(q.pop(0)))
            res += [eng.msm_finish(j) for j in q]
            return res

        cfg = {"ragged": lambda: eng.msm_ragged(s, p, off), "padded": lambda: eng.msm_batch(sp, pp)}
        if not args.no_jobs:
            cfg["jobs"] = jobs
        if kind == "U":
            cfg["batch"] = lambda: eng.msm_batch(s.reshape(S, longest, 32), p.reshape(S, longest, 64))
        ref = cfg["ragged"]()                                                     # warm-up and comparison, every configuration
        torch.cuda.synchronize()
        ref = ref.cpu().numpy()
        for name, fn in cfg.items():
            got = fn()
            got = np.stack(got) if name == "jobs" else got.cpu().numpy()
            want = ref[lens > 0] if name == "jobs" else ref
            assert (got == want).all(), "%s differs from ragged on %s" % (name, kind)
        res = {k: [] for k in cfg}
        for _ in range(args.rounds):
            for name, fn in cfg.items():
                res[name].append(timed(fn, max(1, args.calls // 10) if name == "jobs" else args.calls))
        med = {}
        for name in cfg:
            v = sorted(res[name])
            med[name] = v[len(v) // 2]
            print("%-4s %-8s %10.4f %24s %8.4f %12.2f" % (kind, name, med[name], "[%.4f .. %.4f]" % (v[0], v[-1]), v[-1] - v[0], N / med[name] / 1e3))
        print("%-4s ratios: %s" % (kind, ", ".join("%s / ragged = %.3f" % (k, med[k] / med["ragged"]) for k in cfg if k != "ragged")))
        sys.stdout.flush()
        del sp, pp, segs
    eng.close()


if __name__ == "__main__":
    main()
