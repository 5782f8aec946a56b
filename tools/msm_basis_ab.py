#!/usr/bin/env python3
"""A/B of the fixed-basis MSM (jj_msm_basis_*) against jj_msm, on the GPU box:  python tools/msm_basis_ab.py [--log2n 10 14 17 20] [--calls 200]

One process.  Per size: device-resident inputs, every configuration warmed up and its result compared byte for byte with jj_msm's on the same
inputs (this directory does not use the test suite's oracle; tests/test_gpu_msm_basis.py holds the same sizes to it), then jj_msm, basis mode 1 and basis mode 2 ALTERNATING in five rounds of `calls` synchronous calls each (host clock around calls that end
in a synchronise).  A second table: page-locked HOST scalars (and host points for jj_msm) at 2^17 and 2^20 terms.  Median and min-max of the five
rounds per configuration (the spread is max - min), create time and table bytes per size.  The output is profiles/msm_basis_ab.txt."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="*", default=[10, 14, 17, 20])
    ap.add_argument("--host-log2n", type=int, nargs="*", default=[17, 20])
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import torch

    from jubjub_amd import Engine

    eng = Engine(0)
    print("# fixed-basis MSM A/B: %d rounds x %d synchronous calls, alternating; ms per call: median [min .. max] of the rounds" % (args.rounds, args.calls))

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.calls

    def table(title, sizes, host):
        print("\n## %s" % title)
        print("%-6s %-14s %10s %22s %8s  %s" % ("log2n", "config", "median ms", "[min .. max]", "spread", "notes"))
        for lg in sizes:
            n = 1 << lg
            s = eng.synth_bytes32(n, seed=100 + lg)
            p = eng.random_points(n, seed=200 + lg, subgroup=False)
            want = eng.msm(s, p)
            bases, notes = {}, {}
            for mode in ("points", "windows"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                bases[mode] = eng.msm_basis(p, mode=mode)
                notes[mode] = "create %.2f ms, %s, %.1f MiB, windows %d" % ((time.perf_counter() - t0) * 1e3, bases[mode].info["mode"], bases[mode].info["bytes"] / 2**20, bases[mode].info["windows"])
            auto = eng.msm_basis(p, mode="auto")
            auto_note = "auto takes mode %s" % auto.info["mode"]
            auto.close()
            if host:
                hs, hp = eng.host_alloc((n, 32)), eng.host_alloc((n, 64))
                hs[...] = s
                hp[...] = p
                ds, dpts = hs, hp
            else:
                ds, dpts = torch.from_numpy(s).cuda(), torch.from_numpy(p).cuda()
            cfg = {"jj_msm": lambda: eng.msm(ds, dpts), "basis mode 1": lambda: eng.msm_basis_mul(bases["points"], ds), "basis mode 2": lambda: eng.msm_basis_mul(bases["windows"], ds)}
            for name, fn in cfg.items():
                got = fn()
                got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
                assert (got.reshape(64) == want).all(), "%s differs from jj_msm at 2^%d" % (name, lg)
            res = {k: [] for k in cfg}
            for _ in range(args.rounds):
                for name, fn in cfg.items():
                    res[name].append(timed(fn))
            for name in cfg:
                v = sorted(res[name])
                note = notes.get({"basis mode 1": "points", "basis mode 2": "windows"}.get(name, name), "")
                print("%-6d %-14s %10.4f %22s %8.4f  %s%s" % (lg, name, v[len(v) // 2], "[%.4f .. %.4f]" % (v[0], v[-1]), v[-1] - v[0], note, ", equal to jj_msm" if name != "jj_msm" else ""))
            print("%-6d %s" % (lg, auto_note))
            for b in bases.values():
                b.close()
            sys.stdout.flush()

    table("device-resident scalars (and points for jj_msm)", args.log2n, False)
    table("page-locked HOST scalars (and host points for jj_msm)", args.host_log2n, True)
    eng.close()


if __name__ == "__main__":
    main()
