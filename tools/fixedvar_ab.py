#!/usr/bin/env python3
"""A/B of the fused fixed + variable multiplication (jj_fixedvar_mul_vartime) against what a caller could do before it, on the GPU box:
python tools/fixedvar_ab.py [--log2n 20 16] [--calls 10] [--split-lib PATH]

One process, device-resident inputs, G = one prime-order point.  Per size every configuration is warmed up and its result compared byte for byte with
configuration A's on the same inputs (this directory does not use the test suite's oracle; tests/test_gpu_fixedvar.py holds every unit to it), then
the configurations ALTERNATE in five rounds of `calls` calls each (host clock around calls that end in a synchronise):
  F8 F10 F13  jj_fixedvar_mul_vartime on gathered tables of width 8, 10, 13 (k_varbase_fixed)
  F7          jj_fixedvar_mul_vartime on the default LDS table (k_varbase<true>, then k_fixedbase_comb with chain = 1)
  A           jj_fixedbase_mul (default table) + jj_varbase_mul_vartime + jj_point_add: the three calls of a verifier before this entry point
  B           jj_varbase_mul2_vartime with G broadcast
  C           jj_varbase_mul_vartime alone: the floor (the variable term and the normalisation, no fixed term)
Median and min .. max of the rounds' ms per call (spread = max - min).  Latency: one call at a time at n = 1024 on the quad route (the default
vb_quad_max) and on the lane route (vb_quad_max = 1), median of `calls` x `rounds` single calls.
--split-lib: a probe build of the library (python -c "from jubjub_amd import build as b; b.build_variant(PATH, ['-DJJ_EXPERIMENTS',
'-DJJ_FIXEDVAR_PROBE_SPLIT'])") in which gathered tables take k_varbase<true> and then k_fixedbase_gather with chain = 1; the shipped library and the
probe then run F8 F10 F13 and C at 2^20 in child processes, alternating, two runs each.  The output is profiles/fixedvar_ab.txt."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="*", default=[20, 16])
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--split-lib", default=None)
    ap.add_argument("--child", default=None, help="label of a child run: F8 F10 F13 and C only, no latency part")
    args = ap.parse_args()
    import numpy as np
    import torch

    from jubjub_amd import Engine

    eng = Engine(0)
    g = np.ascontiguousarray(eng.random_points(1, seed=7, subgroup=True)).reshape(64)      # the fixed base: one prime-order point
    widths = (8, 10, 13) if args.child else (8, 10, 13, 7)
    tabs = {w: eng.fixedbase_table(g, w) for w in widths}
    t0 = None if args.child else eng.fixedbase_table(g, 0)
    tag = "" if not args.child else " (%s)" % args.child
    if not args.child:
        print("# fused fixed + variable A/B: %d rounds x %d calls, alternating, device-resident; ms per call: median [min .. max] of the rounds" % (args.rounds, args.calls))

    def timed(fn, calls):
        fn()
        torch.cuda.synchronize()
        s = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - s) * 1e3 / calls

    if not args.child:
        print("%-6s %-44s %10s %22s %8s %12s" % ("log2n", "config", "median ms", "[min .. max]", "spread", "M units/s"))
    dev = torch.device("cuda", 0)
    for lg in args.log2n:
        n = 1 << lg
        a, b = eng.synth_bytes32(n, seed=300 + lg, device=dev), eng.synth_bytes32(n, seed=400 + lg, device=dev)
        q = eng.random_points(n, seed=600 + lg, subgroup=True, device=dev)
        gb = torch.from_numpy(g).to(dev).expand(n, 64).contiguous()
        cfg = {}
        for w in widths:
            cfg["F%d fixedvar_mul_vartime, table %d" % (w, w)] = (lambda w=w: eng.fixedvar_mul_vartime(tabs[w], a, b, q))
        if not args.child:
            cfg["A fixedbase_mul + varbase_mul_vartime + point_add"] = lambda: eng.point_add(eng.fixedbase_mul(t0, a), eng.varbase_mul_vartime(b, q))
            cfg["B varbase_mul2_vartime, G broadcast"] = lambda: eng.varbase_mul2_vartime(a, gb, b, q)
        cfg["C varbase_mul_vartime alone (floor)"] = lambda: eng.varbase_mul_vartime(b, q)
        ref = eng.point_add(eng.fixedbase_mul(tabs[8], a), eng.varbase_mul_vartime(b, q))
        for name, fn in cfg.items():
            if not name.startswith("C"):
                assert torch.equal(fn(), ref), "%s differs from the composed calls at 2^%d" % (name, lg)
        res = {k: [] for k in cfg}
        for _ in range(args.rounds):
            for name, fn in cfg.items():
                res[name].append(timed(fn, args.calls))
                assert name.startswith("C") or torch.equal(fn(), ref), "%s differs from the composed calls at 2^%d" % (name, lg)      # every run verified
        med = {}
        for name in cfg:
            v = sorted(res[name])
            med[name] = v[len(v) // 2]
            print("%-6d %-44s %10.4f %22s %8.4f %12.2f" % (lg, name + tag, med[name], "[%.4f .. %.4f]" % (v[0], v[-1]), v[-1] - v[0], n / med[name] / 1e3))
        key = {k.split()[0]: k for k in cfg}
        C = med[key["C"]]
        if args.child:
            print("%-6d ratios%s: %s" % (lg, tag, ", ".join("F%d / C = %.3f" % (w, med[key["F%d" % w]] / C) for w in widths)))
        else:
            A, B = med[key["A"]], med[key["B"]]
            print("%-6d ratios: %s" % (lg, ", ".join("A / F%d = %.3f, B / F%d = %.3f, F%d / C = %.3f" % (w, A / med[key["F%d" % w]], w, B / med[key["F%d" % w]], w, med[key["F%d" % w]] / C)
                                                     for w in widths)))
        sys.stdout.flush()
    if not args.child:
        # latency: single calls at n = 1024, each ending in a synchronise
        n = 1024
        a, b = eng.synth_bytes32(n, seed=301, device=dev), eng.synth_bytes32(n, seed=401, device=dev)
        q = eng.random_points(n, seed=601, subgroup=True, device=dev)
        lane = Engine(0, options={"vb_quad_max": 1})
        ref = eng.point_add(eng.fixedbase_mul(tabs[8], a), eng.varbase_mul_vartime(b, q))
        print("# latency at n = 1024: ms of one call ending in a synchronise, median [min .. max] of %d single calls, routes alternating" % (args.calls * args.rounds))
        lat = {}
        for w in (10, 7):
            lat["F%d quad route (default vb_quad_max)" % w] = (lambda w=w: eng.fixedvar_mul_vartime(tabs[w], a, b, q))
            lat["F%d lane route (vb_quad_max = 1)" % w] = (lambda w=w: lane.fixedvar_mul_vartime(tabs[w], a, b, q))
        lat["A composed three calls"] = lambda: eng.point_add(eng.fixedbase_mul(t0, a), eng.varbase_mul_vartime(b, q))
        res = {k: [] for k in lat}
        for name, fn in lat.items():
            assert torch.equal(fn(), ref), name
        for _ in range(args.calls * args.rounds):
            for name, fn in lat.items():
                res[name].append(timed(fn, 1))
        for name in lat:
            v = sorted(res[name])
            print("1024   %-44s %10.4f %22s" % (name, v[len(v) // 2], "[%.4f .. %.4f]" % (v[0], v[-1])))
        lane.close()
    for t in list(tabs.values()) + ([t0] if t0 else []):
        t.close()
    eng.close()
    if args.split_lib and not args.child:
        print("# fused kernel against its two halves (k_varbase<true>, then k_fixedbase_gather with chain = 1: the probe build), 2^20 units, child processes alternating")
        sys.stdout.flush()
        for run in range(2):
            for label, libpath in (("fused, run %d" % run, None), ("split, run %d" % run, args.split_lib)):
                env = dict(os.environ)
                if libpath:
                    env["JJ_LIB_PATH"] = os.path.abspath(libpath)
                subprocess.run([sys.executable, os.path.abspath(__file__), "--log2n", "20", "--calls", str(args.calls), "--rounds", str(args.rounds), "--child", label],
                               env=env, check=True, timeout=300)


if __name__ == "__main__":
    main()
