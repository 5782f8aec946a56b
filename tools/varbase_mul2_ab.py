#!/usr/bin/env python3
"""A/B of the two-term variable-base multiplication (jj_varbase_mul2_*) against what a caller could do before it, on the GPU box:
python tools/varbase_mul2_ab.py [--log2n 20 16] [--calls 10]

One process, device-resident inputs.  Per size every configuration is warmed up and its result compared byte for byte with configuration A's on
the same inputs (this directory does not use the test suite's oracle; tests/test_gpu_varbase_mul2.py holds every unit to it), then the
configurations ALTERNATE in five rounds of `calls` calls each (host clock around calls that end in a synchronise):
  A  jj_varbase_mul_vartime x 2 + jj_point_add   (entry points this change does not alter: the parent commit's capability)
  B  jj_msm_batch with two-term rows
  C  jj_varbase_mul2_vartime, signed 5-bit windows (option vb_mul2_window = 5)
  D  jj_varbase_mul2_vartime, signed 4-bit windows (vb_mul2_window = 4)
  E  jj_varbase_mul2_scalars (one pair of scalars), the default width
Median and min .. max of the rounds' ms per call (spread = max - min), and the ratios A / C, A / D.  The output is profiles/varbase_mul2_ab.txt."""
import argparse
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="*", default=[20, 16])
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import torch

    from jubjub_amd import Engine

    eng = Engine(0)
    e5, e4 = Engine(0, options={"vb_mul2_window": 5}), Engine(0, options={"vb_mul2_window": 4})
    print("# two-term var-base A/B: %d rounds x %d calls, alternating, device-resident; ms per call: median [min .. max] of the rounds" % (args.rounds, args.calls))
    print("# default vb_mul2_window = %d" % eng.get_option("vb_mul2_window"))

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.calls

    print("%-6s %-34s %10s %22s %8s %12s" % ("log2n", "config", "median ms", "[min .. max]", "spread", "M units/s"))
    for lg in args.log2n:
        n = 1 << lg
        dev = torch.device("cuda", 0)
        a, b = eng.synth_bytes32(n, seed=300 + lg, device=dev), eng.synth_bytes32(n, seed=400 + lg, device=dev)
        p, q = eng.random_points(n, seed=500 + lg, subgroup=False, device=dev), eng.random_points(n, seed=600 + lg, subgroup=True, device=dev)
        ab = torch.cat([a[0], b[0]])
        s2, p2 = torch.stack([a, b], dim=1).contiguous(), torch.stack([p, q], dim=1).contiguous()
        cfg = {
            "A varbase_mul_vartime x2 + point_add": lambda: eng.point_add(eng.varbase_mul_vartime(a, p), eng.varbase_mul_vartime(b, q)),
            "B msm_batch, two-term rows": lambda: eng.msm_batch(s2, p2),
            "C varbase_mul2_vartime w=5": lambda: e5.varbase_mul2_vartime(a, p, b, q),
            "D varbase_mul2_vartime w=4": lambda: e4.varbase_mul2_vartime(a, p, b, q),
            "E varbase_mul2_scalars": lambda: eng.varbase_mul2_scalars(ab, p, q),
        }
        ref = cfg["A varbase_mul_vartime x2 + point_add"]()
        for name, fn in cfg.items():
            if name.startswith("E"):
                a0, b0 = a[0].expand(n, 32).contiguous(), b[0].expand(n, 32).contiguous()
                assert torch.equal(fn(), eng.point_add(eng.varbase_mul_vartime(a0, p), eng.varbase_mul_vartime(b0, q))), "%s differs from A at 2^%d" % (name, lg)
            else:
                assert torch.equal(fn(), ref), "%s differs from A at 2^%d" % (name, lg)
        res = {k: [] for k in cfg}
        for _ in range(args.rounds):
            for name, fn in cfg.items():
                res[name].append(timed(fn))
        med = {}
        for name in cfg:
            v = sorted(res[name])
            med[name] = v[len(v) // 2]
            print("%-6d %-34s %10.4f %22s %8.4f %12.2f" % (lg, name, med[name], "[%.4f .. %.4f]" % (v[0], v[-1]), v[-1] - v[0], n / med[name] / 1e3))
        A = med["A varbase_mul_vartime x2 + point_add"]
        print("%-6d ratios: A / C = %.3f, A / D = %.3f, A / E = %.3f, A / B = %.3f   (derived from the field-operation count: A / C = 1.60)"
              % (lg, A / med["C varbase_mul2_vartime w=5"], A / med["D varbase_mul2_vartime w=4"], A / med["E varbase_mul2_scalars"], A / med["B msm_batch, two-term rows"]))
        sys.stdout.flush()
    for e in (eng, e5, e4):
        e.close()


if __name__ == "__main__":
    main()
